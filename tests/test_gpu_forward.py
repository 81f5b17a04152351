"""GPU parity of the forward decode (HIP kernels through the C ABI) against the reference's golden
outputs and the CPU oracle.  Neural / MS / QMS: bit-exact soft outputs; SP: hard decisions exact and
soft values within the north star's 1e-4 relative and, beyond that, value for value (sp_check).
"""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

BG2 = np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(ROOT, "resources", "wman_N0576_R34_z24.txt"), int, delimiter="\t")
DEV = torch.device("cuda")


def sp_check(o, ref):
    """SP parity (north star: hard decisions bit-exact, soft values within 1e-4 RELATIVE): equal hard
    decisions and every soft value within rtol 1e-4 of the reference (or of the oracle, which
    reproduces the reference's SP bit for bit: tests/test_oracle_golden.py), with no absolute
    allowance.  The number of values that are not identical is reported (NLDPC_SP_LOG=<file> appends
    one line per check): the device SP follows ATen's product order and torch.tanh's recorded values,
    so against the fixtures (made on this container's torch) and against the oracle (same table) it is
    value for value, and the check asserts that after the 1e-4 bound."""
    o, ref = np.asarray(o), np.asarray(ref)
    assert np.array_equal(o > 0, ref > 0), f"{((o > 0) != (ref > 0)).sum()} hard decisions differ"
    ndiff = int((o != ref).sum())
    rel = float(np.max(np.abs(o - ref) / np.maximum(np.abs(ref), 1e-30))) if ndiff else 0.0
    log = os.environ.get("NLDPC_SP_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0]} values {o.size} not_identical {ndiff} "
                    f"max_rel {rel:.3e}\n")
    np.testing.assert_allclose(o, ref, rtol=1e-4, atol=0)
    assert ndiff == 0, f"{ndiff} of {o.size} SP soft values within 1e-4 but not identical (max rel {rel:.2e})"
    return ndiff


def _bg(name):
    return WIMAX if "wimax" in name else BG2


def _graph(bg, Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(bg, Z)


def expand_cn(g, w, code):
    w = torch.as_tensor(w, dtype=torch.float32, device=DEV)
    if code in (1, 4):
        return w
    if code == 2:
        return w[torch.as_tensor(g.chk, device=DEV)]
    return w.reshape(-1)[:1].expand(g.E)


def expand_vn(g, w, code):
    w = torch.as_tensor(w, dtype=torch.float32, device=DEV)
    return w if code == 2 else w.reshape(-1)[:1].expand(g.N)


def boosted_params(d, g, T, nw, fixed):
    cn, ucn, vn = nw

    def fetch(node, code, t):
        if code in (1, 2, 3):
            k = t
        elif fixed:
            v = [i for i in fixed if i <= t]
            k = max(v) if v else fixed[0]
        else:
            k = 0
        return d[f"param__weight_{node}_{k}"]

    w_cn = torch.stack([expand_cn(g, fetch("CN", cn, t), cn) for t in range(T)]) if cn else None
    use_ucn = ucn == cn and cn in (1, 2, 3)
    w_ucn = torch.stack([expand_cn(g, fetch("UCN", ucn, t), ucn) for t in range(T)]) if use_ucn else None
    w_vn = torch.stack([expand_vn(g, fetch("VN", vn, t), vn) for t in range(T)]) if vn in (2, 3) else None
    return w_cn, w_ucn, w_vn, use_ucn


@pytest.mark.parametrize("name", ["neural_cfg1_snr1_default", "neural_cfg1_snr2_default", "neural_cfg1_snr3_default",
                                  "neural_cfg1_snr4_default", "neural_cfg1_snr2_random",
                                  "neural_bg2_z16_b16_t5_random", "neural_wimax_z24_b16_t20_random",
                                  "neural_bg2_z16_edges"])
@pytest.mark.parametrize("path", ["stream", "fused"])
def test_neural_forward_matches_reference(golden, name, path):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    d = golden(name)
    g = _graph(_bg(name), int(d["Z"]))
    T = int(d["T"])
    x = torch.from_numpy(d["x"]).to(DEV)
    outs, _, _ = decode(g, DecodeCfg(KIND_NEURAL, path=path), x, T, w_cn=torch.from_numpy(d["weights"]).to(DEV),
                        bias=torch.from_numpy(d["biases"]).to(DEV))
    o = outs.cpu().numpy()
    assert np.array_equal(o, d["outputs"]), f"{(o != d['outputs']).sum()} of {o.size} soft values differ"


BOOSTED = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "boosted_*.npz")))


@pytest.mark.parametrize("path", ["stream", "auto"])
@pytest.mark.parametrize("name", BOOSTED)
def test_boosted_forward_matches_reference(golden, name, path):
    from nldpc.decode import DecodeCfg, decode
    d = golden(name)
    g = _graph(_bg(name), int(d["Z"]))
    T = 6 if "target6" in name else int(d["T"])
    nw = tuple(int(v) for v in d["nw"])
    fixed = [int(v) for v in d.get("fixed_nodes", [])]
    w_cn, w_ucn, w_vn, use_ucn = boosted_params(d, g, T, nw, fixed)
    kind, q = int(d["dtype"]), int(d["q"])
    cfg = DecodeCfg(kind=kind, qbit=q, ucn=use_ucn, vn_cumulative=w_vn is not None, path=path)
    x = torch.from_numpy(d["x"]).to(DEV)
    outs, _, _ = decode(g, cfg, x, T, w_cn=w_cn, w_ucn=w_ucn, w_vn=w_vn)
    o = outs.cpu().numpy()
    ref = d["outputs"][:T]
    assert np.array_equal(o > 0, ref > 0)
    if kind == 0:
        sp_check(o, ref)
    else:
        assert np.array_equal(o, ref), f"{(o != ref).sum()} of {o.size} soft values differ"


@pytest.mark.parametrize("path", ["stream", "fused"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_neural_z384_matches_oracle(B, path):
    """BG2 z=384 (the headline graph; the reference cannot run it): GPU == CPU oracle bit for bit."""
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    from oracle.ldpc_oracle import OracleGraph, neural_forward
    T = 4
    g = _graph(BG2, 384)
    gen = torch.Generator().manual_seed(B)
    sigma = (1.0 / (2 * 0.2 * 10 ** 0.2)) ** 0.5
    x = (2 * (-1 + sigma * torch.randn(B, 52, 384, generator=gen)) / sigma ** 2).float()
    w = torch.rand(T, g.E, generator=gen) * 1.2
    b = torch.randn(T, g.E, generator=gen) * 0.1
    outs, _, _ = decode(g, DecodeCfg(KIND_NEURAL, path=path), x.to(DEV), T, w_cn=w.to(DEV), bias=b.to(DEV))
    ref = torch.stack(neural_forward(OracleGraph(BG2, 384), x, list(w), list(b))).numpy()
    o = outs.cpu().numpy()
    assert np.array_equal(o, ref), f"{(o != ref).sum()} of {o.size} differ"


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_boosted_z384_fused_equals_stream(kind):
    """Fused (register-resident) and streaming kernels agree bit for bit at BG2 z=384, Boosted kinds,
    with per-check CN weights, cumulative VN weights and the final message state."""
    from nldpc.decode import DecodeCfg, decode
    T, B = 6, 3
    g = _graph(BG2, 384)
    gen = torch.Generator().manual_seed(kind)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, 384, generator=gen)) / 0.81).float().to(DEV)
    w_cn = (0.5 + torch.rand(T, 42, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV)
    w_vn = (0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV)
    res = {}
    for path in ("stream", "fused"):
        cfg = DecodeCfg(kind=kind, qbit=5, vn_cumulative=True, path=path)
        res[path] = decode(g, cfg, x, T, w_cn=w_cn, w_vn=w_vn)
    assert torch.equal(res["stream"][0], res["fused"][0])
    assert torch.equal(res["stream"][1], res["fused"][1])  # final c2v state


@pytest.mark.parametrize("kind", [1, 2])
def test_boosted_z384_ucn_weights_fused_equals_stream(kind):
    """The decode specialised for UCN with CN / UCN / cumulative VN weights (r6: the library's MODE-7 kernel,
    kernel<KIND, 6>) against the streaming kernels, bit for bit, at BG2 z=384: per-edge CN and UCN weights, per-column
    VN weights, and a channel with exact zeros (the punctured columns) for the check node's zero path."""
    from nldpc.decode import DecodeCfg, decode
    T, B = 8, 3
    g = _graph(BG2, 384)
    gen = torch.Generator().manual_seed(40 + kind)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, 384, generator=gen)) / 0.81).float()
    x[:, :2] = 0.0
    x = x.to(DEV)
    w_cn = (0.5 + torch.rand(T, g.E, generator=gen)).to(DEV)
    w_ucn = (0.3 + torch.rand(T, g.E, generator=gen)).to(DEV)
    w_vn = (0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV)
    res = {}
    for path in ("stream", "fused"):
        cfg = DecodeCfg(kind=kind, qbit=5, ucn=True, vn_cumulative=True, path=path)
        res[path] = decode(g, cfg, x, T, w_cn=w_cn, w_ucn=w_ucn, w_vn=w_vn)
    assert torch.equal(res["stream"][0], res["fused"][0])
    assert torch.equal(res["stream"][1], res["fused"][1])  # final c2v state


def test_fast_path_selection():
    import ctypes
    from nldpc import _lib
    from nldpc.decode import KIND_NEURAL, DecodeCfg
    L = _lib.lib()
    from nldpc import jit
    # built in: BG2 z=384/16/96, WiMAX z=24; any other lifting size gets its kernels compiled at run time
    # (nldpc.jit: z=64 and z=104 -- 104 = 8 x 13 needs parts padded to whole waves)
    for bg, Z, want in ((BG2, 384, 1), (BG2, 16, 1), (WIMAX, 24, 1), (BG2, 96, 1), (BG2, 64, 1), (BG2, 104, 1)):
        g = _graph(bg, Z)
        for save, ucn, exp in ((0, False, want), (1, False, want), (0, True, want)):
            kind = KIND_NEURAL if not ucn else 1
            jit.ensure(g, DEV, kind, save)  # (a no-op for the built-in ones)
            cfg = DecodeCfg(kind, ucn=ucn).c_struct(False)
            out = ctypes.c_int32(-1)
            _lib.check(L.nldpc_fast_path(g.handle(DEV), ctypes.byref(cfg), 4, 20, save, ctypes.byref(out)))
            assert out.value == exp, (Z, save, ucn)


@pytest.mark.parametrize("Z,B", [(384, 3), (16, 21)])
@pytest.mark.parametrize("kind,prefix", [(0, 0), (1, 0), (2, 0), (2, 2), (3, 0)])
def test_saved_activations_fused_equal_stream(kind, prefix, Z, B):
    """Training forward: the fused kernel's SAVE variant writes exactly what the streaming kernels
    write for the backward (every iteration's v2c, the posterior clamp masks, the xin chain), and the
    same outputs.  Z=16 packs 16 codewords per workgroup (B=21: a partial last workgroup)."""
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    T = 5
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(100 * kind + Z + prefix)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, Z, generator=gen)) / 0.81).float().to(DEV)
    if kind == KIND_NEURAL:
        kw = dict(w_cn=(torch.rand(T, g.E, generator=gen) * 1.2).to(DEV),
                  bias=(torch.randn(T, g.E, generator=gen) * 0.1).to(DEV))
    else:
        kw = dict(w_cn=(0.5 + torch.rand(T, 42, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV),
                  w_vn=(0.8 + 0.4 * torch.rand(prefix + T, 52, generator=gen)).to(DEV))
    res = {}
    for path in ("stream", "fused"):
        cfg = DecodeCfg(kind=kind, qbit=5, vn_cumulative=kind != KIND_NEURAL, vn_prefix=prefix, path=path)
        res[path] = decode(g, cfg, x, T, save=True, **kw)
    assert torch.equal(res["stream"][0], res["fused"][0])
    assert torch.equal(res["stream"][1], res["fused"][1])
    # sections of the saved buffer (SavedLayout, nldpc_internal.h); the alignment gaps are not written
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    v2c = T * B * g.E * Z * (1 if kind == 2 else 4)  # QMS saves int8 codes (qms_code)
    secs = [(0, v2c)]
    end = v2c
    if kind != KIND_NEURAL:
        secs.append((al(v2c), T * B * 52 * Z))
        end = al(v2c) + T * B * 52 * Z
        secs.append((al(end), T * B * 52 * Z * 4))
    for name, (off, n) in zip(("v2c", "ymask", "xin"), secs):
        assert torch.equal(res["stream"][2][off:off + n], res["fused"][2][off:off + n]), f"saved {name} differs"


@pytest.mark.parametrize("Z,B", [(384, 3), (16, 21)])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_fused_backward_equals_stream(kind, Z, B):
    """Training backward: the register-resident backward kernel gives the streaming kernels' weight
    gradients (same arithmetic; only the order of the batch sums differs)."""
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode, decode_backward
    T = 5
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(7 * kind + Z)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, Z, generator=gen)) / 0.81).float().to(DEV)
    if kind == KIND_NEURAL:
        kw = dict(w_cn=(torch.rand(T, g.E, generator=gen) * 1.2).to(DEV),
                  bias=(torch.randn(T, g.E, generator=gen) * 0.1).to(DEV))
        need = (True, False, True, False)
    else:
        kw = dict(w_cn=(0.5 + torch.rand(T, 42, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV),
                  w_vn=(0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV))
        need = (True, False, False, True)
    go = [(torch.randn(B, 52 * Z, generator=gen) * 1e-2).to(DEV) for _ in range(T)]
    res = {}
    for path in ("stream", "fused"):
        cfg = DecodeCfg(kind=kind, qbit=5, vn_cumulative=kind != KIND_NEURAL, path=path)
        outs, _, saved = decode(g, cfg, x, T, save=True, **kw)
        res[path] = decode_backward(g, cfg, x, T, go, list(outs.unbind(0)), saved, need=need, **kw)[:4]
    n = 0
    for a, b in zip(res["stream"], res["fused"]):
        assert (a is None) == (b is None)
        if a is not None:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            np.testing.assert_allclose(b, a, rtol=1e-4, atol=1e-5 * max(np.abs(a).max(), 1e-12))
            n += 1
    assert n == 2


@pytest.mark.parametrize("bg,Z,B", [("bg2", 384, 5), ("bg2", 16, 37), ("wimax", 24, 23)])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_count_only_decode_equals_decode_then_count(bg, Z, B, kind):
    """§8 F2: the fused count-only kernels (nldpc_forward_count) give exactly the per-iteration
    (bit errors, frame errors) of decode + ber_counts, against the all-zero codeword and against a
    given y, in both decision conventions (partial last workgroup included: B % G != 0)."""
    from nldpc.channel import ber_counts
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode, decode_count
    g = _graph(BG2 if bg == "bg2" else WIMAX, Z)
    T = 7
    gen = torch.Generator().manual_seed(100 * kind + Z)
    x = (2 * (-1 + 1.1 * torch.randn(B, g.N, Z, generator=gen)) / 1.21).float().to(DEV)
    if kind == KIND_NEURAL:
        kw = dict(w_cn=(torch.rand(T, g.E, generator=gen) * 1.2).to(DEV),
                  bias=(torch.randn(T, g.E, generator=gen) * 0.1).to(DEV))
    else:
        kw = dict(w_cn=(0.5 + torch.rand(T, g.M, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV),
                  w_vn=(0.8 + 0.4 * torch.rand(T, g.N, generator=gen)).to(DEV))
    cfg = DecodeCfg(kind=kind, qbit=5, vn_cumulative=kind != KIND_NEURAL, keep_state=False)
    outs, _, _ = decode(g, cfg, x, T, **kw)
    ys = [None, torch.randint(0, 2, (B, g.N * Z), generator=gen).to(DEV),
          torch.ones((B, g.N * Z), dtype=torch.uint8, device=DEV)]
    for y in ys:
        for conv in (0, 1):
            ref = ber_counts(list(outs), y, convention=conv)
            got = decode_count(g, cfg, x, T, y=y, convention=conv, **kw)
            assert torch.equal(got, ref), (y is None, conv, got.cpu().tolist(), ref.cpu().tolist())
    fast = DecodeCfg(kind=kind, qbit=5, vn_cumulative=kind != KIND_NEURAL, path="fused")
    decode(g, fast, x, 1, **{k: v[:1] for k, v in kw.items()})  # this configuration is on the fused path


def test_count_only_decode_ucn():
    """UCN configurations are counted inside the fused kernel too (counts == decode + counter)."""
    from nldpc.channel import ber_counts
    from nldpc.decode import KIND_MS, DecodeCfg, decode, decode_count
    g = _graph(BG2, 16)
    T, B = 4, 9
    gen = torch.Generator().manual_seed(5)
    x = (2 * (-1 + 1.1 * torch.randn(B, g.N, 16, generator=gen)) / 1.21).float().to(DEV)
    w = (0.5 + torch.rand(T, g.E, generator=gen)).to(DEV)
    cfg = DecodeCfg(kind=KIND_MS, ucn=True)
    outs, _, _ = decode(g, cfg, x, T, w_cn=w, w_ucn=w * 0.5)
    assert torch.equal(decode_count(g, cfg, x, T, w_cn=w, w_ucn=w * 0.5), ber_counts(list(outs)))


UCN_FIXTURES = [n for n in BOOSTED if any(t in n for t in ("nw112", "nw223", "nw330", "nw333")) and "wimax" not in n
                or n == "boosted_wimax_z24_qms5_nw112" or n == "boosted_wimax_z24_ms_nw333"]


@pytest.mark.parametrize("name", UCN_FIXTURES)
def test_ucn_fixtures_on_fused_path(golden, name):
    """UCN (unsatisfied-check weighting, Boosted…py:339-374) on the register-resident kernel, required
    with path="fused": the hard decisions of the previous posterior go through an LDS bit array."""
    from nldpc.decode import DecodeCfg, decode
    d = golden(name)
    g = _graph(_bg(name), int(d["Z"]))
    T = int(d["T"])
    nw = tuple(int(v) for v in d["nw"])
    w_cn, w_ucn, w_vn, use_ucn = boosted_params(d, g, T, nw, [])
    if not use_ucn:
        pytest.skip("UCN weights unused for this sharing combination")
    kind, q = int(d["dtype"]), int(d["q"])
    cfg = DecodeCfg(kind=kind, qbit=q, ucn=True, vn_cumulative=w_vn is not None, path="fused")
    outs, _, _ = decode(g, cfg, torch.from_numpy(d["x"]).to(DEV), T, w_cn=w_cn, w_ucn=w_ucn, w_vn=w_vn)
    o, ref = outs.cpu().numpy(), d["outputs"][:T]
    if kind == 0:
        sp_check(o, ref)
    else:
        assert np.array_equal(o, ref), f"{(o != ref).sum()} of {o.size} soft values differ"


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("Z,B", [(384, 2), (16, 19)])
def test_ucn_fused_equals_stream_later_segment(kind, Z, B):
    """A UCN segment that starts at iteration 3 of a forward (first_iter > 0, the previous posterior
    given as app_prev) with per-check CN / UCN weights and cumulative VN weights: fused == streaming,
    outputs and final message state, also when saving for the backward."""
    from nldpc.decode import DecodeCfg, decode
    T = 4
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(31 * kind + Z)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, Z, generator=gen)) / 0.81).float().to(DEV)
    app = (3 * torch.randn(B, 52 * Z, generator=gen)).to(DEV)
    w_cn = (0.5 + torch.rand(T, 42, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV)
    w_ucn = (0.2 + torch.rand(T, 42, generator=gen))[:, torch.as_tensor(g.chk)].contiguous().to(DEV)
    w_vn = (0.8 + 0.4 * torch.rand(T + 3, 52, generator=gen)).to(DEV)
    for save in (False, True):
        res = {}
        for path in ("stream", "fused"):
            cfg = DecodeCfg(kind=kind, qbit=5, ucn=True, vn_cumulative=True, first_iter=3, vn_prefix=3, path=path)
            res[path] = decode(g, cfg, x, T, w_cn=w_cn, w_ucn=w_ucn, w_vn=w_vn, app_prev=app, save=save)
        assert torch.equal(res["stream"][0], res["fused"][0])
        assert torch.equal(res["stream"][1], res["fused"][1])


@pytest.mark.parametrize("kind", [3, 2, 1])
def test_lifting_96_fused_matches_oracle(kind):
    """A lifting size beyond the hand-listed ones (BG2 z=96: geometry chosen by gen_fused.auto_geometry,
    2 codewords x 5 parts x 96 lanes per workgroup, one LDS chunk) decodes on the register-resident
    kernel (path="fused" is required) bit-exactly against the CPU oracle."""
    from nldpc.decode import DecodeCfg, decode
    from oracle.ldpc_oracle import OracleGraph, boosted_forward, neural_forward, quantize
    T, B, Z = 6, 5, 96
    g = _graph(BG2, Z)
    og = OracleGraph(BG2, Z)
    gen = torch.Generator().manual_seed(96 + kind)
    x = (2 * (-1 + 0.85 * torch.randn(B, 52, Z, generator=gen)) / 0.7225).float()
    if kind == 3:
        w = torch.rand(T, g.E, generator=gen) * 1.2
        b = torch.randn(T, g.E, generator=gen) * 0.1
        outs, _, _ = decode(g, DecodeCfg(kind, path="fused"), x.to(DEV), T, w_cn=w.to(DEV), bias=b.to(DEV))
        ref = torch.stack(neural_forward(og, x, list(w), list(b))).numpy()
    else:
        if kind == 2:
            x = quantize(x, 5)
        wc = 0.5 + torch.rand(T, 42, generator=gen)
        wv = 0.8 + 0.4 * torch.rand(T, 52, generator=gen)
        cfg = DecodeCfg(kind, qbit=5, vn_cumulative=True, path="fused")
        outs, _, _ = decode(g, cfg, x.to(DEV), T, w_cn=wc[:, torch.as_tensor(g.chk)].contiguous().to(DEV),
                            w_vn=wv.to(DEV))
        r = boosted_forward(og, x, dtype=kind, q=5, nw=(2, 0, 2), iters=list(range(T)), w_cn=lambda t: wc[t],
                            w_ucn=lambda t: None, w_vn=lambda t: wv[t])
        ref = torch.stack([r[t] for t in range(T)]).numpy()
    o = outs.cpu().numpy()
    assert np.array_equal(o, ref), f"{(o != ref).sum()} of {o.size} differ"


def test_tanh_table_vs_this_hosts_torch():
    """The SP check node's torch.tanh values (lib/nldpc_tanh_ref.bin, recorded by gen_tanh_table.py on
    the machine the fixtures were made on; provenance in its header) against THIS machine's
    torch.tanh.  The device and the oracle both use the table, so SP parity with the fixtures holds on
    any host; what this measures is how far this host's own torch.tanh (the one a reference run here
    would call) is from it: MKL's vector tanh takes host-dependent code paths, each within one ulp of
    the correctly rounded tanh.  Asserted: at most one ulp everywhere; the number of differing values
    is reported (NLDPC_SP_LOG), and a host that needs value-for-value parity with ITS torch rebuilds
    the table there (python3 csrc/gen_tanh_table.py <file>; NLDPC_TANH_TABLE=<file>)."""
    from oracle import ldpc_oracle as lo
    tab = lo._tanh_table()
    assert tab is not None, "lib/nldpc_tanh_ref.bin is missing next to libnldpc.so"
    here = f"{torch.__version__}|{torch.backends.cpu.get_cpu_capability()}"
    gen = torch.Generator().manual_seed(12)
    x = torch.cat([(torch.rand(1 << 20, generator=gen) * 20 - 10),
                   torch.from_numpy(tab[0][::37].astype(np.int32)).view(torch.float32)])
    x = torch.cat([x, -x])
    got, want = lo._tanh(x), torch.tanh(x)
    ulps = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs()
    bad = int((ulps != 0).sum())
    msg = (f"{bad} of {x.numel()} tanh values differ (max {int(ulps.max())} ulp): table built on "
           f"'{lo.tanh_table_provenance()}', this host '{here}'")
    log = os.environ.get("NLDPC_SP_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"tanh table vs this host's torch.tanh: {msg}\n")
    assert int(ulps.max()) <= 1, msg


# one lifting size per run-time geometry class (G codewords, P parts, Q copies per lane, threads, padded
# parts, LDS chunks) of the 5G NR BG2 sizes, enumerated by gen_fused.auto_geometry; the built-in sizes
# (384, 96, 24, 16) excluded.  VERDICT r3: Q=2 (352), P=3 (320, 288, 160, 80, 72), G=16 (12), 512 threads (2).
GEOMETRY_CLASSES = [320, 288, 256, 208, 192, 144, 176, 352, 128, 104, 160, 88, 64, 52, 80, 72, 48, 36, 40, 32,
                    26, 18, 22, 13, 12, 9, 8, 6, 5, 2, 4, 3]


def _runtime_case(Z, kind, T=5, B=3):
    """Outputs of the run-time compiled fused kernel and of the CPU oracle for one (Z, kind)."""
    from nldpc.decode import DecodeCfg, decode
    from oracle.ldpc_oracle import OracleGraph, boosted_forward, neural_forward, quantize
    g = _graph(BG2, Z)
    og = OracleGraph(BG2, Z)
    gen = torch.Generator().manual_seed(Z + kind)
    x = (2 * (-1 + 0.85 * torch.randn(B, 52, Z, generator=gen)) / 0.7225).float()
    if kind == 3:
        w = torch.rand(T, g.E, generator=gen) * 1.2
        b = torch.randn(T, g.E, generator=gen) * 0.1
        kw = dict(w_cn=w.to(DEV), bias=b.to(DEV))
        cfg = DecodeCfg(kind, path="fused")
        ref = torch.stack(neural_forward(og, x, list(w), list(b))).numpy()
    else:
        if kind == 2:
            x = quantize(x, 5)
        wc = 0.5 + torch.rand(T, 42, generator=gen)
        wv = 0.8 + 0.4 * torch.rand(T, 52, generator=gen)
        kw = dict(w_cn=wc[:, torch.as_tensor(g.chk)].contiguous().to(DEV), w_vn=wv.to(DEV))
        cfg = DecodeCfg(kind, qbit=5, vn_cumulative=True, path="fused")
        r = boosted_forward(og, x, dtype=kind, q=5, nw=(2, 0, 2), iters=list(range(T)), w_cn=lambda t: wc[t],
                            w_ucn=lambda t: None, w_vn=lambda t: wv[t])
        ref = torch.stack([r[t] for t in range(T)]).numpy()
    outs, _, _ = decode(g, cfg, x.to(DEV), T, **kw)
    return g, cfg, x, kw, outs, ref


@pytest.mark.parametrize("Z", GEOMETRY_CLASSES)
@pytest.mark.parametrize("kind", [3, 2])
def test_runtime_geometry_classes_match_oracle(Z, kind):
    """Every run-time geometry class of the NR lifting sizes (GEOMETRY_CLASSES) on the register-resident
    path, Neural and Boosted QMS (per-check CN, cumulative VN weights), T=5, B=3: bit-exact against the
    CPU oracle -- so an indexing bug of a Q=2, P=3, G>=16 or 512-thread geometry cannot ship silently."""
    g, cfg, x, kw, outs, ref = _runtime_case(Z, kind)
    got = outs.cpu().numpy()
    assert np.array_equal(got, ref.reshape(got.shape)), f"{(got != ref.reshape(got.shape)).sum()} values differ"


@pytest.mark.parametrize("Z", [52, 104, 208])
@pytest.mark.parametrize("kind", [3, 1, 2])
def test_runtime_kernel_lifting_sizes_match_oracle(Z, kind):
    """5G NR BG2 lifting sizes with no built-in kernel (52 = 4 x 13 and 104 = 8 x 13: parts padded to
    whole waves; 208: 4 parts of 256 lanes) on the register-resident path (path="fused" is required):
    the kernel is generated and compiled at run time (nldpc.jit, cached), and its outputs equal the CPU
    oracle's bit for bit (Neural, Boosted MS / QMS with per-check CN and cumulative VN weights).  The
    count-only variant counts what the outputs hold."""
    from nldpc.channel import ber_counts
    from nldpc.decode import decode_count
    g, cfg, x, kw, outs, ref = _runtime_case(Z, kind)
    T = 5
    got = outs.cpu().numpy()
    assert np.array_equal(got, ref.reshape(got.shape)), f"{(got != ref.reshape(got.shape)).sum()} values differ"
    counts = decode_count(g, cfg, x.to(DEV), T, **kw)
    assert torch.equal(counts, ber_counts(list(outs)))


@pytest.mark.parametrize("kind,Z,B", [(2, 104, 4), (3, 52, 5), (1, 52, 5), (2, 15, 3), (3, 15, 3)])
def test_runtime_kernel_training_step_matches_streaming(kind, Z, B):
    """The run-time compiled saving forward (mode 1) and backward (mode 4) against the streaming kernels:
    the same outputs and weight gradients.  Cases: BG2 z=104 QMS (padded parts); z=52 with an
    odd batch (G=2 codewords per workgroup, a partial last workgroup whose missing codeword's lanes read
    never-staged LDS) for Neural (fp32 LDS-staged backward, bias gradients) and MS; z=15 (odd Z: the
    4-byte staging and scalar save paths) for QMS and Neural."""
    from nldpc.decode import DecodeCfg, decode, decode_backward
    from oracle.ldpc_oracle import quantize
    T = 6
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(Z * 10 + kind)
    x = (2 * (-1 + 0.85 * torch.randn(B, 52, Z, generator=gen)) / 0.7225).float()
    if kind == 2:
        x = quantize(x, 5)
    x = x.to(DEV)
    wc = (0.5 + torch.rand(T, g.E, generator=gen)).to(DEV)
    gy = [torch.randn(B, 52 * Z, generator=gen).to(DEV) for _ in range(T)]
    if kind == 3:
        kw = dict(w_cn=wc, bias=(0.2 * torch.randn(T, g.E, generator=gen)).to(DEV))
        gi = (0, 2)
    else:
        kw = dict(w_cn=wc, w_vn=(0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV))
        gi = (0, 3)
    res = {}
    for path in ("stream", "fused"):
        cfg = DecodeCfg(kind, qbit=5, vn_cumulative=kind != 3, path=path)
        outs, _, saved = decode(g, cfg, x, T, save=True, **kw)
        grads = decode_backward(g, cfg, x, T, gy, list(outs), saved, **kw)
        res[path] = (outs, grads[gi[0]], grads[gi[1]])
    assert torch.equal(res["stream"][0], res["fused"][0])
    for k in (1, 2):
        a, b = res["stream"][k].cpu().numpy(), res["fused"][k].cpu().numpy()
        np.testing.assert_allclose(b, a, rtol=1e-5, atol=1e-5 * np.abs(a).max())


@pytest.mark.parametrize("kind", [1, 2])
def test_tied_cn_backward_row_sums_match_untied(kind):
    """NLDPC_FLAG_CN_TIED (sharing code 3: one CN weight per iteration, expanded to [T][E]): the fused
    backward's tied kernel reduces each row copy once and spreads the iteration's total over a few entries;
    every iteration's row sum must equal the untied kernel's (per-edge gradients summed), and the other
    weight gradient (VN) must be the same (BG2 z=16, built in; z=384 through the cfg5 module test)."""
    from nldpc.decode import DecodeCfg, decode, decode_backward
    from oracle.ldpc_oracle import quantize
    T, B, Z = 5, 3, 16
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(30 + kind)
    x = (2 * (-1 + 0.85 * torch.randn(B, 52, Z, generator=gen)) / 0.7225).float()
    if kind == 2:
        x = quantize(x, 5)
    x = x.to(DEV)
    # (the tied flag is honoured for a stride-0 expand only, as the drop-in module passes code 3: decode._honour_tied)
    wc1 = (0.5 + torch.rand(T, 1, generator=gen)).to(DEV)
    wv = (0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV)
    gy = [torch.randn(B, 52 * Z, generator=gen).to(DEV) for _ in range(T)]
    res = {}
    for tied in (False, True):
        wc = wc1.expand(T, g.E) if tied else wc1.expand(T, g.E).contiguous()
        cfg = DecodeCfg(kind, qbit=5, vn_cumulative=True, path="fused", cn_tied=tied)
        outs, _, saved = decode(g, cfg, x, T, save=True, w_cn=wc, w_vn=wv)
        g_cn, _, _, g_vn, _ = decode_backward(g, cfg, x, T, gy, list(outs), saved, w_cn=wc, w_vn=wv)
        res[tied] = (outs, g_cn.double().sum(1), g_vn)
    assert torch.equal(res[False][0], res[True][0])
    a, b = res[False][1].cpu().numpy(), res[True][1].cpu().numpy()
    np.testing.assert_allclose(b, a, rtol=1e-5, atol=1e-6 * np.abs(a).max())
    assert torch.equal(res[False][2], res[True][2])


@pytest.mark.parametrize("kind", [1, 2])
def test_tied_flag_on_per_edge_weights_gives_the_untied_gradient(kind):
    """cn_tied=True with a per-edge (contiguous, non-uniform) w_cn must not reach the tied kernel (which
    computes a row's masks from its first weight): decode_autograd and decode_backward both fall back to the per-edge
    gradient, bit-identical to cn_tied=False."""
    from nldpc.decode import DecodeCfg, decode, decode_autograd, decode_backward
    from oracle.ldpc_oracle import quantize
    T, B, Z = 4, 3, 16
    g = _graph(BG2, Z)
    gen = torch.Generator().manual_seed(40 + kind)
    x = (2 * (-1 + 0.85 * torch.randn(B, 52, Z, generator=gen)) / 0.7225).float()
    if kind == 2:
        x = quantize(x, 5)
    x = x.to(DEV)
    wc = (0.5 + torch.rand(T, g.E, generator=gen)).to(DEV)  # per-edge: rows are NOT one value
    wv = (0.8 + 0.4 * torch.rand(T, 52, generator=gen)).to(DEV)
    gy = [torch.randn(B, 52 * Z, generator=gen).to(DEV) for _ in range(T)]
    res = {}
    for tied in (False, True):
        cfg = DecodeCfg(kind, qbit=5, vn_cumulative=True, path="fused", cn_tied=tied)
        outs, _, saved = decode(g, cfg, x, T, save=True, w_cn=wc, w_vn=wv)
        g_cn, _, _, g_vn, _ = decode_backward(g, cfg, x, T, gy, list(outs), saved, w_cn=wc, w_vn=wv)
        a = wc.clone().requires_grad_(True)
        v = wv.clone().requires_grad_(True)
        ys, _ = decode_autograd(g, cfg, x, T, w_cn=a, w_vn=v)
        torch.autograd.backward(ys, gy)
        res[tied] = (g_cn, g_vn, a.grad, v.grad)
    for u, t in zip(res[False], res[True]):
        assert torch.equal(u, t)
    assert torch.equal(res[True][0], res[True][2])


@pytest.mark.parametrize("q", [0, 2])
def test_qms_inactive_quantiser_runs_on_streaming_path(q):
    """QMS with a qbit the reference's quantiser does not know (Boosted…py:187-214: the message passes
    unquantised) has no fused kernel (the fused QMS kernels carry only the active quantiser's check
    node): nldpc_fast_path reports 0, path="fused" is refused, and the default path
    decodes on the streaming kernels, bit-exact against the CPU oracle."""
    import ctypes
    from nldpc import _lib
    from nldpc.decode import DecodeCfg, decode
    from oracle.ldpc_oracle import OracleGraph, boosted_forward
    L = _lib.lib()
    T, B, Z = 5, 3, 16
    g = _graph(BG2, Z)
    for save in (0, 1):
        cfg = DecodeCfg(2, qbit=q).c_struct(False)
        out = ctypes.c_int32(-1)
        _lib.check(L.nldpc_fast_path(g.handle(DEV), ctypes.byref(cfg), B, T, save, ctypes.byref(out)))
        assert out.value == 0, (q, save)
    gen = torch.Generator().manual_seed(40 + q)
    x = (2 * (-1 + 0.9 * torch.randn(B, 52, Z, generator=gen)) / 0.81).float()
    w_cn = (0.75 + 0.5 * torch.rand(T, g.E, generator=gen))
    with pytest.raises(_lib.NldpcError):
        decode(g, DecodeCfg(2, qbit=q, path="fused"), x.to(DEV), T, w_cn=w_cn.to(DEV))
    outs, _, _ = decode(g, DecodeCfg(2, qbit=q), x.to(DEV), T, w_cn=w_cn.to(DEV))
    ref = boosted_forward(OracleGraph(BG2, Z), x, dtype=2, q=q, nw=(1, 0, 0), iters=list(range(T)),
                          w_cn=lambda t: w_cn[t], w_ucn=lambda t: None, w_vn=lambda t: None)
    for t in range(T):
        assert torch.equal(outs[t].cpu(), ref[t]), f"iteration {t}"


def test_attach_refuses_a_code_object_of_another_argument_layout(tmp_path):
    """a kernel built against another FusedArgs layout used to return at once and leave its outputs
    unwritten with NLDPC_OK.  Run-time code objects carry the layout they were built for (nldpc_sig) and
    nldpc_graph_attach_kernel refuses a mismatch with NLDPC_EUNSUPPORTED; the library's own kernels are checked
    the same way in fused_launch (FusedSpec::sig)."""
    import ctypes
    import subprocess
    from nldpc import _lib, jit
    gen = jit._generator()
    src, geo = gen.jit_source(BG2, 52, 3, 0)
    assert "nldpc_sig = nldpc::kFusedArgsSig" in src
    bad = src.replace("nldpc_sig = nldpc::kFusedArgsSig", "nldpc_sig = 0x12345678u")
    s, co = str(tmp_path / "k.hip"), str(tmp_path / "k.co")
    open(s, "w").write(bad)
    subprocess.run([jit.HIPCC, *jit.FLAGS, "-O1", s, "-o", co], check=True, capture_output=True)
    data = open(co, "rb").read()
    g = _graph(BG2, 52)
    h = g.handle(DEV)
    st = _lib.lib().nldpc_graph_attach_kernel(h, 0, 3, ctypes.create_string_buffer(data, len(data)), len(data),
                                               geo["G"], geo["threads"], geo["waves_per_part"])
    assert st == _lib.NLDPC_EUNSUPPORTED
    assert "argument layout" in _lib.lib().nldpc_last_error().decode()
