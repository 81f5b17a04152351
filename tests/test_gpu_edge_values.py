"""Forward decode on special values (tests/edge_inputs.py) against the CPU oracle, at the headline size.

The batch holds an erased codeword, punctured columns, an integer grid (ties and exact zeros), values on
the +-20 clamp, values far beyond it and -0.0; the CN weights hold exact zeros and negatives, the Neural
biases kill messages (tests/test_edge_inputs.py asserts on the CPU that the oracle reaches every case).
The oracle reproduces the reference bit for bit on this batch (the *_edges fixtures of
tests/test_oracle_golden.py).  Neural / MS / QMS: bit-exact; SP: sp_check of test_gpu_forward.py.

Sizes: BG2 z=384 B=6, BG2 z=16 B=19 (16 codewords per workgroup: one full workgroup and a partial one),
WiMAX z=24 B=7 (MS, Neural); streaming and register-resident ("fused") kernels; the UCN kernel with
cumulative VN weights at z=384; the count-only and early-stop instantiations of the same check node.
A failure reports how many values differ per codeword, so the failing property names itself.
"""
import functools
import os

import numpy as np
import pytest
import torch

import edge_inputs as ei
from conftest import ROOT
from test_early_stop_gen import unsat_numpy

pytestmark = pytest.mark.gpu

GRAPHS = {"bg2": np.loadtxt(os.path.join(ROOT, "resources", "basegraph2_set0.txt"), int, delimiter="\t"),
          "wimax": np.loadtxt(os.path.join(ROOT, "resources", "wman_N0576_R34_z24.txt"), int, delimiter="\t")}
DEV = torch.device("cuda")
T = 4
SIZES = {("bg2", 384): 6, ("bg2", 16): 19, ("wimax", 24): 7}  # (graph, Z) -> B
SP, MS, QMS, NEURAL = 0, 1, 2, 3

# (graph, Z, kind, qbit): every kind at the two BG2 sizes, every quantiser at z=16, MS and Neural on WiMAX
FORWARD = ([("bg2", Z, k, 5) for Z in (384, 16) for k in (NEURAL, MS, QMS, SP)]
           + [("bg2", 16, QMS, q) for q in (6, -5, 4, 3)] + [("bg2", 384, QMS, 3)]
           + [("wimax", 24, k, 5) for k in (NEURAL, MS)])


@functools.lru_cache(maxsize=None)
def _graph(bg, Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(GRAPHS[bg], Z)


@functools.lru_cache(maxsize=None)
def _case(bg, Z, kind, q, ucn=False):
    """(x [B, N, Z], weight dict (CPU), oracle outputs [T, B, N*Z] numpy) -- computed once, never modified."""
    from oracle.ldpc_oracle import OracleGraph, boosted_forward, neural_forward, quantize
    og = OracleGraph(GRAPHS[bg], Z)
    x = ei.edge_batch(SIZES[bg, Z], og.N, Z)
    if kind == NEURAL:
        w, b = ei.edge_neural_params(T, og.E)
        ref = neural_forward(og, x, list(w), list(b))
        return x, dict(w_cn=w, bias=b), torch.stack(ref).numpy()
    if kind == QMS:
        x = quantize(x, q)
    kw = dict(w_cn=ei.edge_cn_weights(T, og.E), w_vn=ei.edge_vn_weights(T, og.N))
    if ucn:
        kw["w_ucn"] = ei.edge_cn_weights(T, og.E, ei.SEED + 1)
    r = boosted_forward(og, x, dtype=kind, q=q, nw=(1, 1 if ucn else 0, 2), iters=list(range(T)),
                        w_cn=lambda t: kw["w_cn"][t], w_ucn=lambda t: kw["w_ucn"][t] if ucn else None,
                        w_vn=lambda t: kw["w_vn"][t])
    return x, kw, torch.stack([r[t] for t in range(T)]).numpy()


def _cfg(kind, q, path, ucn=False, **extra):
    from nldpc.decode import DecodeCfg
    return DecodeCfg(kind=kind, qbit=q, ucn=ucn, vn_cumulative=kind != NEURAL, path=path, **extra)


def _dev(kw):
    return {k: v.to(DEV) for k, v in kw.items()}


def _assert_outputs(o, ref, kind):
    o = np.asarray(o)
    if kind == SP:
        from test_gpu_forward import sp_check
        try:
            sp_check(o, ref)
        except AssertionError as e:
            raise AssertionError(f"{e}\nnot identical per codeword: {ei.per_codeword_diff(o, ref)}") from None
        return
    assert np.array_equal(o, ref), (f"{(o != ref).sum()} of {o.size} soft values differ; per codeword: "
                                    f"{ei.per_codeword_diff(o, ref)}")


@pytest.mark.parametrize("path", ["stream", "fused"])
@pytest.mark.parametrize("bg,Z,kind,q", FORWARD)
def test_forward_special_values_match_oracle(bg, Z, kind, q, path):
    from nldpc.decode import decode
    x, kw, ref = _case(bg, Z, kind, q)
    outs, _, _ = decode(_graph(bg, Z), _cfg(kind, q, path), x.to(DEV), T, **_dev(kw))
    _assert_outputs(outs.cpu().numpy(), ref, kind)


@pytest.mark.parametrize("path", ["stream", "fused"])
@pytest.mark.parametrize("kind,q", [(MS, 5), (QMS, 5), (QMS, 6)])
def test_ucn_forward_special_values_match_oracle(kind, q, path):
    """CN / UCN / cumulative VN weights at BG2 z=384: the kernel specialised for UCN (path="fused") and the
    streaming kernels.  UCN reads the hard decision of the previous posterior, here also of exact zeros."""
    from nldpc.decode import decode
    x, kw, ref = _case("bg2", 384, kind, q, True)
    outs, _, _ = decode(_graph("bg2", 384), _cfg(kind, q, path, ucn=True), x.to(DEV), T, **_dev(kw))
    _assert_outputs(outs.cpu().numpy(), ref, kind)


@pytest.mark.parametrize("bg,Z,kind,q", [c for c in FORWARD if c[0] == "bg2" and c[3] == 5])
def test_count_only_special_values(bg, Z, kind, q):
    """nldpc_forward_count (a separate instantiation of the check node) counts what the oracle's outputs
    hold: against the all-zero codeword and against a given y, in both decision conventions."""
    from nldpc.decode import decode_count
    x, kw, ref = _case(bg, Z, kind, q)
    B = x.shape[0]
    g = _graph(bg, Z)
    y = torch.from_numpy(np.random.default_rng(Z).integers(0, 2, (B, g.N * Z)).astype(np.uint8))
    for yy in (None, y):
        for conv in (0, 1):
            bits = (ref > 0) if conv == 0 else (ref < 0)
            err = bits != (np.zeros_like(bits) if yy is None else yy.numpy().astype(bool)[None])
            want = np.stack([err.sum(axis=(1, 2)), err.any(axis=2).sum(axis=1)], 1)
            got = decode_count(g, _cfg(kind, q, "fused", keep_state=False), x.to(DEV), T,
                               y=None if yy is None else yy.to(DEV), convention=conv, **_dev(kw))
            assert np.array_equal(got.cpu().numpy(), want), (yy is None, conv, got.cpu().tolist(), want.tolist())


@pytest.mark.parametrize("bg,Z,kind,q", [c for c in FORWARD if c[0] == "bg2" and c[3] == 5])
def test_early_stop_special_values(bg, Z, kind, q):
    """nldpc_forward_early_stop returns, per codeword, the oracle's posterior of the first iteration whose
    hard decision satisfies every check (the last one if none does), that iteration and its syndrome weight.
    The erased codeword decides all-zero at once; others of the batch never converge."""
    from nldpc.decode import decode_early_stop
    x, kw, ref = _case(bg, Z, kind, q)
    B = x.shape[0]
    unsat = np.stack([unsat_numpy((ref[t] > 0).astype(np.int64), GRAPHS[bg], Z) for t in range(T)])
    ok = unsat == 0
    tstar = np.where(ok.any(0), ok.argmax(0), T - 1)
    assert tstar[0] == 0 and len(set(tstar.tolist())) > 1
    out, iters, un = decode_early_stop(_graph(bg, Z), _cfg(kind, q, "fused", keep_state=False), x.to(DEV), T, **_dev(kw))
    assert np.array_equal(iters.cpu().numpy(), tstar + 1), (iters.cpu().tolist(), (tstar + 1).tolist())
    assert np.array_equal(un.cpu().numpy(), unsat[tstar, np.arange(B)])
    _assert_outputs(out.cpu().numpy()[None], ref[tstar, np.arange(B)][None], kind)
