"""The flat block-fading QAM channel with perfect CSI (nldpc_fading_gains / nldpc_qam_demap_csi /
nldpc_qam_fading_channel_llr, nldpc.fading) on the GPU.  Expected values come from fading_model.py (the gain formula on
oracle.philox's words, the faded noisy symbols, the fp32 max-log and the fp64 log-MAP with qam_model's derived bound on
the scaled levels), never from the library.

Shapes (qm, S, B, b_offset, L), the smallest that reach every path: one symbol -- half a Philox pair; odd S with an odd
offset and L = 3 -- pairs straddle rows and blocks, the stream starts mid-pair, the last block of a row is short; the
same with L = S -- one gain per row; S = 1 -- every row is half a pair and, with qm = 6, the element path; the largest
order with L = 64; the row length of the headline graph at rate 1/2 with fast fading.  The Rician factor differs by
order (K = 0 is Rayleigh).
"""
import functools
import os

import numpy as np
import pytest
import torch

import fading_model as fm
import qam_model as qm_
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = [(2, 1, 1, 0, 1), (4, 67, 5, 3, 3), (4, 67, 5, 3, 67), (6, 1, 131, 1, 1), (8, 250, 3, 0, 64), (6, 1280, 3, 0, 1)]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}
RICE = {2: 0.0, 4: 0.0, 6: 1.0, 8: 4.0}
SEED = 4242
METHODS = ["maxlog", "logmap"]
C_INITS = [0x12345, 0x7FFFFFFF, 0x0BADC0DE & 0x7FFFFFFF]
shapes = pytest.mark.parametrize("qm,S,B,off,L", SHAPES)


@functools.lru_cache(maxsize=None)
def _case(qm, S, B, off, L):
    """the shared, read-only reference of one shape"""
    rng = np.random.default_rng(qm * 1000 + S + B)
    f = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, S * qm))
    c = dict(f=f, sigma=float(np.float32(SIGMA[qm])), K=RICE[qm], gains=fm.gains(B, S, L, RICE[qm], SEED, off))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the references are read-only)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


def _run(c, qm, off, L, **kw):
    from nldpc.fading import qam_llr
    kw.setdefault("K", c["K"])
    return qam_llr(kw.pop("f", None) if "f" in kw else _dev(c["f"]), qm, c["sigma"], L=L, seed=SEED, b_offset=off, **kw)


@shapes
def test_gains_equal_the_model_and_shard(qm, S, B, off, L):
    from nldpc.fading import gains, n_blocks
    c = _case(qm, S, B, off, L)
    nb = n_blocks(S, L)
    assert nb == fm.n_blocks(S, L)
    got = gains(B, S, L=L, K=c["K"], seed=SEED, b_offset=off, device=DEV)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, nb)
    g, want = got.cpu().numpy(), c["gains"]
    differ = float((g != want).mean())
    print(f"qm={qm} S={S} B={B} L={L} K={c['K']}: {differ:.2e} of {g.size} gains differ from the model's")
    assert np.isfinite(g).all() and (g >= 0).all()
    assert (np.abs(g.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()
    assert differ < 1e-4
    for k in (1, 2):  # both parities of the first block pair
        if k < B:
            assert _same(gains(B - k, S, L=L, K=c["K"], seed=SEED, b_offset=off + k, device=DEV), got[k:])
    assert not _same(gains(B, S, L=L, K=c["K"], seed=SEED + 1, b_offset=off, device=DEV), got) or got.numel() < 2
    buf, view = _guarded((B, nb), torch.float32, 777.25, 3)
    assert gains(B, S, L=L, K=c["K"], seed=SEED, b_offset=off, out=view).data_ptr() == view.data_ptr()
    assert _same(view, got) and _guards_intact(buf, view, 777.25, 3)


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_fused_channel_equals_demap_of_its_symbols_and_gains(qm, S, B, off, L, method):
    from nldpc.fading import demap, gains
    c = _case(qm, S, B, off, L)
    llr, sym, g = _run(c, qm, off, L, method=method, return_symbols=True, return_gains=True)
    assert llr.dtype == sym.dtype == g.dtype == torch.float32
    assert tuple(llr.shape) == (B, S * qm) and tuple(sym.shape) == (B, S, 2) and tuple(g.shape) == c["gains"].shape
    unfused = demap(sym, qm, c["sigma"], g, L=L, method=method)
    assert _same(llr, unfused)
    assert _same(g, gains(B, S, L=L, K=c["K"], seed=SEED, b_offset=off, device=DEV))
    # the model on the device's own symbols and gains
    s_np, g_np = sym.cpu().numpy(), g.cpu().numpy()
    per_symbol = fm.symbol_gains(g_np, S, L)
    if method == "maxlog":
        assert _bits_equal(unfused.cpu().numpy(), fm.maxlog_csi(s_np, qm, c["sigma"], per_symbol))
    else:
        want, dmax = fm.logmap64_csi(s_np, qm, c["sigma"], per_symbol)
        bound = qm_.logmap_bound(qm, want, dmax)
        err = np.abs(unfused.cpu().numpy().astype(np.float64) - want)
        print(f"qm={qm} S={S} B={B} L={L}: max err / bound = {(err / bound).max():.3f}, max |d*w| = {dmax.max():.4g}")
        assert (err <= bound).all()
    model = fm.faded_symbols(c["f"], qm, c["sigma"], g_np, L, SEED, off)
    miss = float((s_np != model).mean())
    print(f"qm={qm} S={S} B={B} L={L} {method}: {miss:.2e} of the faded symbols differ from the model's")
    assert miss < 1e-4
    assert np.abs(s_np - model).max() <= 4 * np.spacing(np.abs(model).max())
    alone = _run(c, qm, off, L, method=method)
    assert isinstance(alone, torch.Tensor) and _same(alone, llr)
    two = _run(c, qm, off, L, method=method, return_gains=True)
    assert len(two) == 2 and _same(two[0], llr) and _same(two[1], g)


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_unit_gains_reproduce_the_awgn_channel(qm, S, B, off, L, method):
    from nldpc import modulation
    from nldpc.fading import n_blocks
    from nldpc.scrambling import sequence
    c = _case(qm, S, B, off, L)
    f = _dev(c["f"])
    ones = torch.ones((B, n_blocks(S, L)), device=DEV)
    seq = sequence(C_INITS, S * qm, device=DEV)
    for table in (None, seq):
        want, ws = modulation.qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, method=method, return_symbols=True,
                                      scramble=table)
        got, gs, gg = _run(c, qm, off, L, method=method, gain=ones, scramble=table, return_symbols=True,
                           return_gains=True)
        assert _same(got, want) and _same(gs, ws) and _same(gg, ones)


@shapes
def test_given_gains_equal_to_the_drawn_table_reproduce_the_drawn_run(qm, S, B, off, L):
    c = _case(qm, S, B, off, L)
    llr, sym, g = _run(c, qm, off, L, method="logmap", return_symbols=True, return_gains=True)
    l2, s2, g2 = _run(c, qm, off, L, method="logmap", gain=g.clone(), K=0.0, return_symbols=True, return_gains=True)
    assert _same(l2, llr) and _same(s2, sym) and _same(g2, g)


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_scrambling_in_flight_equals_the_three_steps(qm, S, B, off, L, method):
    from nldpc.scrambling import descramble, scramble, sequence
    c = _case(qm, S, B, off, L)
    f = _dev(c["f"])
    for n_seq in (1, 3):
        seq = sequence(C_INITS[:n_seq], S * qm, device=DEV)
        got, gs = _run(c, qm, off, L, method=method, scramble=seq, return_symbols=True)
        mid, ms = _run(c, qm, off, L, f=scramble(f, seq, b_offset=off), method=method, return_symbols=True)
        assert _same(got, descramble(mid, seq, b_offset=off)) and _same(gs, ms)
    plain = _run(c, qm, off, L, method=method)
    assert not _same(plain, got) or plain.numel() < 8


@shapes
def test_a_shard_equals_the_rows_of_the_unsharded_batch(qm, S, B, off, L):
    c = _case(qm, S, B, off, L)
    f = _dev(c["f"])
    llr, sym, g = _run(c, qm, off, L, return_symbols=True, return_gains=True)
    for k in (1, 2):  # both parities of the first pair (B = 1 has no rows to split off)
        if k >= B:
            continue
        l2, s2, g2 = _run(c, qm, off + k, L, f=f[k:].contiguous(), return_symbols=True, return_gains=True)
        assert _same(l2, llr[k:]) and _same(s2, sym[k:]) and _same(g2, g[k:])


@shapes
def test_all_zero_word(qm, S, B, off, L):
    c = _case(qm, S, B, off, L)
    zeros = torch.zeros((B, S * qm), dtype=torch.uint8, device=DEV)
    a = _run(c, qm, off, L, f=None, B=B, E=S * qm, device=DEV, return_symbols=True, return_gains=True)
    b = _run(c, qm, off, L, f=zeros, return_symbols=True, return_gains=True)
    assert all(_same(x, y) for x, y in zip(a, b))
    other = _run(c, qm, off, L, f=zeros, return_symbols=True)
    assert _same(other[0], b[0])
    assert not _same(_run(c, qm, off, L, f=zeros, return_gains=True)[1],
                     _run(c, qm, off, L, f=zeros, K=c["K"] + 1.0, return_gains=True)[1])


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_a_row_of_zero_gain_has_zero_llrs(qm, S, B, off, L, method):
    from nldpc.fading import n_blocks
    c = _case(qm, S, B, off, L)
    table = torch.ones((B, n_blocks(S, L)), device=DEV)
    row = B // 2
    table[row] = 0.0
    llr = _run(c, qm, off, L, method=method, gain=table)
    assert bool(((llr[row].view(torch.int32) & 0x7FFFFFFF) == 0).all())
    if B > 1:
        assert bool((llr[row - 1] != 0).any())


@shapes
def test_nothing_outside_the_outputs_is_written(qm, S, B, off, L):
    from nldpc.fading import demap, n_blocks
    c = _case(qm, S, B, off, L)
    E, nb, sentinel = S * qm, n_blocks(S, L), 777.25
    ref = _run(c, qm, off, L, return_symbols=True, return_gains=True)
    given = ref[2] * 0.5 + 0.25
    refg = _run(c, qm, off, L, gain=given, return_symbols=True, return_gains=True)
    shift = 3
    fbuf = torch.full((B * E + 8,), 0x55, dtype=torch.uint8, device=DEV)
    f = fbuf[1:1 + B * E].view(B, E)  # (the bits start off a dword boundary)
    f.copy_(_dev(c["f"]))
    for gain, want in ((None, ref), (given, refg)):
        gin_buf = None
        if gain is not None:
            gin_buf, gin = _guarded((B, nb), torch.float32, sentinel, shift)
            gin.copy_(gain)
            gain = gin
        lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
        sbuf, sym = _guarded((B, S, 2), torch.float32, sentinel, shift)
        gbuf, g = _guarded((B, nb), torch.float32, sentinel, shift)
        got = _run(c, qm, off, L, f=f, gain=gain, out=llr, return_symbols=sym, return_gains=g)
        assert [t.data_ptr() for t in got] == [llr.data_ptr(), sym.data_ptr(), g.data_ptr()]
        assert _guards_intact(lbuf, llr, sentinel, shift) and _guards_intact(sbuf, sym, sentinel, shift)
        assert _guards_intact(gbuf, g, sentinel, shift)
        assert gin_buf is None or (_guards_intact(gin_buf, gain, sentinel, shift) and _same(gain, given))
        assert bool((fbuf[:1] == 0x55).all()) and bool((fbuf[1 + B * E:] == 0x55).all())
        # the shifted run computes what the unshifted one does, and every element was written
        assert all(_same(x, y) for x, y in zip(got, want))
        # the unfused demapper, shifted the same way
        lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
        assert demap(sym, qm, c["sigma"], g, L=L, out=llr).data_ptr() == llr.data_ptr()
        assert _same(llr, want[0]) and _guards_intact(lbuf, llr, sentinel, shift)
        assert _guards_intact(sbuf, sym, sentinel, shift) and _guards_intact(gbuf, g, sentinel, shift)


def test_bad_arguments_raise_value_error():
    from nldpc.fading import demap, gains, qam_llr
    B, E, qm, L = 2, 24, 4, 2
    S, nb = E // qm, 3
    f = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    sym = torch.zeros((B, S, 2), device=DEV)
    table = torch.ones((B, nb), device=DEV)
    assert qam_llr(f, qm, 0.5, L=L, gain=table).shape == (B, E) and demap(sym, qm, 0.5, table, L=L).shape == (B, E)
    for bad_L in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, L=bad_L)
        with pytest.raises(ValueError):
            gains(B, S, L=bad_L, device=DEV)
        with pytest.raises(ValueError):
            demap(sym, qm, 0.5, table, L=bad_L)
    for bad_K in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, K=bad_K)
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, L=L, K=bad_K, gain=table)
        with pytest.raises(ValueError):
            gains(B, S, K=bad_K, device=DEV)
    wide = torch.ones((B, 2 * nb), device=DEV)
    for bad in (torch.ones((B, nb + 1), device=DEV), torch.ones((B + 1, nb), device=DEV), torch.ones((B * nb,), device=DEV),
                table.double(), table.cpu(), wide[:, ::2], torch.ones((nb, B), device=DEV).t(), [[1.0] * nb] * B):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, L=L, gain=bad)
        with pytest.raises(ValueError):
            demap(sym, qm, 0.5, bad, L=L)
        if isinstance(bad, torch.Tensor):
            with pytest.raises(ValueError):
                qam_llr(f, qm, 0.5, L=L, return_gains=bad)
            with pytest.raises(ValueError):
                gains(B, S, L=L, out=bad)
    with pytest.raises(ValueError):
        qam_llr(f, qm, 0.5, L=L, gain=table, return_gains=table)
    for bad_qm in (1, 3, 10):
        with pytest.raises(ValueError):
            qam_llr(f, bad_qm, 0.5)
        with pytest.raises(ValueError):
            demap(sym, bad_qm, 0.5, table, L=L)
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            qam_llr(f, qm, sigma)
        with pytest.raises(ValueError):
            demap(sym, qm, sigma, table, L=L)
    for bad in (f.cpu(), f.float(), f.reshape(-1), f[:, :-2]):
        with pytest.raises(ValueError):
            qam_llr(bad, qm, 0.5)
    for bad in (sym.cpu(), sym.double(), sym.reshape(B, -1), sym[:, :, :1]):
        with pytest.raises(ValueError):
            demap(bad, qm, 0.5, table, L=L)
    for kw in (dict(method="exact"), dict(b_offset=-1), dict(out=torch.empty((B, E + 1), device=DEV)),
               dict(return_symbols=torch.empty((B, S, 3), device=DEV)), dict(scramble=torch.zeros((1, 2), dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, **kw)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, B=2, E=10)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, B=2, E=8, device="cpu")
    with pytest.raises(ValueError):
        gains(0, S, device=DEV)
    with pytest.raises(ValueError):
        gains(B, S, b_offset=-1, device=DEV)
    # the library's own answer surfaces as ValueError too
    from nldpc import _lib
    assert _lib.lib().nldpc_qam_fading_channel_llr(4, 0, f.data_ptr(), B, E, 0.5, 1, 0, 0, 0.0, None, None, 0,
                                                   sym.data_ptr(), None, None, None) == _lib.NLDPC_EINVAL
    with pytest.raises(ValueError):
        _lib.check(_lib.NLDPC_EINVAL, "nldpc_qam_fading_channel_llr")


# ---------------------------------------------------------------- end to end: encode -> match -> 16-QAM over Rayleigh -> recover -> decode
RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
EBN0_DB = 10.0


def test_rate_half_16qam_rayleigh_end_to_end_decodes():
    """BG2 z=16, rate 1/2 (E = 272, 24 fillers, rv0), 16-QAM log-MAP over Rayleigh fading with L = 1 and perfect CSI,
    Neural T=10, weights 0.75, bias 0, erasures 1e-3, 8 encoded words: test_rate_half_16qam_end_to_end_decodes of
    test_gpu_modulation.py with the fading channel in place of AWGN.  Eb/N0 = 10.0 dB (sigma = sigma_for(10, 1/2, 4)):
    the lowest of a 0.5 dB grid (8.0 .. 26.0 dB, every point from 10.0 dB on qualifies) at which the CPU chain
    (fading_model's gains, channel and fp64 log-MAP rounded to fp32, ratematch_model's recovery, the oracle decoder)
    has no frame error from iteration 6 on for seeds 77, 78 and 79.  CPU frame errors per iteration, interleaver qm = 4:
       9.5 dB  77: [8, 8, 8, 5, 3, 2, 1, 1, 0, 0]  78: [8, 8, 8, 5, 1, 1, 1, 0, 0, 0]  79: [8, 8, 8, 6, 5, 2, 0, 0, 0, 0]
      10.0 dB  77: [8, 8, 7, 5, 2, 1, 0, 0, 0, 0]  78: [8, 8, 8, 3, 1, 1, 0, 0, 0, 0]  79: [8, 8, 8, 5, 2, 1, 0, 0, 0, 0]
      10.5 dB  77: [8, 8, 7, 4, 1, 1, 0, 0, 0, 0]  78: [8, 8, 8, 3, 1, 0, 0, 0, 0, 0]  79: [8, 8, 8, 5, 1, 0, 0, 0, 0, 0]
    and with RateMatch(qm=1) in front of the same 16-QAM (for comparison only; its lowest such point is 11.0 dB):
      10.0 dB  77: [8, 8, 8, 4, 2, 2, 0, 0, 0, 0]  78: [8, 8, 8, 5, 2, 2, 0, 0, 0, 0]  79: [8, 8, 8, 6, 2, 2, 2, 0, 0, 0]
    AWGN needs 6.5 dB in the same setting.  The device runs seed 77 with the qm = 4 interleaver."""
    from nldpc.channel import ber_counts, encode, syndrome_weight
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    from nldpc.fading import qam_llr
    from nldpc.graph import LiftedGraph
    from nldpc.modulation import sigma_for
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    g = LiftedGraph(BG2, 16)
    info = np.random.default_rng(5).integers(0, 2, (8, 160))
    info[:, -24:] = 0
    y = encode(g, torch.from_numpy(info).to(DEV))
    rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=4)
    R = code_rate(g, rm)
    assert R == 136 / 272
    sigma = float(np.float32(sigma_for(EBN0_DB, R, 4)))
    llr = qam_llr(rate_match(g, rm, y), 4, sigma, L=1, K=0.0, seed=77, method="logmap")
    xa = rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0)
    T = 10
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    outs = list(outs)
    counts = ber_counts(outs, y).cpu().numpy()
    unsat = syndrome_weight(outs, g).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist(), "unsatisfied checks:", unsat.sum(1).tolist())
    assert not counts[6:, 0].any()
    assert not unsat[6:].any()
