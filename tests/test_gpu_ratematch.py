"""Circular-buffer rate matching and rate recovery (nldpc_rate_match / nldpc_rate_recover, nldpc.ratematch) on the GPU.

Expected values come from the sequential models of ratematch_model.py (the loop of TS 38.212 §5.4.2; fp32 sums in
ascending selection order), never from the library's closed-form maps.

Shapes: the encoder tests' smallest-that-can-go-wrong set -- many codewords per workgroup with an odd remainder (z=2), an
odd lifting size below a wave (z=13), z=16 with odd B, the headline graph (z=384), and WiMAX z=24 without punctured
columns.  Parameter sets per shape: (a) high rate, odd E below Nv; (b) repetition E = 2*Nv + 6*5 (2*Nv rounded up to a
multiple of 6 where it is none: qm = 6 must divide E) with the interleaver, Z + 1 fillers and the start of rv2; (c) a
limited buffer (full - 5) turned one and a half times, with k0 inside the filler range and qm = 2.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from ratematch_model import model_index, model_recover

pytestmark = pytest.mark.gpu

RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
WIMAX = np.loadtxt(os.path.join(RES, "wman_N0576_R34_z24.txt"), int, delimiter="\t")
GRAPHS = {"bg2": BG2, "wimax": WIMAX}
DEV = torch.device("cuda")

SHAPES = [("bg2", 2, 130), ("bg2", 13, 5), ("bg2", 16, 37), ("bg2", 384, 3), ("wimax", 24, 29)]
SETS = ["a", "b", "c"]
ERASURE, FILLER = 0.001, -20.0


@functools.lru_cache(maxsize=None)
def _graph(name, Z):
    from nldpc.graph import LiftedGraph
    return LiftedGraph(GRAPHS[name], Z)


@functools.lru_cache(maxsize=None)
def _params(name, Z, which):
    """keyword arguments of RateMatch / model_index for one (shape, set)"""
    hb = GRAPHS[name]
    M, N = hb.shape
    K, pc = N - M, 2 if name == "bg2" else 0
    P, full = pc * Z, N * Z - pc * Z
    if which == "a":
        E = (full // 2) | 1  # odd, below Nv = full
        return dict(E=E, k0=0, punct_cols=pc, n_filler=0, ncb=0, qm=1)
    if which == "b":
        F = Z + 1
        k0 = 25 * full // (50 * Z) * Z if name == "bg2" else full // 2  # rv2 of Table 5.4.2.1-2
        # 2 * Nv + 6 * 5, with 2 * Nv rounded up to a multiple of qm where it is none (qm must divide E)
        return dict(E=-(-2 * (full - F) // 6) * 6 + 6 * 5, k0=k0, punct_cols=pc, n_filler=F, ncb=0, qm=6)
    F = Z + 1
    f0, Nv = K * Z - F - P, full - 5 - F
    # one and a half turns of the limited buffer: the wrap at Ncb is crossed
    return dict(E=(3 * Nv // 2) & ~1, k0=f0 + F // 2, punct_cols=pc, n_filler=F, ncb=full - 5, qm=2)


@functools.lru_cache(maxsize=None)
def _index(name, Z, which):
    hb = GRAPHS[name]
    idx = model_index(hb.shape[0], hb.shape[1], Z, **_params(name, Z, which))
    idx.setflags(write=False)
    return idx


def _rm(name, Z, which):
    from nldpc.ratematch import RateMatch
    return RateMatch(**_params(name, Z, which))


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name,Z,B", SHAPES)
def test_rate_match_equals_the_sequential_model(name, Z, B, which):
    from nldpc.ratematch import index, rate_match
    g, rm, idx = _graph(name, Z), _rm(name, Z, which), _index(name, Z, which)
    assert np.array_equal(index(g, rm), idx)
    rng = np.random.default_rng(Z * 1000 + B)
    y = torch.from_numpy(rng.integers(0, 2, (B, g.N * Z)).astype(np.uint8)).to(DEV)
    sel = torch.from_numpy(idx.copy()).to(DEV)
    f = rate_match(g, rm, y)
    assert f.dtype == torch.uint8 and tuple(f.shape) == (B, rm.E)
    assert torch.equal(f, y[:, sel])
    # any non-zero byte is a 1; the output is 0 / 1; nothing outside the output is written, wherever it starts
    raw = torch.from_numpy(rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, g.N * Z))).to(DEV)
    for shift in (0, 3):
        buf, out = _guarded((B, rm.E), torch.uint8, 0xAA, shift)
        got = rate_match(g, rm, raw, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert int(got.max()) <= 1
        assert torch.equal(got, (raw != 0).to(torch.uint8)[:, sel])
        assert _guards_intact(buf, out, 0xAA, shift)


@pytest.mark.parametrize("clip", [0.0, 7.5])
@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name,Z,B", SHAPES)
def test_rate_recover_is_bit_identical_to_the_fp32_model(name, Z, B, which, clip):
    from nldpc.ratematch import rate_recover
    g, rm, kw = _graph(name, Z), _rm(name, Z, which), _params(name, Z, which)
    L, K, F = g.N * Z, g.K, kw["n_filler"]
    gen = torch.Generator().manual_seed(Z * 100 + B)
    llr = torch.randn((B, rm.E), generator=gen) * 4
    llr2 = torch.randn((B, rm.E), generator=gen) * 4
    want, got_mask = model_recover(g.M, g.N, Z, kw, llr.numpy(), erasure=ERASURE, filler=FILLER, clip=clip)
    sentinel = 777.25
    for shift in (0, 1):
        buf, out = _guarded((B, g.N, Z), torch.float32, sentinel, shift)
        xa = rate_recover(g, rm, llr.to(DEV), out=out, erasure_value=ERASURE, filler_value=FILLER, clip=clip)
        assert xa.data_ptr() == out.data_ptr() and tuple(xa.shape) == (B, g.N, Z)
        got = xa.reshape(B, L).cpu().numpy()
        assert np.array_equal(got, want)
        assert _guards_intact(buf, out, sentinel, shift)
        # erased and filler positions hold exactly the two constants
        erased = ~got_mask
        erased[K * Z - F:K * Z] = False
        assert erased.any() or which == "b"
        assert (got[:, erased] == np.float32(ERASURE)).all()
        assert (got[:, K * Z - F:K * Z] == np.float32(FILLER)).all()
        # a second transmission on top: positions that receive nothing keep what they held (here: a sentinel)
        held = torch.from_numpy(want).clone()
        held[:, torch.from_numpy(erased)] = sentinel
        out.copy_(held.view(B, g.N, Z))
        want2, _ = model_recover(g.M, g.N, Z, kw, llr2.numpy(), prev=held.numpy(), filler=FILLER, clip=clip)
        rate_recover(g, rm, llr2.to(DEV), out=out, accumulate=True, erasure_value=ERASURE, filler_value=FILLER,
                     clip=clip)
        got2 = out.reshape(B, L).cpu().numpy()
        assert np.array_equal(got2, want2)
        assert (got2[:, erased] == np.float32(sentinel)).all()
        assert _guards_intact(buf, out, sentinel, shift)
    fresh = rate_recover(g, rm, llr.to(DEV), erasure_value=ERASURE, filler_value=FILLER, clip=clip)
    assert np.array_equal(fresh.reshape(B, L).cpu().numpy(), want)


def test_recover_keeps_nan_through_the_clip():
    from nldpc.ratematch import rate_recover
    g, rm = _graph("bg2", 16), _rm("bg2", 16, "a")
    llr = torch.ones((2, rm.E))
    llr[1, 5] = float("nan")
    xa = rate_recover(g, rm, llr.to(DEV), clip=0.5).reshape(2, -1).cpu().numpy()
    n = _index("bg2", 16, "a")[5]
    assert np.isnan(xa[1, n]) and xa[0, n] == 0.5 and np.isnan(xa).sum() == 1


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("name,Z,B", SHAPES)
def test_round_trip_keeps_the_sign_of_every_sent_bit(name, Z, B, which):
    from nldpc.ratematch import rate_match, rate_recover
    g, rm = _graph(name, Z), _rm(name, Z, which)
    y = torch.from_numpy(np.random.default_rng(B).integers(0, 2, (B, g.N * Z)).astype(np.uint8)).to(DEV)
    f = rate_match(g, rm, y)
    xa = rate_recover(g, rm, 2.0 * f.float() - 1.0).reshape(B, -1)
    sent = torch.from_numpy(np.unique(_index(name, Z, which))).to(DEV)
    assert torch.equal(torch.sign(xa[:, sent]), 2.0 * y[:, sent].float() - 1.0)
    unsent = torch.ones(g.N * Z, dtype=torch.bool, device=DEV)
    unsent[sent] = False
    K, F = g.K, rm.n_filler
    unsent[K * Z - F:K * Z] = False
    assert (xa[:, unsent] == 0).all() and (xa[:, K * Z - F:K * Z] == -20.0).all()


# ---------------------------------------------------------------- end to end: encode -> match -> channel -> recover -> decode
def _words():
    from nldpc.channel import encode
    info = np.random.default_rng(5).integers(0, 2, (8, 160))
    info[:, -24:] = 0
    return encode(_graph("bg2", 16), torch.from_numpy(info).to(DEV))


def _neural(xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph("bg2", 16)
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def test_rate_half_end_to_end_decodes():
    """BG2 z=16, rate 1/2 (E = 272, 24 fillers, rv0, qm = 2), 6 dB, Neural T=10, weights 0.75, bias 0, erasures 1e-3.
    On the CPU (the oracle decoder fed by oracle.philox's restatement of the channel) the frame errors per iteration
    are [8, 8, 2, 1, 0, 0, 0, 0, 0, 0] for seed 77 (seeds 78 and 79 reach 0 earlier): iterations 6-9 leave two
    iterations of margin for last-bit differences between the device's and glibc's fp64 in the channel."""
    from nldpc.channel import awgn_llr, ber_counts, syndrome_weight
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    g = _graph("bg2", 16)
    y = _words()
    rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=2)
    R = code_rate(g, rm)
    assert R == 136 / 272
    sigma = float(np.float32(np.sqrt(1 / (2 * R * 10 ** 0.6))))
    f = rate_match(g, rm, y)
    llr = awgn_llr(8, 272, 1, sigma, seed=77, device=DEV, y=f).reshape(8, 272)
    xa = rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0)
    outs = _neural(xa)
    counts = ber_counts(outs, y).cpu().numpy()
    unsat = syndrome_weight(outs, g).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist(), "unsatisfied checks:", unsat.sum(1).tolist())
    assert not counts[6:, 0].any()
    assert not unsat[6:].any()


def test_harq_two_redundancy_versions_combine():
    """The same words at E = 160 (R = 136/160), 4 dB: rv0 (seed 77) and rv2 (k0 = 400, seed 78) combined with
    accumulate=True.  On the CPU the combined frame errors per iteration are [8, 8, 1, 0, 0, 0, 0, 0, 0, 0]; rv0
    alone still has 2 frame errors at iteration 9 there (near threshold, so not asserted)."""
    from nldpc.channel import awgn_llr, ber_counts
    from nldpc.ratematch import RateMatch, rate_match, rate_recover
    g = _graph("bg2", 16)
    y = _words()
    sigma = float(np.float32(np.sqrt(1 / (2 * (136 / 160) * 10 ** 0.4))))
    xa, want = None, None
    for rv, seed in ((0, 77), (2, 78)):
        rm = RateMatch.nr5g(g, 160, rv=rv, n_filler=24, qm=2)
        assert rm.k0 == (0, 400)[rv // 2]
        llr = awgn_llr(8, 160, 1, sigma, seed=seed, device=DEV, y=rate_match(g, rm, y)).reshape(8, 160)
        xa = rate_recover(g, rm, llr, out=xa, accumulate=xa is not None, erasure_value=1e-3, filler_value=-20.0)
        kw = dict(E=160, k0=rm.k0, punct_cols=2, n_filler=24, ncb=0, qm=2)
        want, _ = model_recover(g.M, g.N, 16, kw, llr.cpu().numpy(), prev=want, erasure=1e-3, filler=-20.0)
    assert np.array_equal(xa.reshape(8, -1).cpu().numpy(), want)
    counts = ber_counts(_neural(xa), y).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist())
    assert not counts[6:, 0].any()


def test_bad_tensors_raise_value_error():
    from nldpc import _lib
    from nldpc.ratematch import rate_match, rate_recover
    g, rm = _graph("bg2", 16), _rm("bg2", 16, "a")
    B, L, E = 2, 832, rm.E
    y = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
    llr = torch.zeros((B, E), device=DEV)
    for bad in (y.cpu(), y.float(), y[:, :-1], y.t().contiguous().t(), y.reshape(-1)):
        with pytest.raises(ValueError):
            rate_match(g, rm, bad)
    for out in (torch.empty((B, E + 1), dtype=torch.uint8, device=DEV), torch.empty((B, E), device=DEV),
                torch.empty((B, E), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            rate_match(g, rm, y, out=out)
    for bad in (llr.cpu(), llr.double(), llr[:, :-1], llr.t().contiguous().t(), llr.reshape(-1)):
        with pytest.raises(ValueError):
            rate_recover(g, rm, bad)
    for out in (torch.empty((B, L), device=DEV), torch.empty((B, 52, 16), dtype=torch.float64, device=DEV),
                torch.empty((B, 52, 16))):
        with pytest.raises(ValueError):
            rate_recover(g, rm, llr, out=out)
    with pytest.raises(ValueError):
        rate_recover(g, rm, llr, accumulate=True)
    # the C entry points: NULL pointers, B <= 0, a rule of nldpc_rm
    Lb, h, c = _lib.lib(), g.handle(DEV), rm._c()
    f = torch.empty((B, E), dtype=torch.uint8, device=DEV)
    xa = torch.empty((B, 52, 16), device=DEV)
    import ctypes
    assert Lb.nldpc_rate_match(h, ctypes.byref(c), y.data_ptr(), 0, f.data_ptr(), None) == _lib.NLDPC_EINVAL
    assert Lb.nldpc_rate_match(h, ctypes.byref(c), None, B, f.data_ptr(), None) == _lib.NLDPC_EINVAL
    assert Lb.nldpc_rate_match(h, None, y.data_ptr(), B, f.data_ptr(), None) == _lib.NLDPC_EINVAL
    assert Lb.nldpc_rate_recover(h, ctypes.byref(c), llr.data_ptr(), -1, 0.0, -20.0, 0.0, 0, xa.data_ptr(),
                                 None) == _lib.NLDPC_EINVAL
    assert Lb.nldpc_rate_recover(h, ctypes.byref(c), llr.data_ptr(), B, 0.0, -20.0, 0.0, 0, None,
                                 None) == _lib.NLDPC_EINVAL
    bad_rm = _lib.NldpcRm(2, 1, 0, 0, 800, E)  # k0 == Ncb
    assert Lb.nldpc_rate_match(h, ctypes.byref(bad_rm), y.data_ptr(), B, f.data_ptr(), None) == _lib.NLDPC_EINVAL
