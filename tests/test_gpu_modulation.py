"""QAM modulation, soft demapping and the fused QAM/AWGN channel (nldpc_qam_modulate / nldpc_qam_demap /
nldpc_qam_channel_llr, nldpc.modulation) on the GPU.  Expected values come from qam_model.py (the 38.211 formulas, the
fp32 max-log, the fp64 log-MAP with its derived bound, the Philox noise), never from the library.

Shapes (qm, S, B, b_offset): one symbol -- half a Philox pair; odd S with an odd offset -- pairs straddle rows and the
stream starts mid-pair; S = 1 -- every row is half a pair; the largest order; the row length of the headline graph at
rate 1/2 (E = 7680, qm = 6).  The fused kernel's thread owns one Philox counter (two symbols): with qm = 4 and an odd
first symbol its 16-byte stores stay aligned, with qm = 6 they do not (the element path), and the guard test shifts
every output by 3 elements and the bits by one byte.
"""
import functools
import os

import numpy as np
import pytest
import torch

import qam_model as qm_
from conftest import ROOT
from ratematch_model import model_index

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = [(2, 1, 1, 0), (4, 67, 5, 3), (6, 1, 131, 1), (8, 250, 3, 0), (6, 1280, 3, 0)]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}
SEED = 4242
METHODS = ["maxlog", "logmap"]


@functools.lru_cache(maxsize=None)
def _case(qm, S, B, off):
    """the shared, read-only reference of one shape"""
    rng = np.random.default_rng(qm * 1000 + S + B)
    f = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, S * qm))
    sigma = float(np.float32(SIGMA[qm]))
    c = dict(f=f, sigma=sigma, sym=qm_.modulate(f, qm), noisy=qm_.noisy_symbols(f, qm, sigma, SEED, off))
    c["maxlog"] = qm_.maxlog(c["noisy"], qm, sigma)
    c["logmap"], c["dmax"] = qm_.logmap64(c["noisy"], qm, sigma)
    c["bound"] = qm_.logmap_bound(qm, c["logmap"], c["dmax"])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the references are read-only)


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


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_modulate_equals_the_model(qm, S, B, off):
    from nldpc.modulation import modulate
    c = _case(qm, S, B, off)
    sym = modulate(_dev(c["f"]), qm)
    assert sym.dtype == torch.float32 and tuple(sym.shape) == (B, S, 2)
    assert _bits_equal(sym.cpu().numpy(), c["sym"])


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_demap_maxlog_is_bit_identical_to_the_fp32_model(qm, S, B, off):
    from nldpc.modulation import demap
    c = _case(qm, S, B, off)
    llr = demap(_dev(c["noisy"]), qm, c["sigma"], method="maxlog")
    assert llr.dtype == torch.float32 and tuple(llr.shape) == (B, S * qm)
    assert _bits_equal(llr.cpu().numpy(), c["maxlog"])


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_demap_logmap_is_within_the_derived_bound_of_the_fp64_model(qm, S, B, off):
    """the bound of qam_model.logmap_bound (per LLR, scaling with max |d*w| of its dimension)"""
    import ctypes
    from nldpc import _lib
    from nldpc.modulation import demap
    c = _case(qm, S, B, off)
    got = demap(_dev(c["noisy"]), qm, c["sigma"], method="logmap").cpu().numpy()
    err = np.abs(got.astype(np.float64) - c["logmap"])
    host = np.zeros(B * S * qm, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    noisy = np.ascontiguousarray(c["noisy"])
    assert _lib.lib().nldpc_qam_demap_ref(qm, 1, c["sigma"], noisy.ctypes.data_as(fp), B * S,
                                          host.ctypes.data_as(fp)) == _lib.NLDPC_OK
    differ = int((got.reshape(-1).view(np.uint32) != host.view(np.uint32)).sum())
    print(f"qm={qm} S={S} B={B}: max err / bound = {(err / c['bound']).max():.3f}, max |d*w| = {c['dmax'].max():.4g}, "
          f"{differ} of {host.size} values differ from the host demapper's")
    assert (err <= c["bound"]).all()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_fused_channel_equals_demap_of_its_symbols(qm, S, B, off, method):
    from nldpc.modulation import demap, qam_llr
    c = _case(qm, S, B, off)
    f = _dev(c["f"])
    llr, sym = qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, method=method, return_symbols=True)
    assert llr.dtype == sym.dtype == torch.float32 and tuple(llr.shape) == (B, S * qm) and tuple(sym.shape) == (B, S, 2)
    assert _bits_equal(llr.cpu().numpy(), demap(sym, qm, c["sigma"], method=method).cpu().numpy())
    got = sym.cpu().numpy()
    miss = float((got != c["noisy"]).mean())
    print(f"qm={qm} S={S} B={B} {method}: {miss:.2e} of the noisy symbols differ from the model's")
    assert miss < 1e-4
    assert np.abs(got - c["noisy"]).max() <= 4 * np.spacing(np.abs(c["noisy"]).max())
    alone = qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, method=method)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.view(torch.int32), llr.view(torch.int32))


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_a_shard_draws_the_noise_of_the_unsharded_batch(qm, S, B, off):
    from nldpc.modulation import qam_llr
    c = _case(qm, S, B, off)
    f = _dev(c["f"])
    llr, sym = qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, return_symbols=True)
    for k in (1, 2):  # both parities of the first pair (B = 1 has no rows to split off)
        if k >= B:
            continue
        l2, s2 = qam_llr(f[k:].contiguous(), qm, c["sigma"], seed=SEED, b_offset=off + k, return_symbols=True)
        assert torch.equal(l2.view(torch.int32), llr[k:].view(torch.int32))
        assert torch.equal(s2.view(torch.int32), sym[k:].view(torch.int32))


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_all_zero_word_seed_and_noise_stream(qm, S, B, off):
    from oracle.philox import awgn_llr
    from nldpc.modulation import modulate, qam_llr
    c = _case(qm, S, B, off)
    sigma = c["sigma"]
    zeros = torch.zeros((B, S * qm), dtype=torch.uint8, device=DEV)
    a, sa = qam_llr(None, qm, sigma, B=B, E=S * qm, seed=SEED, b_offset=off, return_symbols=True)
    b, sb = qam_llr(zeros, qm, sigma, seed=SEED, b_offset=off, return_symbols=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    other, so = qam_llr(zeros, qm, sigma, seed=SEED + 1, b_offset=off, return_symbols=True)
    assert not torch.equal(so, sb) and not torch.equal(other, b)
    # the normals are not the BPSK channel's at the same seed: normal j of global symbol G comes from counter G >> 1,
    # the counter of BPSK element 2 G + j -- but counter word 2 differs
    n = ((sb - modulate(zeros, qm)) / sigma).cpu().numpy().reshape(-1).astype(np.float64)
    bpsk = awgn_llr(B, 2 * S, sigma, SEED, off).reshape(-1).astype(np.float64)
    n_bpsk = (bpsk * sigma * sigma / 2.0 + 1.0) / sigma
    print(f"qm={qm} S={S} B={B}: max |n - n_bpsk| = {np.abs(n - n_bpsk).max():.3f}, "
          f"{float((np.abs(n - n_bpsk) < 1e-3).mean()):.2e} of the normals within 1e-3")
    assert np.abs(n - n_bpsk).max() > 0.05 and (np.abs(n - n_bpsk) < 1e-3).mean() <= 0.01


@pytest.mark.parametrize("qm,S,B,off", SHAPES)
def test_nothing_outside_the_outputs_is_written(qm, S, B, off):
    from nldpc.modulation import demap, modulate, qam_llr
    c = _case(qm, S, B, off)
    E, sentinel = S * qm, 777.25
    for shift in (0, 3):
        fbuf = torch.full((B * E + 8,), 0x55, dtype=torch.uint8, device=DEV)
        f = fbuf[shift // 3:shift // 3 + B * E].view(B, E)  # (the bits start off a dword boundary when shifted)
        f.copy_(_dev(c["f"]))
        sbuf, sym = _guarded((B, S, 2), torch.float32, sentinel, shift)
        assert modulate(f, qm, out=sym).data_ptr() == sym.data_ptr()
        assert _bits_equal(sym.cpu().numpy(), c["sym"]) and _guards_intact(sbuf, sym, sentinel, shift)
        nbuf, noisy = _guarded((B, S, 2), torch.float32, sentinel, shift)
        noisy.copy_(_dev(c["noisy"]))
        lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
        assert demap(noisy, qm, c["sigma"], out=llr).data_ptr() == llr.data_ptr()
        assert _bits_equal(llr.cpu().numpy(), c["maxlog"]) and _guards_intact(lbuf, llr, sentinel, shift)
        assert _guards_intact(nbuf, noisy, sentinel, shift)
        lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
        obuf, so = _guarded((B, S, 2), torch.float32, sentinel, shift)
        got, gs = qam_llr(f, qm, c["sigma"], seed=SEED, b_offset=off, out=llr, return_symbols=so)
        assert got.data_ptr() == llr.data_ptr() and gs.data_ptr() == so.data_ptr()
        assert _guards_intact(lbuf, llr, sentinel, shift) and _guards_intact(obuf, so, sentinel, shift)
        assert bool((fbuf[:shift // 3] == 0x55).all()) and bool((fbuf[shift // 3 + B * E:] == 0x55).all())
        # the shifted run computes what the unshifted one does, and every element was written
        ref, rs = qam_llr(_dev(c["f"]), qm, c["sigma"], seed=SEED, b_offset=off, return_symbols=True)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
        assert torch.equal(gs.view(torch.int32), rs.view(torch.int32))


def test_noise_statistics():
    from nldpc.modulation import modulate, qam_llr
    qm, S, B = 6, 1280, 64
    sigma = float(np.float32(SIGMA[qm]))
    f = torch.from_numpy(np.random.default_rng(9).integers(0, 2, (B, S * qm)).astype(np.uint8)).to(DEV)
    _, sym = qam_llr(f, qm, sigma, seed=SEED, return_symbols=True)
    n = ((sym - modulate(f, qm)).double() / sigma).cpu().numpy()
    for dim, name in ((0, "I"), (1, "Q")):
        mean, std = n[..., dim].mean(), n[..., dim].std()
        print(f"{name}: mean {mean:+.5f}, std {std:.5f} over {n[..., dim].size} samples")
        assert abs(mean) < 0.01 and abs(std - 1.0) < 0.01
    assert abs(np.mean(n[..., 0] * n[..., 1])) < 0.01


def test_bad_arguments_raise_value_error():
    from nldpc.modulation import demap, modulate, qam_llr
    B, E, qm = 2, 24, 4
    f = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    sym = torch.zeros((B, E // qm, 2), device=DEV)
    for bad in (f.cpu(), f.float(), f.t().contiguous().t(), f.reshape(-1), f[:, :-2]):
        with pytest.raises(ValueError):
            modulate(bad, qm)
        with pytest.raises(ValueError):
            qam_llr(bad, qm, 0.5)
    for bad in (sym.cpu(), sym.double(), sym.transpose(0, 1).contiguous().transpose(0, 1), sym.reshape(B, -1), sym[:, :, :1]):
        with pytest.raises(ValueError):
            demap(bad, qm, 0.5)
    for out in (torch.empty((B, E + 1), device=DEV), torch.empty((B, E), dtype=torch.float64, device=DEV),
                torch.empty((B, E)), torch.empty((E, B), device=DEV).t()):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, out=out)
        with pytest.raises(ValueError):
            demap(sym, qm, 0.5, out=out)
    for out in (torch.empty((B, E // qm, 3), device=DEV), torch.empty((B, E // qm, 2))):
        with pytest.raises(ValueError):
            modulate(f, qm, out=out)
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, return_symbols=out)
    for bad_qm in (1, 3, 10):
        with pytest.raises(ValueError):
            modulate(f, bad_qm)
        with pytest.raises(ValueError):
            qam_llr(f, bad_qm, 0.5)
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            qam_llr(f, qm, sigma)
        with pytest.raises(ValueError):
            demap(sym, qm, sigma)
    with pytest.raises(ValueError):
        qam_llr(f, qm, 0.5, method="exact")
    with pytest.raises(ValueError):
        demap(sym, qm, 0.5, method=1)
    with pytest.raises(ValueError):
        qam_llr(f[:, :20].contiguous(), 8, 0.5)  # 20 % 8
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, B=2, E=10)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5)
    with pytest.raises(ValueError):
        qam_llr(f, qm, 0.5, b_offset=-1)
    # the library's own answer surfaces as ValueError too
    from nldpc import _lib
    assert _lib.lib().nldpc_qam_channel_llr(4, 0, f.data_ptr(), B, 22, 0.5, 1, 0, sym.data_ptr(), None,
                                            None) == _lib.NLDPC_EINVAL
    with pytest.raises(ValueError):
        _lib.check(_lib.NLDPC_EINVAL, "nldpc_qam_channel_llr")


# ---------------------------------------------------------------- end to end: encode -> match -> 16-QAM -> recover -> decode
RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
EBN0_DB = 6.5


@functools.lru_cache(maxsize=None)
def _graph():
    from nldpc.graph import LiftedGraph
    return LiftedGraph(BG2, 16)


def _words():
    from nldpc.channel import encode
    info = np.random.default_rng(5).integers(0, 2, (8, 160))
    info[:, -24:] = 0
    return encode(_graph(), torch.from_numpy(info).to(DEV))


def _neural(xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    g = _graph()
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def _chain(y, rm, seed):
    from nldpc.modulation import qam_llr, sigma_for
    from nldpc.ratematch import code_rate, rate_match, rate_recover
    g = _graph()
    R = code_rate(g, rm)
    assert R == 136 / 272
    sigma = float(np.float32(sigma_for(EBN0_DB, R, 4)))
    llr = qam_llr(rate_match(g, rm, y), 4, sigma, seed=seed, method="logmap")
    return _neural(rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0))


def test_rate_half_16qam_end_to_end_decodes():
    """BG2 z=16, rate 1/2 (E = 272, 24 fillers, rv0), 16-QAM log-MAP, Neural T=10, weights 0.75, bias 0, erasures 1e-3.
    Eb/N0 = 6.5 dB (sigma = sigma_for(6.5, 1/2, 4) = 0.236576): the lowest of a 0.5 dB grid at which the CPU chain
    (qam_model's channel and fp64 log-MAP rounded to fp32, ratematch_model's recovery, the oracle decoder) has no frame
    error from iteration 6 on for seeds 77, 78 and 79.  CPU frame errors per iteration, interleaver qm = 4:
      6.0 dB  77: [8, 8, 8, 5, 0, 0, 0, 0, 0, 0]  78: [8, 8, 8, 7, 5, 3, 2, 0, 0, 0]  79: [8, 8, 8, 5, 2, 2, 1, 0, 0, 0]
      6.5 dB  77: [8, 8, 8, 3, 0, 0, 0, 0, 0, 0]  78: [8, 8, 8, 6, 4, 1, 0, 0, 0, 0]  79: [8, 8, 8, 4, 2, 1, 0, 0, 0, 0]
    and with RateMatch(qm=1) in front of the same 16-QAM (the bits reach other symbol positions; any grouping is valid):
      6.5 dB  77: [8, 8, 8, 7, 3, 0, 0, 0, 0, 0]  78: [8, 8, 8, 7, 4, 1, 0, 0, 0, 0]  79: [8, 8, 8, 7, 3, 1, 1, 0, 0, 0]
    The device runs seed 77: iterations 6-9 leave two iterations (one without the interleaver) of margin for last-bit
    differences between the device's and glibc's fp64 in the channel."""
    from nldpc.channel import ber_counts, syndrome_weight
    from nldpc.modulation import modulate
    from nldpc.ratematch import RateMatch, rate_match
    g = _graph()
    y = _words()
    idx = {}
    for qm in (4, 1):
        rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=qm)
        outs = _chain(y, rm, 77)
        counts = ber_counts(outs, y).cpu().numpy()
        unsat = syndrome_weight(outs, g).cpu().numpy()
        print(f"interleaver qm={qm}: bit / frame errors per iteration:", counts.tolist(), "unsatisfied checks:",
              unsat.sum(1).tolist())
        assert not counts[6:, 0].any()
        assert not unsat[6:].any()
        # sent bit m = codeword bit idx[m] rides on bit m % 4 of symbol m // 4: the model's index, then the grouping
        idx[qm] = model_index(g.M, g.N, 16, E=272, k0=rm.k0, punct_cols=2, n_filler=24, ncb=0, qm=qm)
        sym = modulate(rate_match(g, rm, y), 4).cpu().numpy()
        assert _bits_equal(sym, qm_.modulate(y.cpu().numpy()[:, idx[qm]], 4))
    # the interleaver now has an effect: other bits share a symbol
    assert not np.array_equal(idx[4], idx[1])
    assert sorted(idx[4].tolist()) == sorted(idx[1].tolist())
