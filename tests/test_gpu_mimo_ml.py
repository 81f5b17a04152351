"""Exact max-log ML MIMO detection (nldpc_mimo_detect_ml / nldpc_mimo_channel_llr_ml, nldpc.mimo.detect_ml /
qam_llr_ml) on the GPU.  Expected values come from mimo_ml_model.py (the sliced two-pass detector in the stated order)
and mimo_model.py (channels, received samples), never from the library; the detector is also compared with the host
reference, which test_mimo_ml_host.py pins to the model and to an exhaustive float64 search.  Everything here is bit for
bit, so no tolerance appears.

Shapes (qm, nt, nr, R, B, b_offset, L): a single resource element; odd R with an odd offset and L = 3 -- a short last
block, rows that end inside a wave; the same with L = R on 2 x 4; receive diversity only with qm = 6 (6 floats per RE: the
8-byte staging path); 64-QAM and 256-QAM on two layers (64 and 256 candidates per pass, the largest of nt = 2); 4 x 4 at
QPSK and 16-QAM (64 and 4096 candidates per pass, the largest of nt = 4); more than one workgroup of whole waves.  One
thread owns one resource element in every instantiation, so no shape depends on a group size.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mimo_ml_model as ml
import mimo_model as mm
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = [(2, 1, 1, 1, 1, 0, 1), (4, 2, 2, 67, 5, 3, 3), (4, 2, 4, 67, 5, 3, 67), (6, 1, 2, 131, 2, 1, 1),
          (6, 2, 2, 33, 3, 1, 1), (8, 2, 2, 19, 2, 0, 4), (2, 4, 4, 65, 3, 0, 64), (4, 4, 4, 9, 2, 1, 2),
          (2, 2, 2, 640, 3, 0, 1)]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}
SEED = 4242
C_INITS = [0x12345, 0x7FFFFFFF, 0x0BADC0DE & 0x7FFFFFFF]
_FP = ctypes.POINTER(ctypes.c_float)
shapes = pytest.mark.parametrize("qm,nt,nr,R,B,off,L", SHAPES)


@functools.lru_cache(maxsize=None)
def _case(qm, nt, nr, R, B, off, L):
    """the shared, read-only reference of one shape"""
    rng = np.random.default_rng(qm * 1000 + R + B + 10 * nt + nr)
    f = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (B, R * nt * qm))
    c = dict(f=f, sigma=float(np.float32(SIGMA[qm])), h=mm.channels(B, R, L, nt, nr, SEED, off))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the references are read-only)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def _guarded(shape, dtype, fill, shift):
    """a tensor of `shape` that is a view into a larger buffer filled with `fill`, `shift` elements from its start"""
    n = int(np.prod(shape))
    buf = torch.full((shift + n + 19,), fill, dtype=dtype, device=DEV)
    return buf, buf[shift:shift + n].view(shape)


def _guards_intact(buf, view, fill, shift):
    n = view.numel()
    return bool((buf[:shift] == fill).all()) and bool((buf[shift + n:] == fill).all())


def _run(c, qm, nt, nr, off, L, **kw):
    from nldpc.mimo import qam_llr_ml
    f = kw.pop("f") if "f" in kw else _dev(c["f"])
    return qam_llr_ml(f, qm, c["sigma"], nt=nt, nr=nr, L=L, seed=SEED, b_offset=off, **kw)


@shapes
def test_fused_equals_unfused_equals_the_host_reference_and_the_model(qm, nt, nr, R, B, off, L):
    from nldpc import _lib
    from nldpc.mimo import detect_ml
    c = _case(qm, nt, nr, R, B, off, L)
    llr, y, h = _run(c, qm, nt, nr, off, L, return_symbols=True, return_channels=True)
    assert llr.dtype == y.dtype == h.dtype == torch.float32
    assert tuple(llr.shape) == (B, R * nt * qm) and tuple(y.shape) == (B, R, nr, 2) and tuple(h.shape) == c["h"].shape
    unfused = detect_ml(y, qm, c["sigma"], h, L=L)
    assert _same(llr, unfused)
    y_np, h_np, got = y.cpu().numpy(), h.cpu().numpy(), unfused.cpu().numpy()
    assert np.isfinite(got).all()
    ref = np.full((B, R * nt * qm), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_detect_ml_ref(qm, nt, nr, c["sigma"], y_np.ctypes.data_as(_FP), h_np.ctypes.data_as(_FP),
                                               B, R, L, ref.ctypes.data_as(_FP)) == _lib.NLDPC_OK
    assert _bits_equal(got, ref)
    assert _bits_equal(got, ml.detect_ml(y_np, h_np, qm, c["sigma"], L))
    alone = _run(c, qm, nt, nr, off, L)
    assert isinstance(alone, torch.Tensor) and _same(alone, llr)
    two = _run(c, qm, nt, nr, off, L, return_channels=True)
    assert len(two) == 2 and _same(two[0], llr) and _same(two[1], h)


@shapes
def test_samples_and_channels_are_those_of_the_lmmse_channel(qm, nt, nr, R, B, off, L):
    from nldpc.mimo import qam_llr
    c = _case(qm, nt, nr, R, B, off, L)
    llr, y, h = _run(c, qm, nt, nr, off, L, return_symbols=True, return_channels=True)
    lin, y2, h2 = qam_llr(_dev(c["f"]), qm, c["sigma"], nt=nt, nr=nr, L=L, seed=SEED, b_offset=off, return_symbols=True,
                          return_channels=True)
    assert _same(y, y2) and _same(h, h2)
    assert llr.shape == lin.shape and (nt == 1 or R < 4 or not _same(llr, lin))


@shapes
def test_given_channels_equal_to_the_drawn_table_reproduce_the_drawn_run(qm, nt, nr, R, B, off, L):
    c = _case(qm, nt, nr, R, B, off, L)
    llr, y, h = _run(c, qm, nt, nr, off, L, return_symbols=True, return_channels=True)
    l2, y2, h2 = _run(c, qm, nt, nr, off, L, h=h.clone(), return_symbols=True, return_channels=True)
    assert _same(l2, llr) and _same(y2, y) and _same(h2, h)


@shapes
def test_scrambling_in_flight_equals_the_three_steps(qm, nt, nr, R, B, off, L):
    from nldpc.scrambling import descramble, scramble, sequence
    c = _case(qm, nt, nr, R, B, off, L)
    f = _dev(c["f"])
    for n_seq in (1, 3):
        seq = sequence(C_INITS[:n_seq], R * nt * qm, device=DEV)
        got, gy = _run(c, qm, nt, nr, off, L, scramble=seq, return_symbols=True)
        mid, my = _run(c, qm, nt, nr, off, L, f=scramble(f, seq, b_offset=off), return_symbols=True)
        assert _same(got, descramble(mid, seq, b_offset=off)) and _same(gy, my)
    plain = _run(c, qm, nt, nr, off, L)
    assert not _same(plain, got) or plain.numel() < 8


@shapes
def test_a_shard_equals_the_rows_of_the_unsharded_batch(qm, nt, nr, R, B, off, L):
    c = _case(qm, nt, nr, R, B, off, L)
    f = _dev(c["f"])
    llr, y, h = _run(c, qm, nt, nr, off, L, return_symbols=True, return_channels=True)
    for k in (1, 2):  # (B = 1 has no rows to split off)
        if k >= B:
            continue
        l2, y2, h2 = _run(c, qm, nt, nr, off + k, L, f=f[k:].contiguous(), return_symbols=True, return_channels=True)
        assert _same(l2, llr[k:]) and _same(y2, y[k:]) and _same(h2, h[k:])


@shapes
def test_all_zero_word_decodes_to_zeros_at_low_noise(qm, nt, nr, R, B, off, L):
    from nldpc.mimo import qam_llr_ml
    c = _case(qm, nt, nr, R, B, off, L)
    E = R * nt * qm
    zeros = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    a = _run(c, qm, nt, nr, off, L, f=None, B=B, E=E, device=DEV, return_symbols=True, return_channels=True)
    b = _run(c, qm, nt, nr, off, L, f=zeros, return_symbols=True, return_channels=True)
    assert all(_same(x, y) for x, y in zip(a, b))
    if c["f"].any():
        assert not _same(a[1], _run(c, qm, nt, nr, off, L, return_symbols=True)[1])
    # sigma = 1e-3 and channels of gain one: |H x - H x'| is far above the noise for every pair of symbol vectors
    table = torch.zeros((B, mm.n_blocks(R, L), nr, nt, 2), device=DEV)
    for t in range(nt):
        table[..., t, t, 0] = 1.0
    quiet = qam_llr_ml(None, qm, 1e-3, nt=nt, nr=nr, L=L, h=table, B=B, E=E, seed=SEED, b_offset=off, device=DEV)
    assert bool((quiet < 0).all())


@shapes
def test_a_row_of_zero_channels_has_zero_llrs(qm, nt, nr, R, B, off, L):
    c = _case(qm, nt, nr, R, B, off, L)
    table = _dev(c["h"])
    row = B // 2
    table[row] = 0.0
    llr = _run(c, qm, nt, nr, off, L, h=table)
    assert bool(torch.isfinite(llr).all())
    assert bool(((llr[row].view(torch.int32) & 0x7FFFFFFF) == 0).all())
    if B > 1:
        assert bool((llr[row - 1] != 0).any())


@shapes
def test_nothing_outside_the_outputs_is_written(qm, nt, nr, R, B, off, L):
    from nldpc.mimo import detect_ml, n_blocks
    c = _case(qm, nt, nr, R, B, off, L)
    E, nb, sentinel = R * nt * qm, n_blocks(R, L), 777.25
    ref = _run(c, qm, nt, nr, off, L, return_symbols=True, return_channels=True)
    given = ref[2] * 0.5 + 0.25
    refg = _run(c, qm, nt, nr, off, L, h=given, return_symbols=True, return_channels=True)
    fbuf = torch.full((B * E + 8,), 0x55, dtype=torch.uint8, device=DEV)
    f = fbuf[1:1 + B * E].view(B, E)  # (the bits start off a dword boundary)
    f.copy_(_dev(c["f"]))
    for shift in (3, 4):  # off and on a 16-byte boundary
        for table, want in ((None, ref), (given, refg)):
            hin_buf = None
            if table is not None:
                hin_buf, hin = _guarded((B, nb, nr, nt, 2), torch.float32, sentinel, shift)
                hin.copy_(table)
                table = hin
            lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
            ybuf, y = _guarded((B, R, nr, 2), torch.float32, sentinel, shift)
            hbuf, h = _guarded((B, nb, nr, nt, 2), torch.float32, sentinel, shift)
            got = _run(c, qm, nt, nr, off, L, f=f, h=table, out=llr, return_symbols=y, return_channels=h)
            assert [t.data_ptr() for t in got] == [llr.data_ptr(), y.data_ptr(), h.data_ptr()]
            assert _guards_intact(lbuf, llr, sentinel, shift) and _guards_intact(ybuf, y, sentinel, shift)
            assert _guards_intact(hbuf, h, sentinel, shift)
            assert hin_buf is None or (_guards_intact(hin_buf, table, sentinel, shift) and _same(table, given))
            assert bool((fbuf[:1] == 0x55).all()) and bool((fbuf[1 + B * E:] == 0x55).all())
            # the shifted run computes what the unshifted one does, and every element was written
            assert all(_same(a, b) for a, b in zip(got, want))
            # the unfused detector, shifted the same way
            lbuf, llr = _guarded((B, E), torch.float32, sentinel, shift)
            assert detect_ml(y, qm, c["sigma"], h, L=L, out=llr).data_ptr() == llr.data_ptr()
            assert _same(llr, want[0]) and _guards_intact(lbuf, llr, sentinel, shift)
            assert _guards_intact(ybuf, y, sentinel, shift) and _guards_intact(hbuf, h, sentinel, shift)


def test_bad_arguments_and_the_unsupported_pair_raise():
    from nldpc import _lib
    from nldpc.mimo import detect_ml, qam_llr_ml
    B, qm, nt, nr, L = 2, 4, 2, 2, 2
    R, nb = 6, 3
    E = R * nt * qm
    f = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    y = torch.zeros((B, R, nr, 2), device=DEV)
    table = torch.ones((B, nb, nr, nt, 2), device=DEV)
    kw = dict(nt=nt, nr=nr)
    assert qam_llr_ml(f, qm, 0.5, L=L, h=table, **kw).shape == (B, E) and detect_ml(y, qm, 0.5, table, L=L).shape == (B, E)
    for bad_L in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            qam_llr_ml(f, qm, 0.5, L=bad_L, **kw)
        with pytest.raises(ValueError):
            detect_ml(y, qm, 0.5, table, L=bad_L)
    for bad in ((2, 1), (4, 2), (3, 3), (1, 3), (0, 1), (8, 8), (True, 1), (1.5, 2)):
        with pytest.raises(ValueError):
            qam_llr_ml(None, qm, 0.5, nt=bad[0], nr=bad[1], B=2, E=96, device=DEV)
    with pytest.raises(ValueError):
        qam_llr_ml(f[:, :E - qm].contiguous(), qm, 0.5, **kw)  # an odd number of symbols on two layers
    wide = torch.ones((B, nb, nr, nt, 4), device=DEV)
    for bad in (torch.ones((B, nb + 1, nr, nt, 2), device=DEV), torch.ones((B + 1, nb, nr, nt, 2), device=DEV),
                torch.ones((B, nb, nr * nt * 2), device=DEV), table.double(), table.cpu(), wide[..., ::2],
                torch.ones((B, nb, nr, nt, 3), device=DEV), [[1.0]]):
        with pytest.raises(ValueError):
            qam_llr_ml(f, qm, 0.5, L=L, h=bad, **kw)
        with pytest.raises(ValueError):
            detect_ml(y, qm, 0.5, bad, L=L)
        if isinstance(bad, torch.Tensor):
            with pytest.raises(ValueError):
                qam_llr_ml(f, qm, 0.5, L=L, return_channels=bad, **kw)
    with pytest.raises(ValueError):
        qam_llr_ml(f, qm, 0.5, L=L, h=table, return_channels=table, **kw)
    for bad_qm in (1, 3, 10):
        with pytest.raises(ValueError):
            qam_llr_ml(f, bad_qm, 0.5, **kw)
        with pytest.raises(ValueError):
            detect_ml(y, bad_qm, 0.5, table, L=L)
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            qam_llr_ml(f, qm, sigma, **kw)
        with pytest.raises(ValueError):
            detect_ml(y, qm, sigma, table, L=L)
    for bad in (f.cpu(), f.float(), f.reshape(-1), f[:, :-2]):
        with pytest.raises(ValueError):
            qam_llr_ml(bad, qm, 0.5, **kw)
    for bad in (y.cpu(), y.double(), y.reshape(B, -1), y[..., :1]):
        with pytest.raises(ValueError):
            detect_ml(bad, qm, 0.5, table, L=L)
    for more in (dict(b_offset=-1), dict(out=torch.empty((B, E + 1), device=DEV)),
                 dict(return_symbols=torch.empty((B, R, nr, 3), device=DEV)),
                 dict(scramble=torch.zeros((1, 3), dtype=torch.int32, device=DEV))):  # (E = 48: two words per row)
        with pytest.raises(ValueError):
            qam_llr_ml(f, qm, 0.5, **kw, **more)
    with pytest.raises(TypeError):
        qam_llr_ml(f, qm, 0.5, method="logmap", **kw)  # max-log only: there is no method argument
    with pytest.raises(TypeError):
        detect_ml(y, qm, 0.5, table, L=L, method="maxlog")
    with pytest.raises(ValueError):
        qam_llr_ml(None, qm, 0.5, **kw)
    with pytest.raises(ValueError):
        qam_llr_ml(None, qm, 0.5, B=2, E=10, **kw)
    with pytest.raises(ValueError):
        qam_llr_ml(None, qm, 0.5, B=2, E=16, device="cpu", **kw)
    # four layers stop at 16-QAM
    y4 = torch.zeros((B, R, 4, 2), device=DEV)
    t4 = torch.ones((B, R, 4, 4, 2), device=DEV)
    for big in (6, 8):
        with pytest.raises(_lib.NldpcUnsupported):
            detect_ml(y4, big, 0.5, t4)
        with pytest.raises(_lib.NldpcUnsupported):
            qam_llr_ml(None, big, 0.5, nt=4, nr=4, B=B, E=R * 4 * big, device=DEV)
    assert detect_ml(y4, 4, 0.5, t4).shape == (B, R * 16)


# ---------------------------------------------------------------- end to end: what the detector buys the decoder
RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
EBN0_DB = 6.0
# frame errors of the CPU chain (model (a), ratematch_model, the oracle decoder) after iterations 1 .. 10 at EBN0_DB
CPU_ML_FRAME_ERRORS = [32, 32, 32, 31, 24, 18, 11, 11, 8, 3]


def _neural(g, xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def test_rate_half_16qam_2x2_rayleigh_ml_beats_lmmse_end_to_end():
    """BG2 z=16, rate 1/2 (E = 272, 24 fillers, rv0), 16-QAM on two layers over a 2 x 2 Rayleigh channel with L = 1,
    Neural T=10, weights 0.75, bias 0, erasures 1e-3: the setting of test_gpu_mimo.py's
    test_rate_half_16qam_2x2_rayleigh_end_to_end_decodes, with 32 words (info bits from default_rng(5), the last 24
    zeroed) in place of 8.  The channels and the received samples are mimo_model's (seed 77), uploaded, so the device
    detectors see the model's inputs exactly; the chains are detect_ml -> rate_recover -> decode and
    detect(method="maxlog") -> the same.  The ML chain's frame errors per iteration must equal those of the CPU chain
    (mimo_ml_model.detect_ml, ratematch_model.model_recover, oracle.neural_forward; the codewords from the generator
    matrix), and after ten iterations be strictly fewer than the LMMSE chain's.  CPU frame errors after iterations
    1 .. 10 of 32, (a) max-log ML and (b) LMMSE max-log (mimo_model.detect_maxlog), sigma = mimo.sigma_for(., 1/2, 4, 2):
       5.5 dB  77: (a) [32, 32, 32, 32, 29, 22, 18, 11, 11, 8]  (b) [32, 32, 32, 32, 31, 29, 25, 19, 17, 15]
               78: (a) [32, 32, 32, 32, 29, 21, 15, 12, 10, 9]  (b) [32, 32, 32, 32, 29, 28, 22, 19, 17, 15]
       6.0 dB  77: (a) [32, 32, 32, 31, 24, 18, 11, 11, 8, 3]   (b) [32, 32, 32, 31, 29, 26, 20, 17, 13, 7]
               78: (a) [32, 32, 32, 30, 25, 18, 12, 9, 7, 6]    (b) [32, 32, 32, 32, 29, 24, 21, 16, 15, 12]
       6.5 dB  77: (a) [32, 32, 32, 29, 18, 12, 10, 4, 3, 3]    (b) [32, 32, 32, 31, 28, 21, 14, 10, 6, 5]
               78: (a) [32, 32, 32, 28, 19, 11, 8, 4, 3, 3]     (b) [32, 32, 32, 31, 27, 21, 16, 12, 10, 6]
       7.0 dB  77: (a) [32, 32, 31, 26, 15, 10, 7, 3, 1, 1]     (b) [32, 32, 32, 31, 23, 15, 9, 4, 2, 2]
               78: (a) [32, 32, 32, 26, 16, 7, 5, 3, 2, 1]      (b) [32, 32, 32, 28, 24, 18, 13, 9, 4, 2]
    The fp32 model gives a strict inequality at 6.0 dB (3 against 7), the point the device runs, seed 77."""
    from nldpc.channel import ber_counts, encode
    from nldpc.graph import LiftedGraph
    from nldpc.mimo import detect, detect_ml, sigma_for
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    g = LiftedGraph(BG2, 16)
    info = np.random.default_rng(5).integers(0, 2, (32, 160))
    info[:, -24:] = 0
    cw = encode(g, torch.from_numpy(info).to(DEV))
    rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=4)
    rate = code_rate(g, rm)
    assert rate == 136 / 272
    sigma = float(np.float32(sigma_for(EBN0_DB, rate, 4, 2)))
    f = rate_match(g, rm, cw).cpu().numpy()
    # the model's channels and samples, uploaded: both device detectors see the model's inputs exactly
    R = 272 // 4 // 2
    h_np = mm.channels(32, R, 1, 2, 2, 77)
    y_np = mm.received(f, 4, sigma, h_np, 1, 2, 2, 77)
    y, h = _dev(y_np), _dev(h_np)
    frames = {}
    for name, llr in (("ml", detect_ml(y, 4, sigma, h, L=1)), ("lmmse", detect(y, 4, sigma, h, L=1, method="maxlog"))):
        xa = rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0)
        frames[name] = ber_counts(_neural(g, xa, 10), cw).cpu().numpy()[:, 1].tolist()
        print(f"{name}: frame errors per iteration {frames[name]}")
    assert frames["ml"] == CPU_ML_FRAME_ERRORS
    assert frames["ml"][-1] < frames["lmmse"][-1]
