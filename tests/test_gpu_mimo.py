"""MIMO spatial multiplexing with LMMSE soft detection (nldpc_mimo_channels / nldpc_mimo_filter / nldpc_mimo_detect /
nldpc_mimo_channel_llr, nldpc.mimo) on the GPU.  Expected values come from mimo_model.py (the drawn entries on
oracle.philox's words, the received samples, the filter in the stated order, the fp32 max-log and the fp64 log-MAP with
qam_model's derived bound), never from the library; the filter is also compared with the host reference, which
test_mimo_host.py pins to the model and to numpy.linalg.

Shapes (qm, nt, nr, R, B, b_offset, L): a single resource element; odd R with an odd offset and L = 3 -- a short last
block, rows that are no multiple of a wave; the same with L = R on 2 x 4 -- one matrix per row; receive diversity only,
with qm = 6 on one layer (an LLR run of 6 floats per RE: the 8-byte staging path); 4 x 4 with 24 LLRs per RE; the largest
order on 4 x 4 with L = 64; more than one workgroup of whole waves.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import crc_model as cm
import mimo_model as mm
import qam_model as qm_
import tb_model as tm
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
SHAPES = [(2, 1, 1, 1, 1, 0, 1), (4, 2, 2, 67, 5, 3, 3), (4, 2, 4, 67, 5, 3, 67), (6, 1, 2, 131, 2, 1, 1),
          (6, 4, 4, 33, 3, 1, 1), (8, 4, 4, 250, 3, 0, 64), (2, 2, 2, 640, 3, 0, 1)]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}
SEED = 4242
METHODS = ["maxlog", "logmap"]
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
    from nldpc.mimo import qam_llr
    f = kw.pop("f") if "f" in kw else _dev(c["f"])
    return qam_llr(f, qm, c["sigma"], nt=nt, nr=nr, L=L, seed=SEED, b_offset=off, **kw)


@shapes
def test_channels_equal_the_model_and_shard(qm, nt, nr, R, B, off, L):
    from nldpc.mimo import channels, n_blocks
    c = _case(qm, nt, nr, R, B, off, L)
    nb = n_blocks(R, L)
    assert nb == mm.n_blocks(R, L)
    kw = dict(nt=nt, nr=nr, L=L, seed=SEED)
    got = channels(B, R, b_offset=off, device=DEV, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, nb, nr, nt, 2)
    h, want = got.cpu().numpy(), c["h"]
    differ = float((h != want).mean())
    print(f"nt={nt} nr={nr} R={R} B={B} L={L}: {differ:.2e} of {h.size} components differ from the model's")
    assert np.isfinite(h).all()
    assert (np.abs(h.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert differ < 1e-4
    for k in (1, 2):
        if k < B:
            assert _same(channels(B - k, R, b_offset=off + k, device=DEV, **kw), got[k:])
    assert not _same(channels(B, R, b_offset=off, device=DEV, **dict(kw, seed=SEED + 1)), got)
    buf, view = _guarded((B, nb, nr, nt, 2), torch.float32, 777.25, 3)
    assert channels(B, R, b_offset=off, out=view, **kw).data_ptr() == view.data_ptr()
    assert _same(view, got) and _guards_intact(buf, view, 777.25, 3)


@shapes
def test_filter_equals_the_host_reference(qm, nt, nr, R, B, off, L):
    from nldpc import _lib
    from nldpc.mimo import filter as mimo_filter
    c = _case(qm, nt, nr, R, B, off, L)
    table = np.array(c["h"])
    table[B // 2, 0] = 0.0  # a zero channel among them
    W, mu, w = mimo_filter(_dev(table), c["sigma"])
    nb = table.shape[1]
    assert tuple(W.shape) == (B, nb, nt, nr, 2) and tuple(mu.shape) == tuple(w.shape) == (B, nb, nt)
    rW = np.full((B, nb, nt, nr, 2), np.nan, dtype=np.float32)
    rmu = np.full((B, nb, nt), np.nan, dtype=np.float32)
    rw = np.full((B, nb, nt), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_filter_ref(nt, nr, c["sigma"], table.ctypes.data_as(_FP), B * nb, rW.ctypes.data_as(_FP),
                                            rmu.ctypes.data_as(_FP), rw.ctypes.data_as(_FP)) == _lib.NLDPC_OK
    assert _bits_equal(W.cpu().numpy(), rW) and _bits_equal(mu.cpu().numpy(), rmu) and _bits_equal(w.cpu().numpy(), rw)
    assert not rW[B // 2, 0].any() and not rmu[B // 2, 0].any() and not rw[B // 2, 0].any()
    model = mm.filter_ordered(table, c["sigma"])
    assert _bits_equal(rW, model[0]) and _bits_equal(rmu, model[1]) and _bits_equal(rw, model[2])


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_fused_channel_equals_detect_of_its_samples_and_channels(qm, nt, nr, R, B, off, L, method):
    from nldpc.mimo import channels, detect
    c = _case(qm, nt, nr, R, B, off, L)
    llr, y, h = _run(c, qm, nt, nr, off, L, method=method, return_symbols=True, return_channels=True)
    assert llr.dtype == y.dtype == h.dtype == torch.float32
    assert tuple(llr.shape) == (B, R * nt * qm) and tuple(y.shape) == (B, R, nr, 2) and tuple(h.shape) == c["h"].shape
    unfused = detect(y, qm, c["sigma"], h, L=L, method=method)
    assert _same(llr, unfused)
    assert _same(h, channels(B, R, nt=nt, nr=nr, L=L, seed=SEED, b_offset=off, device=DEV))
    # the model on the device's own samples and channels
    y_np, h_np = y.cpu().numpy(), h.cpu().numpy()
    if method == "maxlog":
        assert _bits_equal(unfused.cpu().numpy(), mm.detect_maxlog(y_np, h_np, qm, c["sigma"], L))
    else:
        want, dmax = mm.detect_logmap64(y_np, h_np, qm, c["sigma"], L)
        bound = qm_.logmap_bound(qm, want, dmax)
        err = np.abs(unfused.cpu().numpy().astype(np.float64) - want)
        print(f"qm={qm} {nt}x{nr} R={R} B={B} L={L}: max err / bound = {(err / bound).max():.3f}, max |d*w| = {dmax.max():.4g}")
        assert (err <= bound).all()
    model = mm.received(c["f"], qm, c["sigma"], h_np, L, nt, nr, SEED, off)
    miss = float((y_np != model).mean())
    print(f"qm={qm} {nt}x{nr} R={R} B={B} L={L} {method}: {miss:.2e} of the received components differ from the model's")
    assert miss < 1e-4
    assert np.abs(y_np - model).max() <= 4 * np.spacing(np.abs(model).max())
    alone = _run(c, qm, nt, nr, off, L, method=method)
    assert isinstance(alone, torch.Tensor) and _same(alone, llr)
    two = _run(c, qm, nt, nr, off, L, method=method, return_channels=True)
    assert len(two) == 2 and _same(two[0], llr) and _same(two[1], h)


@shapes
def test_given_channels_equal_to_the_drawn_table_reproduce_the_drawn_run(qm, nt, nr, R, B, off, L):
    c = _case(qm, nt, nr, R, B, off, L)
    llr, y, h = _run(c, qm, nt, nr, off, L, method="logmap", return_symbols=True, return_channels=True)
    l2, y2, h2 = _run(c, qm, nt, nr, off, L, method="logmap", h=h.clone(), return_symbols=True, return_channels=True)
    assert _same(l2, llr) and _same(y2, y) and _same(h2, h)


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_scrambling_in_flight_equals_the_three_steps(qm, nt, nr, R, B, off, L, method):
    from nldpc.scrambling import descramble, scramble, sequence
    c = _case(qm, nt, nr, R, B, off, L)
    f = _dev(c["f"])
    for n_seq in (1, 3):
        seq = sequence(C_INITS[:n_seq], R * nt * qm, device=DEV)
        got, gy = _run(c, qm, nt, nr, off, L, method=method, scramble=seq, return_symbols=True)
        mid, my = _run(c, qm, nt, nr, off, L, f=scramble(f, seq, b_offset=off), method=method, return_symbols=True)
        assert _same(got, descramble(mid, seq, b_offset=off)) and _same(gy, my)
    plain = _run(c, qm, nt, nr, off, L, method=method)
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
def test_all_zero_word(qm, nt, nr, R, B, off, L):
    c = _case(qm, nt, nr, R, B, off, L)
    E = R * nt * qm
    zeros = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    a = _run(c, qm, nt, nr, off, L, f=None, B=B, E=E, device=DEV, return_symbols=True, return_channels=True)
    b = _run(c, qm, nt, nr, off, L, f=zeros, return_symbols=True, return_channels=True)
    assert all(_same(x, y) for x, y in zip(a, b))
    if c["f"].any():
        assert not _same(a[1], _run(c, qm, nt, nr, off, L, return_symbols=True)[1])


@pytest.mark.parametrize("method", METHODS)
@shapes
def test_a_row_of_zero_channels_has_zero_llrs(qm, nt, nr, R, B, off, L, method):
    c = _case(qm, nt, nr, R, B, off, L)
    table = _dev(c["h"])
    row = B // 2
    table[row] = 0.0
    llr = _run(c, qm, nt, nr, off, L, method=method, h=table)
    assert bool(torch.isfinite(llr).all())
    assert bool(((llr[row].view(torch.int32) & 0x7FFFFFFF) == 0).all())
    if B > 1:
        assert bool((llr[row - 1] != 0).any())


@shapes
def test_nothing_outside_the_outputs_is_written(qm, nt, nr, R, B, off, L):
    from nldpc.mimo import detect, n_blocks
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
            assert detect(y, qm, c["sigma"], h, L=L, out=llr).data_ptr() == llr.data_ptr()
            assert _same(llr, want[0]) and _guards_intact(lbuf, llr, sentinel, shift)
            assert _guards_intact(ybuf, y, sentinel, shift) and _guards_intact(hbuf, h, sentinel, shift)


def test_bad_arguments_raise_value_error():
    from nldpc.mimo import channels, detect, filter as mimo_filter, qam_llr
    B, qm, nt, nr, L = 2, 4, 2, 2, 2
    R, nb = 6, 3
    E = R * nt * qm
    f = torch.zeros((B, E), dtype=torch.uint8, device=DEV)
    y = torch.zeros((B, R, nr, 2), device=DEV)
    table = torch.ones((B, nb, nr, nt, 2), device=DEV)
    kw = dict(nt=nt, nr=nr)
    assert qam_llr(f, qm, 0.5, L=L, h=table, **kw).shape == (B, E) and detect(y, qm, 0.5, table, L=L).shape == (B, E)
    for bad_L in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, L=bad_L, **kw)
        with pytest.raises(ValueError):
            channels(B, R, L=bad_L, device=DEV, **kw)
        with pytest.raises(ValueError):
            detect(y, qm, 0.5, table, L=bad_L)
    for bad in ((2, 1), (4, 2), (3, 3), (1, 3), (0, 1), (8, 8), (True, 1), (1.5, 2)):
        with pytest.raises(ValueError):
            qam_llr(None, qm, 0.5, nt=bad[0], nr=bad[1], B=2, E=96, device=DEV)
        with pytest.raises(ValueError):
            channels(B, R, nt=bad[0], nr=bad[1], device=DEV)
    with pytest.raises(ValueError):
        qam_llr(f[:, :E - qm].contiguous(), qm, 0.5, **kw)  # an odd number of symbols on two layers
    wide = torch.ones((B, nb, nr, nt, 4), device=DEV)
    for bad in (torch.ones((B, nb + 1, nr, nt, 2), device=DEV), torch.ones((B + 1, nb, nr, nt, 2), device=DEV),
                torch.ones((B, nb, nr * nt * 2), device=DEV), table.double(), table.cpu(), wide[..., ::2],
                torch.ones((B, nb, nr, nt, 3), device=DEV), [[1.0]]):
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, L=L, h=bad, **kw)
        with pytest.raises(ValueError):
            detect(y, qm, 0.5, bad, L=L)
        if isinstance(bad, torch.Tensor):
            with pytest.raises(ValueError):
                qam_llr(f, qm, 0.5, L=L, return_channels=bad, **kw)
            with pytest.raises(ValueError):
                channels(B, R, L=L, out=bad, **kw)
    with pytest.raises(ValueError):
        qam_llr(f, qm, 0.5, L=L, h=table, return_channels=table, **kw)
    for bad in (table.cpu(), table.double(), table[..., 0], wide[..., ::2], torch.ones((B, nb, 1, 2, 2), device=DEV)):
        with pytest.raises(ValueError):
            mimo_filter(bad, 0.5)
    for bad_qm in (1, 3, 10):
        with pytest.raises(ValueError):
            qam_llr(f, bad_qm, 0.5, **kw)
        with pytest.raises(ValueError):
            detect(y, bad_qm, 0.5, table, L=L)
    for sigma in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            qam_llr(f, qm, sigma, **kw)
        with pytest.raises(ValueError):
            detect(y, qm, sigma, table, L=L)
        with pytest.raises(ValueError):
            mimo_filter(table, sigma)
    for bad in (f.cpu(), f.float(), f.reshape(-1), f[:, :-2]):
        with pytest.raises(ValueError):
            qam_llr(bad, qm, 0.5, **kw)
    for bad in (y.cpu(), y.double(), y.reshape(B, -1), y[..., :1]):
        with pytest.raises(ValueError):
            detect(bad, qm, 0.5, table, L=L)
    for more in (dict(method="exact"), dict(b_offset=-1), dict(out=torch.empty((B, E + 1), device=DEV)),
                 dict(return_symbols=torch.empty((B, R, nr, 3), device=DEV)),
                 dict(scramble=torch.zeros((1, 3), dtype=torch.int32, device=DEV))):  # (E = 48: two words per row)
        with pytest.raises(ValueError):
            qam_llr(f, qm, 0.5, **kw, **more)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, **kw)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, B=2, E=10, **kw)
    with pytest.raises(ValueError):
        qam_llr(None, qm, 0.5, B=2, E=16, device="cpu", **kw)
    with pytest.raises(ValueError):
        channels(0, R, device=DEV, **kw)
    with pytest.raises(ValueError):
        channels(B, R, b_offset=-1, device=DEV, **kw)
    # the library's own answers surface as ValueError too: h_out inside h_in, and a symbol count that nt does not divide
    from nldpc import _lib
    assert _lib.lib().nldpc_mimo_channel_llr(4, 0, 2, 2, f.data_ptr(), B, E, 0.5, 1, 0, L, table.data_ptr(), None, 0,
                                             y.data_ptr(), None, table.data_ptr() + 32, None) == _lib.NLDPC_EINVAL
    assert _lib.lib().nldpc_mimo_channel_llr(4, 0, 2, 2, f.data_ptr(), B, E - 4, 0.5, 1, 0, L, None, None, 0,
                                             y.data_ptr(), None, None, None) == _lib.NLDPC_EINVAL
    with pytest.raises(ValueError):
        _lib.check(_lib.NLDPC_EINVAL, "nldpc_mimo_channel_llr")


# ---------------------------------------------------------------- end to end: encode -> match -> 16-QAM on 2 x 2 -> recover -> decode
RES = os.path.join(ROOT, "resources")
BG2 = np.loadtxt(os.path.join(RES, "basegraph2_set0.txt"), int, delimiter="\t")
EBN0_DB = 8.5


def _neural(g, xa, T=10):
    from nldpc.decode import KIND_NEURAL, DecodeCfg, decode
    w, b = torch.full((T, g.E), 0.75, device=DEV), torch.zeros((T, g.E), device=DEV)
    outs, _, _ = decode(g, DecodeCfg(kind=KIND_NEURAL, keep_state=False), xa, T, w_cn=w, bias=b)
    return list(outs)


def test_rate_half_16qam_2x2_rayleigh_end_to_end_decodes():
    """BG2 z=16, rate 1/2 (E = 272, 24 fillers, rv0), 16-QAM log-MAP on two layers over a 2 x 2 Rayleigh channel with
    L = 1 and LMMSE detection, Neural T=10, weights 0.75, bias 0, erasures 1e-3, 8 encoded words:
    test_rate_half_16qam_rayleigh_end_to_end_decodes of test_gpu_fading.py with the MIMO channel in place of the
    single-antenna one.  Eb/N0 = 8.5 dB (sigma = mimo.sigma_for(8.5, 1/2, 4, 2)): the lowest of a 0.5 dB grid (6.0 ..
    16.0 dB, every point from 8.5 dB on qualifies) at which the CPU chain (mimo_model's channels, received samples,
    ordered filter and fp64 log-MAP rounded to fp32, ratematch_model's recovery, the oracle decoder) has no frame error
    from iteration 6 on for seeds 77, 78 and 79.  CPU frame errors per iteration, interleaver qm = 4:
       8.0 dB  77: [8, 8, 8, 8, 4, 2, 1, 0, 0, 0]  78: [8, 8, 8, 6, 5, 3, 1, 0, 0, 0]  79: [8, 8, 8, 6, 4, 2, 2, 0, 0, 0]
       8.5 dB  77: [8, 8, 8, 7, 2, 1, 0, 0, 0, 0]  78: [8, 8, 8, 5, 5, 1, 0, 0, 0, 0]  79: [8, 8, 8, 4, 4, 2, 0, 0, 0, 0]
       9.0 dB  77: [8, 8, 8, 5, 2, 0, 0, 0, 0, 0]  78: [8, 8, 8, 5, 2, 0, 0, 0, 0, 0]  79: [8, 8, 8, 4, 3, 0, 0, 0, 0, 0]
    The single-antenna Rayleigh channel needs 10.0 dB in the same setting (two receive antennas per two layers give the
    LMMSE receiver no diversity, but Eb here counts the energy at one antenna only).  The device runs seed 77."""
    from nldpc.channel import ber_counts, encode, syndrome_weight
    from nldpc.graph import LiftedGraph
    from nldpc.mimo import qam_llr, sigma_for
    from nldpc.ratematch import RateMatch, code_rate, rate_match, rate_recover
    g = LiftedGraph(BG2, 16)
    info = np.random.default_rng(5).integers(0, 2, (8, 160))
    info[:, -24:] = 0
    y = encode(g, torch.from_numpy(info).to(DEV))
    rm = RateMatch.nr5g(g, 272, rv=0, n_filler=24, qm=4)
    R = code_rate(g, rm)
    assert R == 136 / 272
    sigma = float(np.float32(sigma_for(EBN0_DB, R, 4, 2)))
    llr = qam_llr(rate_match(g, rm, y), 4, sigma, nt=2, nr=2, L=1, seed=77, method="logmap")
    xa = rate_recover(g, rm, llr, erasure_value=1e-3, filler_value=-20.0)
    outs = _neural(g, xa, 10)
    counts = ber_counts(outs, y).cpu().numpy()
    unsat = syndrome_weight(outs, g).cpu().numpy()
    print("bit / frame errors per iteration:", counts.tolist(), "unsatisfied checks:", unsat.sum(1).tolist())
    assert not counts[6:, 0].any()
    assert not unsat[6:].any()


TB_EBN0_DB = 12.0


def test_transport_block_chain_over_two_layers():
    """BG2 z=16, A = 300 (C = 3, F = 28), Btb = 4, 16-QAM on two layers over 2 x 2 Rayleigh, L = 1, G = 824:
    split_E(n_layers=2) gives E = 272, 272, 280 (multiples of n_layers qm = 8; with one layer they are 272, 276, 276), so
    every code block starts on a resource element.  segment -> encode -> rate_match_blocks(n_layers=2) -> mimo.qam_llr ->
    rate_recover_blocks(n_layers=2) -> Neural T=10 -> check(the 10 posteriors, ref_tb=tb).  Verdicts and counts are compared
    with tb_model applied to the downloaded posteriors.  Eb/N0 = 12 dB, where the CPU chain (tb_model, the generator
    matrix, ratematch_model, mimo_model with the fp64 log-MAP rounded to fp32, the oracle decoder) on the same payload
    and seed passes every TB from iteration 2 on (at 10 dB from iteration 3 on, at 8 dB from iteration 6 on): its counts
    (TB failures, undetected, TB errors, CB failures) per iteration are CPU_COUNTS.  The device's fp32 log-MAP differs
    from the model's fp64 one in the last bits, which can move a marginal block by an iteration while the decoder is
    still converging, so the counts are compared from iteration 4 on, two iterations after the CPU chain's last
    failure."""
    from nldpc.channel import encode
    from nldpc.mimo import qam_llr, sigma_for
    from nldpc.transport import TBPlan, check, rate_match_blocks, rate_recover_blocks, segment, split_E
    from nldpc.graph import LiftedGraph
    g, Btb, T, G, qm, nt = LiftedGraph(BG2, 16), 4, 10, 824, 4, 2
    plan = TBPlan.make(300, W=160, tb_crc="24A", kcb=160)
    p = tm.plan(300, "24A", 160)
    assert (plan.C, plan.F) == (3, 28)
    assert split_E(plan, G, qm, n_layers=nt) == (272, 280, 2) and tm.split_E(G, qm, 3, nt) == [272, 272, 280]
    raw = np.random.default_rng(11).integers(0, 2, (Btb, 300)).astype(np.uint8)
    info, tb = segment(plan, _dev(raw))
    tb_np = tb.cpu().numpy()
    assert np.array_equal(tb_np, cm.attach(raw, "24A")) and np.array_equal(info.cpu().numpy(), tm.segment(tb_np, p))
    y = encode(g, info)
    f = rate_match_blocks(g, plan, y, G, qm=qm, n_layers=nt)
    assert tuple(f.shape) == (Btb, G)
    sigma = float(np.float32(sigma_for(TB_EBN0_DB, 3 * plan.Kp / G, qm, nt)))
    llr = qam_llr(f, qm, sigma, nt=nt, nr=2, L=1, seed=77, method="logmap")
    xa = rate_recover_blocks(g, plan, llr, G, qm=qm, n_layers=nt, erasure_value=1e-3, filler_value=-20.0)
    assert tuple(xa.shape) == (3 * Btb, g.N, g.Z)
    outs = _neural(g, xa, T)
    res = check(plan, outs, ref_tb=tb, counts=True, tb_out=True)
    for t, o in enumerate(outs):
        cb_want, tb_want, out_want, cnt_want = tm.check((o.cpu().numpy() > 0).astype(np.uint8), p, tb_np)
        assert np.array_equal(res.cb_ok[t].cpu().numpy(), cb_want.astype(np.uint8)), t
        assert np.array_equal(res.tb_ok[t].cpu().numpy(), tb_want.astype(np.uint8)), t
        assert np.array_equal(res.tb_out[t].cpu().numpy(), out_want), t
        assert np.array_equal(res.counts[t].cpu().numpy(), cnt_want), t
    print("(TB failures, undetected, TB errors, CB failures) per iteration:", res.counts.cpu().tolist())
    assert res.counts[4:].cpu().tolist() == CPU_COUNTS[4:]


CPU_COUNTS = [[4, 0, 4, 12], [4, 0, 4, 5]] + [[0, 0, 0, 0]] * 8
