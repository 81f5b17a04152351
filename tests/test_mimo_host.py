"""The MIMO detector's arithmetic on the host (nldpc_mimo_entry_ref, nldpc_mimo_filter_ref, nldpc_mimo_detect_ref;
csrc/nldpc_mimo.h is what the kernels run) and the argument rules of all seven entry points, without a GPU.  Expected
values come from mimo_model.py: (a) the float64 / float32 restatement in the order include/nldpc.h states, which the
library equals bit for bit wherever no log / cos / sin is involved, and (b) an independent numpy.linalg LMMSE.

Against (b), and for the drawn entries against the model's (glibc's and numpy's log / cos / sin differ by a few double
ulps), a value is a chain of double operations rounded to fp32 once: the one rounding can land on the neighbouring fp32
value, never further, and the share that differs at all stays below 1e-4, the project's cap for such chains
(test_fading_host.py).  Log-MAP is held to qam_model.logmap_bound, which carries over unchanged (mimo_model's
docstring), and the single-antenna detector to mimo_model.siso_bound of the fading channel's demapper.
"""
import ctypes
import functools

import numpy as np
import pytest

import fading_model as fm
import mimo_model as mm
import qam_model as qm_

_FP = ctypes.POINTER(ctypes.c_float)
_UP = ctypes.POINTER(ctypes.c_uint32)
SEED = 4242
# (nt, nr, sigma): 3000 Rayleigh draws each; the condition number of G reaches 1.3e4
FILTER_CASES = [(1, 1, 0.5), (2, 2, 0.25), (2, 4, 0.12), (4, 4, 0.25), (4, 4, 0.06), (4, 4, 0.01)]
N_DRAWS = 3000
N_ENTRIES = 2 ** 18
# (qm, nt, nr): every order, every pair
DETECT_CASES = [(2, 1, 1), (4, 1, 2), (6, 1, 4), (8, 2, 2), (4, 2, 4), (6, 4, 4), (8, 4, 4), (2, 4, 4)]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}


def _fp(a):
    return a.ctypes.data_as(_FP)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def _filter_ref(h, sigma):
    from nldpc import _lib
    h = np.ascontiguousarray(h, dtype=np.float32)
    n, nr, nt = h.shape[0], h.shape[-3], h.shape[-2]
    W = np.full((n, nt, nr, 2), np.nan, dtype=np.float32)
    mu = np.full((n, nt), np.nan, dtype=np.float32)
    w = np.full((n, nt), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_filter_ref(nt, nr, sigma, _fp(h), n, _fp(W), _fp(mu), _fp(w)) == _lib.NLDPC_OK
    return W, mu, w


def _detect_ref(qm, method, sigma, y, h, L):
    from nldpc import _lib
    y = np.ascontiguousarray(y, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    B, R, nr = y.shape[:3]
    nt = h.shape[-2]
    llr = np.full((B, R * nt * qm), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_detect_ref(qm, method, nt, nr, sigma, _fp(y), _fp(h), B, R, L, _fp(llr)) == _lib.NLDPC_OK
    return llr


@functools.lru_cache(maxsize=None)
def _draws(nt, nr):
    h = mm.channels(N_DRAWS, 1, 1, nt, nr, SEED)[:, 0]
    h.setflags(write=False)
    return h


@pytest.mark.parametrize("nt,nr,sigma", FILTER_CASES)
def test_filter_ref_is_bit_identical_to_the_ordered_model(nt, nr, sigma):
    h = _draws(nt, nr)
    got, want = _filter_ref(h, sigma), mm.filter_ordered(h, sigma)
    for g, m in zip(got, want):
        assert g.dtype == m.dtype == np.float32 and np.isfinite(g).all() and _bits_equal(g, m)
    assert (got[1] > 0).all() and (got[1] < 1).all() and (got[2] > 0).all()


@pytest.mark.parametrize("nt,nr,sigma", FILTER_CASES)
def test_filter_ref_is_within_one_ulp_of_numpy_linalg(nt, nr, sigma):
    h = _draws(nt, nr)
    H = h[..., 0].astype(np.float64) + 1j * h[..., 1]
    G = np.conj(np.swapaxes(H, -1, -2)) @ H + 2.0 * np.float64(np.float32(sigma)) ** 2 * np.eye(nt)
    print(f"nt={nt} nr={nr} sigma={sigma}: cond(G) up to {np.linalg.cond(G).max():.3g}")
    for name, g, m in zip(("W", "mu", "w"), _filter_ref(h, sigma), mm.filter_linalg(h, sigma)):
        differ = float((g != m).mean())
        print(f"  {name}: {differ:.2e} of {g.size} values differ from numpy.linalg's")
        assert (np.abs(g.astype(np.float64) - m.astype(np.float64)) <= np.spacing(np.abs(m))).all(), name
        assert differ < 1e-4, name


def test_filter_of_special_channels():
    # a zero channel: W = 0, mu = 0 exactly and w = 0 by the rule (mu e is zero); a huge one stays finite
    for nt, nr in mm.DIMS:
        W, mu, w = _filter_ref(np.zeros((2, nr, nt, 2), dtype=np.float32), 0.3)
        assert not W.any() and not mu.any() and not w.any()
        h = np.zeros((1, nr, nt, 2), dtype=np.float32)
        for t in range(nt):
            h[0, t, t, 0] = 1e18
        got, want = _filter_ref(h, 0.3), mm.filter_ordered(h, 0.3)
        assert all(_bits_equal(g, m) and np.isfinite(g).all() for g, m in zip(got, want))
    # one layer of two has no path: its LLR weight is 0, the other layer is the single-antenna filter
    h = np.zeros((1, 2, 2, 2), dtype=np.float32)
    h[0, 0, 0] = (0.6, -0.8)
    W, mu, w = _filter_ref(h, 0.25)
    assert mu[0, 1] == 0 and w[0, 1] == 0 and not W[0, 1].any() and 0 < mu[0, 0] < 1 and w[0, 0] > 0


@functools.lru_cache(maxsize=None)
def _entry_words():
    w = mm.block_words(np.arange(N_ENTRIES // 16, dtype=np.int64), 4, 4, SEED).reshape(-1, 2)
    w = np.ascontiguousarray(w)
    w.setflags(write=False)
    return w


def _entry_ref(nt):
    from nldpc import _lib
    w = _entry_words()
    h = np.full((len(w), 2), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_entry_ref(nt, w.ctypes.data_as(_UP), len(w), _fp(h)) == _lib.NLDPC_OK
    return h


@pytest.mark.parametrize("nt", (1, 2, 4))
def test_entry_ref_is_within_one_ulp_of_the_model_and_has_the_stated_energy(nt):
    w = _entry_words()
    assert len(w) == N_ENTRIES
    got, want = _entry_ref(nt), mm.entry_of_words(nt, w[:, 0], w[:, 1])
    assert got.dtype == want.dtype == np.float32 and np.isfinite(got).all()
    differ = float((got != want).mean())
    print(f"nt={nt}: {differ:.2e} of {got.size} components differ from the model's")
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()
    assert differ < 1e-4
    # |h|^2 is exponential with mean 1 / nt: the standard error of the mean over n entries is (1 / nt) / sqrt(n)
    p = (got.astype(np.float64) ** 2).sum(axis=1)
    print(f"nt={nt}: mean |h|^2 = {p.mean():.6f} (1 / nt = {1 / nt})")
    assert abs(p.mean() - 1.0 / nt) <= 5.0 * (1.0 / nt) / np.sqrt(len(p))
    assert abs(got.astype(np.float64).mean()) <= 5.0 * np.sqrt(0.5 / nt / got.size)


@functools.lru_cache(maxsize=None)
def _case(qm, nt, nr):
    """B = 3 rows of R = 11 resource elements in blocks of L = 4 (a short last block): drawn channels with one zero
    block, received samples of random bits plus samples far outside"""
    B, R, L, sigma = 3, 11, 4, SIGMA[qm]
    rng = np.random.default_rng(100 * qm + 10 * nt + nr)
    f = rng.integers(0, 2, (B, R * nt * qm)).astype(np.uint8)
    table = np.array(mm.channels(B, R, L, nt, nr, SEED))
    table[1, 1] = 0.0
    y = np.array(mm.received(f, qm, sigma, table, L, nt, nr, SEED))
    y[2, -2:, 0] = [(4, -4), (-100, 1000)]
    c = dict(B=B, R=R, L=L, sigma=float(np.float32(sigma)), table=table, y=y)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("qm,nt,nr", DETECT_CASES)
def test_maxlog_detect_ref_is_bit_identical_to_the_ordered_model(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _detect_ref(qm, 0, c["sigma"], c["y"], c["table"], c["L"])
    want = mm.detect_maxlog(c["y"], c["table"], qm, c["sigma"], c["L"])
    assert np.isfinite(got).all() and _bits_equal(got, want)
    # the zero block gives +-0, its neighbours do not
    per = got.reshape(c["B"], c["R"], nt * qm)
    assert ((per[1, 4:8].view(np.uint32) & 0x7FFFFFFF) == 0).all() and per[1, :4].any() and per[1, 8:].any()


@pytest.mark.parametrize("qm,nt,nr", DETECT_CASES)
def test_logmap_detect_ref_is_within_the_derived_bound_of_the_fp64_model(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _detect_ref(qm, 1, c["sigma"], c["y"], c["table"], c["L"])
    want, dmax = mm.detect_logmap64(c["y"], c["table"], qm, c["sigma"], c["L"])
    bound = qm_.logmap_bound(qm, want, dmax)
    err = np.abs(got.astype(np.float64) - want)
    print(f"qm={qm} nt={nt} nr={nr}: max err / bound = {(err / bound).max():.3f}, max |d*w| = {dmax.max():.4g}")
    assert np.isfinite(got).all() and (err <= bound).all()
    per = got.reshape(c["B"], c["R"], nt * qm)
    assert ((per[1, 4:8].view(np.uint32) & 0x7FFFFFFF) == 0).all()


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("qm,nt,nr", DETECT_CASES)
def test_a_zero_channel_gives_zero_llrs(qm, nt, nr, method):
    c = _case(qm, nt, nr)
    got = _detect_ref(qm, method, c["sigma"], c["y"], np.zeros_like(c["table"]), c["L"])
    assert ((got.view(np.uint32) & 0x7FFFFFFF) == 0).all()


@pytest.mark.parametrize("qm", (2, 4, 6, 8))
def test_single_antenna_real_channel_is_the_fading_demapper(qm):
    """nt = nr = 1, h = g real: the detector against fading_model.maxlog_csi within mimo_model.siso_bound"""
    B, S, L, sigma = 3, 41, 4, SIGMA[qm]
    rng = np.random.default_rng(qm)
    f = rng.integers(0, 2, (B, S * qm)).astype(np.uint8)
    gains = np.array(fm.gains(B, S, L, 0.0, SEED))
    gains[0, 1], gains[1, 2] = 0.0, 1.0
    sym = fm.faded_symbols(f, qm, sigma, gains, L, SEED)
    table = np.zeros((B, gains.shape[1], 1, 1, 2), dtype=np.float32)
    table[..., 0, 0, 0] = gains
    got = _detect_ref(qm, 0, sigma, sym.reshape(B, S, 1, 2), table, L).astype(np.float64)
    g = fm.symbol_gains(gains, S, L)
    want = fm.maxlog_csi(sym, qm, sigma, g).astype(np.float64)
    bound = mm.siso_bound(sym, qm, sigma, g)
    err = np.abs(got - want)
    print(f"qm={qm}: max err = {err.max():.3g}, max bound = {bound.max():.3g}, max err / bound = "
          f"{(err / np.maximum(bound, 1e-300)).max():.3f}, max |LLR| = {np.abs(want).max():.4g}")
    assert (err <= bound).all()
    # the blocks of gain 0 and 1: +-0 on both sides, and nothing special
    per = got.reshape(B, S, qm)
    assert not per[0, 4:8].any() and per[1, 8:12].any()


def test_block_structure():
    # the last block of a row may be short and blocks never span rows: row b, RE i uses table[b, i // L]
    qm, nt, nr, B, R, L, sigma = 4, 2, 2, 2, 7, 3, 0.3
    rng = np.random.default_rng(1)
    y = np.tile(rng.normal(size=(1, 1, nr, 2)).astype(np.float32), (B, R, 1, 1))
    table = mm.channels(B, R, L, nt, nr, SEED)
    got = _detect_ref(qm, 0, sigma, y, table, L).reshape(B, R, nt * qm)
    for b in range(B):
        for i in range(R):
            one = _detect_ref(qm, 0, sigma, y[:1, :1], table[b:b + 1, i // L:i // L + 1], 1)
            assert _bits_equal(got[b, i], one.reshape(-1)), (b, i)
    big = _detect_ref(qm, 0, sigma, y, table[:, :1], R + 5)
    assert _bits_equal(big, _detect_ref(qm, 0, sigma, y, table[:, :1], R))
    assert mm.n_blocks(R, L) == 3 and mm.block_index(R, L).tolist() == [0, 0, 0, 1, 1, 1, 2]


def test_host_calls_reject_bad_arguments():
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL, OK = _lib.NLDPC_EINVAL, _lib.NLDPC_OK
    w = np.zeros((4, 2), dtype=np.uint32)
    buf = np.zeros(256, dtype=np.float32)
    wp, p = w.ctypes.data_as(_UP), _fp(buf)
    assert lib.nldpc_mimo_entry_ref(2, wp, 4, p) == OK
    for nt in (0, 3, 8, -1):
        assert lib.nldpc_mimo_entry_ref(nt, wp, 4, p) == EINVAL
    for n in (0, -1):
        assert lib.nldpc_mimo_entry_ref(2, wp, n, p) == EINVAL
    assert lib.nldpc_mimo_entry_ref(2, None, 4, p) == EINVAL and lib.nldpc_mimo_entry_ref(2, wp, 4, None) == EINVAL
    assert b"nldpc_mimo_entry_ref" in lib.nldpc_last_error()
    assert lib.nldpc_mimo_filter_ref(2, 2, 0.5, p, 2, p, p, p) == OK
    for nt, nr in ((2, 1), (4, 2), (3, 3), (1, 3), (0, 1), (8, 8), (1, 8)):
        assert lib.nldpc_mimo_filter_ref(nt, nr, 0.5, p, 2, p, p, p) == EINVAL, (nt, nr)
    for sigma in (0.0, -1.0, float("nan")):
        assert lib.nldpc_mimo_filter_ref(2, 2, sigma, p, 2, p, p, p) == EINVAL
    for n in (0, -1):
        assert lib.nldpc_mimo_filter_ref(2, 2, 0.5, p, n, p, p, p) == EINVAL
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.nldpc_mimo_filter_ref(2, 2, 0.5, args[0], 2, *args[1:]) == EINVAL
    assert b"nldpc_mimo_filter_ref" in lib.nldpc_last_error()
    assert lib.nldpc_mimo_detect_ref(4, 0, 2, 2, 1.0, p, p, 2, 4, 1, p) == OK
    for qm in (0, 1, 3, 10, -2):
        assert lib.nldpc_mimo_detect_ref(qm, 0, 2, 2, 1.0, p, p, 2, 4, 1, p) == EINVAL
    for method in (-1, 2):
        assert lib.nldpc_mimo_detect_ref(4, method, 2, 2, 1.0, p, p, 2, 4, 1, p) == EINVAL
    for sigma in (0.0, -1.0, float("nan")):
        assert lib.nldpc_mimo_detect_ref(4, 0, 2, 2, sigma, p, p, 2, 4, 1, p) == EINVAL
    for nt, nr in ((2, 1), (4, 2), (3, 3)):
        assert lib.nldpc_mimo_detect_ref(4, 0, nt, nr, 1.0, p, p, 2, 4, 1, p) == EINVAL
    for B, R, L in ((0, 4, 1), (-1, 4, 1), (2, 0, 1), (2, -4, 1), (2, 4, 0), (2, 4, -1), (2, 2 ** 28, 1), (2 ** 20, 2 ** 11, 1)):
        assert lib.nldpc_mimo_detect_ref(4, 0, 2, 2, 1.0, p, p, B, R, L, p) == EINVAL, (B, R, L)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.nldpc_mimo_detect_ref(4, 0, 2, 2, 1.0, args[0], args[1], 2, 4, 1, args[2]) == EINVAL
    assert b"nldpc_mimo_detect_ref" in lib.nldpc_last_error()


# (qm, method, nt, nr, B, E, sigma, L): the rules of the device calls are checked on the host before anything is launched
BAD = {
    "qm_1": (1, 0, 2, 2, 2, 8, 1.0, 1), "qm_3": (3, 0, 1, 1, 2, 9, 1.0, 1), "method_2": (4, 2, 2, 2, 2, 8, 1.0, 1),
    "nt_3": (4, 0, 3, 4, 2, 24, 1.0, 1), "nr_below_nt": (4, 0, 2, 1, 2, 8, 1.0, 1), "nr_8": (4, 0, 4, 8, 2, 16, 1.0, 1),
    "nt_0": (4, 0, 0, 1, 2, 8, 1.0, 1),
    "E_not_multiple_of_qm": (4, 0, 2, 2, 2, 10, 1.0, 1), "S_not_multiple_of_nt": (4, 0, 2, 2, 2, 12, 1.0, 1),
    "S_not_multiple_of_4": (2, 0, 4, 4, 2, 12, 1.0, 1), "E_zero": (4, 0, 2, 2, 2, 0, 1.0, 1),
    "E_2_31": (4, 0, 2, 2, 2, 2 ** 31, 1.0, 1), "B_zero": (4, 0, 2, 2, 0, 8, 1.0, 1),
    "sigma_zero": (4, 0, 2, 2, 2, 8, 0.0, 1), "sigma_nan": (4, 0, 2, 2, 2, 8, float("nan"), 1),
    "L_zero": (4, 0, 2, 2, 2, 8, 1.0, 0), "L_negative": (4, 0, 2, 2, 2, 8, 1.0, -3),
    "blocks_2_31": (2, 0, 1, 1, 2 ** 20, 2 ** 12, 1.0, 1),
}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_device_calls_reject_bad_arguments_on_the_host(rule):
    """every rule is refused before a launch: the pointers are (aligned) host addresses that no kernel ever sees"""
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    qm, method, nt, nr, B, E, sigma, L = BAD[rule]
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    out = p + 8192
    for h_in in (None, p):
        for seq in (None, p):
            assert lib.nldpc_mimo_channel_llr(qm, method, nt, nr, None, B, E, sigma, 1, 0, L, h_in, seq, 1, out, out, out,
                                              None) == EINVAL
    if not rule.startswith(("E_not", "S_not", "E_2_31")):
        R = max(E // max(qm, 1) // max(nt, 1), 0)
        assert lib.nldpc_mimo_detect(qm, method, nt, nr, sigma, p, p, B, R, L, p, None) == EINVAL
    if rule.startswith(("nt_", "nr_", "B_zero", "blocks", "sigma")):
        n_blk = max(E // max(qm, 1) // max(nt, 1), 1)
        assert lib.nldpc_mimo_filter(nt, nr, sigma, p, B, n_blk, p, p, p, None) == EINVAL
    if rule.startswith(("nt_", "nr_", "B_zero", "blocks")):
        assert lib.nldpc_mimo_channels(nt, nr, 1, B, max(E // max(qm, 1) // max(nt, 1), 1), 0, p, None) == EINVAL


def test_null_misaligned_and_overlapping_pointers_are_rejected():
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    assert lib.nldpc_mimo_channels(2, 2, 1, 2, 2, 0, None, None) == EINVAL
    assert lib.nldpc_mimo_channels(2, 2, 1, 2, 2, 0, p + 2, None) == EINVAL
    assert lib.nldpc_mimo_channels(2, 2, 1, 2, 0, 0, p, None) == EINVAL
    assert lib.nldpc_mimo_channels(2, 2, 1, 2, 2, -1, p, None) == EINVAL
    assert b"nldpc_mimo_channels" in lib.nldpc_last_error()
    for h, W, mu, w in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None), (p + 1, p, p, p),
                        (p, p + 2, p, p), (p, p, p + 3, p), (p, p, p, p + 2)):
        assert lib.nldpc_mimo_filter(2, 2, 0.5, h, 2, 2, W, mu, w, None) == EINVAL
    assert lib.nldpc_mimo_filter(2, 2, 0.5, p, 2, 0, p, p, p, None) == EINVAL
    assert b"nldpc_mimo_filter" in lib.nldpc_last_error()
    for y, h, llr in ((None, p, p), (p, None, p), (p, p, None), (p + 1, p, p), (p, p + 2, p), (p, p, p + 3)):
        assert lib.nldpc_mimo_detect(4, 0, 2, 2, 1.0, y, h, 2, 2, 1, llr, None) == EINVAL
    assert b"nldpc_mimo_detect" in lib.nldpc_last_error()

    # B = 2 rows of E = 16 bits of 16-QAM on 2 layers: R = 2, L = 1: 4 blocks of 2 x 2 x 2 floats = 128 bytes
    def fused(h_in=None, seq=None, n_seq=1, llr=p, sym=None, h_out=None, b_offset=0):
        return lib.nldpc_mimo_channel_llr(4, 0, 2, 2, None, 2, 16, 1.0, 1, b_offset, 1, h_in, seq, n_seq, llr, sym, h_out,
                                          None)
    assert fused(llr=None) == EINVAL
    assert fused(llr=p + 2) == EINVAL
    assert fused(sym=p + 1) == EINVAL
    assert fused(h_in=p + 2) == EINVAL
    assert fused(h_out=p + 2) == EINVAL
    assert fused(seq=p + 2) == EINVAL
    assert fused(seq=p, n_seq=0) == EINVAL
    assert fused(b_offset=-1) == EINVAL
    for shift in (0, 4, 124, -124):  # h_out inside, or partly inside, h_in
        assert fused(h_in=p + 1024, h_out=p + 1024 + shift) == EINVAL
    assert b"overlap" in lib.nldpc_last_error()
    assert b"nldpc_mimo_channel_llr" in lib.nldpc_last_error()


def test_python_helpers():
    from nldpc.mimo import n_blocks, sigma_for
    from nldpc.modulation import sigma_for as siso_sigma
    assert [n_blocks(67, L) for L in (1, 3, 66, 67, 68, 10 ** 12)] == [67, 23, 2, 1, 1, 1]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            n_blocks(67, bad)
    with pytest.raises(ValueError):
        n_blocks(0, 1)
    assert sigma_for(7.0, 0.5, 4, 1) == siso_sigma(7.0, 0.5, 4)
    assert sigma_for(7.0, 0.5, 4, 2) == siso_sigma(7.0, 0.5, 8) and sigma_for(7.0, 0.5, 2, 4) == siso_sigma(7.0, 0.5, 8)
