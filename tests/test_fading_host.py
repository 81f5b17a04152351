"""The flat-fading channel's arithmetic on the host (nldpc_fading_gain_ref, nldpc_qam_demap_csi_ref; csrc/nldpc_fading.h
is what the kernels run) and the argument rules of all five entry points, without a GPU.  Expected values come from
fading_model.py (the gain formula in double on oracle.philox's words, the fp32 max-log and the fp64 log-MAP on the
scaled levels), never from the library.

A gain is a chain of double operations rounded to fp32 once: two evaluations (glibc's and numpy's log / cos / sin)
differ by a few double ulps, and the one rounding to fp32 can then land on the neighbouring value, never further -- so
every value is within 1 fp32 ulp and the share that differs at all stays below 1e-4, the cap test_gpu_modulation.py
uses for the noisy symbols (the same kind of arithmetic).  Log-MAP is held to qam_model.logmap_bound, which carries
over unchanged (fading_model's docstring).
"""
import ctypes
import functools

import numpy as np
import pytest

import fading_model as fm
import qam_model as qm_

ORDERS = (2, 4, 6, 8)
KS = (0.0, 1.0, 10.0)
_FP = ctypes.POINTER(ctypes.c_float)
_UP = ctypes.POINTER(ctypes.c_uint32)
N_GAINS = 2 ** 18
SEED = 4242


def _fp(a):
    return a.ctypes.data_as(_FP)


@functools.lru_cache(maxsize=None)
def _words():
    w = np.ascontiguousarray(fm.block_words(N_GAINS, SEED))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _gain_ref(K):
    from nldpc import _lib
    w = _words()
    g = np.full(len(w), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_fading_gain_ref(K, w.ctypes.data_as(_UP), len(w), _fp(g)) == _lib.NLDPC_OK
    g.setflags(write=False)
    return g


def _demap_csi_ref(qm, method, sigma, sym, gain, L):
    from nldpc import _lib
    sym = np.ascontiguousarray(sym, dtype=np.float32)
    gain = np.ascontiguousarray(gain, dtype=np.float32)
    B, S = sym.shape[:2]
    llr = np.full((B, S * qm), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_qam_demap_csi_ref(qm, method, sigma, _fp(sym), _fp(gain), B, S, L, _fp(llr)) == _lib.NLDPC_OK
    return llr


@pytest.mark.parametrize("K", KS)
def test_gain_ref_is_within_one_ulp_of_the_model(K):
    w = _words()
    got, want = _gain_ref(K), fm.gain_of_words(K, w[:, 0], w[:, 1])
    assert got.dtype == want.dtype == np.float32 and np.isfinite(got).all() and (got >= 0).all()
    differ = float((got != want).mean())
    print(f"K={K}: {differ:.2e} of {got.size} gains differ from the model's")
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want)).all()
    assert differ < 1e-4


@pytest.mark.parametrize("K", KS)
def test_gain_statistics(K):
    """Var(g^2) = (1 + 2K) / (1 + K)^2 <= 1: the standard error of the mean over 2^18 gains is at most 2^-9 ~ 0.002, and
    0.01 is five of them"""
    g2 = _gain_ref(K).astype(np.float64) ** 2
    print(f"K={K}: mean g^2 = {g2.mean():.5f}, var g^2 = {g2.var():.4f} (model {(1 + 2 * K) / (1 + K) ** 2:.4f})")
    assert abs(g2.mean() - 1.0) < 0.01


def test_rician_tends_to_a_constant_gain():
    # sanity of the formula's direction: a large K leaves almost no fading
    g = _gain_ref(1e6)
    assert np.abs(g - 1.0).max() < 0.01


@functools.lru_cache(maxsize=None)
def _case(qm):
    """B = 3 rows of S = 41 symbols in blocks of L = 4 (a short last block), gains from the model with one exact 0 and one
    exact 1; symbols faded and noisy, plus points far outside"""
    B, S, L, sigma = 3, 41, 4, {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}[qm]
    rng = np.random.default_rng(qm)
    f = rng.integers(0, 2, (B, S * qm)).astype(np.uint8)
    table = np.array(fm.gains(B, S, L, 0.0, SEED))
    table[0, 1], table[1, 2] = 0.0, 1.0
    sym = np.array(fm.faded_symbols(f, qm, sigma, table, L, SEED))
    sym[2, -3:] = [(4, -4), (-100, 100), (1000, 0.1)]
    c = dict(B=B, S=S, L=L, sigma=float(np.float32(sigma)), table=table, sym=sym, g=fm.symbol_gains(table, S, L))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("qm", ORDERS)
def test_maxlog_csi_ref_is_bit_identical_to_the_fp32_model(qm):
    c = _case(qm)
    got = _demap_csi_ref(qm, 0, c["sigma"], c["sym"], c["table"], c["L"])
    want = fm.maxlog_csi(c["sym"], qm, c["sigma"], c["g"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("qm", ORDERS)
def test_logmap_csi_ref_is_within_the_derived_bound_of_the_fp64_model(qm):
    c = _case(qm)
    got = _demap_csi_ref(qm, 1, c["sigma"], c["sym"], c["table"], c["L"]).astype(np.float64)
    want, dmax = fm.logmap64_csi(c["sym"], qm, c["sigma"], c["g"])
    bound = qm_.logmap_bound(qm, want, dmax)
    err = np.abs(got - want)
    print(f"qm={qm}: max err / bound = {(err / bound).max():.3f}, max |d*w| = {dmax.max():.4g}")
    assert np.isfinite(got).all() and (err <= bound).all()


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("qm", ORDERS)
def test_unit_gain_is_the_awgn_demapper_and_zero_gain_gives_zero(qm, method):
    from nldpc import _lib
    c = _case(qm)
    B, S = c["B"], c["S"]
    for L in (1, 4, S, S + 5):
        nb = fm.n_blocks(S, min(L, S))
        ones = _demap_csi_ref(qm, method, c["sigma"], c["sym"], np.ones((B, nb), dtype=np.float32), L)
        awgn = np.full(B * S * qm, np.nan, dtype=np.float32)
        sym = np.ascontiguousarray(c["sym"])
        assert _lib.lib().nldpc_qam_demap_ref(qm, method, c["sigma"], _fp(sym), B * S, _fp(awgn)) == _lib.NLDPC_OK
        assert np.array_equal(ones.reshape(-1).view(np.uint32), awgn.view(np.uint32))
        zeros = _demap_csi_ref(qm, method, c["sigma"], c["sym"], np.zeros((B, nb), dtype=np.float32), L)
        assert ((zeros.view(np.uint32) & 0x7FFFFFFF) == 0).all()
    # and inside a table: the block with gain 0 gives +-0, the block with gain 1 the AWGN demapper's values
    got = _demap_csi_ref(qm, method, c["sigma"], c["sym"], c["table"], c["L"]).reshape(B, S, qm)
    assert ((got[0, 4:8].view(np.uint32) & 0x7FFFFFFF) == 0).all()
    assert np.array_equal(got[1, 8:12].view(np.uint32), awgn.reshape(B, S, qm)[1, 8:12].view(np.uint32))


def test_block_structure():
    # the last block of a row may be short and blocks never span rows: row b symbol j uses table[b, j // L]
    qm, B, S, L, sigma = 4, 2, 7, 3, 0.3
    sym = np.tile(np.array([[0.3, -0.2]], dtype=np.float32), (B, S, 1))
    table = np.arange(1, 1 + B * 3, dtype=np.float32).reshape(B, 3) / 4
    got = _demap_csi_ref(qm, 0, sigma, sym, table, L).reshape(B, S, qm)
    for b in range(B):
        for j in range(S):
            one = _demap_csi_ref(qm, 0, sigma, sym[:1, :1], table[b:b + 1, j // L:j // L + 1], 1)
            assert np.array_equal(got[b, j].view(np.uint32), one.reshape(-1).view(np.uint32)), (b, j)
    assert fm.n_blocks(S, L) == 3 and fm.block_index(S, L).tolist() == [0, 0, 0, 1, 1, 1, 2]


def test_host_calls_reject_bad_arguments():
    from nldpc import _lib
    L = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    w = np.zeros((4, 2), dtype=np.uint32)
    g = np.zeros(4, dtype=np.float32)
    wp = w.ctypes.data_as(_UP)
    assert L.nldpc_fading_gain_ref(0.0, wp, 4, _fp(g)) == _lib.NLDPC_OK
    for K in (-1.0, -1e-300, float("nan"), float("inf")):
        assert L.nldpc_fading_gain_ref(K, wp, 4, _fp(g)) == EINVAL
    for n in (0, -1):
        assert L.nldpc_fading_gain_ref(0.0, wp, n, _fp(g)) == EINVAL
    assert L.nldpc_fading_gain_ref(0.0, None, 4, _fp(g)) == EINVAL
    assert L.nldpc_fading_gain_ref(0.0, wp, 4, None) == EINVAL
    assert b"nldpc_fading_gain_ref" in L.nldpc_last_error()
    sym = np.zeros((2, 4, 2), dtype=np.float32)
    gain = np.ones((2, 4), dtype=np.float32)
    llr = np.zeros(2 * 4 * 8, dtype=np.float32)
    assert L.nldpc_qam_demap_csi_ref(4, 0, 1.0, _fp(sym), _fp(gain), 2, 4, 1, _fp(llr)) == _lib.NLDPC_OK
    for qm in (0, 1, 3, 10, -2):
        assert L.nldpc_qam_demap_csi_ref(qm, 0, 1.0, _fp(sym), _fp(gain), 2, 4, 1, _fp(llr)) == EINVAL
    for method in (-1, 2):
        assert L.nldpc_qam_demap_csi_ref(4, method, 1.0, _fp(sym), _fp(gain), 2, 4, 1, _fp(llr)) == EINVAL
    for sigma in (0.0, -1.0, float("nan")):
        assert L.nldpc_qam_demap_csi_ref(4, 0, sigma, _fp(sym), _fp(gain), 2, 4, 1, _fp(llr)) == EINVAL
    for B, S, Lc in ((0, 4, 1), (-1, 4, 1), (2, 0, 1), (2, -4, 1), (2, 4, 0), (2, 4, -1), (2, 2 ** 29, 1),
                     (2 ** 20, 2 ** 11, 1)):
        assert L.nldpc_qam_demap_csi_ref(4, 0, 1.0, _fp(sym), _fp(gain), B, S, Lc, _fp(llr)) == EINVAL, (B, S, Lc)
    assert L.nldpc_qam_demap_csi_ref(4, 0, 1.0, None, _fp(gain), 2, 4, 1, _fp(llr)) == EINVAL
    assert L.nldpc_qam_demap_csi_ref(4, 0, 1.0, _fp(sym), None, 2, 4, 1, _fp(llr)) == EINVAL
    assert L.nldpc_qam_demap_csi_ref(4, 0, 1.0, _fp(sym), _fp(gain), 2, 4, 1, None) == EINVAL
    assert b"nldpc_qam_demap_csi_ref" in L.nldpc_last_error()


# (qm, method, B, E, sigma, L, K): the rules of the device calls are checked on the host before anything is launched
BAD = {
    "qm_1": (1, 0, 2, 8, 1.0, 1, 0.0), "qm_3": (3, 0, 2, 9, 1.0, 1, 0.0), "method_2": (4, 2, 2, 8, 1.0, 1, 0.0),
    "E_not_multiple": (4, 0, 2, 10, 1.0, 1, 0.0), "E_zero": (4, 0, 2, 0, 1.0, 1, 0.0), "E_2_31": (4, 0, 2, 2 ** 31, 1.0, 1, 0.0),
    "B_zero": (4, 0, 0, 8, 1.0, 1, 0.0), "sigma_zero": (4, 0, 2, 8, 0.0, 1, 0.0), "sigma_nan": (4, 0, 2, 8, float("nan"), 1, 0.0),
    "L_zero": (4, 0, 2, 8, 1.0, 0, 0.0), "L_negative": (4, 0, 2, 8, 1.0, -3, 0.0),
    "K_negative": (4, 0, 2, 8, 1.0, 1, -0.5), "K_nan": (4, 0, 2, 8, 1.0, 1, float("nan")), "K_inf": (4, 0, 2, 8, 1.0, 1, float("inf")),
    "blocks_2_31": (4, 0, 2 ** 20, 2 ** 13, 1.0, 1, 0.0),
}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_device_calls_reject_bad_arguments_on_the_host(rule):
    """every rule is refused before a launch: the pointers are (aligned) host addresses that no kernel ever sees"""
    from nldpc import _lib
    lib = _lib.lib()
    qm, method, B, E, sigma, L, K = BAD[rule]
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    for gain_in in (None, p):
        for seq in (None, p):
            assert lib.nldpc_qam_fading_channel_llr(qm, method, None, B, E, sigma, 1, 0, L, K, gain_in, seq, 1, p, p, p,
                                                    None) == _lib.NLDPC_EINVAL
    if not rule.startswith(("K_", "E_not")):
        S = E // qm if E % qm == 0 else E
        assert lib.nldpc_qam_demap_csi(qm, method, sigma, p, p, B, S, L, p, None) == _lib.NLDPC_EINVAL
    if rule.startswith(("K_", "B_zero", "blocks")):
        assert lib.nldpc_fading_gains(K, 1, B, max(E // qm, 1), 0, p, None) == _lib.NLDPC_EINVAL


def test_null_and_misaligned_pointers_are_rejected():
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    assert lib.nldpc_fading_gains(0.0, 1, 2, 2, 0, None, None) == EINVAL
    assert lib.nldpc_fading_gains(0.0, 1, 2, 2, 0, p + 2, None) == EINVAL
    assert lib.nldpc_fading_gains(0.0, 1, 2, 0, 0, p, None) == EINVAL
    assert lib.nldpc_fading_gains(0.0, 1, 2, 2, -1, p, None) == EINVAL
    assert b"nldpc_fading_gains" in lib.nldpc_last_error()
    for sym, gain, llr in ((None, p, p), (p, None, p), (p, p, None), (p + 1, p, p), (p, p + 2, p), (p, p, p + 3)):
        assert lib.nldpc_qam_demap_csi(4, 0, 1.0, sym, gain, 2, 2, 1, llr, None) == EINVAL
    assert b"nldpc_qam_demap_csi" in lib.nldpc_last_error()

    def fused(gain_in=None, seq=None, n_seq=1, llr=p, sym=None, gain_out=None, b_offset=0):
        return lib.nldpc_qam_fading_channel_llr(4, 0, None, 2, 8, 1.0, 1, b_offset, 1, 0.0, gain_in, seq, n_seq, llr, sym,
                                                gain_out, None)
    assert fused(llr=None) == EINVAL
    assert fused(llr=p + 2) == EINVAL
    assert fused(sym=p + 1) == EINVAL
    assert fused(gain_in=p + 2) == EINVAL
    assert fused(gain_out=p + 2) == EINVAL
    assert fused(seq=p + 2) == EINVAL
    assert fused(seq=p, n_seq=0) == EINVAL
    assert fused(b_offset=-1) == EINVAL
    assert b"nldpc_qam_fading_channel_llr" in lib.nldpc_last_error()


def test_n_blocks():
    from nldpc.fading import n_blocks
    assert [n_blocks(67, L) for L in (1, 3, 66, 67, 68, 10 ** 12)] == [67, 23, 2, 1, 1, 1]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            n_blocks(67, bad)
    with pytest.raises(ValueError):
        n_blocks(0, 1)
