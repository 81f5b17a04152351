"""QAM constellation and soft demapper on the host (nldpc_qam_points, nldpc_qam_demap_ref; csrc/nldpc_qam.h is the
arithmetic the kernels run), and the argument rules of all five entry points, without a GPU.  Expected values come from
qam_model.py (the 38.211 formulas per order, the fp32 max-log with its stated roundings, the fp64 log-MAP).

Log-MAP is compared with the fp64 model under qam_model.logmap_bound, derived there from the roundings of t, d, d*w,
the max-subtracted expf / logf (2 ulp each) and the two final additions: per LLR, with D = max |d*w| of its dimension,
2e + u(|LLR| + 2e) + 2^-40 (1 + D), e = e1 + e3 + e4 of that docstring -- about 14 u D + 50 u; no fixed tolerance.
"""
import ctypes
import functools

import numpy as np
import pytest

import qam_model as qm_

ORDERS = (2, 4, 6, 8)
SIGMAS = (0.05, 0.3, 1.0)
_FP = ctypes.POINTER(ctypes.c_float)


def _fp(a):
    return a.ctypes.data_as(_FP)


def _demap_ref(qm, method, sigma, sym):
    from nldpc import _lib
    sym = np.ascontiguousarray(sym, dtype=np.float32)
    S = sym.shape[0]
    llr = np.full(S * qm, np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_qam_demap_ref(qm, method, sigma, _fp(sym), S, _fp(llr)) == _lib.NLDPC_OK
    return llr


@functools.lru_cache(maxsize=None)
def _symbols(qm, sigma):
    """fp32 [S, 2]: every constellation point exactly; eight noisy copies of each; every midpoint between two
    neighbouring levels (in I with every level in Q, and the transpose); points far outside the constellation"""
    rng = np.random.default_rng(qm * 100 + int(sigma * 100))
    pts = qm_.constellation(qm)
    lv = np.sort(qm_.dim_levels(qm)[0])
    mid = (lv[:-1] + lv[1:]) * np.float32(0.5)
    grid = np.array([(m, l) for m in mid for l in lv] + [(l, m) for m in mid for l in lv], dtype=np.float32)
    far = np.array([(4, -4), (-100, 100), (1000, 0.1), (-3.5, 1e-3), (lv[-1] * 2, lv[0] * 2), (0, 0)], dtype=np.float32)
    noisy = (np.repeat(pts, 8, axis=0) + sigma * rng.standard_normal((8 * len(pts), 2))).astype(np.float32)
    sym = np.concatenate([pts, noisy, grid, far]).astype(np.float32)
    sym.setflags(write=False)
    return sym


@pytest.mark.parametrize("qm", ORDERS)
def test_points_equal_the_38211_formulas(qm):
    from nldpc.modulation import points
    got = points(qm)
    assert got.dtype == np.complex64 and got.shape == (2 ** qm,)
    want = qm_.constellation(qm)
    assert np.array_equal(got.view(np.float32).reshape(-1, 2), want)
    # A is one rounding of 1 / sqrt(.), a level one more: the mean energy is 1 within (1 + u)^4 - 1
    energy = (want.astype(np.float64) ** 2).sum(axis=1).mean()
    print(f"qm={qm}: mean energy - 1 = {energy - 1:.3e}")
    assert abs(energy - 1.0) <= (1 + qm_.U) ** 4 - 1
    # the amplitudes are the odd integers +-1 .. +-(2^h - 1), each 2^h times per dimension
    h = qm // 2
    amps = np.rint(want.astype(np.float64) / float(qm_.scale(qm))).astype(int)
    for dim in (0, 1):
        vals, counts = np.unique(amps[:, dim], return_counts=True)
        assert vals.tolist() == list(range(-(2 ** h - 1), 2 ** h, 2)) and (counts == 2 ** h).all()


@pytest.mark.parametrize("qm", ORDERS)
def test_points_are_gray(qm):
    from nldpc.modulation import points
    p = points(qm)
    amps = np.rint(np.stack([p.real, p.imag], 1).astype(np.float64) / float(qm_.scale(qm))).astype(int)
    where = {tuple(a): v for v, a in enumerate(amps)}
    assert len(where) == 2 ** qm
    pairs = 0
    for (i, q), v in where.items():
        for nb in ((i + 2, q), (i, q + 2)):  # the nearest neighbour along I, along Q
            if nb in where:
                assert bin(v ^ where[nb]).count("1") == 1, (v, where[nb])
                pairs += 1
    h = qm // 2
    assert pairs == 2 * (2 ** h - 1) * 2 ** h


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("qm", ORDERS)
def test_maxlog_ref_is_bit_identical_to_the_fp32_model(qm, sigma):
    sym = _symbols(qm, sigma)
    got = _demap_ref(qm, 0, sigma, sym)
    want = qm_.maxlog(sym, qm, sigma)
    assert got.dtype == want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a noiseless symbol: negative LLRs for its 0 bits, positive for its 1 bits
    n = 2 ** qm
    bits = np.stack([(np.arange(n) >> (qm - 1 - i)) & 1 for i in range(qm)], axis=1).reshape(-1)
    assert ((got[:n * qm] > 0) == (bits == 1)).all() and (got[:n * qm] != 0).all()


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("qm", ORDERS)
def test_logmap_ref_is_within_the_derived_bound_of_the_fp64_model(qm, sigma):
    sym = _symbols(qm, sigma)
    got = _demap_ref(qm, 1, sigma, sym).astype(np.float64)
    want, dmax = qm_.logmap64(sym, qm, sigma)
    bound = qm_.logmap_bound(qm, want, dmax)
    err = np.abs(got - want)
    worst = int(np.argmax(err / bound))
    print(f"qm={qm} sigma={sigma}: max |d*w| = {dmax.max():.4g}, worst err / bound = {err[worst] / bound[worst]:.3f} "
          f"(err {err[worst]:.3e}, bound {bound[worst]:.3e}, D {dmax[worst]:.4g})")
    assert np.isfinite(got).all()
    assert (err <= bound).all()
    # the bound follows each LLR's own D (about 14 u D + 50 u): the far symbols do not set a tolerance for all
    assert (bound <= qm_.U * (20 * dmax + 80 + np.abs(want))).all()


def test_logmap_and_maxlog_agree_at_high_snr():
    # sanity of the two models against each other: log-MAP -> max-log as sigma -> 0 (not a library check)
    sym = _symbols(4, 0.05)[:16]
    a, _ = qm_.logmap64(sym, 4, 0.05)
    b = qm_.maxlog(sym, 4, 0.05).astype(np.float64)
    assert np.allclose(a, b, rtol=1e-6)


def test_host_calls_reject_bad_arguments():
    from nldpc import _lib
    from nldpc.modulation import points
    L = _lib.lib()
    iq = np.zeros(512, dtype=np.float32)
    sym = np.zeros((4, 2), dtype=np.float32)
    llr = np.zeros(32, dtype=np.float32)
    for qm in (0, 1, 3, 5, 7, 10, -2):
        assert L.nldpc_qam_points(qm, _fp(iq)) == _lib.NLDPC_EINVAL
        assert L.nldpc_qam_demap_ref(qm, 0, 1.0, _fp(sym), 4, _fp(llr)) == _lib.NLDPC_EINVAL
        with pytest.raises(ValueError):
            points(qm)
    assert L.nldpc_qam_points(4, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap_ref(4, 0, 1.0, _fp(sym), 4, _fp(llr)) == _lib.NLDPC_OK
    assert L.nldpc_qam_demap_ref(4, 1, 1.0, _fp(sym), 4, _fp(llr)) == _lib.NLDPC_OK
    for method in (-1, 2):
        assert L.nldpc_qam_demap_ref(4, method, 1.0, _fp(sym), 4, _fp(llr)) == _lib.NLDPC_EINVAL
    for sigma in (0.0, -1.0, float("nan")):
        assert L.nldpc_qam_demap_ref(4, 0, sigma, _fp(sym), 4, _fp(llr)) == _lib.NLDPC_EINVAL
    for S in (0, -1):
        assert L.nldpc_qam_demap_ref(4, 0, 1.0, _fp(sym), S, _fp(llr)) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap_ref(4, 0, 1.0, None, 4, _fp(llr)) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap_ref(4, 0, 1.0, _fp(sym), 4, None) == _lib.NLDPC_EINVAL
    assert b"nldpc_qam_demap_ref" in L.nldpc_last_error()


# (qm, method, B, E, sigma): the rules of the device calls are checked on the host before anything is launched
BAD_SHAPES = {
    "qm_1": (1, 0, 2, 8, 1.0), "qm_3": (3, 0, 2, 9, 1.0), "qm_10": (10, 0, 2, 20, 1.0),
    "method_2": (4, 2, 2, 8, 1.0), "method_negative": (4, -1, 2, 8, 1.0),
    "E_not_multiple": (4, 0, 2, 10, 1.0), "E_zero": (4, 0, 2, 0, 1.0), "E_negative": (4, 0, 2, -4, 1.0),
    "E_2_31": (4, 0, 2, 2 ** 31, 1.0), "B_zero": (4, 0, 0, 8, 1.0), "B_negative": (4, 0, -1, 8, 1.0),
    "sigma_zero": (4, 0, 2, 8, 0.0), "sigma_negative": (4, 0, 2, 8, -0.5), "sigma_nan": (4, 0, 2, 8, float("nan")),
}


@pytest.mark.parametrize("rule", sorted(BAD_SHAPES))
def test_device_calls_reject_bad_arguments_on_the_host(rule):
    """every rule is refused before a launch: the pointers are (aligned) host addresses that no kernel ever sees"""
    from nldpc import _lib
    L = _lib.lib()
    qm, method, B, E, sigma = BAD_SHAPES[rule]
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    assert L.nldpc_qam_channel_llr(qm, method, p, B, E, sigma, 1, 0, p, p, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_channel_llr(qm, method, None, B, E, sigma, 1, 0, p, None, None) == _lib.NLDPC_EINVAL
    if not rule.startswith(("method", "sigma")):
        assert L.nldpc_qam_modulate(qm, p, B, E, p, None) == _lib.NLDPC_EINVAL
    if not rule.startswith("E_not"):
        S = E // qm if E % qm == 0 else E
        assert L.nldpc_qam_demap(qm, method, sigma, p, B, S, p, None) == _lib.NLDPC_EINVAL


def test_null_and_misaligned_pointers_are_rejected():
    from nldpc import _lib
    L = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data
    assert L.nldpc_qam_modulate(4, None, 2, 8, p, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_modulate(4, p, 2, 8, None, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_modulate(4, p, 2, 8, p + 2, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap(4, 0, 1.0, None, 2, 2, p, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap(4, 0, 1.0, p, 2, 2, None, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap(4, 0, 1.0, p + 1, 2, 2, p, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_demap(4, 0, 1.0, p, 2, 2, p + 2, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_channel_llr(4, 0, None, 2, 8, 1.0, 1, 0, None, None, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_channel_llr(4, 0, None, 2, 8, 1.0, 1, 0, p + 2, None, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_channel_llr(4, 0, None, 2, 8, 1.0, 1, 0, p, p + 1, None) == _lib.NLDPC_EINVAL
    assert L.nldpc_qam_channel_llr(4, 0, None, 2, 8, 1.0, 1, -1, p, None, None) == _lib.NLDPC_EINVAL
    assert b"nldpc_qam_channel_llr" in L.nldpc_last_error()


def test_sigma_for():
    from nldpc.channel import sigma_for as bpsk_sigma
    from nldpc.modulation import sigma_for
    assert sigma_for(3.0, 0.5, 4) == np.sqrt(1.0 / (2.0 * 4 * 0.5 * 10.0 ** 0.3))
    # per real dimension QPSK is BPSK at the same Eb/N0 once the symbol energy is split over I and Q
    assert np.isclose(sigma_for(5.0, 0.5, 2) * np.sqrt(2.0), bpsk_sigma(5.0, 0.5))
