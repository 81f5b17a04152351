"""The exact max-log ML detector's arithmetic on the host (nldpc_mimo_detect_ml_ref; csrc/nldpc_mimo_ml.h is what the
kernels run) and the argument rules of the three ML entry points, without a GPU.  Expected values come from
mimo_ml_model.py: (a) the float32 restatement of the sliced two-pass detector in the order include/nldpc.h states, which
the library equals bit for bit, and (b) an independent float64 search over all M^nt symbol vectors, to which the
library is held within mimo_ml_model.ml_bound (derived from the arithmetic: the metric's rounding and the near-tie
slice).  For one layer, and for channels with exactly orthogonal columns, max-log ML is analytically the LMMSE max-log
detector: the two host references are compared within the sum of ml_bound and mimo_ml_model.lmmse_orthogonal_bound.
"""
import ctypes
import functools

import numpy as np
import pytest

import mimo_ml_model as ml
import mimo_model as mm

_FP = ctypes.POINTER(ctypes.c_float)
SEED = 4242
# every supported (qm, nt, nr): all of nt = 1 and 2, nt = 4 up to 16-QAM
CASES = [(qm, nt, nr) for qm in (2, 4, 6, 8) for nt, nr in mm.DIMS if ml.supported(qm, nt)]
ONE_LAYER = [c for c in CASES if c[1] == 1]
SEVERAL = [c for c in CASES if c[1] > 1]
SIGMA = {2: 0.5, 4: 0.25, 6: 0.12, 8: 0.06}


def _fp(a):
    return a.ctypes.data_as(_FP)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def _ml_ref(qm, sigma, y, h, L):
    from nldpc import _lib
    y = np.ascontiguousarray(y, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    B, R, nr = y.shape[:3]
    nt = h.shape[-2]
    llr = np.full((B, R * nt * qm), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_detect_ml_ref(qm, nt, nr, sigma, _fp(y), _fp(h), B, R, L, _fp(llr)) == _lib.NLDPC_OK
    return llr


def _lmmse_ref(qm, sigma, y, h, L):
    from nldpc import _lib
    y = np.ascontiguousarray(y, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    B, R, nr = y.shape[:3]
    nt = h.shape[-2]
    llr = np.full((B, R * nt * qm), np.nan, dtype=np.float32)
    assert _lib.lib().nldpc_mimo_detect_ref(qm, 0, nt, nr, sigma, _fp(y), _fp(h), B, R, L, _fp(llr)) == _lib.NLDPC_OK
    return llr


@functools.lru_cache(maxsize=None)
def _case(qm, nt, nr):
    """B = 3 rows of R = 11 resource elements in blocks of L = 4 (a short last block): drawn channels with one zero
    block, received samples of random bits plus samples far outside; the references (a) and (b), computed once"""
    B, R, L, sigma = 3, 11, 4, SIGMA[qm]
    rng = np.random.default_rng(100 * qm + 10 * nt + nr)
    f = rng.integers(0, 2, (B, R * nt * qm)).astype(np.uint8)
    table = np.array(mm.channels(B, R, L, nt, nr, SEED))
    table[1, 1] = 0.0
    y = np.array(mm.received(f, qm, sigma, table, L, nt, nr, SEED))
    y[2, -2:, 0] = [(4, -4), (-100, 1000)]
    sigma = float(np.float32(sigma))
    c = dict(B=B, R=R, L=L, sigma=sigma, table=table, y=y, a=ml.detect_ml(y, table, qm, sigma, L),
             b=ml.detect_exhaustive64(y, table, qm, sigma, L))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@pytest.mark.parametrize("qm,nt,nr", CASES)
def test_detect_ml_ref_is_bit_identical_to_the_ordered_model(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _ml_ref(qm, c["sigma"], c["y"], c["table"], c["L"])
    assert got.dtype == np.float32 and np.isfinite(got).all() and _bits_equal(got, c["a"])
    # the zero block gives +-0, its neighbours do not
    per = got.reshape(c["B"], c["R"], nt * qm)
    assert ((per[1, 4:8].view(np.uint32) & 0x7FFFFFFF) == 0).all() and per[1, :4].any() and per[1, 8:].any()


@pytest.mark.parametrize("qm,nt,nr", CASES)
def test_detect_ml_ref_is_within_the_derived_bound_of_the_exhaustive_fp64_search(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _ml_ref(qm, c["sigma"], c["y"], c["table"], c["L"]).astype(np.float64)
    bound = ml.ml_bound(c["y"], c["table"], qm, c["sigma"], c["L"], c["b"])
    err = np.abs(got - c["b"])
    print(f"qm={qm} nt={nt} nr={nr}: max err = {err.max():.3g}, max err / bound = "
          f"{(err / np.maximum(bound, 1e-300)).max():.3g}, max |LLR| = {np.abs(c['b']).max():.4g}, "
          f"bound infinite on {float(np.isinf(bound).mean()):.3f} of the LLRs")
    assert (err <= bound).all()
    assert np.isfinite(bound).all()  # (no channel of the test is so ill-conditioned that the slice term is undefined)
    # the model in the stated order is held to the same bound: what differs from (b) is the arithmetic, not the library
    assert (np.abs(c["a"].astype(np.float64) - c["b"]) <= bound).all()


@pytest.mark.parametrize("qm,nt,nr", ONE_LAYER)
def test_one_layer_is_the_lmmse_maxlog_detector(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _ml_ref(qm, c["sigma"], c["y"], c["table"], c["L"]).astype(np.float64)
    lin = _lmmse_ref(qm, c["sigma"], c["y"], c["table"], c["L"]).astype(np.float64)
    bound = ml.ml_bound(c["y"], c["table"], qm, c["sigma"], c["L"], c["b"]) + \
        ml.lmmse_orthogonal_bound(c["y"], c["table"], qm, c["sigma"], c["L"], c["b"])
    err = np.abs(got - lin)
    print(f"qm={qm} nr={nr}: max err = {err.max():.3g}, max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()


@functools.lru_cache(maxsize=None)
def _orthogonal_case(qm, nt, nr):
    """every block a scaled unitary: c (the block's own fp32 scale) times entries 1, i, -1 with exactly orthogonal
    columns; one block of scale 0"""
    B, R, L, sigma = 3, 11, 4, SIGMA[qm]
    rng = np.random.default_rng(7 * qm + nt + nr)
    f = rng.integers(0, 2, (B, R * nt * qm)).astype(np.uint8)
    scale = rng.uniform(0.2, 1.5, (B, 3)).astype(np.float32) / np.float32(np.sqrt(nr))
    scale[1, 1] = 0.0
    u = ml.unitary(nt, nr)
    table = np.zeros((B, 3, nr, nt, 2), dtype=np.float32)
    table[..., 0] = scale[..., None, None] * u.real.astype(np.float32)
    table[..., 1] = scale[..., None, None] * u.imag.astype(np.float32)
    y = mm.received(f, qm, sigma, table, L, nt, nr, SEED)
    return dict(L=L, sigma=float(np.float32(sigma)), table=table, y=y, f=f)


@pytest.mark.parametrize("qm,nt,nr", SEVERAL)
def test_orthogonal_columns_decouple_into_the_lmmse_maxlog_detector(qm, nt, nr):
    c = _orthogonal_case(qm, nt, nr)
    got = _ml_ref(qm, c["sigma"], c["y"], c["table"], c["L"]).astype(np.float64)
    lin = _lmmse_ref(qm, c["sigma"], c["y"], c["table"], c["L"]).astype(np.float64)
    exact = ml.detect_exhaustive64(c["y"], c["table"], qm, c["sigma"], c["L"])
    b_ml = ml.ml_bound(c["y"], c["table"], qm, c["sigma"], c["L"], exact)
    b_lin = ml.lmmse_orthogonal_bound(c["y"], c["table"], qm, c["sigma"], c["L"], exact)
    err = np.abs(got - lin)
    print(f"qm={qm} nt={nt} nr={nr}: max |ML - LMMSE| = {err.max():.3g}, / bound = "
          f"{(err / np.maximum(b_ml + b_lin, 1e-300)).max():.3g}, max |LLR| = {np.abs(exact).max():.4g}")
    assert (np.abs(got - exact) <= b_ml).all() and (np.abs(lin - exact) <= b_lin).all()
    assert (err <= b_ml + b_lin).all()
    assert np.abs(exact).max() > 1.0


@pytest.mark.parametrize("qm,nt,nr", CASES)
def test_a_zero_channel_gives_zero_llrs(qm, nt, nr):
    c = _case(qm, nt, nr)
    got = _ml_ref(qm, c["sigma"], c["y"], np.zeros_like(c["table"]), c["L"])
    assert ((got.view(np.uint32) & 0x7FFFFFFF) == 0).all()


@pytest.mark.parametrize("qm,nt,nr", CASES)
def test_hard_decisions_at_high_snr_are_the_sent_bits(qm, nt, nr):
    B, R, L, sigma = 2, 9, 2, float(np.float32(1e-3))
    rng = np.random.default_rng(qm + nt + nr)
    f = rng.integers(0, 2, (B, R * nt * qm)).astype(np.uint8)
    table = mm.channels(B, R, L, nt, nr, SEED)
    y = mm.received(f, qm, sigma, table, L, nt, nr, SEED)
    model = ml.detect_ml(y, table, qm, sigma, L)
    assert np.array_equal(model > 0, f != 0)  # (the premise: sigma is small enough for the model)
    got = _ml_ref(qm, sigma, y, table, L)
    assert np.array_equal(got > 0, f != 0) and _bits_equal(got, model)


def test_block_structure():
    qm, nt, nr, B, R, L, sigma = 4, 2, 2, 2, 7, 3, 0.3
    rng = np.random.default_rng(1)
    y = np.tile(rng.normal(size=(1, 1, nr, 2)).astype(np.float32), (B, R, 1, 1))
    table = mm.channels(B, R, L, nt, nr, SEED)
    got = _ml_ref(qm, sigma, y, table, L).reshape(B, R, nt * qm)
    for b in range(B):
        for i in range(R):
            one = _ml_ref(qm, sigma, y[:1, :1], table[b:b + 1, i // L:i // L + 1], 1)
            assert _bits_equal(got[b, i], one.reshape(-1)), (b, i)
    big = _ml_ref(qm, sigma, y, table[:, :1], R + 5)
    assert _bits_equal(big, _ml_ref(qm, sigma, y, table[:, :1], R))


def test_model_helpers():
    # the slice picks the nearest level, ties and the outside included, and K is 1 / (2 A) to fp32
    import qam_model as qm_
    for qm in (2, 4, 6, 8):
        lv = np.sort(qm_.dim_levels(qm)[0])
        assert abs(float(ml.step(qm)) * 2.0 * float(qm_.scale(qm)) - 1.0) < 2.0 ** -22
        z = np.linspace(-2.0, 2.0, 4001).astype(np.float32)
        got = ml.slice_level(z, qm)
        d = np.abs(z[:, None].astype(np.float64) - lv[None, :].astype(np.float64))
        assert (np.abs(got.astype(np.float64) - z) <= d.min(axis=1) + 1e-6).all() and np.isin(got, lv).all()
        assert ml.slice_level(np.array([np.nan, -np.inf, np.inf], dtype=np.float32), qm).tolist() == \
            [lv[0], lv[0], lv[-1]]
    assert [ml.candidates(*c) for c in ((8, 1), (8, 2), (2, 4), (4, 4))] == [256, 512, 128, 8192]


def test_host_call_rejects_bad_arguments():
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL, OK, EUNSUPPORTED = _lib.NLDPC_EINVAL, _lib.NLDPC_OK, _lib.NLDPC_EUNSUPPORTED
    buf = np.zeros(512, dtype=np.float32)
    p = _fp(buf)
    assert lib.nldpc_mimo_detect_ml_ref(4, 2, 2, 1.0, p, p, 2, 4, 1, p) == OK
    for qm in (0, 1, 3, 10, -2):
        assert lib.nldpc_mimo_detect_ml_ref(qm, 2, 2, 1.0, p, p, 2, 4, 1, p) == EINVAL
    for sigma in (0.0, -1.0, float("nan")):
        assert lib.nldpc_mimo_detect_ml_ref(4, 2, 2, sigma, p, p, 2, 4, 1, p) == EINVAL
    for nt, nr in ((2, 1), (4, 2), (3, 3), (1, 3), (0, 1), (8, 8)):
        assert lib.nldpc_mimo_detect_ml_ref(4, nt, nr, 1.0, p, p, 2, 4, 1, p) == EINVAL
    for B, R, L in ((0, 4, 1), (-1, 4, 1), (2, 0, 1), (2, -4, 1), (2, 4, 0), (2, 4, -1), (2, 2 ** 28, 1), (2 ** 20, 2 ** 11, 1)):
        assert lib.nldpc_mimo_detect_ml_ref(4, 2, 2, 1.0, p, p, B, R, L, p) == EINVAL, (B, R, L)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.nldpc_mimo_detect_ml_ref(4, 2, 2, 1.0, args[0], args[1], 2, 4, 1, args[2]) == EINVAL
    assert b"nldpc_mimo_detect_ml_ref" in lib.nldpc_last_error()
    for qm in (6, 8):
        assert lib.nldpc_mimo_detect_ml_ref(qm, 4, 4, 1.0, p, p, 1, 1, 1, p) == EUNSUPPORTED
        assert b"tree search" in lib.nldpc_last_error()
        with pytest.raises(_lib.NldpcUnsupported):
            _lib.check(EUNSUPPORTED, "nldpc_mimo_detect_ml_ref")
    for qm in (2, 4):
        assert lib.nldpc_mimo_detect_ml_ref(qm, 4, 4, 1.0, p, p, 1, 1, 1, p) == OK


# (qm, nt, nr, B, E, sigma, L): the rules of the device calls are checked on the host before anything is launched
BAD = {
    "qm_1": (1, 2, 2, 2, 8, 1.0, 1), "qm_3": (3, 1, 1, 2, 9, 1.0, 1),
    "nt_3": (4, 3, 4, 2, 24, 1.0, 1), "nr_below_nt": (4, 2, 1, 2, 8, 1.0, 1), "nr_8": (4, 4, 8, 2, 16, 1.0, 1),
    "nt_0": (4, 0, 1, 2, 8, 1.0, 1),
    "E_not_multiple_of_qm": (4, 2, 2, 2, 10, 1.0, 1), "S_not_multiple_of_nt": (4, 2, 2, 2, 12, 1.0, 1),
    "S_not_multiple_of_4": (2, 4, 4, 2, 12, 1.0, 1), "E_zero": (4, 2, 2, 2, 0, 1.0, 1),
    "E_2_31": (4, 2, 2, 2, 2 ** 31, 1.0, 1), "B_zero": (4, 2, 2, 0, 8, 1.0, 1),
    "sigma_zero": (4, 2, 2, 2, 8, 0.0, 1), "sigma_nan": (4, 2, 2, 2, 8, float("nan"), 1),
    "L_zero": (4, 2, 2, 2, 8, 1.0, 0), "L_negative": (4, 2, 2, 2, 8, 1.0, -3),
    "blocks_2_31": (2, 1, 1, 2 ** 20, 2 ** 12, 1.0, 1),
}


@pytest.mark.parametrize("rule", sorted(BAD))
def test_device_calls_reject_bad_arguments_on_the_host(rule):
    """every rule is refused before a launch: the pointers are (aligned) host addresses that no kernel ever sees"""
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL = _lib.NLDPC_EINVAL
    qm, nt, nr, B, E, sigma, L = BAD[rule]
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    out = p + 8192
    for h_in in (None, p):
        for seq in (None, p):
            assert lib.nldpc_mimo_channel_llr_ml(qm, nt, nr, None, B, E, sigma, 1, 0, L, h_in, seq, 1, out, out, out,
                                                 None) == EINVAL
    if not rule.startswith(("E_not", "S_not", "E_2_31")):
        R = max(E // max(qm, 1) // max(nt, 1), 0)
        assert lib.nldpc_mimo_detect_ml(qm, nt, nr, sigma, p, p, B, R, L, p, None) == EINVAL


def test_unsupported_null_misaligned_and_overlapping_pointers_are_rejected():
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = _lib.NLDPC_EINVAL, _lib.NLDPC_EUNSUPPORTED
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data
    for y, h, llr in ((None, p, p), (p, None, p), (p, p, None), (p + 1, p, p), (p, p + 2, p), (p, p, p + 3)):
        assert lib.nldpc_mimo_detect_ml(4, 2, 2, 1.0, y, h, 2, 2, 1, llr, None) == EINVAL
    assert b"nldpc_mimo_detect_ml" in lib.nldpc_last_error()
    for qm in (6, 8):  # refused before anything is launched
        assert lib.nldpc_mimo_detect_ml(qm, 4, 4, 1.0, p, p, 2, 2, 1, p, None) == EUNSUPPORTED
        assert lib.nldpc_mimo_channel_llr_ml(qm, 4, 4, None, 2, 8 * qm, 1.0, 1, 0, 1, None, None, 0, p, None, None,
                                             None) == EUNSUPPORTED
        assert b"nldpc_mimo_channel_llr_ml" in lib.nldpc_last_error()

    def fused(h_in=None, seq=None, n_seq=1, llr=p, sym=None, h_out=None, b_offset=0):
        return lib.nldpc_mimo_channel_llr_ml(4, 2, 2, None, 2, 16, 1.0, 1, b_offset, 1, h_in, seq, n_seq, llr, sym,
                                             h_out, None)
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
