"""Gold-sequence scrambling without a GPU: the host generator (nldpc_gold_ref / nldpc_gold_cinit, nldpc.scrambling.gold /
c_init) against gold_model.py (TS 38.211 §5.2.1 bit by bit; the far window by a GF(2) matrix power), the argument rules
of every new entry point, and the Python wrappers' ValueErrors.  Expected values never come from the library.
"""
import ctypes

import numpy as np
import pytest
import torch

import gold_model as gm

C_INITS = [0, 0x12345, 0x7FFFFFFF, 0x1F4002A, 1]
# the first three packed words of c, from a bit-serial transcription of §5.2.1
WORDS = {0: (0x5E485840, 0x6AC0A9A4, 0xB3CC5E48), 0x12345: (0xDE5EEA6B, 0x92CDE15C, 0x0148D59A),
         0x7FFFFFFF: (0x71CFD0BF, 0x71EA0674, 0x2A445D53), 0x1F4002A: (0x7EEA82CC, 0x34A704B8, 0x154CECF3)}


def test_the_model_gives_the_table_words():
    assert gm.c_init(1000, 42) == 0x1F4002A
    for ci, want in WORDS.items():
        assert tuple(int(w) for w in gm.pack(gm.gold(ci, 96))) == want
    # packing: bit n in bit n & 31 of word n >> 5, zeros beyond E; the matrix-power jump equals running from 0
    assert gm.pack(np.array([1, 0, 1] + [0] * 30 + [1])).tolist() == [5, 2]
    for ci in (0x12345, 1):
        assert np.array_equal(gm.gold_far(ci, 64, 4097), gm.gold(ci, 64, 4097))


@pytest.mark.parametrize("ci", C_INITS)
def test_gold_equals_the_model(ci):
    from nldpc.scrambling import gold
    for n0 in (0, 1, 31, 32, 1599, 4097):
        got = gold(ci, 200, n0)
        assert got.dtype == np.uint8 and got.shape == (200,)
        assert np.array_equal(got, gm.gold(ci, 200, n0)), n0
    assert np.array_equal(gold(ci, 64, 2 ** 31 - 64), gm.gold_far(ci, 64, 2 ** 31 - 64))
    if ci in WORDS:
        assert tuple(int(w) for w in gm.pack(gold(ci, 96))) == WORDS[ci]
    # a window does not depend on where it starts
    assert np.array_equal(gold(ci, 1, 77), gold(ci, 100, 0)[77:78])


def test_c_init_values_and_rules():
    from nldpc import _lib
    from nldpc.scrambling import c_init
    assert c_init(1000, 42) == 0x1F4002A == gm.c_init(1000, 42)
    assert c_init(0, 0) == 0 and c_init(65535, 1023, 1) == 65535 * 2 ** 15 + 2 ** 14 + 1023 < 2 ** 31 and c_init(1, 0, 1) == 2 ** 15 + 2 ** 14
    assert c_init(3, 5, q=0) == gm.c_init(3, 5)
    for bad in ((-1, 0, 0), (65536, 0, 0), (0, -1, 0), (0, 1024, 0), (0, 0, 2), (0, 0, -1), (1.5, 0, 0)):
        with pytest.raises(ValueError):
            c_init(bad[0], bad[1], bad[2])
    lib = _lib.lib()
    out = ctypes.c_uint32(7)
    assert lib.nldpc_gold_cinit(1, 0, 1, None) == _lib.NLDPC_EINVAL
    assert lib.nldpc_gold_cinit(65536, 0, 1, ctypes.byref(out)) == _lib.NLDPC_EINVAL
    assert lib.nldpc_gold_cinit(1, 2, 1, ctypes.byref(out)) == _lib.NLDPC_EINVAL
    assert lib.nldpc_gold_cinit(1, 0, 1024, ctypes.byref(out)) == _lib.NLDPC_EINVAL and out.value == 7
    assert lib.nldpc_gold_cinit(1, 1, 1, ctypes.byref(out)) == _lib.NLDPC_OK and out.value == 2 ** 15 + 2 ** 14 + 1


def test_gold_ref_argument_rules():
    from nldpc import _lib
    from nldpc.scrambling import gold
    lib = _lib.lib()
    buf = np.full(80, 9, dtype=np.uint8)
    p = buf.ctypes.data
    for args in ((2 ** 31, 0, 8, p), (0, -1, 8, p), (0, 0, 0, p), (0, 0, -3, p), (0, 2 ** 31 - 7, 8, p), (0, 2 ** 31, 1, p),
                 (0, 0, 8, None)):
        assert lib.nldpc_gold_ref(*args) == _lib.NLDPC_EINVAL, args
    assert b"nldpc_gold_ref" in lib.nldpc_last_error()
    assert (buf == 9).all()
    # the last legal window, and nothing behind the n bytes is written
    assert lib.nldpc_gold_ref(5, 2 ** 31 - 8, 8, p) == _lib.NLDPC_OK
    assert (buf[8:] == 9).all() and buf[:8].max() <= 1
    assert lib.nldpc_gold_ref(5, 3, 33, p) == _lib.NLDPC_OK
    assert (buf[33:] == 9).all() and np.array_equal(buf[:33], gm.gold(5, 33, 3))
    for bad in (lambda: gold(2 ** 31, 8), lambda: gold(-1, 8), lambda: gold(0, 0), lambda: gold(0, 8, -1),
                lambda: gold(0, 8, 2 ** 31 - 7), lambda: gold(0.5, 8)):
        with pytest.raises(ValueError):
            bad()


def test_device_entry_points_validate_on_the_host():
    """NULL / misaligned / out-of-range arguments are refused before any device is touched (fake addresses are never
    dereferenced)"""
    from nldpc import _lib
    lib = _lib.lib()
    EINVAL, EUNS = _lib.NLDPC_EINVAL, _lib.NLDPC_EUNSUPPORTED
    P, Q, ODD = 0x10000, 0x20000, 0x10002  # never dereferenced
    big = 2 ** 31
    for args in ((None, 1, 32, P), (P, 1, 32, None), (ODD, 1, 32, P), (P, 1, 32, ODD), (P, 0, 32, Q), (P, -1, 32, Q),
                 (P, 1, 0, Q), (P, 1, big, Q)):
        assert lib.nldpc_gold_sequence(*args, None) == EINVAL, args
    assert b"nldpc_gold_sequence" in lib.nldpc_last_error()
    assert lib.nldpc_gold_sequence(P, 2 ** 26, 32 * 32, Q, None) == EUNS   # n_seq * Wc = 2^31
    assert lib.nldpc_gold_sequence(P, big, 1, Q, None) == EUNS
    # f, seq, n_seq, B, E, b_offset, out
    for args in ((P, None, 1, 1, 8, 0, Q), (P, ODD, 1, 1, 8, 0, Q), (P, Q, 0, 1, 8, 0, P), (P, Q, 1, 0, 8, 0, P),
                 (P, Q, 1, 1, 0, 0, P), (P, Q, 1, 1, big, 0, P), (P, Q, 1, 1, 8, -1, P), (P, Q, 1, 1, 8, 0, None)):
        assert lib.nldpc_scramble(*args, None) == EINVAL, args
    assert b"nldpc_scramble" in lib.nldpc_last_error()
    for args in ((P, Q, 1, big, 8, 0, P), (P, Q, 1, 1, 8, big, P), (P, Q, 2 ** 26, 1, 32 * 32, 0, P)):
        assert lib.nldpc_scramble(*args, None) == EUNS, args
    for args in ((None, Q, 1, 1, 8, 0, P), (ODD, Q, 1, 1, 8, 0, P), (P, Q, 1, 1, 8, 0, ODD), (P, None, 1, 1, 8, 0, P),
                 (P, ODD, 1, 1, 8, 0, P), (P, Q, 0, 1, 8, 0, P), (P, Q, 1, 0, 8, 0, P), (P, Q, 1, 1, 0, 0, P),
                 (P, Q, 1, 1, big, 0, P), (P, Q, 1, 1, 8, -1, P), (P, Q, 1, 1, 8, 0, None)):
        assert lib.nldpc_descramble_llr(*args, None) == EINVAL, args
    assert b"nldpc_descramble_llr" in lib.nldpc_last_error()
    assert lib.nldpc_descramble_llr(P, Q, 1, big, 8, 0, P, None) == EUNS
    # qm, method, f, B, E, sigma, seed, b_offset, seq, n_seq, llr, sym_out
    ok = dict(qm=4, method=0, f=P, B=2, E=24, sigma=0.5, seed=1, b_offset=0, seq=Q, n_seq=1, llr=P, sym=None)
    for change in (dict(qm=3), dict(qm=1), dict(method=2), dict(B=0), dict(E=0), dict(E=22), dict(E=big), dict(sigma=0.0),
                   dict(sigma=-1.0), dict(sigma=float("nan")), dict(b_offset=-1), dict(seq=None), dict(seq=ODD),
                   dict(n_seq=0), dict(n_seq=-2), dict(llr=None), dict(llr=ODD), dict(sym=ODD)):
        a = dict(ok, **change)
        assert lib.nldpc_qam_channel_llr_scrambled(a["qm"], a["method"], a["f"], a["B"], a["E"], a["sigma"], a["seed"],
                                                   a["b_offset"], a["seq"], a["n_seq"], a["llr"], a["sym"],
                                                   None) == EINVAL, change
        assert b"nldpc_qam_channel_llr_scrambled" in lib.nldpc_last_error()
    for change in (dict(B=big), dict(b_offset=big), dict(n_seq=big)):
        a = dict(ok, **change)
        assert lib.nldpc_qam_channel_llr_scrambled(a["qm"], a["method"], a["f"], a["B"], a["E"], a["sigma"], a["seed"],
                                                   a["b_offset"], a["seq"], a["n_seq"], a["llr"], a["sym"], None) == EUNS


def test_wrappers_raise_value_error_without_a_device():
    from nldpc.modulation import qam_llr
    from nldpc.scrambling import descramble, scramble, sequence
    f = torch.zeros((2, 24), dtype=torch.uint8)
    llr = torch.zeros((2, 24))
    seq = torch.zeros((1, 1), dtype=torch.int32)
    # CPU tensors: there is no CPU path
    for bad in (lambda: scramble(f, seq), lambda: descramble(llr, seq), lambda: scramble(None, seq, B=2, E=24),
                lambda: sequence(torch.zeros(2, dtype=torch.int32), 24), lambda: sequence([1, 2], 24, device="cpu"),
                lambda: qam_llr(f, 4, 0.5, scramble=seq)):
        with pytest.raises(ValueError):
            bad()
    # arguments refused before any tensor is looked at on a device
    for bad in (lambda: sequence([], 24), lambda: sequence([2 ** 31], 24), lambda: sequence([-1], 24),
                lambda: sequence(1.5, 24), lambda: sequence([1], 0), lambda: sequence([1], 2 ** 31),
                lambda: scramble(None, seq), lambda: scramble(f.float(), seq), lambda: descramble(llr.double(), seq),
                lambda: descramble(llr[0], seq)):
        with pytest.raises(ValueError):
            bad()
    # wrong dtypes, a table of the wrong width and a negative b_offset are named before the device is
    for bad, what in ((lambda: scramble(f.float(), seq), "uint8"), (lambda: scramble(f[0], seq), "uint8"),
                      (lambda: descramble(llr.double(), seq), "float32"), (lambda: descramble(llr[0], seq), "float32"),
                      (lambda: scramble(f, seq.long()), "int32"), (lambda: descramble(llr, seq.float()), "int32"),
                      (lambda: scramble(f, seq[0]), "int32"), (lambda: scramble(f, [[0]]), "int32"),
                      (lambda: scramble(f, torch.zeros((1, 2), dtype=torch.int32)), "words per sequence"),
                      (lambda: descramble(llr, torch.zeros((3, 2), dtype=torch.int32)), "words per sequence"),
                      (lambda: scramble(None, seq, B=2, E=33), "words per sequence"),
                      (lambda: descramble(torch.zeros((2, 33)), seq), "words per sequence"),
                      (lambda: scramble(f, seq, b_offset=-1), "b_offset"), (lambda: descramble(llr, seq, b_offset=-1), "b_offset"),
                      (lambda: scramble(None, seq, B=0, E=24), "B must be positive"),
                      (lambda: scramble(f, seq, B=3), r"not \[B, E\]"), (lambda: scramble(f, seq, E=25), r"not \[B, E\]"),
                      (lambda: sequence(torch.zeros(2, dtype=torch.int64), 24), "int32"),
                      (lambda: sequence(torch.zeros((2, 1), dtype=torch.int32), 24), "int32")):
        with pytest.raises(ValueError, match=what):
            bad()
    for bad in (lambda: scramble(f, seq), lambda: descramble(llr, seq), lambda: scramble(None, seq, B=2, E=24)):
        with pytest.raises(ValueError, match="ROCm device"):
            bad()
