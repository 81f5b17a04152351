"""The CRCs of TS 38.212 §5.1 on the host (nldpc_crc_ref: the inline functions of csrc/nldpc_crc.h the kernels run, driven
through their table, bit-serial and multiply-by-x^n paths by the chunk argument) and the argument rules of the three
entry points, without a GPU.  Expected values come from crc_model.py (long division) and from published check values.
"""
import ctypes

import numpy as np
import pytest

import crc_model as cm

NAMES = ("24A", "24B", "24C", "16", "11", "6")
# parity of the 72 bits of ASCII "123456789", most significant bit of each byte first (by bit-serial division; 24A, 24B
# and 16 are the catalogued CRC-24/LTE-A, CRC-24/LTE-B and CRC-16/XMODEM check values)
CHECK = {"24A": 0xCDE703, "24B": 0x23EF52, "24C": 0xF48279, "16": 0x31C3, "11": 0x5CA, "6": 0x15}
LENGTHS = (1, 2, 7, 8, 23, 24, 25, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 8448)


def _ref(name, bits, chunk):
    """nldpc_crc_ref on raw bytes (values other than 0 / 1 included)"""
    from nldpc import _lib
    from nldpc.crc import CRCS
    raw = np.ascontiguousarray(bits, dtype=np.uint8)
    p = ctypes.c_uint32(0xFFFFFFFF)
    assert _lib.lib().nldpc_crc_ref(CRCS[name][0], raw.ctypes.data, raw.size, chunk, ctypes.byref(p)) == _lib.NLDPC_OK
    return p.value


def test_the_table_of_polynomials_is_the_models():
    from nldpc.crc import CRCS
    assert tuple(CRCS) == NAMES == cm.NAMES
    for i, name in enumerate(NAMES):
        cid, L, poly = CRCS[name]
        g = cm.generator(name)
        assert cid == i and L == cm.length(name) == len(g) - 1
        assert g[0] == 1 and int("".join(map(str, g[1:])), 2) == poly


@pytest.mark.parametrize("name", NAMES)
def test_fixed_check_values(name):
    from nldpc.crc import parity
    bits = np.unpackbits(np.frombuffer(b"123456789", dtype=np.uint8))
    assert bits.size == 72
    assert int(cm.parity_int(bits, name)[0]) == CHECK[name]
    assert parity(bits, name) == CHECK[name]
    for chunk in (1, 8, 32, 33, 72, 2048):
        assert parity(bits, name, chunk=chunk) == CHECK[name]


@pytest.mark.parametrize("name", NAMES)
def test_chunked_path_equals_long_division(name):
    rng = np.random.default_rng(len(name) * 7 + cm.length(name))
    for A in LENGTHS:
        raw = rng.choice(np.array([0, 0, 0, 1, 1, 2, 128, 255], dtype=np.uint8), A)
        want = int(cm.parity_int(raw, name)[0])
        for chunk in sorted({1, 8, 32, 33, 2048, A}):
            assert _ref(name, raw, chunk) == want, (A, chunk)


@pytest.mark.parametrize("name", NAMES)
def test_algebra(name):
    from nldpc.crc import parity
    L = cm.length(name)
    rng = np.random.default_rng(L)
    A = 200 - L
    u, v = rng.integers(0, 2, (2, A)).astype(np.uint8)
    # the appended block has remainder 0, in the model and (its parity over all A + L bits is 0) in the library
    block = cm.attach(u, name)[0]
    assert block.size == 200 and cm.passes(block, name, A)[0]
    pu = parity(u, name)
    assert [int(b) for b in block[A:]] == [(pu >> (L - 1 - i)) & 1 for i in range(L)]
    assert parity(block, name) == 0 and parity(block, name, chunk=7) == 0
    # every single-bit flip of the 200-bit block is detected
    flipped = np.repeat(block[None], 200, axis=0)
    flipped[np.arange(200), np.arange(200)] ^= 1
    assert not cm.passes(flipped, name, A).any()
    lib_rem = parity(flipped, name, chunk=64)
    assert lib_rem.shape == (200,) and (lib_rem != 0).all()
    # linearity
    assert parity(u ^ v, name) == pu ^ parity(v, name)
    # leading zeros change nothing; the all-zero block passes
    for z in (1, 31, 32, 2048):
        assert parity(np.concatenate([np.zeros(z, np.uint8), u]), name, chunk=33) == pu
    assert parity(np.zeros(77, np.uint8), name) == 0 and cm.passes(np.zeros(77 + L, np.uint8), name, 77)[0]


def test_argument_rules_of_the_entry_points():
    """every NLDPC_EINVAL / NLDPC_EUNSUPPORTED case; the launches reject them before touching a device (the pointers
    here are host memory and never dereferenced)"""
    from nldpc import _lib
    Lb = _lib.lib()
    EINVAL, EUNS = _lib.NLDPC_EINVAL, _lib.NLDPC_EUNSUPPORTED
    buf = np.zeros(256, dtype=np.uint8)
    p = buf.ctypes.data
    assert p % 8 == 0
    par = ctypes.c_uint32(0)
    # nldpc_crc_ref
    assert Lb.nldpc_crc_ref(0, p, 8, 8, ctypes.byref(par)) == _lib.NLDPC_OK
    for crc in (-1, 6, 24):
        assert Lb.nldpc_crc_ref(crc, p, 8, 8, ctypes.byref(par)) == EINVAL
    assert Lb.nldpc_crc_ref(0, None, 8, 8, ctypes.byref(par)) == EINVAL
    assert Lb.nldpc_crc_ref(0, p, 8, 8, None) == EINVAL
    for A, chunk in ((0, 8), (-1, 8), (8, 0), (8, -3)):
        assert Lb.nldpc_crc_ref(0, p, A, chunk, ctypes.byref(par)) == EINVAL
    assert b"nldpc_crc_ref" in Lb.nldpc_last_error()
    # nldpc_crc_attach(crc, a, B, A, W, seed, b_offset, info, stream)
    big = 2 ** 31
    for args in ((6, p, 2, 8, 32, 1, 0, p), (-1, p, 2, 8, 32, 1, 0, p),
                 (0, p, 0, 8, 32, 1, 0, p), (0, p, -1, 8, 32, 1, 0, p),     # B >= 1
                 (0, p, 2, 0, 32, 1, 0, p), (0, None, 2, -4, 32, 1, 0, p),  # A >= 1
                 (0, p, 2, 9, 32, 1, 0, p), (3, p, 2, 17, 32, 1, 0, p), (5, None, 2, 27, 32, 1, 0, p),  # A + L <= W
                 (0, p, 2, 8, big, 1, 0, p), (0, p, 2, 8, 2 ** 40, 1, 0, p),  # W < 2^31
                 (0, p, 2, 8, 32, 1, -1, p),                                  # b_offset >= 0
                 (0, p, 2, 8, 32, 1, 0, None)):                               # info
        assert Lb.nldpc_crc_attach(*args, None) == EINVAL, args
    assert b"nldpc_crc_attach" in Lb.nldpc_last_error()
    for args in ((0, p, big, 8, 32, 1, 0, p), (0, None, 2, 8, 32, 1, big, p)):
        assert Lb.nldpc_crc_attach(*args, None) == EUNS, args
    # nldpc_crc_check(crc, llr, bits, B, A, stride, convention, ref, ref_stride, ok, counts, stream)
    for args in ((6, p, None, 2, 8, 32, 0, None, 0, p, None), (-1, None, p, 2, 8, 32, 0, None, 0, p, None),
                 (0, p, p, 2, 8, 32, 0, None, 0, p, None), (0, None, None, 2, 8, 32, 0, None, 0, p, None),  # one input
                 (0, p, None, 2, 8, 32, 0, None, 0, None, None),       # ok or counts
                 (0, p, None, 0, 8, 32, 0, None, 0, p, None), (0, None, p, -2, 8, 32, 0, None, 0, p, None),  # B >= 1
                 (0, p, None, 2, 0, 32, 0, None, 0, p, None),          # A >= 1
                 (0, p, None, 2, 8, 31, 0, None, 0, p, None), (3, None, p, 2, 8, 23, 0, None, 0, p, None),  # stride
                 (0, p, None, 2, big - 24, 2 ** 32, 0, None, 0, p, None),  # A + L < 2^31
                 (0, p, None, 2, 8, 32, 2, None, 0, p, None), (0, None, p, 2, 8, 32, -1, None, 0, p, None),  # convention
                 (0, p, None, 2, 8, 32, 0, p, 31, p, None),            # ref_stride
                 (0, p + 2, None, 2, 8, 32, 0, None, 0, p, None),      # llr alignment
                 (0, p, None, 2, 8, 32, 0, None, 0, None, p + 4)):     # counts alignment
        assert Lb.nldpc_crc_check(*args, None) == EINVAL, args
    assert b"nldpc_crc_check" in Lb.nldpc_last_error()
    assert Lb.nldpc_crc_check(0, p, None, big, 8, 32, 0, None, 0, p, None, None) == EUNS


def test_python_argument_errors():
    import torch
    from nldpc.crc import attach, check, first_pass, parity, payload_len

    class G:  # (the dimensions of BG2 z=16)
        K, Z = 10, 16

    assert payload_len(G, "24A") == 136 and payload_len(G, "16", 24) == 120
    for bad in (dict(crc="24"), dict(crc=0), dict(crc="24A", n_filler=-1), dict(crc="24A", n_filler=137),
                dict(crc="24A", n_filler="3"), dict(crc="24A", n_filler=None), dict(crc="24A", n_filler=1.5),
                dict(crc="24A", n_filler=float("inf"))):
        with pytest.raises(ValueError):
            payload_len(G, **bad)
    bits = np.ones(8, dtype=np.uint8)
    for bad in (lambda: parity(bits, "24D"), lambda: parity(bits, "16", chunk=0), lambda: parity(bits[:0], "16"),
                lambda: parity(bits.reshape(2, 2, 2), "16")):
        with pytest.raises(ValueError):
            bad()
    # a CPU tensor is refused (there is no CPU path), before anything is launched
    cpu_bits = torch.zeros((2, 40), dtype=torch.uint8)
    cpu_llr = torch.zeros((2, 40))
    for bad in (lambda: attach(cpu_bits, "16"), lambda: attach(None, "16", B=2, A=8, device="cpu"),
                lambda: attach(None, "16"), lambda: attach(None, "16", B=0, A=8), lambda: attach(None, "16", B=2, A=0),
                lambda: attach(None, "16", B=2, A=20, W=35), lambda: attach(None, "16", B=2, A=8, W=161, graph=G),
                lambda: attach(None, "16", B=2, A=8, b_offset=-1), lambda: attach(None, "nope", B=2, A=8),
                lambda: attach(None, "16", B="2", A=8), lambda: attach(None, "16", B=2, A=8, W="40"),
                lambda: check(cpu_llr, "16", "8"), lambda: check(cpu_llr, "16", None), lambda: parity(bits, "16", chunk="8"),
                lambda: check(cpu_llr, "16", 8), lambda: check(cpu_bits, "16", 8), lambda: check([], "16", 8),
                lambda: check(cpu_llr, "16", 8, convention=2), lambda: check(cpu_llr, "16", 0),
                lambda: first_pass([cpu_llr, cpu_llr], "16", 8)):
        with pytest.raises(ValueError):
            bad()
