"""The cyclic redundancy checks of 3GPP TS 38.212 §5.1 restated in numpy as plain long division over GF(2), bit by bit:
the expected values of test_crc_host.py and test_gpu_crc.py.  Nothing here is shared with csrc/nldpc_crc.h (no table, no
chunks, no multiplication by x^n): a block is a row of 0/1 coefficients, highest power first, and wherever the current
leading coefficient is 1 the generator is subtracted (XORed) under it.

g_CRC24A(D) = D^24 + D^23 + D^18 + D^17 + D^14 + D^11 + D^10 + D^7 + D^6 + D^5 + D^4 + D^3 + D + 1
g_CRC24B(D) = D^24 + D^23 + D^6 + D^5 + D + 1
g_CRC24C(D) = D^24 + D^23 + D^21 + D^20 + D^17 + D^15 + D^13 + D^12 + D^8 + D^4 + D^2 + D + 1
g_CRC16(D)  = D^16 + D^12 + D^5 + 1
g_CRC11(D)  = D^11 + D^10 + D^9 + D^5 + 1
g_CRC6(D)   = D^6 + D^5 + 1
"""
import numpy as np

# the exponents of §5.1, leading term included
EXPONENTS = {
    "24A": (24, 23, 18, 17, 14, 11, 10, 7, 6, 5, 4, 3, 1, 0),
    "24B": (24, 23, 6, 5, 1, 0),
    "24C": (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0),
    "16": (16, 12, 5, 0),
    "11": (11, 10, 9, 5, 0),
    "6": (6, 5, 0),
}
NAMES = tuple(EXPONENTS)


def length(name) -> int:
    return EXPONENTS[name][0]


def generator(name) -> np.ndarray:
    """the L + 1 coefficients of g, x^L first"""
    L = length(name)
    g = np.zeros(L + 1, dtype=np.uint8)
    for e in EXPONENTS[name]:
        g[L - e] = 1
    return g


def remainder(block, name) -> np.ndarray:
    """[B, L] coefficients (x^{L-1} first) of block(x) mod g(x); block: [B, n] (or [n]) of 0/1, x^{n-1} first"""
    b = np.atleast_2d(np.asarray(block)).astype(np.uint8)
    assert b.max(initial=0) <= 1
    L, g = length(name), generator(name)
    n = b.shape[1]
    if n < L:  # (already a remainder)
        return np.concatenate([np.zeros((b.shape[0], L - n), np.uint8), b], axis=1)
    work = b.copy()
    for i in range(n - L):
        lead = work[:, i].astype(bool)
        work[lead, i:i + L + 1] ^= g
    return work[:, n - L:]


def parity_bits(bits, name) -> np.ndarray:
    """[B, L] parity p_0 .. p_{L-1} of the rows of bits [B, A] (any non-zero value is 1): the remainder of
    a(x) * x^L"""
    a = (np.atleast_2d(np.asarray(bits)) != 0).astype(np.uint8)
    return remainder(np.concatenate([a, np.zeros((a.shape[0], length(name)), np.uint8)], axis=1), name)


def parity_int(bits, name) -> np.ndarray:
    """int64 [B]: the parity as a number, p_0 the most significant of its L bits"""
    p = parity_bits(bits, name).astype(np.int64)
    return (p << np.arange(length(name) - 1, -1, -1)).sum(axis=1)


def attach(bits, name, W=None) -> np.ndarray:
    """uint8 [B, W]: payload as 0/1 | parity | zeros"""
    a = (np.atleast_2d(np.asarray(bits)) != 0).astype(np.uint8)
    out = np.concatenate([a, parity_bits(a, name)], axis=1)
    W = out.shape[1] if W is None else W
    assert W >= out.shape[1]
    return np.concatenate([out, np.zeros((a.shape[0], W - out.shape[1]), np.uint8)], axis=1)


def passes(block, name, A) -> np.ndarray:
    """bool [B]: the first A + L bits of every row are divisible by g"""
    b = (np.atleast_2d(np.asarray(block)) != 0).astype(np.uint8)[:, :A + length(name)]
    return ~remainder(b, name).any(axis=1)


def counts(block, name, A, ref=None) -> np.ndarray:
    """int64 [3]: CRC failures, undetected errors, block errors (the last two 0 without ref)"""
    ok = passes(block, name, A)
    n = A + length(name)
    if ref is None:
        return np.array([(~ok).sum(), 0, 0], dtype=np.int64)
    err = ((np.asarray(block) != 0)[:, :n] != (np.asarray(ref) != 0)[:, :n]).any(axis=1)
    return np.array([(~ok).sum(), (ok & err).sum(), err.sum()], dtype=np.int64)
