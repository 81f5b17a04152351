"""numpy model of Gold-sequence scrambling for the tests, written from 3GPP TS 38.211 §5.2.1 and the definitions of
include/nldpc.h, never from the library:

  gold                 c(n0) .. c(n0 + n - 1), the two recurrences run bit by bit from 0 (no jump, no packing)
  gold_far             the same window from the register states at n0 + 1600, reached by raising each register's 31 x 31
                       transition matrix over GF(2) to that power (square and multiply on numpy matrices)
  c_init               rnti * 2^15 + q * 2^14 + n_id
  pack                 bits -> words: bit n in bit n & 31 of word n >> 5, zeros beyond E
  scramble / descramble  (f != 0) ^ c per row, and the sign-bit XOR of fp32 LLRs (on the uint32 view)
"""
import functools

import numpy as np

NC = 1600


def c_init(rnti, n_id, q=0):
    return rnti * 2 ** 15 + q * 2 ** 14 + n_id


@functools.lru_cache(maxsize=None)
def _serial(ci, total):
    """c(0) .. c(total - 1), bit by bit"""
    n = total + NC
    x1 = np.zeros(n + 31, dtype=np.uint8)
    x2 = np.zeros(n + 31, dtype=np.uint8)
    x1[0] = 1
    for i in range(31):
        x2[i] = (ci >> i) & 1
    for i in range(n):
        x1[i + 31] = x1[i + 3] ^ x1[i]
        x2[i + 31] = x2[i + 3] ^ x2[i + 2] ^ x2[i + 1] ^ x2[i]
    c = x1[NC:NC + total] ^ x2[NC:NC + total]
    c.setflags(write=False)
    return c


def gold(ci, n, n0=0):
    """uint8 [n]: c(n0 + i)"""
    assert 0 <= ci < 2 ** 31
    return np.array(_serial(int(ci), int(n0 + n))[n0:n0 + n])


def _transition(taps):
    """A with state(n + 1) = A state(n) over GF(2), state(n)[j] = x(n + j): a shift, and the recurrence in the last row"""
    A = np.zeros((31, 31), dtype=np.uint8)
    for j in range(30):
        A[j, j + 1] = 1
    for t in taps:
        A[30, t] = 1
    return A


def _matpow(A, e):
    R = np.eye(31, dtype=np.uint8)
    while e:
        if e & 1:
            R = (R.astype(np.int64) @ A.astype(np.int64) % 2).astype(np.uint8)
        A = (A.astype(np.int64) @ A.astype(np.int64) % 2).astype(np.uint8)
        e >>= 1
    return R


def gold_far(ci, n, n0):
    """uint8 [n]: c(n0 + i) from the states at n0 + 1600 (matrix power), then bit by bit"""
    out = np.zeros(n, dtype=np.uint8)
    for taps, init in (((0, 3), [1] + [0] * 30), ((0, 1, 2, 3), [(ci >> i) & 1 for i in range(31)])):
        s = list((_matpow(_transition(taps), n0 + NC).astype(np.int64) @ np.array(init, dtype=np.int64)) % 2)
        for i in range(n):
            out[i] ^= s[0]
            s = s[1:] + [int(sum(s[t] for t in taps) % 2)]
    return out


def pack(bits):
    """bits [..., E] of 0 / 1 -> uint32 [..., ceil(E / 32)]"""
    bits = np.asarray(bits, dtype=np.uint8)
    E = bits.shape[-1]
    W = (E + 31) // 32
    padded = np.zeros(bits.shape[:-1] + (W * 32,), dtype=np.uint64)
    padded[..., :E] = bits
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(bits.shape[:-1] + (W, 32)) * weights).sum(axis=-1).astype(np.uint32)


def table(c_inits, E):
    """uint32 [n_seq, ceil(E / 32)]"""
    return np.stack([pack(gold(ci, E)) for ci in c_inits])


def rows(c_inits, B, E, b_offset=0):
    """uint8 [B, E]: the sequence bits of every row, row b from c_inits[(b_offset + b) % n_seq]"""
    return np.stack([gold(c_inits[(b_offset + b) % len(c_inits)], E) for b in range(B)])


def scramble(f, c_inits, b_offset=0):
    """f [B, E] bytes (non-zero = 1) -> uint8 0 / 1"""
    f = np.asarray(f)
    return ((f != 0).astype(np.uint8)) ^ rows(c_inits, f.shape[0], f.shape[1], b_offset)


def descramble(llr, c_inits, b_offset=0):
    """fp32 [B, E] -> fp32 with the sign bit XORed with the sequence bit, on the bit pattern"""
    u = np.ascontiguousarray(llr, dtype=np.float32).view(np.uint32)
    c = rows(c_inits, u.shape[0], u.shape[1], b_offset).astype(np.uint32)
    return (u ^ (c << np.uint32(31))).view(np.float32)
