// The length-31 Gold sequence of 3GPP TS 38.211 §5.2.1 as inline functions shared by the host (nldpc_gold_ref) and the
// kernels of nldpc_scramble.hip / nldpc_modulation.hip: the same functions jump, step and extract on both sides, so the
// arithmetic is testable without a device.
//
//   x1(n+31) = x1(n+3) ^ x1(n),                      x1(0) = 1, x1(1..30) = 0
//   x2(n+31) = x2(n+3) ^ x2(n+2) ^ x2(n+1) ^ x2(n),  x2(i) = (c_init >> i) & 1, i < 31
//   c(n) = x1(n + 1600) ^ x2(n + 1600)
//
// A register's STATE at n is the 31-bit word with x(n + j) in bit j.  Its characteristic polynomial is
// p(x) = x^31 + (the taps); with r = x^n mod p = sum_k r_k x^k the recurrence gives x(n + j) = XOR_{k: r_k = 1} x(k + j),
// so the state at any n is the XOR of the windows [k, k + 31) of the sequence's first 61 bits selected by r
// (gold_jump).  r comes from crc_xpow of nldpc_crc.h with L = 31: a remainder there is left-aligned, r_k in bit k + 1.
//
// A packed row holds bit n of c in bit n & 31 of word n >> 5.
#pragma once

#include <stdint.h>

#include "nldpc_crc.h"

#define NLDPC_GOLD_HD NLDPC_CRC_HD

namespace nldpc {

constexpr int kGoldL = 31;
constexpr uint32_t kGoldPoly1 = 0x12u;  // x^31 + x^3 + 1, without the leading term, left-aligned
constexpr uint32_t kGoldPoly2 = 0x1Eu;  // x^31 + x^3 + x^2 + x + 1
constexpr uint32_t kGoldInit1 = 1u;     // the state of x1 at 0
constexpr uint64_t kGoldNc = 1600;
constexpr uint32_t kGoldMask = 0x7FFFFFFFu;

// x(n + 31 + i) in bit i, from v with x(n + i) in bit i: valid up to 3 bits short of v's valid bits
NLDPC_GOLD_HD uint64_t gold_feedback(uint64_t v, uint32_t poly) {
    return poly == kGoldPoly1 ? v ^ (v >> 3) : v ^ (v >> 1) ^ (v >> 2) ^ (v >> 3);
}

// x(n) .. x(n + 63) from the state at n, word-parallel: 31 bits give the next 28, the 59 the last 5
NLDPC_GOLD_HD uint64_t gold_expand(uint32_t state, uint32_t poly) {
    uint64_t v = state & kGoldMask;
    v |= (gold_feedback(v, poly) & 0xFFFFFFFull) << 31;
    v |= ((gold_feedback(v, poly) >> 28) & 0x1Full) << 59;
    return v;
}

// the state at n of the register that starts from `init` (its state at 0)
NLDPC_GOLD_HD uint32_t gold_jump(uint32_t init, uint64_t n, uint32_t poly) {
    const uint64_t head = gold_expand(init, poly);  // (its first 61 bits are used)
    uint32_t r = crc_xpow(n, poly, kGoldL) >> 1;    // r_k in bit k
    uint32_t s = 0;
    for (int k = 0; k < kGoldL; ++k, r >>= 1) s ^= (r & 1u) ? (uint32_t)(head >> k) : 0u;
    return s & kGoldMask;
}

// both registers at the sequence position n of c (n + 1600 of x1 and x2); c_init's low 31 bits are used
NLDPC_GOLD_HD void gold_seek(uint32_t c_init, uint64_t n, uint32_t& s1, uint32_t& s2) {
    s1 = gold_jump(kGoldInit1, n + kGoldNc, kGoldPoly1);
    s2 = gold_jump(c_init & kGoldMask, n + kGoldNc, kGoldPoly2);
}

// the next 32 bits of c (the first in bit 0); both states advance by 32
NLDPC_GOLD_HD uint32_t gold_next32(uint32_t& s1, uint32_t& s2) {
    const uint64_t v1 = gold_expand(s1, kGoldPoly1), v2 = gold_expand(s2, kGoldPoly2);
    s1 = (uint32_t)(v1 >> 32) & kGoldMask;
    s2 = (uint32_t)(v2 >> 32) & kGoldMask;
    return (uint32_t)(v1 ^ v2);
}

// bits [off, off + k) of a packed row, the first in bit 0; k <= 8, and they may straddle two words (the second is read
// only then, so nothing beyond the word of bit off + k - 1 is touched)
NLDPC_GOLD_HD uint32_t gold_bits(const uint32_t* row, int64_t off, int k) {
    const int64_t w = off >> 5;
    const int s = (int)(off & 31);
    uint32_t v = row[w] >> s;
    if (s + k > 32) v |= row[w + 1] << (32 - s);
    return v & ((1u << k) - 1u);
}

}  // namespace nldpc
