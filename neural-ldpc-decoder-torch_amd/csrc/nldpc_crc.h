// The six cyclic redundancy checks of 3GPP TS 38.212 §5.1 as inline functions shared by the host (nldpc_crc_ref) and the
// kernels of nldpc_crc.hip: the same functions take a remainder on both sides, so the arithmetic is testable without a
// device.
//
// g(x) = x^L + (the polynomial word); bits a_0 .. a_{n-1} are the polynomial a_0 x^{n-1} + .. + a_{n-1}.  The register
// starts at zero, nothing is reflected and there is no final XOR, so
//   R(a) = a(x) * x^L mod g(x)
// is the parity of a (p_0 the coefficient of x^{L-1}), leading zero bits do not change it, and R over a block with its
// parity attached is zero exactly when g divides the block (x is invertible mod g: g has the constant term 1).
//
// A remainder lives LEFT-ALIGNED in a 32-bit word: the coefficient of x^{L-1} in bit 31, bits below 32 - L zero.  In
// that form one bit-serial step, the byte table and the table-driven update are the same code for every L (L = 6 < 8
// included); only the multiplication needs L.
//
// R is linear over GF(2): for the concatenation u | v with |v| = n bits, R(u | v) = R(u) * x^n mod g  xor  R(v).  That
// is what lets a row be cut into pieces whose remainders are taken independently (crc_mul, crc_xpow).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NLDPC_CRC_HD __host__ __device__ __forceinline__
#else
#define NLDPC_CRC_HD inline
#endif

namespace nldpc {

constexpr int kCrcKinds = 6;  // enum nldpc_crc: 24A, 24B, 24C, 16, 11, 6

NLDPC_CRC_HD bool crc_ok(int id) { return id >= 0 && id < kCrcKinds; }
NLDPC_CRC_HD int crc_len(int id) { return id <= 2 ? 24 : id == 3 ? 16 : id == 4 ? 11 : 6; }
// the polynomial without its leading term, left-aligned
NLDPC_CRC_HD uint32_t crc_poly(int id) {
    const uint32_t g = id == 0 ? 0x864CFBu : id == 1 ? 0x800063u : id == 2 ? 0xB2B117u : id == 3 ? 0x1021u : id == 4 ? 0x621u : 0x21u;
    return g << (32 - crc_len(id));
}

// r * x mod g
NLDPC_CRC_HD uint32_t crc_xtime(uint32_t r, uint32_t poly) { return (r << 1) ^ ((r & 0x80000000u) ? poly : 0u); }

// the register after one more message bit: R(a | bit) from r = R(a)
NLDPC_CRC_HD uint32_t crc_step(uint32_t r, uint32_t bit, uint32_t poly) { return crc_xtime(r ^ (bit << 31), poly); }

// entry v of the byte table: R of the 8 bits of v, most significant first
NLDPC_CRC_HD uint32_t crc_table_entry(uint32_t v, uint32_t poly) {
    uint32_t r = v << 24;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = crc_xtime(r, poly);
    return r;
}

// R(a | the 32 bits of w, most significant first) from r = R(a): four look-ups in the byte table
template <class Table>
NLDPC_CRC_HD uint32_t crc_word(uint32_t r, uint32_t w, const Table& tab) {
    r ^= w;
    r = (r << 8) ^ tab[r >> 24];
    r = (r << 8) ^ tab[r >> 24];
    r = (r << 8) ^ tab[r >> 24];
    r = (r << 8) ^ tab[r >> 24];
    return r;
}

// a * b mod g for two remainders: L shift-and-XOR steps (Horner over the coefficients of b, x^{L-1} first)
NLDPC_CRC_HD uint32_t crc_mul(uint32_t a, uint32_t b, uint32_t poly, int L) {
    uint32_t acc = 0;
    for (int k = 0; k < L; ++k) {
        acc = crc_xtime(acc, poly) ^ ((b & 0x80000000u) ? a : 0u);
        b <<= 1;
    }
    return acc;
}

// x^n mod g, by squaring
NLDPC_CRC_HD uint32_t crc_xpow(uint64_t n, uint32_t poly, int L) {
    uint32_t acc = 1u << (32 - L);  // x^0
    uint32_t sq = 1u << (33 - L);   // x^1 (L >= 2)
    while (n) {
        if (n & 1) acc = crc_mul(acc, sq, poly, L);
        sq = crc_mul(sq, sq, poly, L);
        n >>= 1;
    }
    return acc;
}

}  // namespace nldpc
