// Device and host helpers shared by the CRC kernels (nldpc_crc.hip) and the transport-block kernels (nldpc_tb.hip):
// how a wave turns a 2048-element step of a row into 64 words and back, the LDS tables, the per-polynomial launch
// constants and the host remainder of a piece.  The layout of a step is described at the top of nldpc_crc.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "nldpc_crc.h"

// a variant measured in DESIGN §4.4 F9: NLDPC_CRC_X4 = 0 takes the one-element path everywhere
#ifndef NLDPC_CRC_X4
#define NLDPC_CRC_X4 1
#endif

namespace nldpc {
// the byte table and, for rows of more than one step, the three tables of (b << 24, 16, 8) * x^2048
struct CrcTables {
    uint32_t byte[256];
    uint32_t mul[3][256];
};

__device__ __forceinline__ bool crc_hard(float x, int convention) { return convention == 0 ? x > 0.f : x < 0.f; }
__device__ __forceinline__ bool crc_hard(uint8_t x, int) { return x != 0; }

// four consecutive bytes as one load
__device__ __forceinline__ bool crc_quad_bit(uint32_t v, int c) { return ((v >> (8 * c)) & 0xFFu) != 0; }

// bit t of b (8 bits) to bit 4 t
__device__ __forceinline__ uint32_t crc_spread8(uint32_t b) {
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    return (b | (b << 3)) & 0x11111111u;
}

// acc * x^2048 mod g (L <= 24: the remainder's low byte is zero)
__device__ __forceinline__ uint32_t crc_mul_x2048(uint32_t acc, const CrcTables& t) {
    return t.mul[0][acc >> 24] ^ t.mul[1][(acc >> 16) & 0xFFu] ^ t.mul[2][(acc >> 8) & 0xFFu];
}

// The word functions return lane l's word of the step that starts at element `base` of the row with the step's element
// 32 l + t in bit t; elements before 0 are padding (bit 0) and exist only when PAD.

// one element per lane and load
template <class T, bool PAD>
__device__ __forceinline__ uint32_t crc_words_x1(const T* src, int64_t base, int lane, int convention) {
    const int64_t i0 = base + lane;
    T v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = !PAD || i0 + 64 * k >= 0 ? src[i0 + 64 * k] : T(0);  // (0 is bit 0 either way)
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const unsigned long long m = __ballot(crc_hard(v[k], convention));
        if ((lane >> 1) == k) w = (lane & 1) ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
    return w;
}

// 4 bytes per lane and load; src + base is on a 4-byte boundary of memory, and base is a multiple of 4 when PAD
template <bool PAD>
__device__ __forceinline__ uint32_t crc_words_x4(const uint8_t* src, int64_t base, int lane) {
    const int64_t i0 = base + 4 * lane;
    uint32_t v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = !PAD || i0 + 256 * q >= 0 ? *reinterpret_cast<const uint32_t*>(src + (i0 + 256 * q)) : 0u;
    unsigned long long sel[4] = {0, 0, 0, 0};  // the masks of the run q = lane / 8: bit l of sel[c] is element 4 l + c
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long m = __ballot(crc_quad_bit(v[q], c));  // (a zero group is bit 0)
            if ((lane >> 3) == q) sel[c] = m;
        }
    }
    const int sh = 8 * (lane & 7);  // word 8 q + j of the step is elements 32 j .. 32 j + 31 of run q: lanes 8 j .. 8 j + 7
    uint32_t w = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) w |= crc_spread8((uint32_t)(sel[c] >> sh) & 0xFFu) << c;
    return w;
}

// (the same branches in every lane; the alignment is that of every step of the row: a step is 2048 elements.  A padded
// step whose padding is no multiple of 4 would begin inside a group of four: it goes one element at a time)
__device__ __forceinline__ uint32_t crc_words(const uint8_t* src, int64_t base, int lane, int) {
    if (NLDPC_CRC_X4 && (reinterpret_cast<uintptr_t>(src + base) & 3) == 0 && (base >= 0 || (base & 3) == 0))
        return base < 0 ? crc_words_x4<true>(src, base, lane) : crc_words_x4<false>(src, base, lane);
    return base < 0 ? crc_words_x1<uint8_t, true>(src, base, lane, 0) : crc_words_x1<uint8_t, false>(src, base, lane, 0);
}
__device__ __forceinline__ uint32_t crc_words(const float* src, int64_t base, int lane, int convention) {
    return base < 0 ? crc_words_x1<float, true>(src, base, lane, convention) : crc_words_x1<float, false>(src, base, lane, convention);
}

// the row's bit i is bit (i & 31) of word (i >> 5) of a stream, and rnd holds the stream's words from word first_word on
// (base < 0: first_word == 0)
__device__ __forceinline__ uint32_t crc_words_stream(const uint32_t* rnd, int64_t base, int64_t first_word, int lane) {
    const int64_t i0 = base + 32 * lane;
    uint32_t v = 0;
    if (i0 >= 0) {
        const int k = (int)((i0 >> 5) - first_word), sh = (int)(i0 & 31);
        v = rnd[k] >> sh;
        if (sh) v |= rnd[k + 1] << (32 - sh);  // (the word of bit i0 + 31, inside the row)
    } else if (i0 > -32) {
        v = rnd[0] << (int)(-i0);
    }
    return v;
}

// one more step's word into the lane's running remainder (element 0 of the word is its most significant bit)
__device__ __forceinline__ uint32_t crc_accumulate(uint32_t acc, bool first, uint32_t w, const CrcTables& t) {
    const uint32_t r = crc_word(0u, __brev(w), t.byte);
    return first ? r : crc_mul_x2048(acc, t) ^ r;
}

// the step's bits back to memory as bytes 0 / 1, elements before 0 not written: one byte per lane and store ..
template <bool PAD>
__device__ __forceinline__ void crc_store_x1(uint8_t* dst, int64_t base, uint32_t w, int lane) {
    const int64_t i0 = base + lane;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const uint32_t ww = __shfl(w, 2 * k + (lane >> 5), 64);
        if (!PAD || i0 + 64 * k >= 0) dst[i0 + 64 * k] = (uint8_t)((ww >> (lane & 31)) & 1u);
    }
}

// .. or four; dst + base is on a 4-byte boundary, and base is a multiple of 4 when PAD
template <bool PAD>
__device__ __forceinline__ void crc_store_x4(uint8_t* dst, int64_t base, uint32_t w, int lane) {
    const int64_t i0 = base + 4 * lane;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t ww = __shfl(w, 8 * q + (lane >> 3), 64);
        const uint32_t nib = (ww >> (4 * (lane & 7))) & 0xFu;  // elements 4 l .. 4 l + 3 of run q, the first in bit 0
        // bit c to bit 8 c: the 16 partial products of nib * (1 + 2^7 + 2^14 + 2^21) fall on 16 different bits
        const uint32_t v = __umul24(nib, 0x00204081u) & 0x01010101u;
        const int64_t i = i0 + 256 * q;
        if (!PAD || i >= 0) *reinterpret_cast<uint32_t*>(dst + i) = v;
    }
}

// the launch constants of the six polynomials, computed once
struct CrcConsts {
    uint32_t x2048, lane_c[64];
};
inline const CrcConsts& crc_consts(int32_t crc) {
    static const struct All {
        CrcConsts c[kCrcKinds];
        All() {
            for (int id = 0; id < kCrcKinds; ++id) {
                const uint32_t poly = crc_poly(id);
                const int L = crc_len(id);
                c[id].x2048 = crc_xpow(2048, poly, L);
                for (int l = 0; l < 64; ++l) c[id].lane_c[l] = crc_xpow((uint64_t)32 * (63 - l), poly, L);
            }
        }
    } all;
    return all.c[crc];
}

// R of bits[s, e) (any non-zero byte is 1): the leading (e - s) % 32 bits one by one, then whole words through the table
inline uint32_t crc_piece(const uint8_t* bits, int64_t s, int64_t e, uint32_t poly, const uint32_t* tab) {
    uint32_t r = 0;
    int64_t i = s;
    for (const int64_t head = s + (e - s) % 32; i < head; ++i) r = crc_step(r, bits[i] ? 1u : 0u, poly);
    for (; i < e; i += 32) {
        uint32_t w = 0;
        for (int t = 0; t < 32; ++t) w |= (bits[i + t] ? 1u : 0u) << (31 - t);
        r = crc_word(r, w, tab);
    }
    return r;
}
}  // namespace nldpc
