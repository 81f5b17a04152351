// CRC attachment and checking of coded blocks (3GPP TS 38.212 §5.1; include/nldpc.h): nldpc_crc_ref (host),
// nldpc_crc_attach, nldpc_crc_check.  The arithmetic is the inline functions of nldpc_crc.h on both sides.
//
// A wave owns a row (4 rows per workgroup, grid-stride over the rows).  The row's n bits are right-aligned in
// S = ceil(n / 2048) steps of 2048 bits -- the leading zeros this adds do not change a remainder --, so step s covers the
// row's bits [2048 s - pad, 2048 (s + 1) - pad), pad = 2048 S - n.  In a step lane l holds word l of the step's 64 32-bit
// words.  Over the steps it carries the remainder of ITS words in Horner form, acc = acc * x^2048 xor R(word): R(word) is
// four look-ups in the byte table, the multiplication by the fixed x^2048 three look-ups in tables of b * x^2048 for the
// remainder's bytes (all in LDS, built from crc_table_entry / crc_mul at kernel start; CDNA has no carry-less
// multiply).  After the last step the lane multiplies by x^(32 (63 - l)) mod g, the bits behind its word inside a step
// (crc_mul, L shift-and-XOR steps, against a per-lane constant from the host), and the wave XORs the 64 products
// together: one general multiplication and one reduction per row.
//
// How the words are made (every load instruction of a wave covers consecutive addresses):
//   x4   uint8 rows whose step starts on a 4-byte boundary of memory: 8 loads of 4 elements per lane (lane l reads
//        elements 256 q + 4 l .. + 3), a ballot per element slot, and the lane that owns word 8 q + j picks byte j of
//        the four masks and interleaves their bits (crc_spread8);
//   x1   fp32 rows (4 bytes per lane already; a form with 16 per lane measured no faster) and uint8
//        rows of any other alignment (an odd stride, an odd A): 32 loads of one element per lane (lane l reads element
//        64 k + l), a ballot each, two words per ballot;
//   drawn payloads: a lane shifts its word out of the step's Philox words, which the wave keeps in LDS.
// The attach kernel writes a step's bytes back the same two ways (4 per lane after a shuffle, or 1 per lane).  Only a
// row's first step can hold padding (PAD): the others skip the index tests.  A padded step goes four elements at a time
// only when the padding is whole groups of four (otherwise x1), so no load or store touches an address outside the
// row's elements: nothing outside [B][stride] is read, nothing outside the outputs written.
#include <hip/hip_runtime.h>

#include "nldpc_crc.h"
#include "nldpc_crc_dev.h"
#include "nldpc_internal.h"
#include "nldpc_philox.h"

// a variant measured in DESIGN §4.4 F9: NLDPC_CRC_MAX_BLOCKS is the grid the rows are strided over (1024 and 4096 were
// the others; NLDPC_CRC_X4 is in nldpc_crc_dev.h)
#ifndef NLDPC_CRC_MAX_BLOCKS
#define NLDPC_CRC_MAX_BLOCKS 2048
#endif

namespace nldpc {
constexpr int kCrcThreads = 256;
constexpr int kCrcRows = kCrcThreads / 64;        // rows (waves) per workgroup
constexpr int kCrcMaxBlocks = NLDPC_CRC_MAX_BLOCKS;  // more rows: grid-stride
constexpr uint32_t kCrcEncTag = 0x454E4331u;  // the encoder's info-bit stream (nldpc_aux.hip kEncTag)
constexpr int kCrcRndWords = 68;  // a step's 2048 bits touch at most 17 Philox counters of 128 bits

struct CrcArgs {
    uint32_t poly;        // left-aligned
    int32_t L;
    uint32_t x2048;       // x^2048 mod g
    uint32_t lane_c[64];  // x^(32 (63 - l)) mod g
    int64_t B, A;
    // check
    const void* in;   // [B][stride] fp32 or uint8
    int64_t stride;
    int32_t convention;
    const uint8_t* ref;
    int64_t ref_stride;
    uint8_t* ok;
    unsigned long long* counts;
    // attach
    const uint8_t* a;  // [B][A] or nullptr
    uint8_t* info;     // [B][W]
    int64_t W, b_offset;
    uint64_t seed;
};

// the tables into LDS (256 threads, one entry of each); returns the calling lane's constant
__device__ __forceinline__ uint32_t crc_setup(const CrcArgs& a, CrcTables& t, bool steps) {
    t.byte[threadIdx.x] = crc_table_entry(threadIdx.x, a.poly);
    if (steps) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t.mul[k][threadIdx.x] = crc_mul(a.x2048, threadIdx.x << (24 - 8 * k), a.poly, a.L);
    }
    __syncthreads();
    return a.lane_c[threadIdx.x & 63];
}

// the row's remainder from the 64 running remainders, the same value in all 64 lanes
__device__ __forceinline__ uint32_t crc_finish(uint32_t acc, uint32_t lane_c, const CrcArgs& a) {
    uint32_t r = crc_mul(acc, lane_c, a.poly, a.L);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r ^= __shfl_xor(r, off, 64);
    return r;
}

template <class T>
__global__ __launch_bounds__(kCrcThreads) void crc_check_kernel(CrcArgs a) {
    __shared__ CrcTables tab;
    const int64_t n = a.A + a.L, S = (n + 2047) >> 11, pad = (S << 11) - n;
    const uint32_t lane_c = crc_setup(a, tab, S > 1);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long c_fail = 0, c_undet = 0, c_err = 0;
    for (int64_t row = (int64_t)blockIdx.x * kCrcRows + wid; row < a.B; row += (int64_t)gridDim.x * kCrcRows) {
        const T* src = static_cast<const T*>(a.in) + row * a.stride;
        const uint8_t* rr = a.ref ? a.ref + row * a.ref_stride : nullptr;
        uint32_t acc = 0;
        bool diff = false;
        for (int64_t s = 0; s < S; ++s) {
            const int64_t base = (s << 11) - pad;
            const uint32_t w = crc_words(src, base, lane, a.convention);
            if (rr) diff |= w != crc_words(rr, base, lane, 0);
            acc = crc_accumulate(acc, s == 0, w, tab);
        }
        const bool pass = crc_finish(acc, lane_c, a) == 0, err = __ballot(diff) != 0;
        if (a.ok && lane == 0) a.ok[row] = pass ? 1 : 0;
        c_fail += !pass;
        c_undet += pass && err;
        c_err += err;
    }
    if (a.counts) {  // (the same in every thread) the workgroup's sums first: at most three atomics per workgroup
        __shared__ unsigned long long part[kCrcRows][3];
        if (lane == 0) part[wid][0] = c_fail, part[wid][1] = c_undet, part[wid][2] = c_err;
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned long long sum = 0;
#pragma unroll
            for (int r = 0; r < kCrcRows; ++r) sum += part[r][threadIdx.x];
            if (sum) atomicAdd(&a.counts[threadIdx.x], sum);
        }
    }
}

// payload copy, parity and filler zeros of a row in one pass
__global__ __launch_bounds__(kCrcThreads) void crc_attach_kernel(CrcArgs a) {
    __shared__ CrcTables tab;
    __shared__ uint32_t rnd_all[kCrcRows * kCrcRndWords];
    const int64_t n = a.A, S = (n + 2047) >> 11, pad = (S << 11) - n, Wq = (a.W + 127) >> 7;
    const uint32_t lane_c = crc_setup(a, tab, S > 1);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t* rnd = rnd_all + wid * kCrcRndWords;  // this wave's Philox words of the current step
    for (int64_t row = (int64_t)blockIdx.x * kCrcRows + wid; row < a.B; row += (int64_t)gridDim.x * kCrcRows) {
        const uint8_t* src = a.a ? a.a + row * a.A : nullptr;
        uint8_t* dst = a.info + row * a.W;
        uint32_t acc = 0;
        for (int64_t s = 0; s < S; ++s) {
            const int64_t base = (s << 11) - pad;
            uint32_t w;
            if (src) {
                w = crc_words(src, base, lane, 0);
            } else {
                // bit i of the row is bit (i & 31) of word (i >> 5) & 3 of the row's Philox counter i >> 7: the step's
                // bits lie in at most 17 counters from cb on, one per lane.  (The wave reads what its other lanes
                // wrote, and rewrites it next step: LDS operations of a wave complete in order.)
                const int64_t cb = (base > 0 ? base : 0) >> 7;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (lane < kCrcRndWords / 4 && cb + lane < Wq) {
                    const uint64_t ctr = (uint64_t)(a.b_offset + row) * (uint64_t)Wq + (uint64_t)(cb + lane);
                    const U4 r = philox4x32_10(U4{(uint32_t)ctr, (uint32_t)(ctr >> 32), kCrcEncTag, 0u}, (uint32_t)a.seed,
                                               (uint32_t)(a.seed >> 32));
                    rnd[4 * lane] = r.x, rnd[4 * lane + 1] = r.y, rnd[4 * lane + 2] = r.z, rnd[4 * lane + 3] = r.w;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                w = crc_words_stream(rnd, base, 4 * cb, lane);
            }
            if (NLDPC_CRC_X4 && (reinterpret_cast<uintptr_t>(dst + base) & 3) == 0 && (base >= 0 || (base & 3) == 0)) {
                if (base < 0) crc_store_x4<true>(dst, base, w, lane);
                else crc_store_x4<false>(dst, base, w, lane);
            } else {
                if (base < 0) crc_store_x1<true>(dst, base, w, lane);
                else crc_store_x1<false>(dst, base, w, lane);
            }
            acc = crc_accumulate(acc, s == 0, w, tab);
        }
        const uint32_t run = crc_finish(acc, lane_c, a);
        if (lane < a.L) dst[a.A + lane] = (uint8_t)((run >> (31 - lane)) & 1u);  // p_0 first
        for (int64_t j = a.A + a.L + lane; j < a.W; j += 64) dst[j] = 0;
    }
}

static void crc_fill(CrcArgs& a, int32_t crc) {
    const CrcConsts& c = crc_consts(crc);
    a.poly = crc_poly(crc);
    a.L = crc_len(crc);
    a.x2048 = c.x2048;
    for (int l = 0; l < 64; ++l) a.lane_c[l] = c.lane_c[l];
}

static int crc_launch(const char* who, void (*k)(CrcArgs), const CrcArgs& a, void* stream) {
    const int64_t want = (a.B + kCrcRows - 1) / kCrcRows;
    const int64_t blocks = want < kCrcMaxBlocks ? want : kCrcMaxBlocks;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kCrcThreads), 0, static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, who);
}

}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_crc_ref(int32_t crc, const uint8_t* bits, int64_t A, int64_t chunk, uint32_t* parity) {
    if (!crc_ok(crc)) return fail(NLDPC_EINVAL, "nldpc_crc_ref: crc is one of enum nldpc_crc");
    if (!bits || !parity || A <= 0 || chunk <= 0) return fail(NLDPC_EINVAL, "nldpc_crc_ref: bad argument");
    const uint32_t poly = crc_poly(crc);
    const int L = crc_len(crc);
    uint32_t tab[256];
    for (uint32_t v = 0; v < 256; ++v) tab[v] = crc_table_entry(v, poly);
    uint32_t acc = 0;
    for (int64_t s = 0; s < A; s += chunk) {
        const int64_t e = A - s < chunk ? A : s + chunk;
        acc ^= crc_mul(crc_piece(bits, s, e, poly, tab), crc_xpow((uint64_t)(A - e), poly, L), poly, L);
    }
    *parity = acc >> (32 - L);
    return NLDPC_OK;
}

extern "C" int nldpc_crc_attach(int32_t crc, const uint8_t* a, int64_t B, int64_t A, int64_t W, uint64_t seed,
                                int64_t b_offset, uint8_t* info, void* stream) {
    if (!crc_ok(crc)) return fail(NLDPC_EINVAL, "nldpc_crc_attach: crc is one of enum nldpc_crc");
    if (!info || B <= 0 || A <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, "nldpc_crc_attach: bad argument");
    if (W >= (int64_t)1 << 31 || A > W - crc_len(crc))
        return fail(NLDPC_EINVAL, "nldpc_crc_attach: A + L <= W < 2^31 does not hold");
    if (B >= (int64_t)1 << 31 || b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, "nldpc_crc_attach: too large");
    CrcArgs k{};
    crc_fill(k, crc);
    k.B = B;
    k.A = A;
    k.a = a;
    k.info = info;
    k.W = W;
    k.b_offset = b_offset;
    k.seed = seed;
    return crc_launch("nldpc_crc_attach", crc_attach_kernel, k, stream);
}

extern "C" int nldpc_crc_check(int32_t crc, const float* llr, const uint8_t* bits, int64_t B, int64_t A, int64_t stride,
                               int32_t convention, const uint8_t* ref, int64_t ref_stride, uint8_t* ok, int64_t* counts,
                               void* stream) {
    if (!crc_ok(crc)) return fail(NLDPC_EINVAL, "nldpc_crc_check: crc is one of enum nldpc_crc");
    if ((llr != nullptr) == (bits != nullptr)) return fail(NLDPC_EINVAL, "nldpc_crc_check: exactly one of llr and bits is given");
    if (!ok && !counts) return fail(NLDPC_EINVAL, "nldpc_crc_check: ok and counts are both NULL");
    if (convention != 0 && convention != 1) return fail(NLDPC_EINVAL, "nldpc_crc_check: convention is 0 or 1");
    if (B <= 0 || A <= 0) return fail(NLDPC_EINVAL, "nldpc_crc_check: bad argument");
    const int64_t n = A + crc_len(crc);
    if (A >= (int64_t)1 << 31 || n >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, "nldpc_crc_check: A + L must be below 2^31");
    if (stride < n || (ref && ref_stride < n)) return fail(NLDPC_EINVAL, "nldpc_crc_check: a stride is below A + L");
    if (llr && (reinterpret_cast<uintptr_t>(llr) & 3)) return fail(NLDPC_EINVAL, "nldpc_crc_check: llr must be 4-byte aligned");
    if (counts && (reinterpret_cast<uintptr_t>(counts) & 7)) return fail(NLDPC_EINVAL, "nldpc_crc_check: counts must be 8-byte aligned");
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, "nldpc_crc_check: too large");
    CrcArgs k{};
    crc_fill(k, crc);
    k.B = B;
    k.A = A;
    k.in = llr ? static_cast<const void*>(llr) : static_cast<const void*>(bits);
    k.stride = stride;
    k.convention = convention;
    k.ref = ref;
    k.ref_stride = ref_stride;
    k.ok = ok;
    k.counts = reinterpret_cast<unsigned long long*>(counts);
    return crc_launch("nldpc_crc_check", llr ? crc_check_kernel<float> : crc_check_kernel<uint8_t>, k, stream);
}
