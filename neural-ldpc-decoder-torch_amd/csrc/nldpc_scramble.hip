// Gold-sequence scrambling (3GPP TS 38.211 §5.2.1, §6.3.1.1, §7.3.1.1; include/nldpc.h): nldpc_gold_cinit, nldpc_gold_ref
// (host), nldpc_gold_sequence, nldpc_scramble, nldpc_descramble_llr.  The arithmetic is the inline functions of
// nldpc_gold.h on both sides.  (The fused channel that scrambles in flight is in nldpc_modulation.hip.)
//
// nldpc_gold_sequence: a thread owns a run of consecutive words of one sequence (whole 16-byte groups).  It jumps both
// registers to the run's first bit (gold_seek: x^n mod p by squaring, then the XOR of the selected windows of the
// register's first 61 bits), steps 32 bits at a time and stores four words per instruction where the group is whole and
// its address aligned (a row of an odd Wc starts off the boundary: word stores).  A jump costs about what stepping
// through 200 words does, so the host picks the run (gold_run): 4 words while that leaves the device short of
// threads, doubled until the table is kGoldThreads runs or fewer.  The jump lands on the same state whatever the run,
// so the words do not depend on the run length or the grid.
//
// nldpc_scramble / nldpc_descramble_llr: bits and LLRs of a batch are flat streams, a thread owns 16 bytes of them (16
// bits, or 4 LLRs).  It finds its row and in-row offset with one division, takes its sequence bits from the packed table
// with gold_bits when its elements lie in one row and bit by bit across a row end otherwise, and reads / writes the 16
// bytes as one vector when the address is aligned and the group whole, else by element.  A thread reads its own elements
// before it writes them, so out == in works.  Nothing outside the outputs is touched.
#include <hip/hip_runtime.h>

#include "nldpc_gold.h"
#include "nldpc_internal.h"

// words per thread of nldpc_gold_sequence: -1 = chosen per call (gold_run); a multiple of 4 = fixed; 0 = one thread steps
// through a whole sequence, the naive form tools/bench_scramble.py compares against
#ifndef NLDPC_GOLD_RUN
#define NLDPC_GOLD_RUN -1
#endif

namespace nldpc {
constexpr int kScrThreads = 256;
constexpr int kGoldRun = NLDPC_GOLD_RUN;
static_assert(kGoldRun == -1 || (kGoldRun >= 0 && kGoldRun % 4 == 0), "a run is whole 16-byte groups");
constexpr int64_t kGoldThreads = 65536;  // one wave per SIMD of the device: beyond it, longer runs instead of more jumps

struct GoldArgs {
    const int32_t* c_init;  // [n_seq]
    uint32_t* seq;          // [n_seq][Wc]
    int64_t E, Wc;
    int64_t run;   // words per thread, a multiple of 4
    int64_t runs;  // threads per sequence
    int64_t total;  // n_seq * runs
};

__global__ __launch_bounds__(kScrThreads) void gold_sequence_kernel(GoldArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kScrThreads + threadIdx.x;
    if (t >= a.total) return;
    const int64_t s = t / a.runs, w0 = (t - s * a.runs) * a.run;
    const int64_t w1 = w0 + a.run < a.Wc ? w0 + a.run : a.Wc;
    uint32_t s1, s2;
    gold_seek((uint32_t)a.c_init[s], (uint64_t)w0 << 5, s1, s2);
    uint32_t* dst = a.seq + s * a.Wc;
    const uint32_t tail = (a.E & 31) ? (1u << (a.E & 31)) - 1u : 0xFFFFFFFFu;
    for (int64_t w = w0; w < w1; w += 4) {
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = gold_next32(s1, s2);
            if (w + q == a.Wc - 1) v[q] &= tail;
        }
        if (w + 4 <= w1 && (reinterpret_cast<uintptr_t>(dst + w) & 15) == 0) {
            *reinterpret_cast<uint4*>(dst + w) = uint4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (w + q < w1) dst[w + q] = v[q];
        }
    }
}

struct ScrArgs {
    const void* in;  // [B][E] uint8 (nullable) or fp32
    void* out;
    const uint32_t* seq;  // [n_seq][Wc]
    int64_t n_seq, E, Wc, b_offset;
    int64_t total;  // B * E
};

// T = uint8_t, N = 16: out = (in != 0) ^ c;  T = uint32_t, N = 4: out = in ^ (c << 31)
template <class T, int N>
__global__ __launch_bounds__(kScrThreads) void scramble_kernel(ScrArgs a) {
    static_assert(N * sizeof(T) == 16, "a thread owns 16 bytes");
    const int64_t g0 = ((int64_t)blockIdx.x * kScrThreads + threadIdx.x) * N;
    if (g0 >= a.total) return;
    const int cnt = a.total - g0 < N ? (int)(a.total - g0) : N;
    const int64_t row = g0 / a.E, i0 = g0 - row * a.E;
    // (b_offset + row < 2^32 and n_seq < 2^31: a 32-bit remainder)
    const uint32_t* srow = a.seq + (int64_t)((uint32_t)(a.b_offset + row) % (uint32_t)a.n_seq) * a.Wc;

    union {
        uint4 q;
        T e[N];
    } v;
    v.q = uint4{0u, 0u, 0u, 0u};
    const T* src = static_cast<const T*>(a.in);
    if (src) {
        if (cnt == N && (reinterpret_cast<uintptr_t>(src + g0) & 15) == 0) {
            v.q = *reinterpret_cast<const uint4*>(src + g0);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (e < cnt) v.e[e] = src[g0 + e];
        }
    }

    uint32_t bits = 0;  // bit e: the sequence bit of element e
    if (i0 + cnt <= a.E) {
#pragma unroll
        for (int c = 0; c < N; c += 8)
            if (c < cnt) bits |= gold_bits(srow, i0 + c, cnt - c < 8 ? cnt - c : 8) << c;
    } else {  // the elements cross a row end (several when E < N)
        int64_t r = row, i = i0;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            if (e < cnt) {
                bits |= gold_bits(srow, i, 1) << e;
                if (++i == a.E) {
                    i = 0, ++r;
                    srow = a.seq + (int64_t)((uint32_t)(a.b_offset + r) % (uint32_t)a.n_seq) * a.Wc;
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const uint32_t c = (bits >> e) & 1u;
        if (sizeof(T) == 1) v.e[e] = (T)((v.e[e] != 0 ? 1u : 0u) ^ c);
        else v.e[e] = (T)((uint32_t)v.e[e] ^ (c << 31));
    }

    T* dst = static_cast<T*>(a.out);
    if (cnt == N && (reinterpret_cast<uintptr_t>(dst + g0) & 15) == 0) {
        *reinterpret_cast<uint4*>(dst + g0) = v.q;
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e)
            if (e < cnt) dst[g0 + e] = v.e[e];
    }
}

// words per thread for a table of n_seq rows of Wc words
static int64_t gold_run(int64_t n_seq, int64_t Wc) {
    if (kGoldRun == 0) return (Wc + 3) / 4 * 4;
    if (kGoldRun > 0) return kGoldRun;
    int64_t run = 4;
    while (run < Wc && n_seq * ((Wc + run - 1) / run) > kGoldThreads) run *= 2;
    return run;
}

static bool off4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// the checks the three users of a sequence table share; 0 = fine
static int scr_check(const char* who, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E, int64_t b_offset) {
    if (!seq || off4(seq)) return fail(NLDPC_EINVAL, std::string(who) + ": seq must be non-NULL and 4-byte aligned");
    if (n_seq < 1 || B < 1 || E < 1 || b_offset < 0) return fail(NLDPC_EINVAL, std::string(who) + ": bad argument");
    if (E >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, std::string(who) + ": E must be below 2^31");
    if (B >= (int64_t)1 << 31 || b_offset >= (int64_t)1 << 31 || n_seq >= (int64_t)1 << 31 ||
        n_seq * ((E + 31) >> 5) >= (int64_t)1 << 31)
        return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    return NLDPC_OK;
}

template <class T, int N>
static int scr_launch(const char* who, const void* in, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E,
                      int64_t b_offset, void* out, void* stream) {
    ScrArgs a{};
    a.in = in;
    a.out = out;
    a.seq = seq;
    a.n_seq = n_seq;
    a.E = E;
    a.Wc = (E + 31) >> 5;
    a.b_offset = b_offset;
    a.total = B * E;
    const int64_t blocks = ((a.total + N - 1) / N + kScrThreads - 1) / kScrThreads;
    if (blocks > 0x7FFFFFFF) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    hipLaunchKernelGGL((scramble_kernel<T, N>), dim3((unsigned)blocks), dim3(kScrThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, who);
}
}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_gold_cinit(int32_t rnti, int32_t q, int32_t n_id, uint32_t* c_init) {
    if (!c_init) return fail(NLDPC_EINVAL, "nldpc_gold_cinit: c_init is NULL");
    if (rnti < 0 || rnti >= 1 << 16 || (q != 0 && q != 1) || n_id < 0 || n_id >= 1024)
        return fail(NLDPC_EINVAL, "nldpc_gold_cinit: 0 <= rnti < 2^16, q in {0, 1}, 0 <= n_id < 1024");
    *c_init = ((uint32_t)rnti << 15) + ((uint32_t)q << 14) + (uint32_t)n_id;
    return NLDPC_OK;
}

extern "C" int nldpc_gold_ref(uint32_t c_init, int64_t n0, int64_t n, uint8_t* c) {
    if (!c) return fail(NLDPC_EINVAL, "nldpc_gold_ref: c is NULL");
    if (c_init >= 1u << 31) return fail(NLDPC_EINVAL, "nldpc_gold_ref: c_init must be below 2^31");
    if (n0 < 0 || n < 1 || n0 > ((int64_t)1 << 31) - n)
        return fail(NLDPC_EINVAL, "nldpc_gold_ref: n0 >= 0, n >= 1 and n0 + n <= 2^31 do not hold");
    uint32_t s1, s2;
    gold_seek(c_init, (uint64_t)n0, s1, s2);
    for (int64_t i = 0; i < n; i += 32) {
        const uint32_t w = gold_next32(s1, s2);
        for (int64_t b = 0; b < 32 && i + b < n; ++b) c[i + b] = (uint8_t)((w >> b) & 1u);
    }
    return NLDPC_OK;
}

extern "C" int nldpc_gold_sequence(const int32_t* c_init, int64_t n_seq, int64_t E, uint32_t* seq, void* stream) {
    if (!c_init || !seq || off4(c_init) || off4(seq))
        return fail(NLDPC_EINVAL, "nldpc_gold_sequence: c_init and seq must be non-NULL and 4-byte aligned");
    if (n_seq < 1 || E < 1 || E >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, "nldpc_gold_sequence: n_seq >= 1 and 1 <= E < 2^31 do not hold");
    GoldArgs a{};
    a.c_init = c_init;
    a.seq = seq;
    a.E = E;
    a.Wc = (E + 31) >> 5;
    if (n_seq >= (int64_t)1 << 31 || n_seq * a.Wc >= (int64_t)1 << 31)
        return fail(NLDPC_EUNSUPPORTED, "nldpc_gold_sequence: too large");
    a.run = gold_run(n_seq, a.Wc);
    a.runs = (a.Wc + a.run - 1) / a.run;
    a.total = n_seq * a.runs;
    const int64_t blocks = (a.total + kScrThreads - 1) / kScrThreads;
    hipLaunchKernelGGL(gold_sequence_kernel, dim3((unsigned)blocks), dim3(kScrThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, "nldpc_gold_sequence");
}

extern "C" int nldpc_scramble(const uint8_t* f, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E,
                              int64_t b_offset, uint8_t* out, void* stream) {
    if (!out) return fail(NLDPC_EINVAL, "nldpc_scramble: out is NULL");
    if (int rc = scr_check("nldpc_scramble", seq, n_seq, B, E, b_offset)) return rc;
    return scr_launch<uint8_t, 16>("nldpc_scramble", f, seq, n_seq, B, E, b_offset, out, stream);
}

extern "C" int nldpc_descramble_llr(const float* llr, const uint32_t* seq, int64_t n_seq, int64_t B, int64_t E,
                                    int64_t b_offset, float* out, void* stream) {
    if (!llr || !out || off4(llr) || off4(out))
        return fail(NLDPC_EINVAL, "nldpc_descramble_llr: llr and out must be non-NULL and 4-byte aligned");
    if (int rc = scr_check("nldpc_descramble_llr", seq, n_seq, B, E, b_offset)) return rc;
    return scr_launch<uint32_t, 4>("nldpc_descramble_llr", llr, seq, n_seq, B, E, b_offset, out, stream);
}
