// Transport blocks (3GPP TS 38.212 §5.2.2, §5.4.2.1, §5.5; include/nldpc.h): nldpc_tb_plan, nldpc_tb_lifting_size,
// nldpc_tb_er, nldpc_tb_crc_ref (host), nldpc_tb_segment, nldpc_tb_concat / nldpc_tb_deconcat, nldpc_tb_check.  The
// arithmetic is the inline functions of nldpc_tb.h and nldpc_crc.h on both sides.
//
// Layout: code block r of transport block t is row r * Btb + t of every per-code-block array (block-major).
//
// segment / check: a wave owns a code block (4 per workgroup, grid-stride), exactly as in nldpc_crc.hip, whose step
// machinery (nldpc_crc_dev.h) it shares.  The steps are right-aligned on the block's PART, the P = K' - L bits it takes
// from the TB, so the same 64 words per step serve the TB's row tb[t][r P ..) and the block's row -- both are loaded /
// stored with the four-elements-per-lane form when their address allows it and one element per lane otherwise (part
// offsets r P land on any alignment) -- and nothing before or behind a part is touched.  Each lane carries TWO running
// remainders of its words, one under CRC24B (the block's own CRC) and one under the TB's polynomial.
//   segment: the CRC24B remainder of the part is its parity, written behind it, then F zeros.
//   check:   the block passes when the parity computed from its first P hard decisions equals the 24 decisions behind
//            them (one more load of 24 lanes).  The part's TB remainder goes to work[row] (left-aligned: its low byte is
//            free, and holds the flags "part differs from ref_tb" and "block failed").  tb_check_combine_kernel, one
//            thread per TB, then takes acc = acc * x^P xor work[r * Btb + t] over r = 0 .. C-1 (tb_combine; reads
//            coalesced over t): R(TB), without the TB in memory.  It also sums the four counts.
//
// concat / deconcat: one templated ragged-row copy.  A thread owns a run of 16 bytes of one output row, placed on
// 16-byte boundaries of the output ADDRESS (rows start anywhere: E may be odd), as in rate_match_kernel: whole runs
// leave as one 16-byte store, the partial runs at the two ends of a row as element stores.  The source of a run starts
// anywhere: bytes come from the aligned dwords around them (tb_load16) where those lie inside the source array, else
// one by one, as do runs that straddle two blocks.
#include <hip/hip_runtime.h>

#include "nldpc_crc.h"
#include "nldpc_crc_dev.h"
#include "nldpc_internal.h"
#include "nldpc_rm_index.h"
#include "nldpc_tb.h"

namespace nldpc {
constexpr int kTbThreads = 256;
constexpr int kTbRows = kTbThreads / 64;  // code blocks (waves) per workgroup
constexpr int kTbMaxBlocks = 2048;        // more code blocks: grid-stride (nldpc_crc.hip's measured choice)
constexpr uint32_t kTbFlagDiff = 1u, kTbFlagCbFail = 2u;  // the low bits of a work word

// one polynomial's launch constants
struct TbPoly {
    uint32_t poly;        // left-aligned
    int32_t L;
    uint32_t x2048;       // x^2048 mod g
    uint32_t lane_c[64];  // x^(32 (63 - l)) mod g
};

struct TbArgs {
    TbPoly cb, tb;     // CRC24B, the TB's polynomial
    int64_t Btb, rows; // rows = C * Btb < 2^31
    int64_t P, Bp, W;  // part bits K' - L, TB bits C P, bits of a code-block row
    int32_t Lcb;       // 24, or 0 (C == 1: no code-block CRC)
    // check
    const void* in;  // [rows][stride] fp32 or uint8
    int64_t stride;
    int32_t convention;
    const uint8_t* ref_tb;  // [Btb][Bp]
    uint8_t* cb_ok;         // [rows]
    uint8_t* tb_out;        // [Btb][Bp]
    uint32_t* work;         // [rows]
    // segment
    const uint8_t* tbits;  // [Btb][Bp]
    uint8_t* info;         // [rows][W]
};

// the tables of one polynomial into LDS (256 threads, one entry of each)
__device__ __forceinline__ void tb_tables(const TbPoly& p, CrcTables& t, bool steps) {
    t.byte[threadIdx.x] = crc_table_entry(threadIdx.x, p.poly);
    if (steps) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t.mul[k][threadIdx.x] = crc_mul(p.x2048, threadIdx.x << (24 - 8 * k), p.poly, p.L);
    }
}

// the part's remainder from the 64 running remainders, the same value in all 64 lanes
__device__ __forceinline__ uint32_t tb_finish(uint32_t acc, uint32_t lane_c, const TbPoly& p) {
    uint32_t r = crc_mul(acc, lane_c, p.poly, p.L);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) r ^= __shfl_xor(r, off, 64);
    return r;
}

// a step's 2048 bits to dst[base ..) as bytes 0 / 1 (elements before 0 are padding and not written)
__device__ __forceinline__ void tb_store_step(uint8_t* dst, int64_t base, uint32_t w, int lane) {
    if (NLDPC_CRC_X4 && (reinterpret_cast<uintptr_t>(dst + base) & 3) == 0 && (base >= 0 || (base & 3) == 0)) {
        if (base < 0) crc_store_x4<true>(dst, base, w, lane);
        else crc_store_x4<false>(dst, base, w, lane);
    } else {
        if (base < 0) crc_store_x1<true>(dst, base, w, lane);
        else crc_store_x1<false>(dst, base, w, lane);
    }
}

__global__ __launch_bounds__(kTbThreads) void tb_segment_kernel(TbArgs a) {
    __shared__ CrcTables tab;
    const int64_t S = (a.P + 2047) >> 11, pad = (S << 11) - a.P;
    if (a.Lcb) tb_tables(a.cb, tab, S > 1);
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t lane_c = a.cb.lane_c[lane];
    for (int64_t row = (int64_t)blockIdx.x * kTbRows + wid; row < a.rows; row += (int64_t)gridDim.x * kTbRows) {
        const uint32_t r = (uint32_t)row / (uint32_t)a.Btb, t = (uint32_t)row - r * (uint32_t)a.Btb;
        const uint8_t* src = a.tbits + (int64_t)t * a.Bp + (int64_t)r * a.P;
        uint8_t* dst = a.info + row * a.W;
        uint32_t acc = 0;
        for (int64_t s = 0; s < S; ++s) {
            const int64_t base = (s << 11) - pad;
            const uint32_t w = crc_words(src, base, lane, 0);
            tb_store_step(dst, base, w, lane);
            if (a.Lcb) acc = crc_accumulate(acc, s == 0, w, tab);
        }
        if (a.Lcb) {
            const uint32_t run = tb_finish(acc, lane_c, a.cb);
            if (lane < a.Lcb) dst[a.P + lane] = (uint8_t)((run >> (31 - lane)) & 1u);  // p_0 first
        }
        for (int64_t j = a.P + a.Lcb + lane; j < a.W; j += 64) dst[j] = 0;
    }
}

template <class T>
__global__ __launch_bounds__(kTbThreads) void tb_check_kernel(TbArgs a) {
    __shared__ CrcTables tab_cb, tab_tb;
    const int64_t S = (a.P + 2047) >> 11, pad = (S << 11) - a.P;
    tb_tables(a.tb, tab_tb, S > 1);
    if (a.Lcb) tb_tables(a.cb, tab_cb, S > 1);
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t lane_cb = a.cb.lane_c[lane], lane_tb = a.tb.lane_c[lane];
    for (int64_t row = (int64_t)blockIdx.x * kTbRows + wid; row < a.rows; row += (int64_t)gridDim.x * kTbRows) {
        const uint32_t r = (uint32_t)row / (uint32_t)a.Btb, t = (uint32_t)row - r * (uint32_t)a.Btb;
        const T* src = static_cast<const T*>(a.in) + row * a.stride;
        const int64_t at = (int64_t)t * a.Bp + (int64_t)r * a.P;  // the part's place in its TB
        const uint8_t* rr = a.ref_tb ? a.ref_tb + at : nullptr;
        uint8_t* out = a.tb_out ? a.tb_out + at : nullptr;
        uint32_t acc_cb = 0, acc_tb = 0;
        bool diff = false;
        for (int64_t s = 0; s < S; ++s) {
            const int64_t base = (s << 11) - pad;
            const uint32_t w = crc_words(src, base, lane, a.convention);
            if (rr) diff |= w != crc_words(rr, base, lane, 0);
            if (out) tb_store_step(out, base, w, lane);
            acc_tb = crc_accumulate(acc_tb, s == 0, w, tab_tb);
            if (a.Lcb) acc_cb = crc_accumulate(acc_cb, s == 0, w, tab_cb);
        }
        const uint32_t rem = tb_finish(acc_tb, lane_tb, a.tb);
        bool pass = rem == 0;  // (C == 1: the block's verdict is the TB's)
        if (a.Lcb) {
            // bit j of `got` = the decision at position P + j = the received p_j; bit 31 - j of run = the computed p_j
            const uint32_t run = tb_finish(acc_cb, lane_cb, a.cb);
            const T pv = lane < a.Lcb ? src[a.P + lane] : T(0);  // (0 is bit 0 either way)
            const uint32_t got = (uint32_t)__ballot(crc_hard(pv, a.convention));
            pass = got == (__brev(run) & 0x00FFFFFFu);
        }
        const bool err = __ballot(diff) != 0;
        if (lane == 0) {
            if (a.cb_ok) a.cb_ok[row] = pass ? 1 : 0;
            a.work[row] = rem | (err ? kTbFlagDiff : 0u) | (pass ? 0u : kTbFlagCbFail);
        }
    }
}

struct TbCombine {
    const uint32_t* work;  // [C][Btb]
    uint8_t* tb_ok;        // [Btb]
    unsigned long long* counts;
    int64_t Btb;
    int32_t C, L, has_ref;
    uint32_t poly, xP;  // the TB's polynomial, x^P mod g
};

__global__ __launch_bounds__(kTbThreads) void tb_check_combine_kernel(TbCombine a) {
    const int64_t t = (int64_t)blockIdx.x * kTbThreads + threadIdx.x;
    unsigned long long c[4] = {0, 0, 0, 0};
    if (t < a.Btb) {
        uint32_t acc = 0, flags = 0, cb_fail = 0;
        for (int32_t r = 0; r < a.C; ++r) {
            const uint32_t v = a.work[(int64_t)r * a.Btb + t];
            acc = r == 0 ? (v & ~0xFFu) : tb_combine(acc, v & ~0xFFu, a.xP, a.poly, a.L);
            flags |= v;
            cb_fail += (v & kTbFlagCbFail) ? 1u : 0u;
        }
        const bool pass = acc == 0, err = a.has_ref && (flags & kTbFlagDiff);
        if (a.tb_ok) a.tb_ok[t] = pass ? 1 : 0;
        c[0] = !pass, c[1] = pass && err, c[2] = err, c[3] = cb_fail;
    }
    if (a.counts) {  // (the same in every thread) the workgroup's sums first: at most four atomics per workgroup
        __shared__ unsigned long long part[kTbRows][4];
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned long long s = c[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) part[wid][k] = s;
        }
        __syncthreads();
        if (threadIdx.x < 4) {
            unsigned long long sum = 0;
#pragma unroll
            for (int w = 0; w < kTbRows; ++w) sum += part[w][threadIdx.x];
            if (sum) atomicAdd(&a.counts[threadIdx.x], sum);
        }
    }
}

// ---------------------------------------------------------------- concat / deconcat
typedef uint32_t tb_u4 __attribute__((ext_vector_type(4)));

// the variant measured in DESIGN §4.4 F10: NLDPC_TB_WIDE_LOADS = 0 gathers a run of bytes with one load per byte
#ifndef NLDPC_TB_WIDE_LOADS
#define NLDPC_TB_WIDE_LOADS 1
#endif

// 16 consecutive bytes from p (any alignment) out of the aligned dwords that hold them: four loads when p is aligned,
// else five and a funnel shift each.  True when those dwords lie inside [lo, hi), the array p points into; false (nothing
// is read): the caller goes byte by byte.
__device__ __forceinline__ bool tb_load16(const uint8_t* p, const uint8_t* lo, const uint8_t* hi, tb_u4* out) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3);
    const uint8_t* q0 = p - sh;
    if (q0 < lo || q0 + (sh ? 20 : 16) > hi) return false;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(q0);
    uint32_t w[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = q[k];
    w[4] = sh ? q[4] : 0u;
    tb_u4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (uint32_t)(((((uint64_t)w[k + 1]) << 32) | w[k]) >> (8 * sh));
    *out = v;
    return true;
}

struct TbCat {
    int64_t Btb;
    uint32_t C, C_lo, E_lo, E_hi, G, split;  // split = C_lo * E_lo: where the E_hi blocks begin in a row of g
    uint32_t inv_lo, inv_hi;                 // rm_inv of E_lo, E_hi
    uint32_t W, R;                           // the tile: W runs of each of R rows per workgroup
};

// where element m of a row of g lives: block r, element j of it
__device__ __forceinline__ void tb_locate(const TbCat& a, uint32_t m, uint32_t& r, uint32_t& j) {
    if (m < a.split) {
        rm_divmod(m, a.E_lo, a.inv_lo, r, j);
    } else {
        rm_divmod(m - a.split, a.E_hi, a.inv_hi, r, j);
        r += a.C_lo;
    }
}

// the first element of block r of TB t in f_lo / f_hi
template <class T>
__device__ __forceinline__ const T* tb_block(const TbCat& a, const T* f_lo, const T* f_hi, uint32_t r, int64_t t) {
    return r < a.C_lo ? f_lo + ((int64_t)r * a.Btb + t) * a.E_lo : f_hi + ((int64_t)(r - a.C_lo) * a.Btb + t) * a.E_hi;
}

// g[t][m] = block r's element j: a thread walks its run with a cursor (r, j, p)
template <class T>
__global__ __launch_bounds__(kTbThreads) void tb_concat_kernel(TbCat a, const T* __restrict__ f_lo,
                                                               const T* __restrict__ f_hi, T* __restrict__ g) {
    constexpr int RUN = 16 / sizeof(T);
    const uint32_t rr = threadIdx.x / a.W, c = blockIdx.x * a.W + (threadIdx.x - rr * a.W);
    if (rr >= a.R) return;
    for (int64_t t = (int64_t)blockIdx.y * a.R + rr; t < a.Btb; t += (int64_t)gridDim.y * a.R) {
        T* row = g + t * a.G;
        const int64_t m0 = (int64_t)c * RUN - (int64_t)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) & (RUN - 1));
        const int64_t lo = m0 < 0 ? 0 : m0, hi = m0 + RUN < (int64_t)a.G ? m0 + RUN : (int64_t)a.G;
        if (lo >= hi) continue;
        uint32_t r, j;
        tb_locate(a, (uint32_t)lo, r, j);
        uint32_t E = r < a.C_lo ? a.E_lo : a.E_hi;
        const T* p = tb_block(a, f_lo, f_hi, r, t) + j;
        if constexpr (sizeof(T) == 1 && NLDPC_TB_WIDE_LOADS) {  // a whole run inside one block: wide loads
            if (hi - lo == RUN && j + RUN <= E) {
                const T* base = r < a.C_lo ? f_lo : f_hi;
                const int64_t n = r < a.C_lo ? (int64_t)a.C_lo * a.Btb * a.E_lo : (int64_t)(a.C - a.C_lo) * a.Btb * a.E_hi;
                tb_u4 q;
                if (tb_load16(p, base, base + n, &q)) {
                    *reinterpret_cast<tb_u4*>(row + m0) = q;
                    continue;
                }
            }
        }
        T v[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            if (lo + k < hi) {
                v[k] = *p++;
                if (++j == E && lo + k + 1 < hi) {  // (the next element exists: so does block r + 1)
                    ++r, j = 0;
                    E = r < a.C_lo ? a.E_lo : a.E_hi;
                    p = tb_block(a, f_lo, f_hi, r, t);
                }
            }
        }
        if (hi - lo == RUN) {
            tb_u4 q;
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<tb_u4*>(row + m0) = q;
        } else {
#pragma unroll
            for (int k = 0; k < RUN; ++k)
                if (lo + k < hi) row[lo + k] = v[k];
        }
    }
}

// f[q][j] = g[t][offset of block r + j]: output row q = r * Btb + t over both arrays, f_hi's rows after f_lo's
template <class T>
__global__ __launch_bounds__(kTbThreads) void tb_deconcat_kernel(TbCat a, const T* __restrict__ g, T* __restrict__ f_lo,
                                                                 T* __restrict__ f_hi) {
    constexpr int RUN = 16 / sizeof(T);
    const uint32_t rr = threadIdx.x / a.W, c = blockIdx.x * a.W + (threadIdx.x - rr * a.W);
    if (rr >= a.R) return;
    const int64_t rows = (int64_t)a.C * a.Btb, rows_lo = (int64_t)a.C_lo * a.Btb;
    for (int64_t q = (int64_t)blockIdx.y * a.R + rr; q < rows; q += (int64_t)gridDim.y * a.R) {
        const uint32_t r = (uint32_t)q / (uint32_t)a.Btb, t = (uint32_t)q - r * (uint32_t)a.Btb;
        const bool low = q < rows_lo;
        const int64_t E = low ? a.E_lo : a.E_hi;
        T* row = low ? f_lo + q * a.E_lo : f_hi + (q - rows_lo) * a.E_hi;
        const T* src = g + (int64_t)t * a.G + (low ? (int64_t)r * a.E_lo : (int64_t)a.split + (int64_t)(r - a.C_lo) * a.E_hi);
        const int64_t m0 = (int64_t)c * RUN - (int64_t)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) & (RUN - 1));
        const int64_t lo = m0 < 0 ? 0 : m0, hi = m0 + RUN < E ? m0 + RUN : E;
        if (lo >= hi) continue;
        if (hi - lo == RUN) {
            tb_u4 qv = {0u, 0u, 0u, 0u};
            bool wide = false;
            if constexpr (sizeof(T) == 1 && NLDPC_TB_WIDE_LOADS) wide = tb_load16(src + m0, g, g + a.Btb * (int64_t)a.G, &qv);
            if (!wide) {
                T v[RUN];
#pragma unroll
                for (int k = 0; k < RUN; ++k) v[k] = src[m0 + k];
                __builtin_memcpy(&qv, v, 16);
            }
            *reinterpret_cast<tb_u4*>(row + m0) = qv;
        } else {
            for (int64_t m = lo; m < hi; ++m) row[m] = src[m];
        }
    }
}

static void tb_fill(TbPoly& p, int32_t crc) {
    const CrcConsts& c = crc_consts(crc);
    p.poly = crc_poly(crc);
    p.L = crc_len(crc);
    p.x2048 = c.x2048;
    for (int l = 0; l < 64; ++l) p.lane_c[l] = c.lane_c[l];
}

static const char* tb_plan_why(int st) {
    switch (st) {
        case TB_EARG: return "tb_crc is one of enum nldpc_crc, A >= 1, W >= 1, kcb >= 0";
        case TB_ERANGE: return "every size must be below 2^31";
        case TB_EKCB_W: return "kcb exceeds W";
        case TB_EKCB_SMALL: return "kcb must exceed 24 when the block is segmented";
        case TB_EDIV: return "C does not divide B'' = B' + C L";
        case TB_EKP_W: return "K' exceeds W";
    }
    return "bad plan";
}

// the arguments every launch shares; rows = C * Btb
static int tb_common(const char* who, const nldpc_tb* plan, int64_t Btb, TbArgs* k) {
    const std::string w = std::string(who) + ": ";
    if (!plan) return fail(NLDPC_EINVAL, w + "plan is NULL");
    if (!tb_plan_ok(*plan)) return fail(NLDPC_EINVAL, w + "the plan breaks B' = A + L_tb = C (K' - L), L = 24 (C > 1) or 0, K' + F = W < 2^31");
    if (Btb < 1 || (int64_t)plan->C * Btb >= kTbLimit) return fail(NLDPC_EINVAL, w + "Btb >= 1 and C * Btb < 2^31 must hold");
    tb_fill(k->cb, kTbCbCrc);
    tb_fill(k->tb, plan->tb_crc);
    k->Btb = Btb;
    k->rows = (int64_t)plan->C * Btb;
    k->P = tb_part(*plan);
    k->Bp = tb_bits(*plan);
    k->W = plan->W;
    k->Lcb = plan->L;
    return NLDPC_OK;
}

static unsigned tb_grid(int64_t rows) {
    const int64_t want = (rows + kTbRows - 1) / kTbRows;
    return (unsigned)(want < kTbMaxBlocks ? want : kTbMaxBlocks);
}

// how the 256 threads of a workgroup tile the runs of a row (nldpc_ratematch.hip rm_tile)
static void tb_tile(int64_t len, int run, TbCat* a, unsigned* gx) {
    const int64_t C = (len + 2 * run - 2) / run;  // runs of a row at the worst misalignment
    const int64_t g = (C + kTbThreads - 1) / kTbThreads;
    const int64_t W = (C + g - 1) / g;
    a->W = (uint32_t)W;
    a->R = (uint32_t)(kTbThreads / W);
    *gx = (unsigned)g;
}

static int tb_cat_args(const char* who, int32_t elem_bytes, const void* f_lo, const void* f_hi, const void* g, int64_t Btb,
                       int32_t C, int32_t C_lo, int64_t E_lo, int64_t E_hi, TbCat* a) {
    const std::string w = std::string(who) + ": ";
    if (elem_bytes != 1 && elem_bytes != 4) return fail(NLDPC_EINVAL, w + "elem_bytes is 1 or 4");
    if (Btb < 1 || C < 1 || C_lo < 0 || C_lo > C || E_lo < 1 || E_hi < 1) return fail(NLDPC_EINVAL, w + "bad argument");
    if (E_lo >= kTbLimit || E_hi >= kTbLimit) return fail(NLDPC_EINVAL, w + "G must be below 2^31");
    const int64_t G = (int64_t)C_lo * E_lo + (int64_t)(C - C_lo) * E_hi;
    if (G >= kTbLimit || (int64_t)C * Btb >= kTbLimit) return fail(NLDPC_EINVAL, w + "G and C * Btb must be below 2^31");
    if (!g || (C_lo > 0 && !f_lo) || (C_lo < C && !f_hi)) return fail(NLDPC_EINVAL, w + "a pointer is NULL");
    if (elem_bytes == 4 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(f_lo) | reinterpret_cast<uintptr_t>(f_hi)) & 3))
        return fail(NLDPC_EINVAL, w + "4-byte elements must be 4-byte aligned");
    a->Btb = Btb;
    a->C = (uint32_t)C;
    a->C_lo = (uint32_t)C_lo;
    a->E_lo = (uint32_t)E_lo;
    a->E_hi = (uint32_t)E_hi;
    a->G = (uint32_t)G;
    a->split = (uint32_t)((int64_t)C_lo * E_lo);
    a->inv_lo = rm_inv(a->E_lo);
    a->inv_hi = rm_inv(a->E_hi);
    return NLDPC_OK;
}

static int tb_launched(const char* who) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, who);
}
}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_tb_plan(int64_t A, int32_t tb_crc, int64_t W, int64_t kcb, nldpc_tb* plan) {
    if (!plan) return fail(NLDPC_EINVAL, "nldpc_tb_plan: plan is NULL");
    nldpc_tb p{};
    if (int st = tb_plan(A, tb_crc, W, kcb, &p)) return fail(NLDPC_EINVAL, std::string("nldpc_tb_plan: ") + tb_plan_why(st));
    *plan = p;
    return NLDPC_OK;
}

extern "C" int nldpc_tb_lifting_size(int32_t bg, int64_t Bp, int32_t* Kb, int32_t* Zc) {
    if (!Kb || !Zc) return fail(NLDPC_EINVAL, "nldpc_tb_lifting_size: a pointer is NULL");
    if (!tb_lifting_size(bg, Bp, Kb, Zc))
        return fail(NLDPC_EINVAL, "nldpc_tb_lifting_size: bg is 1 or 2, 1 <= Bp < 2^31, and a lifting size up to 384 must hold K'");
    return NLDPC_OK;
}

extern "C" int nldpc_tb_er(int64_t G, int32_t NL, int32_t Qm, int32_t C, int64_t* E_lo, int64_t* E_hi, int32_t* C_lo) {
    if (!E_lo || !E_hi || !C_lo) return fail(NLDPC_EINVAL, "nldpc_tb_er: a pointer is NULL");
    if (!tb_er(G, NL, Qm, C, E_lo, E_hi, C_lo))
        return fail(NLDPC_EINVAL, "nldpc_tb_er: NL, Qm, C >= 1, 1 <= G < 2^31, NL * Qm divides G and G / (NL Qm) >= C must hold");
    return NLDPC_OK;
}

extern "C" int nldpc_tb_crc_ref(const nldpc_tb* plan, const uint8_t* blocks, int64_t stride, uint8_t* cb_ok,
                                uint32_t* tb_rem) {
    if (!plan || !tb_plan_ok(*plan)) return fail(NLDPC_EINVAL, "nldpc_tb_crc_ref: plan is NULL or breaks its relations");
    if (!blocks || stride < plan->Kp) return fail(NLDPC_EINVAL, "nldpc_tb_crc_ref: blocks is NULL or stride is below K'");
    const int tb_L = crc_len(plan->tb_crc);
    const uint32_t tb_poly = crc_poly(plan->tb_crc), cb_poly = crc_poly(kTbCbCrc);
    uint32_t tab_tb[256], tab_cb[256];
    for (uint32_t v = 0; v < 256; ++v) tab_tb[v] = crc_table_entry(v, tb_poly), tab_cb[v] = crc_table_entry(v, cb_poly);
    const int64_t P = tb_part(*plan);
    const uint32_t xP = crc_xpow((uint64_t)P, tb_poly, tb_L);
    uint32_t acc = 0;
    for (int32_t r = 0; r < plan->C; ++r) {
        const uint8_t* row = blocks + (int64_t)r * stride;
        const uint32_t part = crc_piece(row, 0, P, tb_poly, tab_tb);
        acc = r == 0 ? part : tb_combine(acc, part, xP, tb_poly, tb_L);
        if (cb_ok && plan->L) cb_ok[r] = crc_piece(row, 0, plan->Kp, cb_poly, tab_cb) == 0 ? 1 : 0;
    }
    if (cb_ok && !plan->L) cb_ok[0] = acc == 0 ? 1 : 0;
    if (tb_rem) *tb_rem = acc >> (32 - tb_L);
    return NLDPC_OK;
}

extern "C" int nldpc_tb_workspace(const nldpc_tb* plan, int64_t Btb, size_t* bytes) {
    if (!plan || !bytes || !tb_plan_ok(*plan)) return fail(NLDPC_EINVAL, "nldpc_tb_workspace: bad argument");
    if (Btb < 1 || (int64_t)plan->C * Btb >= kTbLimit) return fail(NLDPC_EINVAL, "nldpc_tb_workspace: Btb >= 1 and C * Btb < 2^31 must hold");
    *bytes = sizeof(uint32_t) * (size_t)plan->C * (size_t)Btb;
    return NLDPC_OK;
}

extern "C" int nldpc_tb_segment(const nldpc_tb* plan, const uint8_t* tb, int64_t Btb, uint8_t* info, void* stream) {
    TbArgs k{};
    if (int st = tb_common("nldpc_tb_segment", plan, Btb, &k)) return st;
    if (!tb || !info) return fail(NLDPC_EINVAL, "nldpc_tb_segment: tb and info must not be NULL");
    k.tbits = tb;
    k.info = info;
    hipLaunchKernelGGL(tb_segment_kernel, dim3(tb_grid(k.rows)), dim3(kTbThreads), 0, static_cast<hipStream_t>(stream), k);
    return tb_launched("nldpc_tb_segment");
}

extern "C" int nldpc_tb_concat(int32_t elem_bytes, const void* f_lo, const void* f_hi, int64_t Btb, int32_t C,
                               int32_t C_lo, int64_t E_lo, int64_t E_hi, void* g, void* stream) {
    TbCat a{};
    if (int st = tb_cat_args("nldpc_tb_concat", elem_bytes, f_lo, f_hi, g, Btb, C, C_lo, E_lo, E_hi, &a)) return st;
    unsigned gx;
    tb_tile(a.G, 16 / elem_bytes, &a, &gx);
    const int64_t gy = (Btb + a.R - 1) / a.R;
    const dim3 grid(gx, (unsigned)(gy < 65535 ? gy : 65535));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(tb_concat_kernel<uint8_t>, grid, dim3(kTbThreads), 0, s, a, static_cast<const uint8_t*>(f_lo),
                           static_cast<const uint8_t*>(f_hi), static_cast<uint8_t*>(g));
    else
        hipLaunchKernelGGL(tb_concat_kernel<uint32_t>, grid, dim3(kTbThreads), 0, s, a, static_cast<const uint32_t*>(f_lo),
                           static_cast<const uint32_t*>(f_hi), static_cast<uint32_t*>(g));
    return tb_launched("nldpc_tb_concat");
}

extern "C" int nldpc_tb_deconcat(int32_t elem_bytes, const void* g, int64_t Btb, int32_t C, int32_t C_lo, int64_t E_lo,
                                 int64_t E_hi, void* f_lo, void* f_hi, void* stream) {
    TbCat a{};
    if (int st = tb_cat_args("nldpc_tb_deconcat", elem_bytes, f_lo, f_hi, g, Btb, C, C_lo, E_lo, E_hi, &a)) return st;
    unsigned gx;
    tb_tile(E_lo > E_hi ? E_lo : E_hi, 16 / elem_bytes, &a, &gx);
    const int64_t gy = ((int64_t)C * Btb + a.R - 1) / a.R;
    const dim3 grid(gx, (unsigned)(gy < 65535 ? gy : 65535));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (elem_bytes == 1)
        hipLaunchKernelGGL(tb_deconcat_kernel<uint8_t>, grid, dim3(kTbThreads), 0, s, a, static_cast<const uint8_t*>(g),
                           static_cast<uint8_t*>(f_lo), static_cast<uint8_t*>(f_hi));
    else
        hipLaunchKernelGGL(tb_deconcat_kernel<uint32_t>, grid, dim3(kTbThreads), 0, s, a, static_cast<const uint32_t*>(g),
                           static_cast<uint32_t*>(f_lo), static_cast<uint32_t*>(f_hi));
    return tb_launched("nldpc_tb_deconcat");
}

extern "C" int nldpc_tb_check(const nldpc_tb* plan, const float* llr, const uint8_t* bits, int64_t Btb, int64_t stride,
                              int32_t convention, const uint8_t* ref_tb, uint8_t* cb_ok, uint8_t* tb_ok, uint8_t* tb_out,
                              int64_t* counts, void* work, size_t work_bytes, void* stream) {
    TbArgs k{};
    if (int st = tb_common("nldpc_tb_check", plan, Btb, &k)) return st;
    if ((llr != nullptr) == (bits != nullptr)) return fail(NLDPC_EINVAL, "nldpc_tb_check: exactly one of llr and bits is given");
    if (!cb_ok && !tb_ok && !tb_out && !counts) return fail(NLDPC_EINVAL, "nldpc_tb_check: every output is NULL");
    if (convention != 0 && convention != 1) return fail(NLDPC_EINVAL, "nldpc_tb_check: convention is 0 or 1");
    if (stride < plan->Kp) return fail(NLDPC_EINVAL, "nldpc_tb_check: stride is below K'");
    if (llr && (reinterpret_cast<uintptr_t>(llr) & 3)) return fail(NLDPC_EINVAL, "nldpc_tb_check: llr must be 4-byte aligned");
    if (counts && (reinterpret_cast<uintptr_t>(counts) & 7)) return fail(NLDPC_EINVAL, "nldpc_tb_check: counts must be 8-byte aligned");
    if (!work || (reinterpret_cast<uintptr_t>(work) & 3) || work_bytes < sizeof(uint32_t) * (size_t)k.rows)
        return fail(NLDPC_EINVAL, "nldpc_tb_check: work must be 4-byte aligned and hold nldpc_tb_workspace bytes");
    k.in = llr ? static_cast<const void*>(llr) : static_cast<const void*>(bits);
    k.stride = stride;
    k.convention = convention;
    k.ref_tb = ref_tb;
    k.cb_ok = cb_ok;
    k.tb_out = tb_out;
    k.work = static_cast<uint32_t*>(work);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(llr ? tb_check_kernel<float> : tb_check_kernel<uint8_t>, dim3(tb_grid(k.rows)), dim3(kTbThreads), 0, s, k);
    if (int st = tb_launched("nldpc_tb_check")) return st;
    if (!tb_ok && !counts) return NLDPC_OK;  // (only cb_ok / tb_out were asked for)
    TbCombine c{};
    c.work = k.work;
    c.tb_ok = tb_ok;
    c.counts = reinterpret_cast<unsigned long long*>(counts);
    c.Btb = Btb;
    c.C = plan->C;
    c.L = k.tb.L;
    c.has_ref = ref_tb != nullptr;
    c.poly = k.tb.poly;
    c.xP = crc_xpow((uint64_t)k.P, k.tb.poly, k.tb.L);
    hipLaunchKernelGGL(tb_check_combine_kernel, dim3((unsigned)((Btb + kTbThreads - 1) / kTbThreads)), dim3(kTbThreads), 0, s, c);
    return tb_launched("nldpc_tb_check (combine)");
}
