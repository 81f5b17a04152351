// MIMO spatial multiplexing with LMMSE soft detection (3GPP TS 38.211 §6.3.1.3 / §7.3.1.3 layer mapping of one codeword,
// identity precoding; include/nldpc.h, F13): nldpc_mimo_entry_ref, nldpc_mimo_filter_ref, nldpc_mimo_detect_ref (host),
// nldpc_mimo_channels, nldpc_mimo_filter, nldpc_mimo_detect, nldpc_mimo_channel_llr.  The arithmetic is the inline
// functions of nldpc_mimo.h (and nldpc_qam.h, nldpc_gold.h) on both sides.
//
// A thread owns one resource element (RE): nt consecutive symbols, nt * qm consecutive bytes of f and LLRs, nr received
// samples, one Philox counter per antenna pair at the global RE index.  The filter of the RE's fading block is
// recomputed by every thread that needs it (no table, no second launch, no workspace), so the three
// detecting kernels differ only in where y and H come from.  A wave's 64 REs are one contiguous run of LLRs (and of
// received samples): when every lane owns its RE and the run starts on a 16-byte boundary the wave turns it through LDS
// so that each store instruction writes 64 consecutive 16-byte groups, non-temporally (as qam_store_pair of
// nldpc_modulation.hip does for a pair); the last wave of the batch and a view off the boundary store element by
// element.  Nothing outside the outputs is touched.
//
// Exact max-log ML detection (F14; the arithmetic is nldpc_mimo_ml.h): nldpc_mimo_detect_ml_ref (host),
// nldpc_mimo_detect_ml, nldpc_mimo_channel_llr_ml, a second pair of kernels at the end of the namespace with the same
// thread-per-RE mapping, arguments and stores.
#include <hip/hip_runtime.h>

#include "nldpc_gold.h"
#include "nldpc_internal.h"
#include "nldpc_mimo.h"
#include "nldpc_mimo_ml.h"
#include "nldpc_philox.h"

namespace nldpc {
constexpr int kMimoThreads = 256;
typedef float mimo_f4 __attribute__((ext_vector_type(4)));  // (the nontemporal builtins take native vectors)
typedef float mimo_f2 __attribute__((ext_vector_type(2)));

// rows of R resource elements in fading blocks of L (L <= R)
struct MimoRows {
    int64_t R;
    int32_t L, n_blk;
};

struct MimoArgs {
    const uint8_t* f;     // [total * nt * qm] bits, or nullptr (fused)
    const float* y_in;    // [total][nr][2] (detect)
    const float* h;       // [B][n_blk][nr][nt][2], or nullptr: drawn (fused only)
    float* llr;           // [total * nt * qm]
    float* y_out;         // [total][nr][2], or nullptr (fused)
    float* h_out;         // [B][n_blk][nr][nt][2], or nullptr (fused)
    int64_t total;        // REs of the batch
    int64_t first;        // global index of the batch's first RE
    int64_t b_offset;
    MimoRows r;
    float sigma;
    double scale;         // mimo_entry_scale(nt) (drawn channels)
    uint64_t seed;
    const uint32_t* seq;  // [n_seq][Wc], or nullptr: no scrambling
    int64_t n_seq, Wc;
};

__device__ __forceinline__ U4 mimo_counter(uint64_t c, uint32_t tag, uint32_t q, uint64_t seed) {
    return philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), tag, q}, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// the NR * NT entries of global block Gf: entry e = r * NT + t takes words (x, y) of counter e >> 1 when even, (z, w)
// when odd
template <int NT, int NR>
__device__ __forceinline__ void mimo_draw(uint64_t Gf, double scale, uint64_t seed, float* h) {
#pragma unroll
    for (int c = 0; c < (NR * NT + 1) / 2; ++c) {
        const U4 d = mimo_counter(Gf, kMimoChanTag, (uint32_t)c, seed);
        mimo_entry_of(scale, d.x, d.y, h[4 * c], h[4 * c + 1]);
        if (2 * c + 1 < NR * NT) mimo_entry_of(scale, d.z, d.w, h[4 * c + 2], h[4 * c + 3]);
    }
}

// the wave's staging area: [64][PER] floats, one per wave of the workgroup
template <int PER>
__device__ __forceinline__ float* mimo_stage() {
    __shared__ mimo_f4 stage[kMimoThreads * PER / 4 + 1];
    return reinterpret_cast<float*>(stage) + (threadIdx.x >> 6) * 64 * PER;
}

// a thread's PER floats v to base[loc * PER ..) (every calling lane owns its RE; lanes past the batch have returned).
// PER is even.  The staged path is taken by a whole wave or not at all (the condition is uniform).
template <int PER>
__device__ __forceinline__ void mimo_store_run(float* base, int64_t loc, const float* v, float* stage) {
    static_assert(PER % 2 == 0, "a run of 64 * PER floats is whole 16-byte groups");
    float* dst = base + loc * PER;
    const int lane = threadIdx.x & 63;
    float* run = dst - (int64_t)lane * PER;  // lane 0's RE: the same address in every lane
    if (__ballot(1) == ~0ull && (reinterpret_cast<uintptr_t>(run) & 15) == 0) {
        if constexpr (PER % 4 == 0) {
#pragma unroll
            for (int q = 0; q < PER / 4; ++q)
                reinterpret_cast<mimo_f4*>(stage)[lane * (PER / 4) + q] = mimo_f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        } else {
#pragma unroll
            for (int q = 0; q < PER / 2; ++q)
                reinterpret_cast<mimo_f2*>(stage)[lane * (PER / 2) + q] = mimo_f2{v[2 * q], v[2 * q + 1]};
        }
        // (the wave reads what its other lanes wrote: LDS operations of a wave complete in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int N4 = 16 * PER;  // 16-byte groups of the run
#pragma unroll
        for (int q = 0; q * 64 < N4; ++q) {
            const int g = q * 64 + lane;
            if (g < N4) __builtin_nontemporal_store(reinterpret_cast<const mimo_f4*>(stage)[g], reinterpret_cast<mimo_f4*>(run) + g);
        }
        // (and the next run staged here waits for these reads)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        return;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) dst[i] = v[i];
}

// filter -> equalise -> demap -> (descramble) -> store: the common tail of the detecting kernels.  sm holds the RE's
// NT * QM scrambling bits (0 without scrambling)
template <int H, int METHOD, int NT, int NR>
__device__ __forceinline__ void mimo_detect_store(const MimoArgs& a, int64_t loc, const float* h, const float* y,
                                                  uint32_t sm, float* stage) {
    constexpr int QM = 2 * H, PER = NT * QM;
    float W[2 * NT * NR], mu[NT], w[NT], xh[2 * NT], lvl[1 << H], v[PER];
    mimo_filter<NT, NR>(h, a.sigma, W, mu, w);
    mimo_equalise<NT, NR>(W, y, xh);
    qam_levels<H>(lvl);
    mimo_demap<H, METHOD, NT>(lvl, xh, mu, w, v);
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = __uint_as_float(__float_as_uint(v[i]) ^ (((sm >> i) & 1u) << 31));
    mimo_store_run<PER>(a.llr, loc, v, stage);
}

template <int NT, int NR>
__device__ __forceinline__ void mimo_load_block(const float* __restrict__ tab, int64_t blk, float* h) {
    const float* src = tab + blk * (2 * NR * NT);
#pragma unroll
    for (int e = 0; e < 2 * NR * NT; ++e) h[e] = src[e];
}

// ---------------------------------------------------------------- nldpc_mimo_channels: one thread per fading block
struct MimoChanArgs {
    float* h;       // [total][nr][nt][2]
    int64_t first;  // the first global block
    int64_t total;
    double scale;
    uint64_t seed;
};

template <int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_channels_kernel(MimoChanArgs a) {
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    float h[2 * NR * NT];
    mimo_draw<NT, NR>((uint64_t)(a.first + loc), a.scale, a.seed, h);
    float* dst = a.h + loc * (2 * NR * NT);
#pragma unroll
    for (int e = 0; e < 2 * NR * NT; ++e) dst[e] = h[e];
}

// ---------------------------------------------------------------- nldpc_mimo_filter: one thread per fading block
struct MimoFilterArgs {
    const float* h;  // [total][nr][nt][2]
    float* W;        // [total][nt][nr][2]
    float* mu;       // [total][nt]
    float* w;        // [total][nt]
    int64_t total;
    float sigma;
};

template <int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_filter_kernel(MimoFilterArgs a) {
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    float h[2 * NR * NT], W[2 * NT * NR], mu[NT], w[NT];
    mimo_load_block<NT, NR>(a.h, loc, h);
    mimo_filter<NT, NR>(h, a.sigma, W, mu, w);
#pragma unroll
    for (int e = 0; e < 2 * NT * NR; ++e) a.W[loc * (2 * NT * NR) + e] = W[e];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        a.mu[loc * NT + k] = mu[k];
        a.w[loc * NT + k] = w[k];
    }
}

// ---------------------------------------------------------------- nldpc_mimo_detect: y and H -> LLRs
template <int H, int METHOD, int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_detect_kernel(MimoArgs a) {
    constexpr int PER = NT * 2 * H;
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    const MimoIdx x = mimo_index(loc, a.r.R, a.r.L);
    float h[2 * NR * NT], y[2 * NR];
    mimo_load_block<NT, NR>(a.h, mimo_block(x, a.r.n_blk), h);
#pragma unroll
    for (int e = 0; e < 2 * NR; ++e) y[e] = a.y_in[loc * (2 * NR) + e];
    mimo_detect_store<H, METHOD, NT, NR>(a, loc, h, y, 0u, mimo_stage<PER>());
}

// ---------------------------------------------------------------- nldpc_mimo_channel_llr, the fused channel:
// bits -> (scramble) -> map -> H x -> noise -> filter -> equalise -> demap -> (descramble)
template <int H, int METHOD, int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_channel_kernel(MimoArgs a) {
    constexpr int QM = 2 * H, PER = NT * QM, PERY = 2 * NR, PERS = PER > PERY ? PER : PERY;
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    const MimoIdx x = mimo_index(loc, a.r.R, a.r.L);
    const int64_t blk = mimo_block(x, a.r.n_blk);
    float h[2 * NR * NT];
    if (a.h) mimo_load_block<NT, NR>(a.h, blk, h);  // (a uniform branch)
    else mimo_draw<NT, NR>(mimo_global(a.b_offset, x, a.r.n_blk), a.scale, a.seed, h);
    if (a.h_out && mimo_first(x, a.r.L)) {
        float* dst = a.h_out + blk * (2 * NR * NT);
#pragma unroll
        for (int e = 0; e < 2 * NR * NT; ++e) dst[e] = h[e];
    }
    // the RE's NT * QM bits (bit j = byte j of the RE is non-zero) and scrambling bits
    uint32_t fb = 0u, sm = 0u;
    if (a.f) {
        const uint8_t* src = a.f + loc * PER;
        if (PER % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
            for (int q = 0; q < PER / 4; ++q) {
                const uint32_t wd = reinterpret_cast<const uint32_t*>(src)[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) fb |= (((wd >> (8 * j)) & 0xFFu) ? 1u : 0u) << (4 * q + j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PER; ++j) fb |= (src[j] ? 1u : 0u) << j;
        }
    }
    if (a.seq) {
        // row b uses sequence (b_offset + b) mod n_seq (b_offset + b < 2^32, n_seq < 2^31)
        const uint32_t q = a.n_seq == 1 ? 0u : (uint32_t)(a.b_offset + x.b) % (uint32_t)a.n_seq;
        const uint32_t* row = a.seq + (int64_t)q * a.Wc;
#pragma unroll
        for (int k = 0; k < NT; ++k) sm |= gold_bits(row, (int64_t)x.i * PER + k * QM, QM) << (k * QM);
    }
    fb ^= sm;
    float xs[2 * NT], s[2 * NR], y[2 * NR];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        uint32_t ci, cq;
        qam_labels(H, [&](int i) { return ((fb >> (k * QM + i)) & 1u) != 0; }, ci, cq);
        xs[2 * k] = qam_level(H, ci);
        xs[2 * k + 1] = qam_level(H, cq);
    }
    mimo_apply<NT, NR>(h, xs, s);
    const uint64_t Gre = (uint64_t)(a.first + loc);
    const double sigma = (double)a.sigma;
#pragma unroll
    for (int q = 0; q < (NR + 1) / 2; ++q) {
        const U4 c = mimo_counter(Gre, kMimoNoiseTag, (uint32_t)q, a.seed);
        const double rad0 = sqrt(-2.0 * log(u01(c.x))), th0 = 6.283185307179586 * u01(c.y);
        y[4 * q] = (float)((double)s[4 * q] + sigma * (rad0 * cos(th0)));
        y[4 * q + 1] = (float)((double)s[4 * q + 1] + sigma * (rad0 * sin(th0)));
        if (2 * q + 1 < NR) {
            const double rad1 = sqrt(-2.0 * log(u01(c.z))), th1 = 6.283185307179586 * u01(c.w);
            y[4 * q + 2] = (float)((double)s[4 * q + 2] + sigma * (rad1 * cos(th1)));
            y[4 * q + 3] = (float)((double)s[4 * q + 3] + sigma * (rad1 * sin(th1)));
        }
    }
    float* stage = mimo_stage<PERS>();
    mimo_detect_store<H, METHOD, NT, NR>(a, loc, h, y, sm, stage);
    if (a.y_out) mimo_store_run<PERY>(a.y_out, loc, y, stage);
}

typedef void (*MimoKernel)(MimoArgs);
typedef void (*MimoChanKernel)(MimoChanArgs);
typedef void (*MimoFilterKernel)(MimoFilterArgs);
// [qm / 2 - 1][method][mimo_dims_index]
#define NLDPC_MIMO_DIMS(K, H, M) {K<H, M, 1, 1>, K<H, M, 1, 2>, K<H, M, 1, 4>, K<H, M, 2, 2>, K<H, M, 2, 4>, K<H, M, 4, 4>}
#define NLDPC_MIMO_ORDERS(K) \
    {{NLDPC_MIMO_DIMS(K, 1, 0), NLDPC_MIMO_DIMS(K, 1, 1)}, {NLDPC_MIMO_DIMS(K, 2, 0), NLDPC_MIMO_DIMS(K, 2, 1)}, \
     {NLDPC_MIMO_DIMS(K, 3, 0), NLDPC_MIMO_DIMS(K, 3, 1)}, {NLDPC_MIMO_DIMS(K, 4, 0), NLDPC_MIMO_DIMS(K, 4, 1)}}
static const MimoKernel kMimoChannel[4][2][6] = NLDPC_MIMO_ORDERS(mimo_channel_kernel);
static const MimoKernel kMimoDetect[4][2][6] = NLDPC_MIMO_ORDERS(mimo_detect_kernel);
#define NLDPC_MIMO_PAIRS(K) {K<1, 1>, K<1, 2>, K<1, 4>, K<2, 2>, K<2, 4>, K<4, 4>}
static const MimoChanKernel kMimoChannels[6] = NLDPC_MIMO_PAIRS(mimo_channels_kernel);
static const MimoFilterKernel kMimoFilter[6] = NLDPC_MIMO_PAIRS(mimo_filter_kernel);

// ---------------------------------------------------------------- the host references
template <int NT, int NR>
static void mimo_filter_host(float sigma, const float* h, int64_t n, float* W, float* mu, float* w) {
    for (int64_t i = 0; i < n; ++i)
        mimo_filter<NT, NR>(h + i * (2 * NR * NT), sigma, W + i * (2 * NT * NR), mu + i * NT, w + i * NT);
}
typedef void (*MimoHostFilter)(float, const float*, int64_t, float*, float*, float*);
static const MimoHostFilter kMimoFilterHost[6] = NLDPC_MIMO_PAIRS(mimo_filter_host);

template <int H, int METHOD, int NT, int NR>
static void mimo_detect_host(float sigma, const float* y, const float* h, int64_t B, int64_t R, int32_t L,
                             int32_t n_blk, float* llr) {
    float W[2 * NT * NR], mu[NT], w[NT], xh[2 * NT], lvl[1 << H];
    qam_levels<H>(lvl);
    int64_t have = -1;
    for (int64_t loc = 0; loc < B * R; ++loc) {
        const int64_t blk = mimo_block(mimo_index(loc, R, L), n_blk);
        if (blk != have) mimo_filter<NT, NR>(h + blk * (2 * NR * NT), sigma, W, mu, w);
        have = blk;
        mimo_equalise<NT, NR>(W, y + loc * (2 * NR), xh);
        mimo_demap<H, METHOD, NT>(lvl, xh, mu, w, llr + loc * (NT * 2 * H));
    }
}
typedef void (*MimoHostDetect)(float, const float*, const float*, int64_t, int64_t, int32_t, int32_t, float*);
static const MimoHostDetect kMimoDetectHost[4][2][6] = NLDPC_MIMO_ORDERS(mimo_detect_host);
#undef NLDPC_MIMO_PAIRS
#undef NLDPC_MIMO_ORDERS
#undef NLDPC_MIMO_DIMS

static bool mimo_misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

template <class Kernel, class Args>
static int mimo_launch(const std::string& who, Kernel k, const Args& a, int64_t threads, void* stream) {
    const int64_t blocks = (threads + kMimoThreads - 1) / kMimoThreads;
    if (blocks > 0x7FFFFFFF) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kMimoThreads), 0, static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, who.c_str());
}

// the rules shared by the entry points
static int mimo_dims(const std::string& who, int32_t nt, int32_t nr) {
    if (!mimo_dims_ok(nt, nr)) return fail(NLDPC_EINVAL, who + ": nt and nr are 1, 2 or 4 with nr >= nt");
    return NLDPC_OK;
}
static int mimo_demapper(const std::string& who, int32_t qm, int32_t method, float sigma) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, who + ": qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, who + ": method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, who + ": sigma must be positive");
    return NLDPC_OK;
}
// L for rows of R resource elements (0 < R < 2^31): L >= R is one block per row
static int mimo_rows(const std::string& who, int64_t B, int64_t R, int64_t L, MimoRows& r) {
    if (L < 1) return fail(NLDPC_EINVAL, who + ": L must be at least 1");
    r.R = R;
    r.L = (int32_t)(L < R ? L : R);
    const int64_t n_blk = fading_blocks(R, L);
    if (B * n_blk >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, who + ": B * ceil(R / L) must be below 2^31");
    r.n_blk = (int32_t)n_blk;
    return NLDPC_OK;
}

// ================================================================ exact max-log ML detection (nldpc_mimo_ml.h, F14)
// One thread per RE, as above: the candidates of an RE are enumerated by its thread, two passes of M^(nt-1) for
// nt >= 2.  MimoArgs, the staging area and the stores are those of the LMMSE kernels.

// enumerate -> finish -> (descramble) -> store
template <int H, int NT, int NR>
__device__ __forceinline__ void mimo_ml_store(const MimoArgs& a, int64_t loc, const float* h, const float* y, uint32_t sm,
                                              float* stage) {
    constexpr int PER = NT * 2 * H;
    float v[PER];
    mimo_ml_detect<H, NT, NR>(h, y, mimo_ml_weight(a.sigma), v);
#pragma unroll
    for (int i = 0; i < PER; ++i) v[i] = __uint_as_float(__float_as_uint(v[i]) ^ (((sm >> i) & 1u) << 31));
    mimo_store_run<PER>(a.llr, loc, v, stage);
}

// ---------------------------------------------------------------- nldpc_mimo_detect_ml: y and H -> LLRs
template <int H, int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_ml_detect_kernel(MimoArgs a) {
    constexpr int PER = NT * 2 * H;
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    const MimoIdx x = mimo_index(loc, a.r.R, a.r.L);
    float h[2 * NR * NT], y[2 * NR];
    mimo_load_block<NT, NR>(a.h, mimo_block(x, a.r.n_blk), h);
#pragma unroll
    for (int e = 0; e < 2 * NR; ++e) y[e] = a.y_in[loc * (2 * NR) + e];
    mimo_ml_store<H, NT, NR>(a, loc, h, y, 0u, mimo_stage<PER>());
}

// ---------------------------------------------------------------- nldpc_mimo_channel_llr_ml, the fused channel:
// bits -> (scramble) -> map -> H x -> noise -> ML detect -> (descramble).  The transmit side is mimo_channel_kernel's,
// statement for statement (the same streams, so the same samples and channels)
template <int H, int NT, int NR>
__global__ __launch_bounds__(kMimoThreads) void mimo_ml_channel_kernel(MimoArgs a) {
    constexpr int QM = 2 * H, PER = NT * QM, PERY = 2 * NR, PERS = PER > PERY ? PER : PERY;
    const int64_t loc = (int64_t)blockIdx.x * kMimoThreads + threadIdx.x;
    if (loc >= a.total) return;
    const MimoIdx x = mimo_index(loc, a.r.R, a.r.L);
    const int64_t blk = mimo_block(x, a.r.n_blk);
    float h[2 * NR * NT];
    if (a.h) mimo_load_block<NT, NR>(a.h, blk, h);  // (a uniform branch)
    else mimo_draw<NT, NR>(mimo_global(a.b_offset, x, a.r.n_blk), a.scale, a.seed, h);
    if (a.h_out && mimo_first(x, a.r.L)) {
        float* dst = a.h_out + blk * (2 * NR * NT);
#pragma unroll
        for (int e = 0; e < 2 * NR * NT; ++e) dst[e] = h[e];
    }
    uint32_t fb = 0u, sm = 0u;
    if (a.f) {
        const uint8_t* src = a.f + loc * PER;
        if (PER % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
            for (int q = 0; q < PER / 4; ++q) {
                const uint32_t wd = reinterpret_cast<const uint32_t*>(src)[q];
#pragma unroll
                for (int j = 0; j < 4; ++j) fb |= (((wd >> (8 * j)) & 0xFFu) ? 1u : 0u) << (4 * q + j);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PER; ++j) fb |= (src[j] ? 1u : 0u) << j;
        }
    }
    if (a.seq) {
        const uint32_t q = a.n_seq == 1 ? 0u : (uint32_t)(a.b_offset + x.b) % (uint32_t)a.n_seq;
        const uint32_t* row = a.seq + (int64_t)q * a.Wc;
#pragma unroll
        for (int k = 0; k < NT; ++k) sm |= gold_bits(row, (int64_t)x.i * PER + k * QM, QM) << (k * QM);
    }
    fb ^= sm;
    float xs[2 * NT], s[2 * NR], y[2 * NR];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        uint32_t ci, cq;
        qam_labels(H, [&](int i) { return ((fb >> (k * QM + i)) & 1u) != 0; }, ci, cq);
        xs[2 * k] = qam_level(H, ci);
        xs[2 * k + 1] = qam_level(H, cq);
    }
    mimo_apply<NT, NR>(h, xs, s);
    const uint64_t Gre = (uint64_t)(a.first + loc);
    const double sigma = (double)a.sigma;
#pragma unroll
    for (int q = 0; q < (NR + 1) / 2; ++q) {
        const U4 c = mimo_counter(Gre, kMimoNoiseTag, (uint32_t)q, a.seed);
        const double rad0 = sqrt(-2.0 * log(u01(c.x))), th0 = 6.283185307179586 * u01(c.y);
        y[4 * q] = (float)((double)s[4 * q] + sigma * (rad0 * cos(th0)));
        y[4 * q + 1] = (float)((double)s[4 * q + 1] + sigma * (rad0 * sin(th0)));
        if (2 * q + 1 < NR) {
            const double rad1 = sqrt(-2.0 * log(u01(c.z))), th1 = 6.283185307179586 * u01(c.w);
            y[4 * q + 2] = (float)((double)s[4 * q + 2] + sigma * (rad1 * cos(th1)));
            y[4 * q + 3] = (float)((double)s[4 * q + 3] + sigma * (rad1 * sin(th1)));
        }
    }
    float* stage = mimo_stage<PERS>();
    mimo_ml_store<H, NT, NR>(a, loc, h, y, sm, stage);
    if (a.y_out) mimo_store_run<PERY>(a.y_out, loc, y, stage);
}

template <int H, int NT, int NR>
static void mimo_ml_detect_host(float sigma, const float* y, const float* h, int64_t B, int64_t R, int32_t L,
                                int32_t n_blk, float* llr) {
    const float w = mimo_ml_weight(sigma);
    for (int64_t loc = 0; loc < B * R; ++loc) {
        const int64_t blk = mimo_block(mimo_index(loc, R, L), n_blk);
        mimo_ml_detect<H, NT, NR>(h + blk * (2 * NR * NT), y + loc * (2 * NR), w, llr + loc * (NT * 2 * H));
    }
}

// [qm / 2 - 1][mimo_dims_index]; nt = 4 stops at 16-QAM (mimo_ml_supported)
#define NLDPC_MIMO_ML_LOW(K, H) {K<H, 1, 1>, K<H, 1, 2>, K<H, 1, 4>, K<H, 2, 2>, K<H, 2, 4>, K<H, 4, 4>}
#define NLDPC_MIMO_ML_HIGH(K, H) {K<H, 1, 1>, K<H, 1, 2>, K<H, 1, 4>, K<H, 2, 2>, K<H, 2, 4>, nullptr}
#define NLDPC_MIMO_ML_ORDERS(K) \
    {NLDPC_MIMO_ML_LOW(K, 1), NLDPC_MIMO_ML_LOW(K, 2), NLDPC_MIMO_ML_HIGH(K, 3), NLDPC_MIMO_ML_HIGH(K, 4)}
static const MimoKernel kMimoMlChannel[4][6] = NLDPC_MIMO_ML_ORDERS(mimo_ml_channel_kernel);
static const MimoKernel kMimoMlDetect[4][6] = NLDPC_MIMO_ML_ORDERS(mimo_ml_detect_kernel);
static const MimoHostDetect kMimoMlDetectHost[4][6] = NLDPC_MIMO_ML_ORDERS(mimo_ml_detect_host);
#undef NLDPC_MIMO_ML_ORDERS
#undef NLDPC_MIMO_ML_HIGH
#undef NLDPC_MIMO_ML_LOW

static int mimo_ml_order(const std::string& who, int32_t qm, int32_t nt) {
    if (!mimo_ml_supported(qm, nt))
        return fail(NLDPC_EUNSUPPORTED, who + ": nt = 4 is detected up to qm = 4 (64- and 256-QAM need a tree search)");
    return NLDPC_OK;
}
}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_mimo_entry_ref(int32_t nt, const uint32_t* words, int64_t n, float* h) {
    const std::string who = "nldpc_mimo_entry_ref";
    if (nt != 1 && nt != 2 && nt != 4) return fail(NLDPC_EINVAL, who + ": nt is 1, 2 or 4");
    if (!words || !h || n <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    const double s = mimo_entry_scale(nt);
    for (int64_t i = 0; i < n; ++i) mimo_entry_of(s, words[2 * i], words[2 * i + 1], h[2 * i], h[2 * i + 1]);
    return NLDPC_OK;
}

extern "C" int nldpc_mimo_filter_ref(int32_t nt, int32_t nr, float sigma, const float* h, int64_t n, float* W, float* mu,
                                     float* w) {
    const std::string who = "nldpc_mimo_filter_ref";
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, who + ": sigma must be positive");
    if (!h || !W || !mu || !w || n <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    kMimoFilterHost[mimo_dims_index(nt, nr)](sigma, h, n, W, mu, w);
    return NLDPC_OK;
}

extern "C" int nldpc_mimo_detect_ref(int32_t qm, int32_t method, int32_t nt, int32_t nr, float sigma, const float* y,
                                     const float* h, int64_t B, int64_t R, int64_t L, float* llr) {
    const std::string who = "nldpc_mimo_detect_ref";
    if (int rc = mimo_demapper(who, qm, method, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!y || !h || !llr || B <= 0 || R <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (R * nt * qm >= (int64_t)1 << 31 || R >= (int64_t)1 << 31 || B >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, who + ": B and R * nt * qm must be below 2^31");
    MimoRows r{};
    if (int rc = mimo_rows(who, B, R, L, r)) return rc;
    kMimoDetectHost[qm / 2 - 1][method][mimo_dims_index(nt, nr)](sigma, y, h, B, R, r.L, r.n_blk, llr);
    return NLDPC_OK;
}

extern "C" int nldpc_mimo_channels(int32_t nt, int32_t nr, uint64_t seed, int64_t B, int64_t n_blk, int64_t b_offset,
                                   float* h, void* stream) {
    const std::string who = "nldpc_mimo_channels";
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!h || B <= 0 || n_blk <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (mimo_misaligned4(h)) return fail(NLDPC_EINVAL, who + ": h must be 4-byte aligned");
    if (n_blk >= (int64_t)1 << 31 || B >= (int64_t)1 << 31 || B * n_blk >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, who + ": B * n_blk must be below 2^31");
    if (b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    MimoChanArgs a{};
    a.h = h;
    a.first = b_offset * n_blk;
    a.total = B * n_blk;
    a.scale = mimo_entry_scale(nt);
    a.seed = seed;
    return mimo_launch(who, kMimoChannels[mimo_dims_index(nt, nr)], a, a.total, stream);
}

extern "C" int nldpc_mimo_filter(int32_t nt, int32_t nr, float sigma, const float* h, int64_t B, int64_t n_blk, float* W,
                                 float* mu, float* w, void* stream) {
    const std::string who = "nldpc_mimo_filter";
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, who + ": sigma must be positive");
    if (!h || !W || !mu || !w || B <= 0 || n_blk <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (mimo_misaligned4(h) || mimo_misaligned4(W) || mimo_misaligned4(mu) || mimo_misaligned4(w))
        return fail(NLDPC_EINVAL, who + ": h, W, mu and w must be 4-byte aligned");
    if (n_blk >= (int64_t)1 << 31 || B >= (int64_t)1 << 31 || B * n_blk >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, who + ": B * n_blk must be below 2^31");
    MimoFilterArgs a{};
    a.h = h;
    a.W = W;
    a.mu = mu;
    a.w = w;
    a.total = B * n_blk;
    a.sigma = sigma;
    return mimo_launch(who, kMimoFilter[mimo_dims_index(nt, nr)], a, a.total, stream);
}

extern "C" int nldpc_mimo_detect(int32_t qm, int32_t method, int32_t nt, int32_t nr, float sigma, const float* y,
                                 const float* h, int64_t B, int64_t R, int64_t L, float* llr, void* stream) {
    const std::string who = "nldpc_mimo_detect";
    if (int rc = mimo_demapper(who, qm, method, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!y || !h || !llr || B <= 0 || R <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (R * nt * qm >= (int64_t)1 << 31 || R >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, who + ": R * nt * qm must be below 2^31");
    if (mimo_misaligned4(y) || mimo_misaligned4(h) || mimo_misaligned4(llr))
        return fail(NLDPC_EINVAL, who + ": y, h and llr must be 4-byte aligned");
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    MimoArgs a{};
    if (int rc = mimo_rows(who, B, R, L, a.r)) return rc;
    a.y_in = y;
    a.h = h;
    a.llr = llr;
    a.total = B * R;
    a.sigma = sigma;
    return mimo_launch(who, kMimoDetect[qm / 2 - 1][method][mimo_dims_index(nt, nr)], a, a.total, stream);
}

extern "C" int nldpc_mimo_channel_llr(int32_t qm, int32_t method, int32_t nt, int32_t nr, const uint8_t* f, int64_t B,
                                      int64_t E, float sigma, uint64_t seed, int64_t b_offset, int64_t L,
                                      const float* h_in, const uint32_t* seq, int64_t n_seq, float* llr, float* sym_out,
                                      float* h_out, void* stream) {
    const std::string who = "nldpc_mimo_channel_llr";
    if (int rc = mimo_demapper(who, qm, method, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!llr || B <= 0 || E <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (E >= (int64_t)1 << 31 || E % qm != 0) return fail(NLDPC_EINVAL, who + ": E must be below 2^31 and a multiple of qm");
    if ((E / qm) % nt != 0) return fail(NLDPC_EINVAL, who + ": E / qm must be a multiple of nt");
    if (mimo_misaligned4(llr) || mimo_misaligned4(sym_out) || mimo_misaligned4(h_in) || mimo_misaligned4(h_out))
        return fail(NLDPC_EINVAL, who + ": llr, sym_out, h_in and h_out must be 4-byte aligned");
    if (B >= (int64_t)1 << 31 || b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    MimoArgs a{};
    const int64_t R = E / qm / nt;
    if (int rc = mimo_rows(who, B, R, L, a.r)) return rc;
    if (h_in && h_out) {
        const uintptr_t bytes = (uintptr_t)(B * a.r.n_blk) * (uintptr_t)(8 * nr * nt);
        const uintptr_t i = reinterpret_cast<uintptr_t>(h_in), o = reinterpret_cast<uintptr_t>(h_out);
        if (i < o + bytes && o < i + bytes) return fail(NLDPC_EINVAL, who + ": h_out must not overlap h_in");
    }
    if (seq) {
        if (mimo_misaligned4(seq)) return fail(NLDPC_EINVAL, who + ": seq must be 4-byte aligned");
        if (n_seq < 1) return fail(NLDPC_EINVAL, who + ": n_seq must be positive");
        a.seq = seq;
        a.n_seq = n_seq;
        a.Wc = (E + 31) >> 5;
        if (n_seq >= (int64_t)1 << 31 || n_seq * a.Wc >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    }
    a.f = f;
    a.h = h_in;
    a.llr = llr;
    a.y_out = sym_out;
    a.h_out = h_out;
    a.total = B * R;
    a.first = b_offset * R;
    a.b_offset = b_offset;
    a.sigma = sigma;
    a.scale = mimo_entry_scale(nt);
    a.seed = seed;
    return mimo_launch(who, kMimoChannel[qm / 2 - 1][method][mimo_dims_index(nt, nr)], a, a.total, stream);
}

extern "C" int nldpc_mimo_detect_ml_ref(int32_t qm, int32_t nt, int32_t nr, float sigma, const float* y, const float* h,
                                        int64_t B, int64_t R, int64_t L, float* llr) {
    const std::string who = "nldpc_mimo_detect_ml_ref";
    if (int rc = mimo_demapper(who, qm, 0, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!y || !h || !llr || B <= 0 || R <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (R * nt * qm >= (int64_t)1 << 31 || R >= (int64_t)1 << 31 || B >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, who + ": B and R * nt * qm must be below 2^31");
    MimoRows r{};
    if (int rc = mimo_rows(who, B, R, L, r)) return rc;
    if (int rc = mimo_ml_order(who, qm, nt)) return rc;
    kMimoMlDetectHost[qm / 2 - 1][mimo_dims_index(nt, nr)](sigma, y, h, B, R, r.L, r.n_blk, llr);
    return NLDPC_OK;
}

extern "C" int nldpc_mimo_detect_ml(int32_t qm, int32_t nt, int32_t nr, float sigma, const float* y, const float* h,
                                    int64_t B, int64_t R, int64_t L, float* llr, void* stream) {
    const std::string who = "nldpc_mimo_detect_ml";
    if (int rc = mimo_demapper(who, qm, 0, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!y || !h || !llr || B <= 0 || R <= 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (R * nt * qm >= (int64_t)1 << 31 || R >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, who + ": R * nt * qm must be below 2^31");
    if (mimo_misaligned4(y) || mimo_misaligned4(h) || mimo_misaligned4(llr))
        return fail(NLDPC_EINVAL, who + ": y, h and llr must be 4-byte aligned");
    MimoArgs a{};
    if (int rc = mimo_rows(who, B, R, L, a.r)) return rc;
    if (int rc = mimo_ml_order(who, qm, nt)) return rc;
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    a.y_in = y;
    a.h = h;
    a.llr = llr;
    a.total = B * R;
    a.sigma = sigma;
    return mimo_launch(who, kMimoMlDetect[qm / 2 - 1][mimo_dims_index(nt, nr)], a, a.total, stream);
}

extern "C" int nldpc_mimo_channel_llr_ml(int32_t qm, int32_t nt, int32_t nr, const uint8_t* f, int64_t B, int64_t E,
                                         float sigma, uint64_t seed, int64_t b_offset, int64_t L, const float* h_in,
                                         const uint32_t* seq, int64_t n_seq, float* llr, float* sym_out, float* h_out,
                                         void* stream) {
    const std::string who = "nldpc_mimo_channel_llr_ml";
    if (int rc = mimo_demapper(who, qm, 0, sigma)) return rc;
    if (int rc = mimo_dims(who, nt, nr)) return rc;
    if (!llr || B <= 0 || E <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (E >= (int64_t)1 << 31 || E % qm != 0) return fail(NLDPC_EINVAL, who + ": E must be below 2^31 and a multiple of qm");
    if ((E / qm) % nt != 0) return fail(NLDPC_EINVAL, who + ": E / qm must be a multiple of nt");
    if (mimo_misaligned4(llr) || mimo_misaligned4(sym_out) || mimo_misaligned4(h_in) || mimo_misaligned4(h_out))
        return fail(NLDPC_EINVAL, who + ": llr, sym_out, h_in and h_out must be 4-byte aligned");
    MimoArgs a{};
    const int64_t R = E / qm / nt;
    if (int rc = mimo_rows(who, B, R, L, a.r)) return rc;
    if (h_in && h_out) {
        const uintptr_t bytes = (uintptr_t)(B * a.r.n_blk) * (uintptr_t)(8 * nr * nt);
        const uintptr_t i = reinterpret_cast<uintptr_t>(h_in), o = reinterpret_cast<uintptr_t>(h_out);
        if (i < o + bytes && o < i + bytes) return fail(NLDPC_EINVAL, who + ": h_out must not overlap h_in");
    }
    if (seq) {
        if (mimo_misaligned4(seq)) return fail(NLDPC_EINVAL, who + ": seq must be 4-byte aligned");
        if (n_seq < 1) return fail(NLDPC_EINVAL, who + ": n_seq must be positive");
    }
    if (int rc = mimo_ml_order(who, qm, nt)) return rc;
    if (B >= (int64_t)1 << 31 || b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    if (seq) {
        a.seq = seq;
        a.n_seq = n_seq;
        a.Wc = (E + 31) >> 5;
        if (n_seq >= (int64_t)1 << 31 || n_seq * a.Wc >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    }
    a.f = f;
    a.h = h_in;
    a.llr = llr;
    a.y_out = sym_out;
    a.h_out = h_out;
    a.total = B * R;
    a.first = b_offset * R;
    a.b_offset = b_offset;
    a.sigma = sigma;
    a.scale = mimo_entry_scale(nt);
    a.seed = seed;
    return mimo_launch(who, kMimoMlChannel[qm / 2 - 1][mimo_dims_index(nt, nr)], a, a.total, stream);
}
