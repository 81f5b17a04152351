// Circular-buffer rate matching and LLR rate recovery (3GPP TS 38.212 §5.4.2): nldpc_rm_k0, nldpc_rm_index,
// nldpc_rate_match, nldpc_rate_recover.  The index maps are the closed forms of nldpc_rm_index.h; the host resolves a
// nldpc_rm against the graph's dimensions into an RmMap (validation included) and the kernels only gather.
//
// Both kernels give a thread one run of RUN consecutive output elements of one codeword, placed on RUN-element
// boundaries of the output ADDRESS (rows start anywhere: E may be odd, the caller's buffer may be a view), so a whole
// run leaves as one vector store and the partial runs at the two ends of a row as element stores.  A workgroup is
// R rows x W runs (R > 1 when a row has fewer than 256 runs); rows beyond the grid's second dimension are looped over.
#include <hip/hip_runtime.h>

#include <string>

#include "nldpc_internal.h"
#include "nldpc_math.h"
#include "nldpc_rm_index.h"

namespace nldpc {
constexpr int kRmThreads = 256;
// the variants of DESIGN §4.4 (a build with -DNLDPC_RM_MATCH_RUN=4 or -DNLDPC_RM_NT=0 measures the others)
#ifndef NLDPC_RM_MATCH_RUN
#define NLDPC_RM_MATCH_RUN 16
#endif
#ifndef NLDPC_RM_NT
#define NLDPC_RM_NT 1
#endif
constexpr int kRmMatchRun = NLDPC_RM_MATCH_RUN;  // output bytes per thread of rate_match_kernel: 4 or 16
constexpr int kRmRecoverRun = 4;                 // output floats per thread of rate_recover_kernel
constexpr bool kRmNonTemporal = NLDPC_RM_NT;     // whole runs leave with non-temporal stores (nothing reads them back soon)
typedef uint32_t rm_u4 __attribute__((ext_vector_type(4)));  // (the nontemporal builtins take native vectors)
typedef float rm_f4 __attribute__((ext_vector_type(4)));

template <typename V>
__device__ __forceinline__ void rm_store(V* p, V v) {
    if constexpr (kRmNonTemporal) {
        __builtin_nontemporal_store(v, p);
    } else {
        *p = v;
    }
}

// how the 256 threads of a workgroup tile the runs of a row: W runs of each of R rows, gx workgroups per row
struct RmTile {
    uint32_t W, R, gx;
};
static RmTile rm_tile(int64_t len, int run) {
    const int64_t C = (len + 2 * run - 2) / run;  // runs of a row at the worst misalignment
    const int64_t gx = (C + kRmThreads - 1) / kRmThreads;
    const int64_t W = (C + gx - 1) / gx;
    return RmTile{(uint32_t)W, (uint32_t)(kRmThreads / W), (uint32_t)gx};
}

// nldpc_rm against (M, N, Z): every rule of include/nldpc.h, then the derived constants
static int rm_resolve(const char* who, int64_t M, int64_t N, int64_t Z, const nldpc_rm* rm, RmMap* out) {
    const std::string w = std::string(who) + ": ";
    if (!rm) return fail(NLDPC_EINVAL, w + "rm is NULL");
    if (M < 1 || N < M || Z < 1) return fail(NLDPC_EINVAL, w + "bad graph dimensions");
    const int64_t K = N - M, NZ = N * Z, KZ = K * Z;
    if (NZ >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, w + "N*Z must be below 2^31");
    if (rm->punct_cols < 0 || rm->punct_cols > K) return fail(NLDPC_EINVAL, w + "punct_cols must be in [0, K]");
    const int64_t P = rm->punct_cols * Z, F = rm->n_filler;
    if (F < 0 || F > KZ - P) return fail(NLDPC_EINVAL, w + "n_filler must be in [0, (K - punct_cols) * Z]");
    if (rm->ncb != 0 && (rm->ncb < KZ - P || rm->ncb > NZ - P))
        return fail(NLDPC_EINVAL, w + "ncb must be 0 or in [K*Z - P, N*Z - P]");
    const int64_t Ncb = rm->ncb ? rm->ncb : NZ - P, Nv = Ncb - F;
    if (Nv < 1) return fail(NLDPC_EINVAL, w + "no valid buffer position (ncb - n_filler < 1)");
    if (rm->k0 < 0 || rm->k0 >= Ncb) return fail(NLDPC_EINVAL, w + "k0 must be in [0, Ncb)");
    if (rm->E < 1 || rm->E >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, w + "E must be in [1, 2^31)");
    if (rm->qm < 1 || rm->E % rm->qm != 0) return fail(NLDPC_EINVAL, w + "qm must be positive and divide E");
    const int64_t f0 = KZ - F - P, f1 = KZ - P, Eq = rm->E / rm->qm;
    RmMap a{};
    a.E = (uint32_t)rm->E;
    a.Eq = (uint32_t)Eq;
    a.Qm = (uint32_t)rm->qm;
    a.P = (uint32_t)P;
    a.Ncb = (uint32_t)Ncb;
    a.NZ = (uint32_t)NZ;
    a.f0 = (uint32_t)f0;
    a.F = (uint32_t)F;
    a.Nv = (uint32_t)Nv;
    a.v0 = (uint32_t)(rm->k0 <= f0 ? rm->k0 : (rm->k0 >= f1 ? rm->k0 - F : f0));
    a.step_i = (uint32_t)(Eq % Nv);
    a.step_j = (uint32_t)((1 + Nv - ((rm->qm - 1) * Eq) % Nv) % Nv);
    a.inv_qm = rm_inv(a.Qm);
    a.inv_nv = rm_inv(a.Nv);
    a.inv_eq = rm_inv(a.Eq);
    *out = a;
    return NLDPC_OK;
}

// ---------------------------------------------------------------- rate_match: f[b][m] = y[b][idx[m]] != 0
template <int RUN>
__global__ __launch_bounds__(kRmThreads) void rate_match_kernel(RmMap a, const uint8_t* __restrict__ y,
                                                                uint8_t* __restrict__ f, int64_t B, uint32_t W,
                                                                uint32_t R) {
    static_assert(RUN == 4 || RUN == 16, "a run is one dword or one 16-byte store");
    const uint32_t r = threadIdx.x / W, c = blockIdx.x * W + (threadIdx.x - r * W);
    if (r >= R) return;
    for (int64_t b = (int64_t)blockIdx.y * R + r; b < B; b += (int64_t)gridDim.y * R) {
        uint8_t* row = f + b * a.E;
        const uint8_t* yb = y + b * a.NZ;
        // the run's first output index; below 0 / past E: the part of a boundary run outside the row
        const int64_t m0 = (int64_t)c * RUN - (int64_t)(reinterpret_cast<uintptr_t>(row) & (RUN - 1));
        const int64_t lo = m0 < 0 ? 0 : m0, hi = m0 + RUN < (int64_t)a.E ? m0 + RUN : (int64_t)a.E;
        if (lo >= hi) continue;
        RmCursor cur = rm_seek(a, (uint32_t)lo);
        if (hi - lo == RUN) {
            uint32_t w[RUN / 4];
#pragma unroll
            for (int q = 0; q < RUN / 4; ++q) {
                w[q] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[q] |= (yb[rm_bit(a, cur)] ? 1u : 0u) << (8 * k);
                    rm_step(a, cur);
                }
            }
            if constexpr (RUN == 16) {
                rm_store(reinterpret_cast<rm_u4*>(row + m0), rm_u4{w[0], w[1], w[2], w[3]});
            } else {
                rm_store(reinterpret_cast<uint32_t*>(row + m0), w[0]);
            }
        } else {
            for (int64_t m = lo; m < hi; ++m) {
                row[m] = yb[rm_bit(a, cur)] ? 1 : 0;
                rm_step(a, cur);
            }
        }
    }
}

// ---------------------------------------------------------------- rate_recover: xa[b][n] from llr[b][.]
struct RecoverArgs {
    const float* llr;
    float* xa;
    int64_t B;
    float erasure, filler, clip;
    int32_t accumulate;
    uint32_t W, R;
};

// one codeword position: true when *val is to be written
__device__ __forceinline__ bool recover_one(const RmMap& a, const RecoverArgs& g, const float* __restrict__ lrow,
                                            const float* xrow, uint32_t n, float* val) {
    uint32_t k = 0;
    const int st = rm_first(a, n, &k);
    if (st == RM_FILLER) {
        *val = g.filler;
        return true;
    }
    if (st == RM_SENT && k < a.E) {
        float acc = g.accumulate ? xrow[n] : 0.f;
        for (; k < a.E; k += a.Nv) acc = fadd(acc, lrow[rm_out_pos(a, k)]);  // ascending k; k + Nv < 2^32
        if (g.clip > 0.f) acc = clampf(acc, -g.clip, g.clip);
        *val = acc;
        return true;
    }
    *val = g.erasure;
    return !g.accumulate;
}

__global__ __launch_bounds__(kRmThreads) void rate_recover_kernel(RmMap a, RecoverArgs g) {
    constexpr int RUN = kRmRecoverRun;
    const uint32_t r = threadIdx.x / g.W, c = blockIdx.x * g.W + (threadIdx.x - r * g.W);
    if (r >= g.R) return;
    for (int64_t b = (int64_t)blockIdx.y * g.R + r; b < g.B; b += (int64_t)gridDim.y * g.R) {
        float* xrow = g.xa + b * a.NZ;
        const float* lrow = g.llr + b * a.E;
        const int64_t m0 = (int64_t)c * RUN - (int64_t)((reinterpret_cast<uintptr_t>(xrow) >> 2) & (RUN - 1));
        const int64_t lo = m0 < 0 ? 0 : m0, hi = m0 + RUN < (int64_t)a.NZ ? m0 + RUN : (int64_t)a.NZ;
        if (lo >= hi) continue;
        if (hi - lo == RUN) {
            float v[RUN];
            bool wr[RUN], all = true;
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
                wr[k] = recover_one(a, g, lrow, xrow, (uint32_t)m0 + k, &v[k]);
                all = all && wr[k];
            }
            if (all) {
                rm_store(reinterpret_cast<rm_f4*>(xrow + m0), rm_f4{v[0], v[1], v[2], v[3]});
            } else {  // (accumulate: a position that received nothing is not written)
#pragma unroll
                for (int k = 0; k < RUN; ++k)
                    if (wr[k]) xrow[m0 + k] = v[k];
            }
        } else {
            for (int64_t n = lo; n < hi; ++n) {
                float v;
                if (recover_one(a, g, lrow, xrow, (uint32_t)n, &v)) xrow[n] = v;
            }
        }
    }
}
}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_rm_k0(int32_t bg, int32_t rv, int64_t ncb, int32_t Z, int64_t* k0) {
    static const int64_t num[2][4] = {{0, 17, 33, 56}, {0, 13, 25, 43}};  // TS 38.212 Table 5.4.2.1-2
    static const int64_t den[2] = {66, 50};
    if (!k0) return fail(NLDPC_EINVAL, "nldpc_rm_k0: k0 is NULL");
    if (bg != 1 && bg != 2) return fail(NLDPC_EINVAL, "nldpc_rm_k0: bg is 1 or 2");
    if (rv < 0 || rv > 3) return fail(NLDPC_EINVAL, "nldpc_rm_k0: rv is 0..3");
    if (ncb <= 0 || ncb >= (int64_t)1 << 31 || Z <= 0) return fail(NLDPC_EINVAL, "nldpc_rm_k0: ncb and Z must be positive");
    *k0 = num[bg - 1][rv] * ncb / (den[bg - 1] * Z) * Z;
    return NLDPC_OK;
}

extern "C" int nldpc_rm_index(int32_t M, int32_t N, int32_t Z, const nldpc_rm* rm, int32_t* idx) {
    RmMap a;
    if (int st = rm_resolve("nldpc_rm_index", M, N, Z, rm, &a)) return st;
    if (!idx) return fail(NLDPC_EINVAL, "nldpc_rm_index: idx is NULL");
    // walked with the cursor as a kernel thread walks its run, and sought afresh at every m as a thread does at the
    // start of its run: the two must agree, and the inverse map must lead back to m
    RmCursor cur = rm_seek(a, 0);
    for (uint32_t m = 0; m < a.E; ++m) {
        const RmCursor s = rm_seek(a, m);
        const uint32_t n = rm_bit(a, cur);
        const uint32_t km = (m % a.Qm) * a.Eq + m / a.Qm;  // the selection index of m: a copy of n's first one
        uint32_t k = 0;
        if (s.i != cur.i || s.v != cur.v || rm_first(a, n, &k) != RM_SENT || km < k || (km - k) % a.Nv != 0 ||
            rm_out_pos(a, km) != m)
            return fail(NLDPC_EINVAL, "nldpc_rm_index: internal error, the index maps disagree");
        idx[m] = (int32_t)n;
        rm_step(a, cur);
    }
    return NLDPC_OK;
}

extern "C" int nldpc_rate_match(const nldpc_graph* g, const nldpc_rm* rm, const uint8_t* y, int64_t B, uint8_t* f,
                                void* stream) {
    if (!g || !y || !f || B <= 0) return fail(NLDPC_EINVAL, "nldpc_rate_match: bad argument");
    RmMap a;
    if (int st = rm_resolve("nldpc_rate_match", g->dev.M, g->dev.N, g->dev.Z, rm, &a)) return st;
    const RmTile t = rm_tile(a.E, kRmMatchRun);
    const int64_t gy = (B + t.R - 1) / t.R;
    DeviceGuard guard(g->device);
    hipLaunchKernelGGL(rate_match_kernel<kRmMatchRun>, dim3(t.gx, (unsigned)(gy < 65535 ? gy : 65535)), dim3(kRmThreads),
                       0, static_cast<hipStream_t>(stream), a, y, f, B, t.W, t.R);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, "rate_match_kernel launch");
}

extern "C" int nldpc_rate_recover(const nldpc_graph* g, const nldpc_rm* rm, const float* llr, int64_t B,
                                  float erasure_value, float filler_value, float clip, int32_t accumulate, float* xa,
                                  void* stream) {
    if (!g || !llr || !xa || B <= 0) return fail(NLDPC_EINVAL, "nldpc_rate_recover: bad argument");
    if ((reinterpret_cast<uintptr_t>(llr) | reinterpret_cast<uintptr_t>(xa)) & 3)
        return fail(NLDPC_EINVAL, "nldpc_rate_recover: llr and xa must be 4-byte aligned");
    if (accumulate != 0 && accumulate != 1) return fail(NLDPC_EINVAL, "nldpc_rate_recover: accumulate is 0 or 1");
    RmMap a;
    if (int st = rm_resolve("nldpc_rate_recover", g->dev.M, g->dev.N, g->dev.Z, rm, &a)) return st;
    const RmTile t = rm_tile(a.NZ, kRmRecoverRun);
    RecoverArgs r{llr, xa, B, erasure_value, filler_value, clip, accumulate, t.W, t.R};
    const int64_t gy = (B + t.R - 1) / t.R;
    DeviceGuard guard(g->device);
    hipLaunchKernelGGL(rate_recover_kernel, dim3(t.gx, (unsigned)(gy < 65535 ? gy : 65535)), dim3(kRmThreads), 0,
                       static_cast<hipStream_t>(stream), a, r);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, "rate_recover_kernel launch");
}
