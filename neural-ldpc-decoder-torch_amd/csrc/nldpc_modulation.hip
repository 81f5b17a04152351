// QAM modulation and soft demapping (3GPP TS 38.211 §5.1.3-5.1.6; include/nldpc.h): nldpc_qam_points,
// nldpc_qam_demap_ref (host), nldpc_qam_modulate, nldpc_qam_demap, nldpc_qam_channel_llr, nldpc_qam_channel_llr_scrambled.
// The arithmetic is the inline functions of nldpc_qam.h (and nldpc_gold.h) on both sides.  The flat-fading channel with
// perfect CSI (nldpc_fading_gain_ref, nldpc_qam_demap_csi_ref (host), nldpc_fading_gains, nldpc_qam_demap_csi,
// nldpc_qam_fading_channel_llr; arithmetic in nldpc_fading.h) shares the pair, load and store helpers below.
//
// Bits, symbols and LLRs of a batch are flat streams ([B][E] bytes, [B][S][2] and [B][E] floats, all contiguous), so a
// row plays no part: a thread owns one PAIR of consecutive symbols -- in the fused kernel the two symbols of one Philox
// counter, global pair index ((b_offset * S + local symbol) >> 1) -- of which it handles those inside the batch (the
// first pair of a shard that starts at an odd symbol and the last pair of an odd total are half pairs).  A pair is
// 2 qm bytes of f, 4 floats of symbols and 2 qm floats of LLRs, each a multiple of 4 bytes / 16 bytes: when a whole
// pair's address is so aligned it is read as dwords and leaves as non-temporal 16-byte stores -- the LLRs of a whole wave
// turned through LDS first, so that a store instruction covers consecutive addresses (qam_store_pair) --, otherwise (a
// half pair, a view that starts off the boundary, an odd first symbol with qm = 2 or 6) element by element.  Nothing
// outside the outputs is touched.
#include <hip/hip_runtime.h>

#include "nldpc_fading.h"
#include "nldpc_gold.h"
#include "nldpc_internal.h"
#include "nldpc_philox.h"
#include "nldpc_qam.h"

namespace nldpc {
constexpr int kQamThreads = 256;
constexpr uint32_t kQamTag = 0x51414D31u;  // counter word 2 of the QAM noise stream ("QAM1")
// the store variants of DESIGN §4.4 (a build with -DNLDPC_QAM_NT=0 measures plain stores, -DNLDPC_QAM_STAGE=0 every lane
// storing its own pair)
#ifndef NLDPC_QAM_NT
#define NLDPC_QAM_NT 1
#endif
#ifndef NLDPC_QAM_STAGE
#define NLDPC_QAM_STAGE 1
#endif
typedef float qam_f4 __attribute__((ext_vector_type(4)));  // (the nontemporal builtins take native vectors)

struct QamArgs {
    const uint8_t* f;   // [total * qm] bits, or nullptr
    const float* in;    // [total][2] symbols (demap)
    float* llr;         // [total * qm]
    float* sym;         // [total][2], or nullptr
    int64_t first;      // global index of the batch's first symbol (fused; else 0)
    int64_t total;      // symbols of the batch
    double sigma;
    float w;            // 1 / (2 sigma^2)
    uint64_t seed;
};

// the thread's pair: loc = the batch-local index of its even symbol (-1: a half pair at the start)
struct QamPair {
    int64_t g, loc;
    bool own0, own1;
};
__device__ __forceinline__ QamPair qam_pair(const QamArgs& a) {
    QamPair p;
    p.g = (a.first >> 1) + (int64_t)blockIdx.x * kQamThreads + threadIdx.x;
    p.loc = 2 * p.g - a.first;
    p.own0 = p.loc >= 0 && p.loc < a.total;
    p.own1 = p.loc + 1 < a.total;  // (loc + 1 >= 0 always)
    return p;
}

// the pair's 2 * QM bytes of f as H = QM / 2 dwords (byte i of the pair = byte i & 3 of word i >> 2); an unowned
// symbol's bytes are not read and stay 0
template <int H>
__device__ __forceinline__ void qam_load_bits(const uint8_t* __restrict__ f, const QamPair& p, uint32_t* w) {
    constexpr int QM = 2 * H;
#pragma unroll
    for (int q = 0; q < H; ++q) w[q] = 0;
    if (!f) return;
    const uint8_t* src = f + p.loc * QM;
    if (p.own0 && p.own1 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < H; ++q) w[q] = reinterpret_cast<const uint32_t*>(src)[q];
    } else {
#pragma unroll
        for (int i = 0; i < 2 * QM; ++i)
            if (i < QM ? p.own0 : p.own1) w[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
}

// the levels (I, Q) of symbol j of the pair
template <int H>
__device__ __forceinline__ void qam_map_pair(const uint32_t* w, int j, float& li, float& lq) {
    constexpr int QM = 2 * H;
    uint32_t ci, cq;
    qam_labels(H, [&](int i) { return ((w[(j * QM + i) >> 2] >> (8 * ((j * QM + i) & 3))) & 0xFFu) != 0; }, ci, cq);
    li = qam_level(H, ci);
    lq = qam_level(H, cq);
}

__device__ __forceinline__ void qam_store4(qam_f4* p, qam_f4 x) {
#if NLDPC_QAM_NT
    __builtin_nontemporal_store(x, p);
#else
    *p = x;
#endif
}

// a pair's 2 * PER floats v to base[loc * PER ..).  A wave's 64 pairs are one contiguous run of 128 * PER floats: when
// every lane owns its whole pair and the run starts on a 16-byte boundary, the wave turns it through LDS (stage: one
// wave's run, [64][2 * PER] floats) so that each store instruction writes 64 consecutive 16-byte groups -- a lane's own
// 2 * PER floats are PER / 2 groups 8 * PER bytes apart from its neighbour's, which costs up to PER / 2 times the
// write requests.  PER = 2 is one group per lane already.  Otherwise (the waves at the two ends of the
// batch, an output off the boundary) a lane stores its own pair: as 16-byte groups when they are aligned, else by element.
template <int PER>
__device__ __forceinline__ void qam_store_pair(float* base, const QamPair& p, const float* v, qam_f4* stage) {
    static_assert((2 * PER) % 4 == 0, "a pair is whole 16-byte groups");
    constexpr int N4 = 2 * PER / 4;
    float* dst = base + p.loc * PER;
    const bool whole = p.own0 && p.own1;
    if constexpr (N4 > 1 && NLDPC_QAM_STAGE) {
        const int lane = threadIdx.x & 63;
        float* run = dst - (int64_t)lane * 2 * PER;  // lane 0's pair: the same address in every lane
        if (__ballot(whole) == ~0ull && (reinterpret_cast<uintptr_t>(run) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < N4; ++q) stage[lane * N4 + q] = qam_f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            // (the wave reads what its other lanes wrote: LDS operations of a wave complete in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int q = 0; q < N4; ++q) qam_store4(reinterpret_cast<qam_f4*>(run) + q * 64 + lane, stage[q * 64 + lane]);
            return;
        }
    }
    if (whole && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < N4; ++q)
            qam_store4(reinterpret_cast<qam_f4*>(dst) + q, qam_f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]});
    } else {
#pragma unroll
        for (int i = 0; i < 2 * PER; ++i)
            if (i < PER ? p.own0 : p.own1) dst[i] = v[i];
    }
}

// the staging area of the calling thread's wave for an LLR run ([64][QM / 2] groups), one per wave of the workgroup
template <int H>
__device__ __forceinline__ qam_f4* qam_stage() {
    __shared__ qam_f4 stage[kQamThreads * H];
    return stage + (threadIdx.x >> 6) * 64 * H;
}

// ---------------------------------------------------------------- bits -> symbols
template <int H>
__global__ __launch_bounds__(kQamThreads) void qam_modulate_kernel(QamArgs a) {
    const QamPair p = qam_pair(a);
    if (!p.own0 && !p.own1) return;
    uint32_t w[H];
    qam_load_bits<H>(a.f, p, w);
    float r[4];
    qam_map_pair<H>(w, 0, r[0], r[1]);
    qam_map_pair<H>(w, 1, r[2], r[3]);
    qam_store_pair<2>(a.sym, p, r, nullptr);
}

// ---------------------------------------------------------------- symbols -> LLRs
template <int H, int METHOD>
__global__ __launch_bounds__(kQamThreads) void qam_demap_kernel(QamArgs a) {
    constexpr int QM = 2 * H;
    const QamPair p = qam_pair(a);
    if (!p.own0) return;  // (first == 0: no half pair at the start)
    const float* src = a.in + p.loc * 2;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.own1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const qam_f4 x = *reinterpret_cast<const qam_f4*>(src);
        r[0] = x.x, r[1] = x.y, r[2] = x.z, r[3] = x.w;
    } else {
        r[0] = src[0], r[1] = src[1];
        if (p.own1) r[2] = src[2], r[3] = src[3];
    }
    float lvl[1 << H], v[2 * QM];
    qam_levels<H>(lvl);
    qam_demap_symbol<H, METHOD>(lvl, r[0], r[1], a.w, v);
    qam_demap_symbol<H, METHOD>(lvl, r[2], r[3], a.w, v + QM);
    qam_store_pair<QM>(a.llr, p, v, qam_stage<H>());
}

// ---------------------------------------------------------------- bits -> symbols + noise -> LLRs, one Philox counter per thread
template <int H, int METHOD>
__global__ __launch_bounds__(kQamThreads) void qam_channel_kernel(QamArgs a) {
    constexpr int QM = 2 * H;
    const QamPair p = qam_pair(a);
    if (!p.own0 && !p.own1) return;
    const U4 c = philox4x32_10(U4{(uint32_t)p.g, (uint32_t)(p.g >> 32), kQamTag, 0u}, (uint32_t)a.seed,
                               (uint32_t)(a.seed >> 32));
    // the Box-Muller of awgn_kernel: (I, Q) of the even symbol, then (I, Q) of the odd one
    const double rad0 = sqrt(-2.0 * log(u01(c.x))), th0 = 6.283185307179586 * u01(c.y);
    const double rad1 = sqrt(-2.0 * log(u01(c.z))), th1 = 6.283185307179586 * u01(c.w);
    const double n[4] = {rad0 * cos(th0), rad0 * sin(th0), rad1 * cos(th1), rad1 * sin(th1)};
    uint32_t w[H];
    qam_load_bits<H>(a.f, p, w);
    float l[4], r[4];
    qam_map_pair<H>(w, 0, l[0], l[1]);
    qam_map_pair<H>(w, 1, l[2], l[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = (float)((double)l[q] + a.sigma * n[q]);
    float lvl[1 << H], v[2 * QM];
    qam_levels<H>(lvl);
    qam_demap_symbol<H, METHOD>(lvl, r[0], r[1], a.w, v);
    qam_demap_symbol<H, METHOD>(lvl, r[2], r[3], a.w, v + QM);
    qam_store_pair<QM>(a.llr, p, v, qam_stage<H>());
    if (a.sym) qam_store_pair<2>(a.sym, p, r, nullptr);
}

// ---------------------------------------------------------------- the same with Gold-sequence scrambling in flight
// (nldpc_qam_channel_llr_scrambled): f ^ c goes into the mapper and the LLRs leave with their sign bits XORed with c, so
// the caller sees the LLRs of f while the symbols on the air are those of the scrambled bits.  The counter, the noise and
// the store path are qam_channel_kernel's.  A symbol's qm sequence bits come from the packed table [n_seq][Wc]
// (gold_bits); its row and in-row index follow from its batch-local index with one division and one remainder per thread:
// the odd symbol is divided, the even one is its predecessor (the last symbol of the row before, with the sequence before,
// when the pair straddles two rows).
struct QamScrArgs {
    QamArgs q;
    const uint32_t* seq;  // [n_seq][Wc]
    int64_t n_seq, Wc;
    int64_t S;         // symbols per row
    int64_t b_offset;  // row b uses sequence (b_offset + b) mod n_seq
};

// qam_map_pair with bit i of the symbol XORed with bit i of m
template <int H>
__device__ __forceinline__ void qam_map_pair_scr(const uint32_t* w, int j, uint32_t m, float& li, float& lq) {
    constexpr int QM = 2 * H;
    uint32_t ci, cq;
    const auto bit = [&](int i) {
        const bool f = ((w[(j * QM + i) >> 2] >> (8 * ((j * QM + i) & 3))) & 0xFFu) != 0;
        return f != (((m >> i) & 1u) != 0);
    };
    qam_labels(H, bit, ci, cq);
    li = qam_level(H, ci);
    lq = qam_level(H, cq);
}

template <int H, int METHOD>
__global__ __launch_bounds__(kQamThreads) void qam_channel_scr_kernel(QamScrArgs s) {
    constexpr int QM = 2 * H;
    const QamArgs& a = s.q;
    const QamPair p = qam_pair(a);
    if (!p.own0 && !p.own1) return;
    const U4 c = philox4x32_10(U4{(uint32_t)p.g, (uint32_t)(p.g >> 32), kQamTag, 0u}, (uint32_t)a.seed,
                               (uint32_t)(a.seed >> 32));
    const double rad0 = sqrt(-2.0 * log(u01(c.x))), th0 = 6.283185307179586 * u01(c.y);
    const double rad1 = sqrt(-2.0 * log(u01(c.z))), th1 = 6.283185307179586 * u01(c.w);
    const double n[4] = {rad0 * cos(th0), rad0 * sin(th0), rad1 * cos(th1), rad1 * sin(th1)};
    // the odd symbol's row b1 and in-row index j1 (loc + 1 >= 0 always), its sequence i1 = (b_offset + b1) mod n_seq
    // (b_offset + b1 < 2^32, n_seq < 2^31), and from them the even symbol's
    const int64_t b1 = (p.loc + 1) / s.S, j1 = (p.loc + 1) - b1 * s.S;
    const uint32_t i1 = s.n_seq == 1 ? 0u : (uint32_t)(s.b_offset + b1) % (uint32_t)s.n_seq;
    const uint32_t i0 = j1 ? i1 : (i1 ? i1 - 1u : (uint32_t)s.n_seq - 1u);
    const int64_t j0 = j1 ? j1 - 1 : s.S - 1;
    uint32_t m[2] = {0u, 0u};
    if (p.own0) m[0] = gold_bits(s.seq + (int64_t)i0 * s.Wc, j0 * QM, QM);
    if (p.own1) m[1] = gold_bits(s.seq + (int64_t)i1 * s.Wc, j1 * QM, QM);
    uint32_t w[H];
    qam_load_bits<H>(a.f, p, w);
    float l[4], r[4];
    qam_map_pair_scr<H>(w, 0, m[0], l[0], l[1]);
    qam_map_pair_scr<H>(w, 1, m[1], l[2], l[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = (float)((double)l[q] + a.sigma * n[q]);
    float lvl[1 << H], v[2 * QM];
    qam_levels<H>(lvl);
    qam_demap_symbol<H, METHOD>(lvl, r[0], r[1], a.w, v);
    qam_demap_symbol<H, METHOD>(lvl, r[2], r[3], a.w, v + QM);
#pragma unroll
    for (int i = 0; i < 2 * QM; ++i) v[i] = __uint_as_float(__float_as_uint(v[i]) ^ (((m[i / QM] >> (i % QM)) & 1u) << 31));
    qam_store_pair<QM>(a.llr, p, v, qam_stage<H>());
    if (a.sym) qam_store_pair<2>(a.sym, p, r, nullptr);
}

// ---------------------------------------------------------------- flat block fading with perfect CSI (nldpc_fading.h)
// nldpc_fading_gains: the table [B][n_blk].  Its entries are a flat stream of global blocks from b_offset * n_blk on, two
// to a Philox counter: QamArgs / qam_pair with blocks for symbols (first = the first global block, total = B * n_blk).
struct FadeGainArgs {
    QamArgs q;
    double mu, s;  // fading_coeff of K
    float* g;      // [total]
};

__global__ __launch_bounds__(kQamThreads) void fading_gains_kernel(FadeGainArgs a) {
    const QamPair p = qam_pair(a.q);
    if (!p.own0 && !p.own1) return;
    const U4 c = philox4x32_10(U4{(uint32_t)p.g, (uint32_t)(p.g >> 32), kFadeTag, 0u}, (uint32_t)a.q.seed,
                               (uint32_t)(a.q.seed >> 32));
    if (p.own0) a.g[p.loc] = fading_gain_of(a.mu, a.s, c.x, c.y);
    if (p.own1) a.g[p.loc + 1] = fading_gain_of(a.mu, a.s, c.z, c.w);
}

// the symbols' side of a faded batch: rows of S symbols in blocks of L, and the given table
struct FadeRows {
    int64_t S;
    int32_t L, n_blk;   // L <= S
    const float* gain;  // [B][n_blk], or nullptr: drawn (fused kernel only)
};

// nldpc_qam_demap_csi: qam_demap_kernel with each symbol demapped against the levels scaled by its block's gain
struct QamCsiArgs {
    QamArgs q;
    FadeRows r;
};

template <int H, int METHOD>
__global__ __launch_bounds__(kQamThreads) void qam_demap_csi_kernel(QamCsiArgs s) {
    constexpr int QM = 2 * H;
    const QamArgs& a = s.q;
    const QamPair p = qam_pair(a);
    if (!p.own0) return;  // (first == 0: no half pair at the start)
    const float* src = a.in + p.loc * 2;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.own1 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const qam_f4 x = *reinterpret_cast<const qam_f4*>(src);
        r[0] = x.x, r[1] = x.y, r[2] = x.z, r[3] = x.w;
    } else {
        r[0] = src[0], r[1] = src[1];
        if (p.own1) r[2] = src[2], r[3] = src[3];
    }
    const FadeIdx i1 = fading_index(p.loc + 1, s.r.S, s.r.L), i0 = fading_prev(i1, s.r.S, s.r.L, s.r.n_blk);
    const float g0 = s.r.gain[fading_entry(i0, s.r.n_blk)];
    const float g1 = p.own1 ? s.r.gain[fading_entry(i1, s.r.n_blk)] : 0.f;
    float lvl[1 << H], lv[1 << H], v[2 * QM];
    qam_levels<H>(lvl);
    fading_levels<H>(g0, lvl, lv);
    qam_demap_symbol<H, METHOD>(lv, r[0], r[1], a.w, v);
    fading_levels<H>(g1, lvl, lv);
    qam_demap_symbol<H, METHOD>(lv, r[2], r[3], a.w, v + QM);
    qam_store_pair<QM>(a.llr, p, v, qam_stage<H>());
}

// nldpc_qam_fading_channel_llr, the fused channel: qam_channel_kernel / qam_channel_scr_kernel (SCR) with a gain between
// the mapper and the noise and the CSI demapper behind it.  Counter, noise, bit loads and stores are theirs.  A thread's
// two symbols lie in the same fading block or in two consecutive global blocks (blocks do not span rows, and the first
// block of a row follows the last of the row before): their rows, in-row indices and blocks follow from one 64-bit and
// one 32-bit division of the odd symbol (fading_index / fading_prev), which also serve the scramble sequence.  The gains
// are loaded from the table or drawn (a uniform branch): global block Gf takes words (x, y) of the Philox counter
// Gf >> 1 with tag "FAD1" when it is even, (z, w) when odd, so two blocks of one thread share a counter when the odd
// symbol's block is odd -- always with L = 1, where Gf is the global symbol index -- and need a second one otherwise.
// gain_out receives each block's gain from the thread that owns the block's first symbol.
struct QamFadeArgs {
    QamArgs q;
    FadeRows r;
    double mu, s;         // fading_coeff of K (drawn gains)
    float* gain_out;      // [B][n_blk], or nullptr
    int64_t b_offset;
    const uint32_t* seq;  // [n_seq][Wc] (SCR)
    int64_t n_seq, Wc;
};

__device__ __forceinline__ U4 fading_counter(uint64_t c, uint64_t seed) {
    return philox4x32_10(U4{(uint32_t)c, (uint32_t)(c >> 32), kFadeTag, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
}

template <int H, int METHOD, bool SCR>
__global__ __launch_bounds__(kQamThreads) void qam_fading_kernel(QamFadeArgs s) {
    constexpr int QM = 2 * H;
    const QamArgs& a = s.q;
    const QamPair p = qam_pair(a);
    if (!p.own0 && !p.own1) return;
    const U4 c = philox4x32_10(U4{(uint32_t)p.g, (uint32_t)(p.g >> 32), kQamTag, 0u}, (uint32_t)a.seed,
                               (uint32_t)(a.seed >> 32));
    const double rad0 = sqrt(-2.0 * log(u01(c.x))), th0 = 6.283185307179586 * u01(c.y);
    const double rad1 = sqrt(-2.0 * log(u01(c.z))), th1 = 6.283185307179586 * u01(c.w);
    const double n[4] = {rad0 * cos(th0), rad0 * sin(th0), rad1 * cos(th1), rad1 * sin(th1)};
    // the odd symbol (loc + 1 >= 0 always; one past the batch when it is not owned) and the even one in front of it
    // (row -1 when it is not owned)
    const FadeIdx i1 = fading_index(p.loc + 1, s.r.S, s.r.L), i0 = fading_prev(i1, s.r.S, s.r.L, s.r.n_blk);
    float g[2] = {0.f, 0.f};
    if (s.r.gain) {
        if (p.own0) g[0] = s.r.gain[fading_entry(i0, s.r.n_blk)];
        if (p.own1) g[1] = s.r.gain[fading_entry(i1, s.r.n_blk)];
    } else {
        // (b_offset + b >= 0 for an owned symbol; an unowned one's gain is computed from a counter of no meaning and
        // never used)
        const uint64_t G1 = fading_global(s.b_offset, i1, s.r.n_blk);
        const bool same = i0.b == i1.b && i0.k == i1.k;  // else G0 = G1 - 1
        const U4 d = fading_counter(G1 >> 1, a.seed);
        g[1] = (G1 & 1) ? fading_gain_of(s.mu, s.s, d.z, d.w) : fading_gain_of(s.mu, s.s, d.x, d.y);
        if (same) {
            g[0] = g[1];
        } else if (G1 & 1) {
            g[0] = fading_gain_of(s.mu, s.s, d.x, d.y);
        } else if (p.own0) {  // (G1 >= 1 here)
            const U4 e = fading_counter((G1 - 1) >> 1, a.seed);
            g[0] = fading_gain_of(s.mu, s.s, e.z, e.w);
        }
    }
    if (s.gain_out) {
        if (p.own0 && fading_first(i0, s.r.L)) s.gain_out[fading_entry(i0, s.r.n_blk)] = g[0];
        if (p.own1 && fading_first(i1, s.r.L)) s.gain_out[fading_entry(i1, s.r.n_blk)] = g[1];
    }
    uint32_t m[2] = {0u, 0u};
    if constexpr (SCR) {
        // row b uses sequence (b_offset + b) mod n_seq (b_offset + b < 2^32, n_seq < 2^31)
        if (p.own0) {
            const uint32_t q = s.n_seq == 1 ? 0u : (uint32_t)(s.b_offset + i0.b) % (uint32_t)s.n_seq;
            m[0] = gold_bits(s.seq + (int64_t)q * s.Wc, (int64_t)i0.j * QM, QM);
        }
        if (p.own1) {
            const uint32_t q = s.n_seq == 1 ? 0u : (uint32_t)(s.b_offset + i1.b) % (uint32_t)s.n_seq;
            m[1] = gold_bits(s.seq + (int64_t)q * s.Wc, (int64_t)i1.j * QM, QM);
        }
    }
    uint32_t w[H];
    qam_load_bits<H>(a.f, p, w);
    float l[4], r[4];
    qam_map_pair_scr<H>(w, 0, m[0], l[0], l[1]);
    qam_map_pair_scr<H>(w, 1, m[1], l[2], l[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float gl = g[q >> 1] * l[q];  // one fp32 rounding: the level the demapper expects for these bits
        r[q] = (float)((double)gl + a.sigma * n[q]);
    }
    float lvl[1 << H], lv[1 << H], v[2 * QM];
    qam_levels<H>(lvl);
    fading_levels<H>(g[0], lvl, lv);
    qam_demap_symbol<H, METHOD>(lv, r[0], r[1], a.w, v);
    fading_levels<H>(g[1], lvl, lv);
    qam_demap_symbol<H, METHOD>(lv, r[2], r[3], a.w, v + QM);
    if constexpr (SCR) {
#pragma unroll
        for (int i = 0; i < 2 * QM; ++i)
            v[i] = __uint_as_float(__float_as_uint(v[i]) ^ (((m[i / QM] >> (i % QM)) & 1u) << 31));
    }
    qam_store_pair<QM>(a.llr, p, v, qam_stage<H>());
    if (a.sym) qam_store_pair<2>(a.sym, p, r, nullptr);
}

typedef void (*QamKernel)(QamArgs);
typedef void (*QamScrKernel)(QamScrArgs);
typedef void (*QamCsiKernel)(QamCsiArgs);
typedef void (*QamFadeKernel)(QamFadeArgs);
static const QamCsiKernel kDemapCsi[4][2] = {{qam_demap_csi_kernel<1, 0>, qam_demap_csi_kernel<1, 1>},
                                             {qam_demap_csi_kernel<2, 0>, qam_demap_csi_kernel<2, 1>},
                                             {qam_demap_csi_kernel<3, 0>, qam_demap_csi_kernel<3, 1>},
                                             {qam_demap_csi_kernel<4, 0>, qam_demap_csi_kernel<4, 1>}};
#define NLDPC_FADE_ROW(H) \
    {{qam_fading_kernel<H, 0, false>, qam_fading_kernel<H, 0, true>}, {qam_fading_kernel<H, 1, false>, qam_fading_kernel<H, 1, true>}}
static const QamFadeKernel kFading[4][2][2] = {NLDPC_FADE_ROW(1), NLDPC_FADE_ROW(2), NLDPC_FADE_ROW(3), NLDPC_FADE_ROW(4)};
#undef NLDPC_FADE_ROW
static const QamScrKernel kChannelScr[4][2] = {{qam_channel_scr_kernel<1, 0>, qam_channel_scr_kernel<1, 1>},
                                               {qam_channel_scr_kernel<2, 0>, qam_channel_scr_kernel<2, 1>},
                                               {qam_channel_scr_kernel<3, 0>, qam_channel_scr_kernel<3, 1>},
                                               {qam_channel_scr_kernel<4, 0>, qam_channel_scr_kernel<4, 1>}};
static const QamKernel kModulate[4] = {qam_modulate_kernel<1>, qam_modulate_kernel<2>, qam_modulate_kernel<3>,
                                       qam_modulate_kernel<4>};
static const QamKernel kDemap[4][2] = {{qam_demap_kernel<1, 0>, qam_demap_kernel<1, 1>},
                                       {qam_demap_kernel<2, 0>, qam_demap_kernel<2, 1>},
                                       {qam_demap_kernel<3, 0>, qam_demap_kernel<3, 1>},
                                       {qam_demap_kernel<4, 0>, qam_demap_kernel<4, 1>}};
static const QamKernel kChannel[4][2] = {{qam_channel_kernel<1, 0>, qam_channel_kernel<1, 1>},
                                         {qam_channel_kernel<2, 0>, qam_channel_kernel<2, 1>},
                                         {qam_channel_kernel<3, 0>, qam_channel_kernel<3, 1>},
                                         {qam_channel_kernel<4, 0>, qam_channel_kernel<4, 1>}};

template <int H, int METHOD>
static void qam_demap_host(float w, const float* sym, int64_t S, float* llr) {
    float lvl[1 << H];
    qam_levels<H>(lvl);
    for (int64_t s = 0; s < S; ++s) qam_demap_symbol<H, METHOD>(lvl, sym[2 * s], sym[2 * s + 1], w, llr + s * 2 * H);
}
typedef void (*QamHostDemap)(float, const float*, int64_t, float*);
static const QamHostDemap kDemapHost[4][2] = {{qam_demap_host<1, 0>, qam_demap_host<1, 1>},
                                              {qam_demap_host<2, 0>, qam_demap_host<2, 1>},
                                              {qam_demap_host<3, 0>, qam_demap_host<3, 1>},
                                              {qam_demap_host<4, 0>, qam_demap_host<4, 1>}};

template <int H, int METHOD>
static void qam_demap_csi_host(float w, const float* sym, const float* gain, int64_t B, int64_t S, int32_t L,
                               int32_t n_blk, float* llr) {
    float lvl[1 << H], lv[1 << H];
    qam_levels<H>(lvl);
    for (int64_t loc = 0; loc < B * S; ++loc) {
        fading_levels<H>(gain[fading_entry(fading_index(loc, S, L), n_blk)], lvl, lv);
        qam_demap_symbol<H, METHOD>(lv, sym[2 * loc], sym[2 * loc + 1], w, llr + loc * 2 * H);
    }
}
typedef void (*QamHostDemapCsi)(float, const float*, const float*, int64_t, int64_t, int32_t, int32_t, float*);
static const QamHostDemapCsi kDemapCsiHost[4][2] = {{qam_demap_csi_host<1, 0>, qam_demap_csi_host<1, 1>},
                                                    {qam_demap_csi_host<2, 0>, qam_demap_csi_host<2, 1>},
                                                    {qam_demap_csi_host<3, 0>, qam_demap_csi_host<3, 1>},
                                                    {qam_demap_csi_host<4, 0>, qam_demap_csi_host<4, 1>}};

static float qam_weight(float sigma) { return (float)(1.0 / (2.0 * (double)sigma * (double)sigma)); }

// one thread per pair of the symbols [first, first + total); a = the kernel's argument, q its QamArgs
template <class Kernel, class Args>
static int qam_launch(const char* who, Kernel k, const Args& a, const QamArgs& q, void* stream) {
    const int64_t pairs = ((q.first + q.total + 1) >> 1) - (q.first >> 1);
    const int64_t blocks = (pairs + kQamThreads - 1) / kQamThreads;
    if (blocks > 0x7FFFFFFF) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kQamThreads), 0, static_cast<hipStream_t>(stream), a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NLDPC_OK : hip_fail(e, who);
}

static bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
}  // namespace nldpc

using namespace nldpc;

extern "C" int nldpc_qam_points(int32_t qm, float* iq) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, "nldpc_qam_points: qm is 2, 4, 6 or 8");
    if (!iq) return fail(NLDPC_EINVAL, "nldpc_qam_points: iq is NULL");
    for (uint32_t v = 0; v < (1u << qm); ++v) {
        uint32_t ci, cq;
        qam_labels(qm / 2, [&](int i) { return ((v >> (qm - 1 - i)) & 1u) != 0; }, ci, cq);
        iq[2 * v] = qam_level(qm / 2, ci);
        iq[2 * v + 1] = qam_level(qm / 2, cq);
    }
    return NLDPC_OK;
}

extern "C" int nldpc_qam_demap_ref(int32_t qm, int32_t method, float sigma, const float* sym, int64_t S, float* llr) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, "nldpc_qam_demap_ref: qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, "nldpc_qam_demap_ref: method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, "nldpc_qam_demap_ref: sigma must be positive");
    if (!sym || !llr || S <= 0) return fail(NLDPC_EINVAL, "nldpc_qam_demap_ref: bad argument");
    kDemapHost[qm / 2 - 1][method](qam_weight(sigma), sym, S, llr);
    return NLDPC_OK;
}

extern "C" int nldpc_qam_modulate(int32_t qm, const uint8_t* f, int64_t B, int64_t E, float* sym, void* stream) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, "nldpc_qam_modulate: qm is 2, 4, 6 or 8");
    if (!f || !sym || B <= 0 || E <= 0) return fail(NLDPC_EINVAL, "nldpc_qam_modulate: bad argument");
    if (E >= (int64_t)1 << 31 || E % qm != 0) return fail(NLDPC_EINVAL, "nldpc_qam_modulate: E must be below 2^31 and a multiple of qm");
    if (misaligned4(sym)) return fail(NLDPC_EINVAL, "nldpc_qam_modulate: sym must be 4-byte aligned");
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, "nldpc_qam_modulate: too large");
    QamArgs a{};
    a.f = f;
    a.sym = sym;
    a.total = B * (E / qm);
    return qam_launch("nldpc_qam_modulate", kModulate[qm / 2 - 1], a, a, stream);
}

extern "C" int nldpc_qam_demap(int32_t qm, int32_t method, float sigma, const float* sym, int64_t B, int64_t S,
                               float* llr, void* stream) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, "nldpc_qam_demap: qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, "nldpc_qam_demap: method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, "nldpc_qam_demap: sigma must be positive");
    if (!sym || !llr || B <= 0 || S <= 0) return fail(NLDPC_EINVAL, "nldpc_qam_demap: bad argument");
    if (S * qm >= (int64_t)1 << 31 || S >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, "nldpc_qam_demap: S * qm must be below 2^31");
    if (misaligned4(sym) || misaligned4(llr)) return fail(NLDPC_EINVAL, "nldpc_qam_demap: sym and llr must be 4-byte aligned");
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, "nldpc_qam_demap: too large");
    QamArgs a{};
    a.in = sym;
    a.llr = llr;
    a.total = B * S;
    a.w = qam_weight(sigma);
    return qam_launch("nldpc_qam_demap", kDemap[qm / 2 - 1][method], a, a, stream);
}

// the argument rules of the two fused channels, and their QamArgs
static int qam_channel_args(const std::string& who, int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E,
                            float sigma, uint64_t seed, int64_t b_offset, float* llr, float* sym_out, QamArgs& a) {
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, who + ": qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, who + ": method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, who + ": sigma must be positive");
    if (!llr || B <= 0 || E <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, who + ": bad argument");
    if (E >= (int64_t)1 << 31 || E % qm != 0) return fail(NLDPC_EINVAL, who + ": E must be below 2^31 and a multiple of qm");
    if (misaligned4(llr) || misaligned4(sym_out)) return fail(NLDPC_EINVAL, who + ": llr and sym_out must be 4-byte aligned");
    if (B >= (int64_t)1 << 31 || b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, who + ": too large");
    const int64_t S = E / qm;
    a.f = f;
    a.llr = llr;
    a.sym = sym_out;
    a.first = b_offset * S;
    a.total = B * S;
    a.sigma = (double)sigma;
    a.w = qam_weight(sigma);
    a.seed = seed;
    return NLDPC_OK;
}

extern "C" int nldpc_qam_channel_llr(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E, float sigma,
                                     uint64_t seed, int64_t b_offset, float* llr, float* sym_out, void* stream) {
    QamArgs a{};
    if (int rc = qam_channel_args("nldpc_qam_channel_llr", qm, method, f, B, E, sigma, seed, b_offset, llr, sym_out, a))
        return rc;
    return qam_launch("nldpc_qam_channel_llr", kChannel[qm / 2 - 1][method], a, a, stream);
}

extern "C" int nldpc_qam_channel_llr_scrambled(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E,
                                               float sigma, uint64_t seed, int64_t b_offset, const uint32_t* seq,
                                               int64_t n_seq, float* llr, float* sym_out, void* stream) {
    const char* who = "nldpc_qam_channel_llr_scrambled";
    QamScrArgs s{};
    if (int rc = qam_channel_args(who, qm, method, f, B, E, sigma, seed, b_offset, llr, sym_out, s.q)) return rc;
    if (!seq || misaligned4(seq)) return fail(NLDPC_EINVAL, std::string(who) + ": seq must be non-NULL and 4-byte aligned");
    if (n_seq < 1) return fail(NLDPC_EINVAL, std::string(who) + ": n_seq must be positive");
    s.seq = seq;
    s.n_seq = n_seq;
    s.Wc = (E + 31) >> 5;
    if (n_seq >= (int64_t)1 << 31 || n_seq * s.Wc >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    s.S = E / qm;
    s.b_offset = b_offset;
    return qam_launch(who, kChannelScr[qm / 2 - 1][method], s, s.q, stream);
}

// ---------------------------------------------------------------- flat block fading with perfect CSI
// the rules of L for rows of S symbols (0 < S < 2^31), and the rows' description: L >= S is one block per row
static int fade_rows(const std::string& who, int64_t B, int64_t S, int64_t L, FadeRows& r) {
    if (L < 1) return fail(NLDPC_EINVAL, who + ": L must be at least 1");
    r.S = S;
    r.L = (int32_t)(L < S ? L : S);
    const int64_t n_blk = fading_blocks(S, L);
    if (B * n_blk >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, who + ": B * ceil(S / L) must be below 2^31");
    r.n_blk = (int32_t)n_blk;
    return NLDPC_OK;
}

extern "C" int nldpc_fading_gain_ref(double K, const uint32_t* words, int64_t n, float* g) {
    if (!fading_k_ok(K)) return fail(NLDPC_EINVAL, "nldpc_fading_gain_ref: K must be finite and not negative");
    if (!words || !g || n <= 0) return fail(NLDPC_EINVAL, "nldpc_fading_gain_ref: bad argument");
    for (int64_t i = 0; i < n; ++i) g[i] = fading_gain(K, words[2 * i], words[2 * i + 1]);
    return NLDPC_OK;
}

extern "C" int nldpc_qam_demap_csi_ref(int32_t qm, int32_t method, float sigma, const float* sym, const float* gain,
                                       int64_t B, int64_t S, int64_t L, float* llr) {
    const char* who = "nldpc_qam_demap_csi_ref";
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, std::string(who) + ": qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, std::string(who) + ": method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, std::string(who) + ": sigma must be positive");
    if (!sym || !gain || !llr || B <= 0 || S <= 0) return fail(NLDPC_EINVAL, std::string(who) + ": bad argument");
    if (S * qm >= (int64_t)1 << 31 || S >= (int64_t)1 << 31 || B >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, std::string(who) + ": B and S * qm must be below 2^31");
    FadeRows r{};
    if (int rc = fade_rows(who, B, S, L, r)) return rc;
    kDemapCsiHost[qm / 2 - 1][method](qam_weight(sigma), sym, gain, B, S, r.L, r.n_blk, llr);
    return NLDPC_OK;
}

extern "C" int nldpc_fading_gains(double K, uint64_t seed, int64_t B, int64_t n_blk, int64_t b_offset, float* g,
                                  void* stream) {
    const char* who = "nldpc_fading_gains";
    if (!fading_k_ok(K)) return fail(NLDPC_EINVAL, std::string(who) + ": K must be finite and not negative");
    if (!g || B <= 0 || n_blk <= 0 || b_offset < 0) return fail(NLDPC_EINVAL, std::string(who) + ": bad argument");
    if (misaligned4(g)) return fail(NLDPC_EINVAL, std::string(who) + ": g must be 4-byte aligned");
    if (n_blk >= (int64_t)1 << 31 || B >= (int64_t)1 << 31 || B * n_blk >= (int64_t)1 << 31)
        return fail(NLDPC_EINVAL, std::string(who) + ": B * n_blk must be below 2^31");
    if (b_offset >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    FadeGainArgs a{};
    a.q.first = b_offset * n_blk;
    a.q.total = B * n_blk;
    a.q.seed = seed;
    fading_coeff(K, a.mu, a.s);
    a.g = g;
    return qam_launch(who, fading_gains_kernel, a, a.q, stream);
}

extern "C" int nldpc_qam_demap_csi(int32_t qm, int32_t method, float sigma, const float* sym, const float* gain,
                                   int64_t B, int64_t S, int64_t L, float* llr, void* stream) {
    const char* who = "nldpc_qam_demap_csi";
    if (!qam_order_ok(qm)) return fail(NLDPC_EINVAL, std::string(who) + ": qm is 2, 4, 6 or 8");
    if (method != 0 && method != 1) return fail(NLDPC_EINVAL, std::string(who) + ": method is 0 (max-log) or 1 (log-MAP)");
    if (!(sigma > 0.f)) return fail(NLDPC_EINVAL, std::string(who) + ": sigma must be positive");
    if (!sym || !gain || !llr || B <= 0 || S <= 0) return fail(NLDPC_EINVAL, std::string(who) + ": bad argument");
    if (S * qm >= (int64_t)1 << 31 || S >= (int64_t)1 << 31) return fail(NLDPC_EINVAL, std::string(who) + ": S * qm must be below 2^31");
    if (misaligned4(sym) || misaligned4(gain) || misaligned4(llr))
        return fail(NLDPC_EINVAL, std::string(who) + ": sym, gain and llr must be 4-byte aligned");
    if (B >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    QamCsiArgs s{};
    if (int rc = fade_rows(who, B, S, L, s.r)) return rc;
    s.r.gain = gain;
    s.q.in = sym;
    s.q.llr = llr;
    s.q.total = B * S;
    s.q.w = qam_weight(sigma);
    return qam_launch(who, kDemapCsi[qm / 2 - 1][method], s, s.q, stream);
}

extern "C" int nldpc_qam_fading_channel_llr(int32_t qm, int32_t method, const uint8_t* f, int64_t B, int64_t E,
                                            float sigma, uint64_t seed, int64_t b_offset, int64_t L, double K,
                                            const float* gain_in, const uint32_t* seq, int64_t n_seq, float* llr,
                                            float* sym_out, float* gain_out, void* stream) {
    const char* who = "nldpc_qam_fading_channel_llr";
    QamFadeArgs s{};
    if (int rc = qam_channel_args(who, qm, method, f, B, E, sigma, seed, b_offset, llr, sym_out, s.q)) return rc;
    if (!fading_k_ok(K)) return fail(NLDPC_EINVAL, std::string(who) + ": K must be finite and not negative");
    if (misaligned4(gain_in) || misaligned4(gain_out))
        return fail(NLDPC_EINVAL, std::string(who) + ": gain_in and gain_out must be 4-byte aligned");
    if (int rc = fade_rows(who, B, E / qm, L, s.r)) return rc;
    s.r.gain = gain_in;
    fading_coeff(K, s.mu, s.s);
    s.gain_out = gain_out;
    s.b_offset = b_offset;
    if (seq) {
        if (misaligned4(seq)) return fail(NLDPC_EINVAL, std::string(who) + ": seq must be 4-byte aligned");
        if (n_seq < 1) return fail(NLDPC_EINVAL, std::string(who) + ": n_seq must be positive");
        s.seq = seq;
        s.n_seq = n_seq;
        s.Wc = (E + 31) >> 5;
        if (n_seq >= (int64_t)1 << 31 || n_seq * s.Wc >= (int64_t)1 << 31) return fail(NLDPC_EUNSUPPORTED, std::string(who) + ": too large");
    }
    return qam_launch(who, kFading[qm / 2 - 1][method][seq ? 1 : 0], s, s.q, stream);
}
