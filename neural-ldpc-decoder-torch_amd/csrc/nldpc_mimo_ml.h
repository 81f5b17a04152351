// Exact max-log ML (joint) soft detection of one resource element (include/nldpc.h, F14) as inline functions shared by
// the host (nldpc_mimo_detect_ml_ref) and the kernels of nldpc_mimo.hip, built on nldpc_mimo.h and nldpc_qam.h.
//
//   LLR(b) = (min_{x: b = 0} d(x) - min_{x: b = 1} d(x)) / n0,  d(x) = sum_r |y_r - sum_t h(r,t) x_t|^2,
// over all 2^(qm nt) symbol vectors, without enumerating them: a pass enumerates the symbols of all layers but one (the
// sliced layer s), whose best symbol given the others is the constellation point nearest to z = h_s^H r / |h_s|^2,
// r = y - sum_{t != s} h_t x_t, found by slicing Re z and Im z independently.  The pass gives the exact minima for every
// bit of every enumerated layer.  Two passes serve any nt >= 2: s = nt - 1 for the layers 0 .. nt - 2, then s = 0 for
// layer nt - 1; nt = 1 enumerates its 2^qm points and slices nothing.
//
// A bit's minimum factors through per-label minima: per enumerated layer minI[c] is the minimum over every candidate
// whose I label is c, minQ likewise; a bit is finished from them as qam_demap_dim finishes from its d[c].  The innermost
// enumerated layer's Q loop is unrolled, so its minima are updated at compile-time indices; the outer loops run at run
// time and update theirs once per iteration through a chain of selects whose indices are compile-time constants again
// (a run-time index would put the arrays in scratch).  Minima are exact, so the order of the candidates does not show in
// the result; every other operation is fp32, one rounding each, no FMA, in the order written here.
#pragma once

#include "nldpc_mimo.h"

namespace nldpc {

// nt = 4 at 64- and 256-QAM is 2 * 64^3 and 2 * 256^3 candidates per resource element: a tree search, not built
NLDPC_MIMO_HD bool mimo_ml_supported(int qm, int nt) { return nt < 4 || qm <= 4; }

// K = 1 / (2 A) = sqrt(2 (4^h - 1) / 3) / 2 evaluated in double (the 17-digit literals), rounded to fp32 once
NLDPC_MIMO_HD float mimo_ml_step(int qm) {
    return qm == 2   ? (float)0.70710678118654752
           : qm == 4 ? (float)1.5811388300841897
           : qm == 6 ? (float)3.2403703492039302
                     : (float)6.5192024052026492;
}

// the level nearest to z: u = fl(fl(z K) + 2^(h-1)), j = floor(u) clamped to 0 .. 2^h - 1 (a NaN gives 0), level
// fl((2 j - (2^h - 1)) A); the integer steps are exact, so the level is qam_level of the label with that amplitude
template <int H>
NLDPC_MIMO_HD float mimo_ml_slice(float z) {
    constexpr float half = (float)(1 << (H - 1)), top = (float)((1 << H) - 1);
    const float u = z * mimo_ml_step(2 * H) + half;
    float j = floorf(u);
    j = j > 0.f ? j : 0.f;
    j = j < top ? j : top;
    return (2.f * j - top) * qam_scale(2 * H);
}

// 1 / |h_S|^2 of the sliced layer: g = sum_r |h(r,S)|^2, r ascending; q = fl(1 / g) when g > 0 and q is finite, else 0
template <int NT, int NR, int S>
NLDPC_MIMO_HD float mimo_ml_inv(const float* h) {
    float g = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float a = h[2 * (r * NT + S)], b = h[2 * (r * NT + S) + 1];
        const float p = a * a + b * b;
        g = r ? g + p : p;
    }
    const float q = 1.f / g;
    return g > 0.f && q <= 3.402823466e38f ? q : 0.f;
}

// the metric of one candidate from the residual res [NR][2] of its enumerated symbols.  S >= 0: z = (sum_r conj(h(r,S))
// res(r)) inv (each component), x^ = (slice Re z, slice Im z), e(r) = res(r) - h(r,S) x^; S < 0 (nt = 1): e = res.
// The metric is sum_r |e(r)|^2, r ascending: that of a true candidate whichever point the slice picked
template <int H, int NT, int NR, int S>
NLDPC_MIMO_HD float mimo_ml_metric(const float* h, float inv, const float* res) {
    float e[2 * NR];
    if constexpr (S >= 0) {
        float zr = 0.f, zi = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float a = h[2 * (r * NT + S)], b = h[2 * (r * NT + S) + 1], c = res[2 * r], d = res[2 * r + 1];
            const float pr = a * c + b * d, pi = a * d - b * c;
            zr = r ? zr + pr : pr;
            zi = r ? zi + pi : pi;
        }
        const float xr = mimo_ml_slice<H>(zr * inv), xi = mimo_ml_slice<H>(zi * inv);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float a = h[2 * (r * NT + S)], b = h[2 * (r * NT + S) + 1];
            e[2 * r] = res[2 * r] - (a * xr - b * xi);
            e[2 * r + 1] = res[2 * r + 1] - (a * xi + b * xr);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2 * NR; ++i) e[i] = res[i];
    }
    float m = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float p = e[2 * r] * e[2 * r] + e[2 * r + 1] * e[2 * r + 1];
        m = r ? m + p : p;
    }
    return m;
}

// res - h(., T) (li + i lq), each component
template <int NT, int NR, int T>
NLDPC_MIMO_HD void mimo_ml_residual(const float* h, const float* res, float li, float lq, float* out) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float a = h[2 * (r * NT + T)], b = h[2 * (r * NT + T) + 1];
        out[2 * r] = res[2 * r] - (a * li - b * lq);
        out[2 * r + 1] = res[2 * r + 1] - (a * lq + b * li);
    }
}

// m into mn[c] for the c that equals the run-time label at: every index is a compile-time constant
template <int LD>
NLDPC_MIMO_HD void mimo_ml_min_at(float* mn, uint32_t at, float m) {
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)LD; ++c) {
        const float v = m < mn[c] ? m : mn[c];
        mn[c] = at == c ? v : mn[c];
    }
}

// Layer T of the enumerated layers T .. END - 1 (ascending, so a residual is y minus the products in ascending layer
// order) with the sliced layer S: returns the minimum over every candidate below res and, for the layers >= TRACK, folds
// the metrics into mn[(layer - TRACK)][I = 0, Q = 1][label].  A NaN metric never becomes a minimum (m < best is false)
template <int H, int NT, int NR, int S, int T, int END, int TRACK>
NLDPC_MIMO_HD float mimo_ml_enum(const float* h, float inv, const float* lvl, const float* res, float* mn) {
    constexpr int LD = 1 << H;
    float* mI = mn + (T >= TRACK ? (T - TRACK) * 2 * LD : 0);  // (used when T >= TRACK only)
    float* mQ = mI + LD;
    float best = INFINITY;
#pragma unroll 1
    for (uint32_t ci = 0; ci < (uint32_t)LD; ++ci) {
        const float li = qam_level(H, ci);
        float mi = INFINITY, nx[2 * NR];
        if constexpr (T + 1 == END) {
#pragma unroll
            for (int cq = 0; cq < LD; ++cq) {
                mimo_ml_residual<NT, NR, T>(h, res, li, lvl[cq], nx);
                const float m = mimo_ml_metric<H, NT, NR, S>(h, inv, nx);
                if constexpr (T >= TRACK) mQ[cq] = m < mQ[cq] ? m : mQ[cq];
                mi = m < mi ? m : mi;
            }
        } else {
#pragma unroll 1
            for (uint32_t cq = 0; cq < (uint32_t)LD; ++cq) {
                mimo_ml_residual<NT, NR, T>(h, res, li, qam_level(H, cq), nx);
                const float m = mimo_ml_enum<H, NT, NR, S, T + 1, END, TRACK>(h, inv, lvl, nx, mn);
                if constexpr (T >= TRACK) mimo_ml_min_at<LD>(mQ, cq, m);
                mi = m < mi ? m : mi;
            }
        }
        if constexpr (T >= TRACK) mimo_ml_min_at<LD>(mI, ci, mi);
        best = mi < best ? mi : best;
    }
    return best;
}

// the qm LLRs of one layer from its per-label minima mn [I, Q][2^H], as qam_demap_dim's max-log finishes from d[c]
template <int H>
NLDPC_MIMO_HD void mimo_ml_finish(const float* mn, float w, float* llr) {
    constexpr int LD = 1 << H;
#pragma unroll
    for (int dim = 0; dim < 2; ++dim) {
#pragma unroll
        for (int k = 0; k < H; ++k) {
            float m0 = INFINITY, m1 = INFINITY;
#pragma unroll
            for (int c = 0; c < LD; ++c) {
                const float d = mn[dim * LD + c];
                if ((c >> (H - 1 - k)) & 1) m1 = d < m1 ? d : m1;
                else m0 = d < m0 ? d : m0;
            }
            llr[2 * k + dim] = (m0 - m1) * w;
        }
    }
}

// w = (float)(1 / (2 sigma^2)) in double from the fp32 sigma, as the QAM section's demapper takes it
NLDPC_MIMO_HD float mimo_ml_weight(float sigma) { return (float)(1.0 / (2.0 * ((double)sigma * (double)sigma))); }

// one resource element: h [NR][NT][2], y [NR][2] -> llr [NT * 2H]
template <int H, int NT, int NR>
NLDPC_MIMO_HD void mimo_ml_detect(const float* h, const float* y, float w, float* llr) {
    constexpr int LD = 1 << H, QM = 2 * H, TRK = NT > 1 ? NT - 1 : 1;
    float lvl[LD], mn[TRK * 2 * LD];
    qam_levels<H>(lvl);
#pragma unroll
    for (int i = 0; i < TRK * 2 * LD; ++i) mn[i] = INFINITY;
    if constexpr (NT == 1) {
        mimo_ml_enum<H, 1, NR, -1, 0, 1, 0>(h, 0.f, lvl, y, mn);
        mimo_ml_finish<H>(mn, w, llr);
    } else {
        mimo_ml_enum<H, NT, NR, NT - 1, 0, NT - 1, 0>(h, mimo_ml_inv<NT, NR, NT - 1>(h), lvl, y, mn);
#pragma unroll
        for (int k = 0; k < NT - 1; ++k) mimo_ml_finish<H>(mn + k * 2 * LD, w, llr + k * QM);
#pragma unroll
        for (int i = 0; i < 2 * LD; ++i) mn[i] = INFINITY;
        mimo_ml_enum<H, NT, NR, 0, 1, NT, NT - 1>(h, mimo_ml_inv<NT, NR, 0>(h), lvl, y, mn);
        mimo_ml_finish<H>(mn, w, llr + (NT - 1) * QM);
    }
}

}  // namespace nldpc
