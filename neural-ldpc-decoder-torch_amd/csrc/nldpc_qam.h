// Gray-mapped square QAM (3GPP TS 38.211 §5.1.3-5.1.6: QPSK, 16-, 64-, 256-QAM) and its soft demapper as inline
// functions shared by the host (nldpc_qam_points, nldpc_qam_demap_ref) and the kernels of nldpc_modulation.hip: the same
// functions compute a level and an LLR on both sides, so the arithmetic is testable without a device.
//
// A symbol carries qm = 2h consecutive bits b_0 .. b_{qm-1}; the I dimension takes c_k = b_{2k}, the Q dimension
// c_k = b_{2k+1}, k < h.  A dimension's h bits are handled as the label c = c_0 c_1 .. c_{h-1} (c_0 the most significant
// bit), its integer amplitude is a = (1-2c_0)[2^{h-1} - (1-2c_1)[2^{h-2} - .. - (1-2c_{h-1})]] (odd, |a| <= 2^h - 1) and
// its level (float)a * A, A = the fp32 nearest to 1/sqrt(2), 1/sqrt(10), 1/sqrt(42), 1/sqrt(170).
//
// Demapper, per dimension, received x: for every label c, t = x - level(c), d(c) = t * t (two fp32 roundings, no FMA:
// the library is built with -ffp-contract=off); w = (float)(1 / (2 sigma^2)), computed in double by the caller.
//   method 0 (max-log): LLR_k = (min_{c_k=0} d - min_{c_k=1} d) * w
//   method 1 (log-MAP): m(c) = -(d(c) * w); lse_v = M_v + logf(sum_{c_k=v} expf(m(c) - M_v)), M_v = max_{c_k=v} m(c), the
//                       sum taken in ascending label order from +0; LLR_k = lse_1 - lse_0
// LLR > 0 means bit 1 (the decoders' convention); 38.211 keeps bit 0 on the positive side, so a noiseless symbol gives
// negative LLRs for its 0 bits.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NLDPC_QAM_HD __host__ __device__ __forceinline__
#else
#define NLDPC_QAM_HD inline
#endif

namespace nldpc {

NLDPC_QAM_HD bool qam_order_ok(int qm) { return qm == 2 || qm == 4 || qm == 6 || qm == 8; }

// A: 1 / sqrt(2 (4^h - 1) / 3) evaluated in double (the 17-digit literals), rounded to fp32 once
NLDPC_QAM_HD float qam_scale(int qm) {
    return qm == 2   ? (float)0.70710678118654752
           : qm == 4 ? (float)0.31622776601683794
           : qm == 6 ? (float)0.15430334996209191
                     : (float)0.076696498884737041;
}

// the integer amplitude of label c (h bits, c_0 = bit h-1 of c)
NLDPC_QAM_HD int qam_amp(int h, uint32_t c) {
    int v = 1 - 2 * (int)(c & 1u);  // 1 - 2 c_{h-1}
    for (int k = h - 2; k >= 0; --k) {
        const int ck = (int)((c >> (h - 1 - k)) & 1u);
        v = (1 - 2 * ck) * ((1 << (h - 1 - k)) - v);
    }
    return v;
}

NLDPC_QAM_HD float qam_level(int h, uint32_t c) { return (float)qam_amp(h, c) * qam_scale(2 * h); }

// the two labels of a symbol's bits: b(i) is true when bit i is set, i < 2h
template <typename BitAt>
NLDPC_QAM_HD void qam_labels(int h, BitAt b, uint32_t& ci, uint32_t& cq) {
    ci = cq = 0;
    for (int k = 0; k < h; ++k) {
        ci = (ci << 1) | (b(2 * k) ? 1u : 0u);
        cq = (cq << 1) | (b(2 * k + 1) ? 1u : 0u);
    }
}

// every level of a dimension, by label
template <int H>
NLDPC_QAM_HD void qam_levels(float* lvl) {
#pragma unroll
    for (uint32_t c = 0; c < (1u << H); ++c) lvl[c] = qam_level(H, c);
}

// one dimension: out[k * stride] = LLR of c_k, k < H
template <int H, int METHOD>
NLDPC_QAM_HD void qam_demap_dim(const float* lvl, float x, float w, float* out, int stride) {
    constexpr int L = 1 << H;
    float d[L];
#pragma unroll
    for (int c = 0; c < L; ++c) {
        const float t = x - lvl[c];
        d[c] = t * t;
    }
    if (METHOD == 0) {
#pragma unroll
        for (int k = 0; k < H; ++k) {
            float m0 = INFINITY, m1 = INFINITY;
#pragma unroll
            for (int c = 0; c < L; ++c) {
                if ((c >> (H - 1 - k)) & 1) m1 = d[c] < m1 ? d[c] : m1;
                else m0 = d[c] < m0 ? d[c] : m0;
            }
            out[k * stride] = (m0 - m1) * w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < L; ++c) d[c] = -(d[c] * w);
#pragma unroll
        for (int k = 0; k < H; ++k) {
            float M0 = -INFINITY, M1 = -INFINITY;
#pragma unroll
            for (int c = 0; c < L; ++c) {
                if ((c >> (H - 1 - k)) & 1) M1 = d[c] > M1 ? d[c] : M1;
                else M0 = d[c] > M0 ? d[c] : M0;
            }
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int c = 0; c < L; ++c) {
                if ((c >> (H - 1 - k)) & 1) s1 = s1 + expf(d[c] - M1);
                else s0 = s0 + expf(d[c] - M0);
            }
            out[k * stride] = (M1 + logf(s1)) - (M0 + logf(s0));
        }
    }
}

// one symbol (xi, xq) -> llr[0 .. 2H) in the order of its bits
template <int H, int METHOD>
NLDPC_QAM_HD void qam_demap_symbol(const float* lvl, float xi, float xq, float w, float* llr) {
    qam_demap_dim<H, METHOD>(lvl, xi, w, llr, 2);
    qam_demap_dim<H, METHOD>(lvl, xq, w, llr + 1, 2);
}

}  // namespace nldpc
