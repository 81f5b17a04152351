// Spatial multiplexing of one codeword over nt layers with a linear MMSE soft detector (include/nldpc.h, F13) as inline
// functions shared by the host (nldpc_mimo_entry_ref, nldpc_mimo_filter_ref, nldpc_mimo_detect_ref) and the kernels of
// nldpc_mimo.hip: the same functions index a resource element, draw a channel entry, build the filter, equalise and
// demap on both sides, so the arithmetic is testable without a device.
//
// A row of S symbols is R = S / nt resource elements (REs); RE i carries the nt consecutive symbols d(nt i + k), one
// per layer k, received on nr antennas as y = H x + sigma n.  REs are cut into n_blk = ceil(R / L) fading blocks of L
// consecutive REs of a row (the last may be short; blocks never span rows); block k of row b is global block
// Gf = (b_offset + b) * n_blk + k and has one channel matrix H, fp32 [nr][nt][2] (re, im).
//
// Every matrix loop below runs over the template parameters NT, NR with constant bounds and is fully unrolled: all
// indices are compile-time constants, so the matrices live in registers (a run-time index would put them in scratch).
// Complex products are four rounded products, one rounded difference and one rounded sum (no FMA: the library is built
// with -ffp-contract=off); a sum over an index starts from its first term and adds the others in ascending order.
#pragma once

#include <math.h>
#include <stdint.h>

#include "nldpc_fading.h"
#include "nldpc_qam.h"

#define NLDPC_MIMO_HD NLDPC_QAM_HD

namespace nldpc {

constexpr uint32_t kMimoNoiseTag = 0x4D494E31u;  // counter word 2 of the MIMO noise stream ("MIN1")
constexpr uint32_t kMimoChanTag = 0x4D494831u;   // counter word 2 of the channel-entry stream ("MIH1")

NLDPC_MIMO_HD bool mimo_dims_ok(int nt, int nr) {
    return (nt == 1 || nt == 2 || nt == 4) && (nr == 1 || nr == 2 || nr == 4) && nr >= nt;
}

// the position of (nt, nr) among the six pairs (1,1) (1,2) (1,4) (2,2) (2,4) (4,4)
NLDPC_MIMO_HD int mimo_dims_index(int nt, int nr) {
    return nt == 1 ? (nr == 1 ? 0 : nr == 2 ? 1 : 2) : nt == 2 ? (nr == 2 ? 3 : 4) : 5;
}

// s of a drawn entry: entries are CN(0, 1 / nt), so each real component has variance 1 / (2 nt)
NLDPC_MIMO_HD double mimo_entry_scale(int nt) { return sqrt(1.0 / (2.0 * (double)nt)); }

// one drawn entry from its two Philox words: everything in double, each component rounded to fp32 once
NLDPC_MIMO_HD void mimo_entry_of(double s, uint32_t r0, uint32_t r1, float& re, float& im) {
    const double rad = sqrt(-2.0 * log(fading_u01(r0))), th = 6.283185307179586 * fading_u01(r1);
    re = (float)(s * (rad * cos(th)));
    im = (float)(s * (rad * sin(th)));
}

// where a resource element lies: its row b, its index i in the row and its fading block k in the row (L <= R < 2^31)
struct MimoIdx {
    int64_t b;
    int32_t i, k;
};

// of the RE with batch-local index loc >= 0: one 64-bit and one 32-bit division
NLDPC_MIMO_HD MimoIdx mimo_index(int64_t loc, int64_t R, int32_t L) {
    MimoIdx x;
    x.b = loc / R;
    x.i = (int32_t)(loc - x.b * R);
    x.k = (int32_t)((uint32_t)x.i / (uint32_t)L);
    return x;
}

// true for the first RE of its fading block (the owner of the block's entry of h_out)
NLDPC_MIMO_HD bool mimo_first(const MimoIdx& x, int32_t L) { return x.i == x.k * L; }

// the block's position in a [B][n_blk] table, and its global index (b_offset + b >= 0)
NLDPC_MIMO_HD int64_t mimo_block(const MimoIdx& x, int32_t n_blk) { return x.b * n_blk + x.k; }
NLDPC_MIMO_HD uint64_t mimo_global(int64_t b_offset, const MimoIdx& x, int32_t n_blk) {
    return (uint64_t)(b_offset + x.b) * (uint64_t)n_blk + (uint64_t)x.k;
}

// s = H x in fp32: for each antenna r the products h(r, t) x(t), t ascending.  h is [NR][NT][2], x [NT][2], s [NR][2]
template <int NT, int NR>
NLDPC_MIMO_HD void mimo_apply(const float* h, const float* x, float* s) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float a = h[2 * (r * NT + t)], b = h[2 * (r * NT + t) + 1], c = x[2 * t], d = x[2 * t + 1];
            const float pr = a * c - b * d, pi = a * d + b * c;
            re = t ? re + pr : pr;
            im = t ? im + pi : pi;
        }
        s[2 * r] = re;
        s[2 * r + 1] = im;
    }
}

// The LMMSE filter of one block, in double from the fp32 table (sigma the fp32 the ABI takes).  With n0 = 2 sigma^2 and
// q = 1 / n0 the Cholesky factorisation is taken of Gn = G / n0 = I + (H^H H) q, so that e_k = n0 [G^-1]_kk = [Gn^-1]_kk
// needs no final product and a zero channel gives e_k = 1 and mu_k = 0 exactly:
//   A(j,k) = sum_r conj(h(r,j)) h(r,k), j >= k (the diagonal is real: sum_r (re re + im im));
//   Gn(j,k) = A(j,k) q (each component), Gn(k,k) = A(k,k) q + 1;
//   Gn = C C^H by columns j = 0 ..: d = Gn(j,j) - sum_{k<j} |C(j,k)|^2, C(j,j) = sqrt(d), c_j = 1 / C(j,j),
//        C(i,j) = (Gn(i,j) - sum_{k<j} C(i,k) conj(C(j,k))) c_j for i > j;
//   M = C^-1 (lower triangular): M(j,j) = c_j, M(i,j) = -(sum_{k=j}^{i-1} C(i,k) M(k,j)) c_i for i > j;
//   e_k = sum_{i>=k} |M(i,k)|^2, mu_k = 1 - e_k, p = mu_k e_k, w_k = 1 / p when p is positive and finite, else 0;
//   T = M H^H: T(i,r) = sum_{k<=i} M(i,k) conj(h(r,k));  W(k,r) = (sum_{i>=k} conj(M(i,k)) T(i,r)) q (each component).
// |z|^2 is re re + im im.  W [NT][NR][2], mu [NT] and w [NT] are each rounded to fp32 once.
template <int NT, int NR>
NLDPC_MIMO_HD void mimo_filter(const float* h, float sigma, float* W, float* mu, float* w) {
    const double n0 = 2.0 * ((double)sigma * (double)sigma), q = 1.0 / n0;
    double hr[NR * NT], hi[NR * NT];
#pragma unroll
    for (int e = 0; e < NR * NT; ++e) {
        hr[e] = (double)h[2 * e];
        hi[e] = (double)h[2 * e + 1];
    }
    // C, then M, in the lower triangle of one pair of arrays (entry (i, j) at i * NT + j)
    double cr[NT * NT], ci[NT * NT], inv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                // conj(h(r,j)) h(r,k)
                const double a = hr[r * NT + j], b = hi[r * NT + j], c = hr[r * NT + k], d = hi[r * NT + k];
                const double pr = a * c + b * d, pi = a * d - b * c;
                re = r ? re + pr : pr;
                im = r ? im + pi : pi;
            }
            cr[j * NT + k] = k == j ? re * q + 1.0 : re * q;
            ci[j * NT + k] = k == j ? 0.0 : im * q;
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        double d = cr[j * NT + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - (cr[j * NT + k] * cr[j * NT + k] + ci[j * NT + k] * ci[j * NT + k]);
        const double cj = sqrt(d);
        inv[j] = 1.0 / cj;
        cr[j * NT + j] = cj;
#pragma unroll
        for (int i = j + 1; i < NT; ++i) {
            double re = cr[i * NT + j], im = ci[i * NT + j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                // C(i,k) conj(C(j,k))
                const double a = cr[i * NT + k], b = ci[i * NT + k], c = cr[j * NT + k], dd = ci[j * NT + k];
                re = re - (a * c + b * dd);
                im = im - (b * c - a * dd);
            }
            cr[i * NT + j] = re * inv[j];
            ci[i * NT + j] = im * inv[j];
        }
    }
    double mr[NT * NT], mi[NT * NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        mr[j * NT + j] = inv[j];
        mi[j * NT + j] = 0.0;
#pragma unroll
        for (int i = j + 1; i < NT; ++i) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int k = j; k < i; ++k) {
                const double a = cr[i * NT + k], b = ci[i * NT + k], c = mr[k * NT + j], d = mi[k * NT + j];
                const double pr = a * c - b * d, pi = a * d + b * c;
                re = k > j ? re + pr : pr;
                im = k > j ? im + pi : pi;
            }
            mr[i * NT + j] = -re * inv[i];
            mi[i * NT + j] = -im * inv[i];
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        double e = mr[k * NT + k] * mr[k * NT + k];
#pragma unroll
        for (int i = k + 1; i < NT; ++i) e = e + (mr[i * NT + k] * mr[i * NT + k] + mi[i * NT + k] * mi[i * NT + k]);
        const double m = 1.0 - e, p = m * e;
        mu[k] = (float)m;
        w[k] = p > 0.0 && p <= 1.79769313486231570e308 ? (float)(1.0 / p) : 0.f;
    }
    double tr[NT * NR], ti[NT * NR];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int k = 0; k <= i; ++k) {
                // M(i,k) conj(h(r,k))
                const double a = mr[i * NT + k], b = mi[i * NT + k], c = hr[r * NT + k], d = hi[r * NT + k];
                const double pr = a * c + b * d, pi = b * c - a * d;
                re = k ? re + pr : pr;
                im = k ? im + pi : pi;
            }
            tr[i * NR + r] = re;
            ti[i * NR + r] = im;
        }
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double re = 0.0, im = 0.0;
#pragma unroll
            for (int i = k; i < NT; ++i) {
                // conj(M(i,k)) T(i,r)
                const double a = mr[i * NT + k], b = mi[i * NT + k], c = tr[i * NR + r], d = ti[i * NR + r];
                const double pr = a * c + b * d, pi = a * d - b * c;
                re = i > k ? re + pr : pr;
                im = i > k ? im + pi : pi;
            }
            W[2 * (k * NR + r)] = (float)(re * q);
            W[2 * (k * NR + r) + 1] = (float)(im * q);
        }
    }
}

// x^ = W y in fp32, r ascending.  W is [NT][NR][2], y [NR][2], xh [NT][2]
template <int NT, int NR>
NLDPC_MIMO_HD void mimo_equalise(const float* W, const float* y, float* xh) {
    mimo_apply<NR, NT>(W, y, xh);
}

// the LLRs of one RE from its equalised symbols: layer k on the levels fl32(mu_k * l) with weight w_k; llr [NT * 2H]
template <int H, int METHOD, int NT>
NLDPC_MIMO_HD void mimo_demap(const float* lvl, const float* xh, const float* mu, const float* w, float* llr) {
    float lv[1 << H];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        fading_levels<H>(mu[k], lvl, lv);
        qam_demap_symbol<H, METHOD>(lv, xh[2 * k], xh[2 * k + 1], w[k], llr + k * 2 * H);
    }
}

}  // namespace nldpc
