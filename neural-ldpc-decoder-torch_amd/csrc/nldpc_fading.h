// Flat block fading with perfect channel state information for the QAM channel (include/nldpc.h, F12) as inline
// functions shared by the host (nldpc_fading_gain_ref, nldpc_qam_demap_csi_ref) and the kernels of
// nldpc_modulation.hip: the same functions compute a gain, a symbol's fading block and its scaled levels on both sides,
// so the arithmetic is testable without a device.
//
// A row of S symbols is cut into n_blk = ceil(S / L) fading blocks of L consecutive symbols (the last may be short);
// blocks never span rows.  Symbol j of row b lies in block k = j div L of its row, global block
// Gf = (b_offset + b) * n_blk + k.  Every symbol of a block passes through the same real gain g >= 0 (the channel's
// magnitude after the receiver's exact phase de-rotation): the level l arrives as fl32(g * l) plus noise, and the
// demapper of nldpc_qam.h runs unchanged on the 2^h levels fl32(g * lvl[c]).
//
// A drawn gain is Rician with factor K >= 0 (K = 0: Rayleigh, no special case), E[g^2] = 1: with (r0, r1) the block's
// two Philox words, the Box-Muller of the noise gives two unit normals a = rad cos(th), b = rad sin(th),
// rad = sqrt(-2 log u01(r0)), th = 2 pi u01(r1); mu = sqrt(K / (K + 1)), s = sqrt(1 / (2 (K + 1)));
// g = (float)sqrt((mu + s a)^2 + (s b)^2), everything in double (no FMA), rounded to fp32 once.
#pragma once

#include <math.h>
#include <stdint.h>

#include "nldpc_qam.h"

#define NLDPC_FADE_HD NLDPC_QAM_HD

namespace nldpc {

constexpr uint32_t kFadeTag = 0x46414431u;  // counter word 2 of the gain stream ("FAD1")

// (word + 1) / 2^32 in (0, 1]: u01 of nldpc_philox.h, for both sides
NLDPC_FADE_HD double fading_u01(uint32_t r) { return ((double)r + 1.0) * (1.0 / 4294967296.0); }

NLDPC_FADE_HD bool fading_k_ok(double K) { return K >= 0.0 && K <= 1.79769313486231570e308; }  // (false for a NaN)

// mu and s of K: the kernels take them from the host, so both sides scale with the same two doubles
NLDPC_FADE_HD void fading_coeff(double K, double& mu, double& s) {
    mu = sqrt(K / (K + 1.0));
    s = sqrt(1.0 / (2.0 * (K + 1.0)));
}

NLDPC_FADE_HD float fading_gain_of(double mu, double s, uint32_t r0, uint32_t r1) {
    const double rad = sqrt(-2.0 * log(fading_u01(r0))), th = 6.283185307179586 * fading_u01(r1);
    const double x = mu + s * (rad * cos(th)), y = s * (rad * sin(th));
    return (float)sqrt(x * x + y * y);
}

NLDPC_FADE_HD float fading_gain(double K, uint32_t r0, uint32_t r1) {
    double mu, s;
    fading_coeff(K, mu, s);
    return fading_gain_of(mu, s, r0, r1);
}

// the levels a symbol of gain g is demapped against: one fp32 multiply per level, shared by I and Q
template <int H>
NLDPC_FADE_HD void fading_levels(float g, const float* lvl, float* out) {
#pragma unroll
    for (int c = 0; c < (1 << H); ++c) out[c] = g * lvl[c];
}

NLDPC_FADE_HD int64_t fading_blocks(int64_t S, int64_t L) { return L >= S ? 1 : (S + L - 1) / L; }

// where a symbol lies: its row b, its index j in the row and its fading block k in the row (L <= S < 2^31)
struct FadeIdx {
    int64_t b;
    int32_t j, k;
};

// of the symbol with batch-local index loc >= 0: one 64-bit and one 32-bit division
NLDPC_FADE_HD FadeIdx fading_index(int64_t loc, int64_t S, int32_t L) {
    FadeIdx i;
    i.b = loc / S;
    i.j = (int32_t)(loc - i.b * S);
    i.k = (int32_t)((uint32_t)i.j / (uint32_t)L);
    return i;
}

// of the symbol in front of i (the last symbol of the row before when i starts a row; b = -1 in front of the batch)
NLDPC_FADE_HD FadeIdx fading_prev(const FadeIdx& i, int64_t S, int32_t L, int32_t n_blk) {
    FadeIdx p;
    if (i.j) {
        p.b = i.b;
        p.j = i.j - 1;
        p.k = i.j - i.k * L ? i.k : i.k - 1;
    } else {
        p.b = i.b - 1;
        p.j = (int32_t)(S - 1);
        p.k = n_blk - 1;
    }
    return p;
}

// true for the first symbol of its fading block (the owner of the block's entry of gain_out)
NLDPC_FADE_HD bool fading_first(const FadeIdx& i, int32_t L) { return i.j == i.k * L; }

// the entry of a [B][n_blk] gain table, and the global block index (b_offset + b >= 0)
NLDPC_FADE_HD int64_t fading_entry(const FadeIdx& i, int32_t n_blk) { return i.b * n_blk + i.k; }
NLDPC_FADE_HD uint64_t fading_global(int64_t b_offset, const FadeIdx& i, int32_t n_blk) {
    return (uint64_t)(b_offset + i.b) * (uint64_t)n_blk + (uint64_t)i.k;
}

}  // namespace nldpc
