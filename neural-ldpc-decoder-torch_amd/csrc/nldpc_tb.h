// Transport-block arithmetic of 3GPP TS 38.212 (§5.2.2 code-block segmentation, §5.4.2.1 the E_r rule, the lifting-size
// choice) as inline functions shared by the host entries (nldpc_tb_plan, nldpc_tb_lifting_size, nldpc_tb_er,
// nldpc_tb_crc_ref) and the kernels of nldpc_tb.hip: the same functions run on both sides, so the arithmetic is testable
// without a device.
//
// A transport block of A payload bits carries a TB CRC of L_tb bits: B' = A + L_tb.  It is cut into C parts of
// K' - L bits; each part gets a CRC24B of L = 24 bits (L = 0 when C == 1) and F filler zeros, a row of W bits.
// B' = C (K' - L), so the TB's remainder under its polynomial is
//   R(TB) = xor_r R(part r) * x^{(C - 1 - r)(K' - L)} mod g_tb
// (nldpc_crc.h: R(u | v) = R(u) x^{|v|} xor R(v)), taken by Horner over r with tb_combine.
#pragma once

#include <stdint.h>

#include "nldpc.h"
#include "nldpc_crc.h"

namespace nldpc {

constexpr int64_t kTbLimit = (int64_t)1 << 31;  // every size is below it
constexpr int kTbCbCrc = 1;                     // NLDPC_CRC24B, the code-block CRC

// why a plan is refused
enum { TB_OK = 0, TB_EARG, TB_ERANGE, TB_EKCB_W, TB_EKCB_SMALL, TB_EDIV, TB_EKP_W };

// number and CRC length of the code blocks of B' bits under kcb (§5.2.2); kcb > 24 when B' > kcb
NLDPC_CRC_HD void tb_blocks(int64_t Bp, int64_t kcb, int64_t* C, int64_t* L) {
    if (Bp <= kcb) {
        *C = 1, *L = 0;
    } else {
        *L = 24;
        *C = (Bp + (kcb - 24) - 1) / (kcb - 24);
    }
}

NLDPC_CRC_HD int tb_plan(int64_t A, int32_t tb_crc, int64_t W, int64_t kcb, nldpc_tb* p) {
    if (!crc_ok(tb_crc) || A < 1 || W < 1 || kcb < 0) return TB_EARG;
    if (A >= kTbLimit || W >= kTbLimit || kcb >= kTbLimit) return TB_ERANGE;
    const int64_t Bp = A + crc_len(tb_crc);
    if (Bp >= kTbLimit) return TB_ERANGE;
    if (kcb == 0) kcb = W;
    if (kcb > W) return TB_EKCB_W;
    if (Bp > kcb && kcb <= 24) return TB_EKCB_SMALL;
    int64_t C, L;
    tb_blocks(Bp, kcb, &C, &L);
    const int64_t Bpp = Bp + C * L;  // C <= B' < 2^31
    if (Bpp >= kTbLimit) return TB_ERANGE;
    if (Bpp % C != 0) return TB_EDIV;
    const int64_t Kp = Bpp / C;
    if (Kp > W) return TB_EKP_W;
    p->A = A;
    p->tb_crc = tb_crc;
    p->W = W;
    p->C = (int32_t)C;
    p->L = (int32_t)L;
    p->Kp = Kp;
    p->F = W - Kp;
    return TB_OK;
}

// B' = C (K' - L) of a plan
NLDPC_CRC_HD int64_t tb_part(const nldpc_tb& p) { return p.Kp - p.L; }
NLDPC_CRC_HD int64_t tb_bits(const nldpc_tb& p) { return (int64_t)p.C * tb_part(p); }

// a plan the entries accept: the relations tb_plan establishes (C need not be the smallest count)
NLDPC_CRC_HD bool tb_plan_ok(const nldpc_tb& p) {
    if (!crc_ok(p.tb_crc) || p.A < 1 || p.C < 1 || p.L != (p.C > 1 ? 24 : 0)) return false;
    if (p.W < 1 || p.W >= kTbLimit || p.F < 0 || p.Kp <= p.L || p.Kp + p.F != p.W) return false;
    return p.A < kTbLimit && tb_bits(p) == p.A + crc_len(p.tb_crc) && tb_bits(p) + (int64_t)p.C * p.L < kTbLimit;
}

// Kb of §5.2.2 and the smallest lifting size of Table 5.3.2-1 (a * 2^j <= 384) with Kb * Z >= K', where
// K' = ceil(B'' / C) for the base graph's own Kcb (8448 / 3840).  False: bg is not 1 or 2, or no size is large enough.
NLDPC_CRC_HD bool tb_lifting_size(int32_t bg, int64_t Bp, int32_t* Kb, int32_t* Zc) {
    if ((bg != 1 && bg != 2) || Bp < 1 || Bp >= kTbLimit) return false;
    int64_t C, L;
    tb_blocks(Bp, bg == 1 ? 8448 : 3840, &C, &L);
    const int64_t Kp = (Bp + C * L + C - 1) / C;
    const int32_t kb = bg == 1 ? 22 : Bp > 640 ? 10 : Bp > 560 ? 9 : Bp > 192 ? 8 : 6;
    int32_t best = 0;
    for (int32_t a = 2; a <= 15; a += (a == 2 ? 1 : 2)) {
        for (int32_t z = a; z <= 384; z *= 2) {
            if ((int64_t)kb * z >= Kp) {
                if (best == 0 || z < best) best = z;
                break;
            }
        }
    }
    if (best == 0) return false;
    *Kb = kb;
    *Zc = best;
    return true;
}

// §5.4.2.1: with G' = G / (NL Qm), blocks j <= C - (G' mod C) - 1 get E_lo = NL Qm floor(G' / C), the rest
// E_hi = NL Qm ceil(G' / C); C_lo = C - (G' mod C) blocks get E_lo
NLDPC_CRC_HD bool tb_er(int64_t G, int32_t NL, int32_t Qm, int32_t C, int64_t* E_lo, int64_t* E_hi, int32_t* C_lo) {
    if (G < 1 || G >= kTbLimit || NL < 1 || Qm < 1 || C < 1) return false;
    const int64_t q = (int64_t)NL * Qm;
    if (G % q != 0) return false;
    const int64_t Gp = G / q, lo = Gp / C, rem = Gp % C;
    if (lo < 1) return false;
    *E_lo = q * lo;
    *E_hi = q * (lo + (rem ? 1 : 0));
    *C_lo = (int32_t)(C - rem);
    return true;
}

// one Horner step over the parts: R(u | part) from acc = R(u), part = R(the part), xP = x^{K' - L} mod g
NLDPC_CRC_HD uint32_t tb_combine(uint32_t acc, uint32_t part, uint32_t xP, uint32_t poly, int L) {
    return crc_mul(acc, xP, poly, L) ^ part;
}

}  // namespace nldpc
