// Circular-buffer rate matching (3GPP TS 38.212 §5.4.2) as closed-form index maps, shared by the host
// (nldpc_rm_index) and the kernels of nldpc_ratematch.hip: the same inline functions compute the index on both sides,
// so the map is testable without a device.
//
// Buffer d[p] = y[P + p], p in [0, Ncb); filler positions [f0, f0 + F) are skipped, which leaves Nv = Ncb - F valid
// positions, numbered v in [0, Nv) in buffer order.  The spec's selection loop reads valid position (v0 + k) mod Nv for
// its k-th bit (v0: valid positions before k0), and its interleaver puts selected bit k = i * (E/Qm) + j at output
// m = i + j * Qm.  All arithmetic is 32-bit: E, N*Z < 2^31 (checked by rm_resolve in nldpc_ratematch.hip).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NLDPC_RM_HD __host__ __device__ __forceinline__
#else
#define NLDPC_RM_HD inline
#endif

namespace nldpc {

// Everything the maps need, resolved on the host once per call (the kernel argument).
struct RmMap {
    uint32_t E, Eq, Qm;        // bits sent, E / Qm, interleaver rows
    uint32_t P, Ncb, NZ;       // punctured head, buffer length, codeword length
    uint32_t f0, F, Nv, v0;    // filler range start and length, valid positions, valid positions before k0
    uint32_t step_i, step_j;   // the valid-position step (mod Nv) from output m to m + 1: inside an interleaver
                               // column (k += Eq) and from its last row to the next column's first (k -= (Qm-1)*Eq - 1)
    uint32_t inv_qm, inv_nv, inv_eq;  // rm_inv of Qm, Nv, Eq
};

// floor(2^32 / d), saturated for d == 1
inline uint32_t rm_inv(uint32_t d) { return d <= 1 ? 0xFFFFFFFFu : (uint32_t)(((uint64_t)1 << 32) / d); }

// x / d and x % d for any x < 2^32, d >= 1 and inv = rm_inv(d): the high product is the quotient or one below it
// (x * inv / 2^32 > x / d - 1), so one correction makes it exact -- no integer division instruction sequence
NLDPC_RM_HD void rm_divmod(uint32_t x, uint32_t d, uint32_t inv, uint32_t& q, uint32_t& r) {
    q = (uint32_t)(((uint64_t)x * inv) >> 32);
    r = x - q * d;
    if (r >= d) {
        ++q;
        r -= d;
    }
}

// The forward map as a cursor over consecutive outputs m: rm_seek places it, rm_bit reads the codeword bit index
// n = idx[m], rm_step moves to m + 1 (two adds and compares; no division after the seek).
struct RmCursor {
    uint32_t i;  // m mod Qm
    uint32_t v;  // valid position (v0 + k) mod Nv
};

NLDPC_RM_HD RmCursor rm_seek(const RmMap& a, uint32_t m) {
    uint32_t i = 0, j = m;
    if (a.Qm > 1) rm_divmod(m, a.Qm, a.inv_qm, j, i);
    const uint32_t k = i * a.Eq + j;  // < E
    uint32_t q, kv;
    rm_divmod(k, a.Nv, a.inv_nv, q, kv);
    uint32_t v = a.v0 + kv;  // v0, kv < Nv
    if (v >= a.Nv) v -= a.Nv;
    return RmCursor{i, v};
}

NLDPC_RM_HD uint32_t rm_bit(const RmMap& a, const RmCursor& c) { return a.P + (c.v < a.f0 ? c.v : c.v + a.F); }

NLDPC_RM_HD void rm_step(const RmMap& a, RmCursor& c) {
    uint32_t step = a.step_i;
    if (++c.i == a.Qm) {
        c.i = 0;
        step = a.step_j;
    }
    c.v += step;  // both below Nv < 2^31
    if (c.v >= a.Nv) c.v -= a.Nv;
}

// The inverse map.  Codeword bit n: RM_NONE when it is outside the buffer (n < P or p >= Ncb), RM_FILLER for a filler
// position, else its first selection index k0n = (v - v0) mod Nv in *k (received at all only if k0n < E; the further
// copies are at k0n + r * Nv).
enum { RM_SENT = 0, RM_NONE = 1, RM_FILLER = 2 };

NLDPC_RM_HD int rm_first(const RmMap& a, uint32_t n, uint32_t* k) {
    if (n < a.P) return RM_NONE;
    const uint32_t p = n - a.P;
    if (p >= a.Ncb) return RM_NONE;
    if (p >= a.f0 && p < a.f0 + a.F) return RM_FILLER;
    const uint32_t v = p < a.f0 ? p : p - a.F;
    *k = v >= a.v0 ? v - a.v0 : v + a.Nv - a.v0;
    return RM_SENT;
}

// selection index k -> output position m (the interleaver)
NLDPC_RM_HD uint32_t rm_out_pos(const RmMap& a, uint32_t k) {
    if (a.Qm == 1) return k;
    uint32_t i, j;
    rm_divmod(k, a.Eq, a.inv_eq, i, j);
    return j * a.Qm + i;
}

}  // namespace nldpc
