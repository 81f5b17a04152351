// Philox-4x32-10 (Salmon et al. 2011) and the fp64 Box-Muller transform the device channels draw their noise with
// (nldpc_aux.hip awgn_kernel and encode_kernel, nldpc_modulation.hip qam_channel_kernel).  Counter word 2 tells the
// streams of one seed apart: 0 the BPSK noise, 0x454E4331 the encoder's info bits, 0x51414D31 the QAM noise, 0x46414431
// the fading gains (nldpc_fading.h), 0x4D494E31 and 0x4D494831 the MIMO noise and channel entries (nldpc_mimo.h).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nldpc {

struct U4 {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

__device__ __forceinline__ double u01(uint32_t r) { return ((double)r + 1.0) * (1.0 / 4294967296.0); }

}  // namespace nldpc
