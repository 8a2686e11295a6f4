// chx_philox.h — the counter-based generator of the kicks that draw inside their kernels (chx_sr.hip, chx_ibs.hip): Philox4x32-10
// (Salmon, Moraes, Dror, Shaw, SC'11) with the standard multipliers and Weyl constants, and the conversion of its four words into
// one standard normal deviate. A kick chooses its own counter layout; nothing of a draw is stored.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// u = ((the 64-bit word >> 11) + 1/2) 2^-53 for both halves, xi = sqrt(-2 ln u1) cospi(2 u2)
__device__ __forceinline__ double philox_normal_of(const uint32_t (&w)[4]) {
    const uint64_t k1 = (((uint64_t)w[0] << 32) | w[1]) >> 11, k2 = (((uint64_t)w[2] << 32) | w[3]) >> 11;
    const double u1 = ((double)k1 + 0.5) * 0x1p-53, u2 = ((double)k2 + 0.5) * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

}  // namespace
