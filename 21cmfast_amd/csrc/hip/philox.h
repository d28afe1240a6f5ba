// philox.h -- the counter-based generator shared by the kernels that draw random numbers
// (ics_kernels.hip: the modes of the initial conditions; halo_sampler_kernels.hip: every draw of the
// halo sampler).  Philox-4x32-10 (Salmon et al. 2011): 128-bit counter, 64-bit key, four 32-bit words.
#ifndef C21_PHILOX_H
#define C21_PHILOX_H

#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ void philox4x32_10_ctr(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                  uint64_t key, uint32_t (&out)[4]) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 64-bit counter in the low words, the high words zero
__device__ __forceinline__ void philox4x32_10(uint64_t counter, uint64_t key, uint32_t (&out)[4]) {
    philox4x32_10_ctr((uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u, key, out);
}

// two uniforms on (0, 1) with 53 random bits each out of one block of four words
__device__ __forceinline__ void philox_uniform_pair(const uint32_t (&x)[4], double *u1, double *u2) {
    *u1 = ((double)(((uint64_t)(x[0] >> 5) << 26) | (x[2] >> 6)) + 0.5) * 0x1p-53;
    *u2 = ((double)(((uint64_t)(x[1] >> 5) << 26) | (x[3] >> 6)) + 0.5) * 0x1p-53;
}

// Box-Muller in double on the pair of uniforms
__device__ __forceinline__ void philox_gaussian_pair(const uint32_t (&x)[4], double *a, double *b) {
    double u1, u2;
    philox_uniform_pair(x, &u1, &u2);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincos(2.0 * M_PI * u2, &s, &c);
    *a = r * c;
    *b = r * s;
}

#endif
