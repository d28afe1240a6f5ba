// wave_bits.h -- two wave-level helpers of the bit-mask kernels (bubble_kernels.hip, cluster_kernels.hip)
#ifndef C21_WAVE_BITS_H
#define C21_WAVE_BITS_H

#include <hip/hip_runtime.h>

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int wave_inclusive(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}

// the position of the j-th set bit of x (0 <= j < popcount(x))
__device__ __forceinline__ int select_bit(unsigned long long x, int j) {
    int pos = 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long lo = x & ((1ull << s) - 1ull);
        const int c = __popcll(lo);
        if (j >= c) {
            j -= c;
            x >>= s;
            pos += s;
        } else {
            x = lo;
        }
    }
    return pos;
}

#endif
