// rsd_kernels.hip -- redshift-space distortions along the line of sight (reference:
// src/py21cmfast/rsds.py:184-255 rsds_shift, with cosmotile.cic.cloud_in_cell_los as the reference's
// tests/test_rsds.py:113-172 pin it down: linear cloud-in-cell on the fine grid, periodic or lossy).
//
// Layout: columns float[n_cols][n] (the line of sight is the fastest axis).  Per column, with
// m = n_sub and N = n m fine cells:
//   D_j      = los_velocity_j * disp_scale[j]                      (pixels, node at j + 0.5)
//   Dt_k     = m * linear interpolation of D at (k + 0.5) / m       (fp64; periodic: ghost nodes at
//              -0.5 = D_{n-1} and n + 0.5 = D_0; else the end intervals extrapolate)
//   fine k   carries field_{k / m} / m to x = k + Dt_k: (1 - w) to cell floor(x), w to the next
//              (modulo N when periodic; else lost outside [0, N))
//   coarse j = sum of fine cells j m .. j m + m - 1.
// A fine cell's deposit goes straight to its coarse bin: the coarse sum of integers is the same
// whatever order the fine cells arrive in.  The accumulators are 64-bit fixed point in LDS with a
// power-of-two scale per (column, field), 2^61 / (2^ceil(log2 n) max|field|), so every partial sum
// of a column fits and two runs give the same bits.  A thread owns one coarse slice at a time,
// walks its m fine cells and adds runs that land in one bin in registers before one LDS atomic.
// HBM: 4 B of velocity + 8 B (load, store) per field and cell; the rest is LDS traffic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 8;
constexpr int kMaxCols = 16;  // columns per workgroup when columns are short
constexpr int kMaxF = C21HIP_RSD_MAX_FIELDS;

struct RsdFields {
    const float *in[kMaxF];
    float *out[kMaxF];
};

// 2^61 / (2^ceil(log2 n) * 2^e), max|field| = f 2^e with f in [0.5, 1): no partial sum of the column
// (at most sum |field| <= n max|field|) reaches 2^61
__device__ inline double fixed_scale(unsigned max_bits, int n) {
    const float mx = __uint_as_float(max_bits);
    if (!(mx > 0.0f)) return 1.0;
    int e_mx, e_n;
    (void)frexp((double)mx, &e_mx);
    (void)frexp((double)(n - 1) + 0.5, &e_n);  // 2^(e_n - 1) <= n - 0.5 < 2^e_n: 2^e_n >= n
    return ldexp(1.0, 61 - e_n - e_mx);
}

// F: the field capacity the registers are sized for (nf <= F); 1, 4 or 16
template <int F>
__global__ void __launch_bounds__(kBlock)
rsd_shift_kernel(RsdFields f, int nf, const float *__restrict__ vel, const double *__restrict__ disp_scale,
                 size_t n_cols, int n, int m, int periodic, int cpb, int *__restrict__ bad) {
    extern __shared__ unsigned long long acc[];  // [cpb][nf][n]
    __shared__ unsigned smax[kMaxCols * kMaxF];  // max|field| of (column, field) as fp32 bits
    const int N = n * m;
    const int span = cpb * n;
    for (size_t c0 = (size_t)blockIdx.x * cpb; c0 < n_cols; c0 += (size_t)gridDim.x * cpb) {
        for (int i = threadIdx.x; i < span * nf; i += kBlock) acc[i] = 0ull;
        for (int i = threadIdx.x; i < cpb * nf; i += kBlock) smax[i] = 0u;
        __syncthreads();

        // pass 1: max|field| per (column, field), and the non-finite check
        {
            float mx[F];
#pragma unroll
            for (int q = 0; q < F; ++q) mx[q] = 0.0f;
            int cur = -1, flag = 0;
            for (int t = threadIdx.x; t < span; t += kBlock) {
                const int c = t / n;
                const size_t col = c0 + (size_t)c;
                if (col >= n_cols) break;
                if (c != cur) {
                    if (cur >= 0) {
#pragma unroll
                        for (int q = 0; q < F; ++q)
                            if (q < nf) atomicMax(&smax[cur * nf + q], __float_as_uint(mx[q]));
                    }
#pragma unroll
                    for (int q = 0; q < F; ++q) mx[q] = 0.0f;
                    cur = c;
                }
                const size_t at = col * (size_t)n + (size_t)(t - c * n);
                if (!isfinite(vel[at])) flag = 1;
#pragma unroll
                for (int q = 0; q < F; ++q) {
                    if (q < nf) {
                        const float a = fabsf(f.in[q][at]);
                        if (a <= 3.402823466e38f) mx[q] = fmaxf(mx[q], a);
                        else flag = 1;  // inf or NaN
                    }
                }
            }
            if (cur >= 0) {
#pragma unroll
                for (int q = 0; q < F; ++q)
                    if (q < nf) atomicMax(&smax[cur * nf + q], __float_as_uint(mx[q]));
            }
            if (flag) atomicOr(bad, 1);
        }
        __syncthreads();

        // pass 2: the deposit
        for (int t = threadIdx.x; t < span; t += kBlock) {
            const int c = t / n;
            const size_t col = c0 + (size_t)c;
            if (col >= n_cols) break;
            const int j = t - c * n;
            const size_t base = col * (size_t)n;
            const float *v = vel + base;
            // the nodes the fine cells of slice j interpolate between: j - 1, j, j + 1
            const int jm = j > 0 ? j - 1 : (periodic ? n - 1 : 0);
            const int jp = j < n - 1 ? j + 1 : (periodic ? 0 : n - 1);
            double Dm = (double)v[jm] * disp_scale[jm];
            double D0 = (double)v[j] * disp_scale[j];
            double Dp = (double)v[jp] * disp_scale[jp];
            if (!isfinite(Dm)) Dm = 0.0;
            if (!isfinite(D0)) D0 = 0.0;
            if (!isfinite(Dp)) Dp = 0.0;
            unsigned long long *a_col = acc + (size_t)c * nf * n;
            double val[F], sc[F];
            long long run[F];
#pragma unroll
            for (int q = 0; q < F; ++q) {
                val[q] = 0.0;
                sc[q] = 1.0;
                run[q] = 0;
                if (q < nf) {
                    const float a = f.in[q][base + j];
                    val[q] = fabsf(a) <= 3.402823466e38f ? (double)a / (double)m : 0.0;
                    sc[q] = fixed_scale(smax[c * nf + q], n);
                }
            }
            int cur_bin = -1;
            auto flush = [&]() {
                if (cur_bin >= 0) {
#pragma unroll
                    for (int q = 0; q < F; ++q)
                        if (q < nf && run[q]) atomicAdd(&a_col[q * n + cur_bin], (unsigned long long)run[q]);
                }
#pragma unroll
                for (int q = 0; q < F; ++q) run[q] = 0;
            };
            for (int s = 0; s < m; ++s) {
                const int k = j * m + s;
                // the fine displacement, interpolated between nodes j0 and j0 + 1 (positions j0 + 0.5)
                const double tpos = ((double)k + 0.5) / (double)m - 0.5;
                int j0 = (int)floor(tpos);
                if (!periodic) j0 = j0 < 0 ? 0 : (j0 > n - 2 ? n - 2 : j0);
                const double fr = tpos - (double)j0;
                double Da, Db;
                if (j0 < j) Da = Dm, Db = D0;
                else if (j0 == j) Da = D0, Db = Dp;
                else Da = Dp, Db = Dp;  // unreachable: j0 <= j for every fine cell of slice j
                const double Dt = (Da * (1.0 - fr) + Db * fr) * (double)m;
                double x = (double)k + Dt;
                // target fine cells i (weight 1 - w) and i + 1 (weight w); -1: lost
                int i_lo = -1, i_hi = -1;
                double w = 0.0;
                if (periodic) {
                    if (!(fabs(x) < 0x1p40)) {
                        x = fmod(x, (double)N);
                        if (x < 0.0) x += (double)N;
                    }
                    const double fl = floor(x);
                    w = x - fl;
                    double r = fl - (double)N * floor(fl / (double)N);
                    if (r < 0.0) r += (double)N;
                    if (r >= (double)N) r -= (double)N;
                    i_lo = (int)r;
                    i_hi = i_lo + 1 == N ? 0 : i_lo + 1;
                } else if (x >= -1.0 && x < (double)N) {
                    const double fl = floor(x);
                    w = x - fl;
                    i_lo = (int)fl;  // -1 .. N - 1
                    i_hi = i_lo + 1 < N ? i_lo + 1 : -1;
                }
                const int b_lo = i_lo >= 0 ? (int)((unsigned)i_lo / (unsigned)m) : -1;
                const int b_hi = i_hi >= 0 ? (int)((unsigned)i_hi / (unsigned)m) : -1;
                // (1 - w) part to b_lo, the rest of the fine cell's quantised value to b_hi
                if (b_lo != cur_bin) {
                    flush();
                    cur_bin = b_lo;
                }
                long long rest[F];
#pragma unroll
                for (int q = 0; q < F; ++q) {
                    rest[q] = 0;
                    if (q < nf) {
                        const long long tot = (long long)rint(val[q] * sc[q]);
                        const long long lo = (long long)rint(val[q] * (1.0 - w) * sc[q]);
                        run[q] += lo;
                        rest[q] = tot - lo;
                    }
                }
                if (b_hi != cur_bin) {
                    flush();
                    cur_bin = b_hi;
                }
#pragma unroll
                for (int q = 0; q < F; ++q) run[q] += rest[q];
            }
            flush();
        }
        __syncthreads();

        // the coarse columns, written once
        for (int t = threadIdx.x; t < span; t += kBlock) {
            const int c = t / n;
            const size_t col = c0 + (size_t)c;
            if (col >= n_cols) break;
            const int j = t - c * n;
#pragma unroll
            for (int q = 0; q < F; ++q) {
                if (q < nf) {
                    const double inv = 1.0 / fixed_scale(smax[c * nf + q], n);  // a power of two: exact
                    const long long s = (long long)acc[((size_t)c * nf + q) * n + j];
                    f.out[q][col * (size_t)n + j] = (float)((double)s * inv);
                }
            }
        }
        __syncthreads();
    }
}
}  // namespace

// LDS bytes of one workgroup for `nf` fields of columns of n slices (cpb columns per workgroup)
extern "C" size_t c21hip_rsd_lds_bytes(int n, int nf, int *cpb_out) {
    int cpb = n >= kBlock ? 1 : kBlock / n;
    if (cpb > kMaxCols) cpb = kMaxCols;
    if (cpb_out) *cpb_out = cpb;
    return (size_t)cpb * (size_t)nf * (size_t)n * sizeof(unsigned long long);
}

extern "C" int c21hip_rsd_shift(const float *const *in, float *const *out, int nf, const float *vel,
                                const double *disp_scale, size_t n_cols, int n, int m, int periodic,
                                int *bad, void *stream) {
    if (nf < 1 || nf > kMaxF || n < 2 || m < 1 || (long long)n * m > 0x7FFFFFFFll) {
        c21hip_set_error("rsd shift: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    int cpb = 1;
    const size_t lds = c21hip_rsd_lds_bytes(n, nf, &cpb);
    if (lds > C21HIP_RSD_MAX_LDS) {
        c21hip_set_error("rsd shift: %zu bytes of accumulators do not fit the LDS", lds);
        return C21CM_VALUE_ERROR;
    }
    if (n_cols == 0) return 0;
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)rsd_shift_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  C21HIP_RSD_MAX_LDS);
        (void)hipFuncSetAttribute((const void *)rsd_shift_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  C21HIP_RSD_MAX_LDS);
        (void)hipFuncSetAttribute((const void *)rsd_shift_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  C21HIP_RSD_MAX_LDS);
        attr_done = true;
    }
    RsdFields f{};
    for (int q = 0; q < nf; ++q) {
        f.in[q] = in[q];
        f.out[q] = out[q];
    }
    size_t groups = (n_cols + (size_t)cpb - 1) / (size_t)cpb;
    const int blocks = (int)(groups < (size_t)kMaxBlocks ? groups : (size_t)kMaxBlocks);
    if (nf == 1)
        hipLaunchKernelGGL(rsd_shift_kernel<1>, dim3(blocks), dim3(kBlock), lds, (hipStream_t)stream, f, nf,
                           vel, disp_scale, n_cols, n, m, periodic, cpb, bad);
    else if (nf <= 4)
        hipLaunchKernelGGL(rsd_shift_kernel<4>, dim3(blocks), dim3(kBlock), lds, (hipStream_t)stream, f, nf,
                           vel, disp_scale, n_cols, n, m, periodic, cpb, bad);
    else
        hipLaunchKernelGGL(rsd_shift_kernel<16>, dim3(blocks), dim3(kBlock), lds, (hipStream_t)stream, f, nf,
                           vel, disp_scale, n_cols, n, m, periodic, cpb, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        return C21CM_IO_ERROR;
    }
    return 0;
}
