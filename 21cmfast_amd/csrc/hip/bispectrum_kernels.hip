// bispectrum_kernels.hip -- bispectra of boxes and lightcone chunks by the FFT estimator (the spec is
// tests/bispectrum_reference.py).  Around the transforms (fft.hip, rocFFT):
//   fill      one pass over the half spectrum complex[nx][ny][nz/2+1]: a mode goes into the padded box of its shell
//             in the stack [n_bins][nx ny][2(nz/2+1)] and a zero into every other box, so each stack element is
//             written exactly once (no memset, no scatter).  The shell is the power kernel's bin: |k|^2 = (kx^2 +
//             ky^2) + kz^2 in fp64 from the driver's tables (numpy's fftfreq(n, L/n) 2 pi; the Makefile compiles
//             without FMA contraction) against the |k|^2 thresholds of the edges, so a shell is exactly a get_power
//             bin.  The double form writes 1 + 0i: the shell indicators the triangle counts come from;
//   products  the hot path, after the batched inverse transform has turned the stack into the n_bins real boxes
//             delta_b(x).  One workgroup per (group, slab): a group is a pair (b1, b2) with 1 to 8 third shells, a
//             slab a run of whole rows.  Per cell p = (double)delta_b1 (double)delta_b2, exact for fp32 boxes, then
//             one fp64 FMA per third shell into 8 register accumulators; lanes strided over the slab's cells, a
//             shuffle tree over the wave, the waves summed in order through LDS: partials[slab][group][j].  The group
//             is the fast index of the work items and each XCD walks a contiguous run of them, so the workgroups in
//             flight on one L2 read the same slab of the stack (measured: every shell box leaves HBM once; DESIGN
//             4.11).  Only the first nz floats of a padded row are cells;
//   finish    S = the partials of a triangle summed over the slabs in a fixed order (strided per lane, then a tree),
//             B = scale S / (N n_tri), or n_tri = rint(S / N) in the indicator pass.
// No float atomics, and the slabs depend on the shape alone: two calls give the same bits, and a triangle's value
// does not depend on which other triangles were asked for (an accumulator never meets another one).
// Plain fp64 instructions only (no packed arithmetic: Makefile, -fno-slp-vectorize).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGroup = C21HIP_BISPEC_GROUP;
constexpr int kGroupInts = C21HIP_BISPEC_GROUP_INTS;
constexpr int kSlabCells = 8192;  // cells one products workgroup aims for (at most, but never less than a row)
constexpr int kMaxSlabs = 65535;  // of one box (rows per slab grow beyond it)

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

// one thread per mode m = (i ny + j) nh + l of the half spectrum; T2 = float2: the mode itself, double2: 1 + 0i
template <typename T2>
__global__ __launch_bounds__(kBlock) void bispec_fill_kernel(const float2 *__restrict__ spec, T2 *__restrict__ stack,
                                                             long long n_modes, int ny, int nh,
                                                             c21hip_bispec_tabs t) {
    __shared__ double thr[C21HIP_BISPEC_MAX_BINS + 1];
    const int nb = t.n_bins;
    if ((int)threadIdx.x <= nb) thr[threadIdx.x] = t.thr[threadIdx.x];
    __syncthreads();
    const long long m = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (m >= n_modes) return;
    const long long row = m / nh;
    const int l = (int)(m - row * nh);
    const int i = (int)(row / ny), j = (int)(row - (long long)i * ny);
    const double kx = t.kx[i], ky = t.ky[j], kz = t.kz[l];
    const double x = (kx * kx + ky * ky) + kz * kz;
    // np.digitize (increasing thresholds): the number of thresholds <= x, less one
    int lo = 0, hi = nb + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    const int bin = lo - 1;  // -1 below the first edge, nb at or above the last: in no shell
    if constexpr (sizeof(T2) == sizeof(float2)) {
        const float2 a = spec[m];
        for (int s = 0; s < nb; ++s)
            stack[(long long)s * n_modes + m] = make_float2(s == bin ? a.x : 0.0f, s == bin ? a.y : 0.0f);
    } else {
        for (int s = 0; s < nb; ++s) stack[(long long)s * n_modes + m] = make_double2(s == bin ? 1.0 : 0.0, 0.0);
    }
}

// the cells of one slab for a group of CNT third shells: lanes strided over the cells, CNT loads beside the pair's two
template <typename T, int CNT>
__device__ __forceinline__ void products_cells(const T *__restrict__ p1, const T *__restrict__ p2, const T *const *p3,
                                      int n_el, int nz, int row_len, double *acc) {
    // cell e = threadIdx.x, + kBlock, ..: (row, l) stepped along, one division per thread
    const int step_r = kBlock / nz, step_l = kBlock - step_r * nz;
    int rl = (int)threadIdx.x / nz, l = (int)threadIdx.x - rl * nz;
    for (int e = threadIdx.x; e < n_el; e += kBlock) {
        const int off = rl * row_len + l;
        const double p = (double)p1[off] * (double)p2[off];
#pragma unroll
        for (int j = 0; j < CNT; ++j) acc[j] = fma(p, (double)p3[j][off], acc[j]);
        rl += step_r;
        l += step_l;
        if (l >= nz) {
            l -= nz;
            ++rl;
        }
    }
}

// One workgroup per item w = slab n_groups + group.  Workgroups are dealt to the 8 XCDs in turn, each with an L2 of
// its own, so workgroup `orig` takes item w(orig) such that the workgroups of one XCD walk a contiguous run of items:
// the groups of a slab, which read the same cells, then meet in one L2.  The map is a bijection for any grid size
// and moves speed only: the partials are indexed by (slab, group).  plane: elements of one padded box; row_len =
// 2(nz/2+1).  The number of third shells of the group picks the loop (uniform over the workgroup), so no box is read
// for an unused place
template <typename T>
__global__ __launch_bounds__(kBlock) void bispec_products_kernel(const T *__restrict__ stack, long long plane, int nz,
                                                                 int row_len, int n_rows, int rows_per_slab,
                                                                 const int *__restrict__ groups, int n_groups,
                                                                 double *__restrict__ partials) {
    __shared__ double red[kWaves][kGroup];
    const unsigned nwg = gridDim.x, orig = blockIdx.x;
    const unsigned q = nwg / 8, r = nwg % 8, xcd = orig % 8;
    const unsigned w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
    const int slab = (int)(w / (unsigned)n_groups), g = (int)(w - (unsigned)slab * (unsigned)n_groups);
    const int n_slots = n_groups * kGroup;
    const int *gr = groups + (long long)g * kGroupInts;
    const int r0 = slab * rows_per_slab;
    const int nr = min(rows_per_slab, n_rows - r0);
    const int n_el = nr * nz;
    const long long base = (long long)r0 * row_len;
    const T *p1 = stack + (long long)gr[0] * plane + base;
    const T *p2 = stack + (long long)gr[1] * plane + base;
    const int cnt = gr[2];
    const T *p3[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) p3[j] = stack + (long long)gr[3 + j] * plane + base;
    double acc[kGroup];
#pragma unroll
    for (int j = 0; j < kGroup; ++j) acc[j] = 0.0;
    static_assert(kGroup == 8, "one case per count below");
    switch (cnt) {
        case 1: products_cells<T, 1>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 2: products_cells<T, 2>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 3: products_cells<T, 3>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 4: products_cells<T, 4>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 5: products_cells<T, 5>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 6: products_cells<T, 6>(p1, p2, p3, n_el, nz, row_len, acc); break;
        case 7: products_cells<T, 7>(p1, p2, p3, n_el, nz, row_len, acc); break;
        default: products_cells<T, 8>(p1, p2, p3, n_el, nz, row_len, acc); break;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
        double s = acc[j];
        for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < kGroup) {
        double s = red[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) s += red[w][threadIdx.x];
        partials[(long long)slab * n_slots + (long long)g * kGroup + threadIdx.x] = s;
    }
}

// one wave per (batch, triangle): lane q sums slabs q, q + 64, .. in order, then a fixed tree
__global__ __launch_bounds__(64) void bispec_finish_kernel(const double *__restrict__ partials, int n_slabs,
                                                           int n_slots, const int *__restrict__ slot, int n_tri,
                                                           double scale, double n_cells,
                                                           const long long *__restrict__ counts_in,
                                                           double *__restrict__ out_b,
                                                           long long *__restrict__ counts_out) {
    const int tri = blockIdx.x;
    const long long b = blockIdx.y;
    const double *src = partials + b * (long long)n_slabs * n_slots + slot[tri];
    double s = 0.0;
    for (int q = threadIdx.x; q < n_slabs; q += 64) s += src[(long long)q * n_slots];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (threadIdx.x != 0) return;
    if (counts_in) {
        const long long c = counts_in[tri];
        out_b[b * n_tri + tri] = c > 0 ? scale * s / (n_cells * (double)c) : __builtin_nan("");
    } else {
        counts_out[tri] = llrint(s / n_cells);
    }
}
}  // namespace

extern "C" int c21hip_bispec_slabs(int nx, int ny, int nz, int *rows_per_slab) {
    const long long n_rows = (long long)nx * ny;
    long long rps = kSlabCells / nz;
    if (rps < 1) rps = 1;
    if ((n_rows + rps - 1) / rps > kMaxSlabs) rps = (n_rows + kMaxSlabs - 1) / kMaxSlabs;
    if (rows_per_slab) *rows_per_slab = (int)rps;
    return (int)((n_rows + rps - 1) / rps);
}

extern "C" int c21hip_bispec_fill(const float *spec, void *stack, int as_double, int nx, int ny, int nz,
                                  const c21hip_bispec_tabs *t, void *stream) {
    if (nx < 2 || ny < 2 || nz < 2 || t->n_bins < 1 || t->n_bins > C21HIP_BISPEC_MAX_BINS || !stack ||
        (!as_double && !spec)) {
        c21hip_set_error("bispectrum fill: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const int nh = nz / 2 + 1;
    const long long n_modes = (long long)nx * ny * nh;
    const long long blocks = (n_modes + kBlock - 1) / kBlock;
    if (blocks > 0x7FFFFFFFll) {
        c21hip_set_error("bispectrum fill: the box is too large for one launch");
        return C21CM_VALUE_ERROR;
    }
    if (as_double)
        hipLaunchKernelGGL(bispec_fill_kernel<double2>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream,
                           (const float2 *)spec, (double2 *)stack, n_modes, ny, nh, *t);
    else
        hipLaunchKernelGGL(bispec_fill_kernel<float2>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream,
                           (const float2 *)spec, (float2 *)stack, n_modes, ny, nh, *t);
    return launch_status("bispectrum fill");
}

extern "C" int c21hip_bispec_products(const void *stack, int as_double, int nx, int ny, int nz, const int *groups,
                                      int n_groups, double *partials, void *stream) {
    // a slab's cells and padded floats are indexed with ints
    if (nx < 2 || ny < 2 || nz < 2 || n_groups < 1 || !stack || !groups || !partials ||
        (long long)nx * ny > 0x7FFFFFFFll || (long long)n_groups * C21HIP_BISPEC_GROUP > 0x7FFFFFFFll) {
        c21hip_set_error("bispectrum products: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    int rps = 0;
    const int n_slabs = c21hip_bispec_slabs(nx, ny, nz, &rps);
    const int row_len = 2 * (nz / 2 + 1);
    if ((long long)rps * row_len > 0x7FFFFFFFll) {
        c21hip_set_error("bispectrum products: a slab of %d rows of %d cells is too large", rps, nz);
        return C21CM_VALUE_ERROR;
    }
    if ((long long)n_groups * n_slabs > 0x7FFFFFFFll) {
        c21hip_set_error("bispectrum products: %d groups of triangles on %d slabs are too many for one launch", n_groups,
                         n_slabs);
        return C21CM_VALUE_ERROR;
    }
    const long long plane = (long long)nx * ny * row_len;
    const dim3 grid((unsigned)n_groups * (unsigned)n_slabs);
    if (as_double)
        hipLaunchKernelGGL(bispec_products_kernel<double>, grid, dim3(kBlock), 0, (hipStream_t)stream,
                           (const double *)stack, plane, nz, row_len, nx * ny, rps, groups, n_groups, partials);
    else
        hipLaunchKernelGGL(bispec_products_kernel<float>, grid, dim3(kBlock), 0, (hipStream_t)stream,
                           (const float *)stack, plane, nz, row_len, nx * ny, rps, groups, n_groups, partials);
    return launch_status("bispectrum products");
}

extern "C" int c21hip_bispec_finish(const double *partials, int n_batch, int n_slabs, int n_slots, const int *slot,
                                    int n_tri, double scale, double n_cells, const long long *counts_in,
                                    double *out_b, long long *counts_out, void *stream) {
    if (n_batch < 1 || n_batch > 65535 || n_slabs < 1 || n_tri < 1 || !partials || !slot ||
        (counts_in ? !out_b : (!counts_out || n_batch != 1))) {
        c21hip_set_error("bispectrum finish: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    hipLaunchKernelGGL(bispec_finish_kernel, dim3((unsigned)n_tri, (unsigned)n_batch), dim3(64), 0,
                       (hipStream_t)stream, partials, n_slabs, n_slots, slot, n_tri, scale, n_cells, counts_in, out_b,
                       counts_out);
    return launch_status("bispectrum finish");
}
