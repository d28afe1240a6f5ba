// moments_kernels.hip -- one-point statistics of boxes and lightcone chunks: mean, central moments, histogram
// (host/moments_driver.c).  Two passes over the field, box b at in[offsets[b] + (i ny + j) row_pitch
// + l] as in power_kernels.hip:
//   pass 1  the mean, fp64 and kept in fp64: one wave per row (lanes strided, then a fixed shuffle tree), then the
//           row sums of a box in two levels, one workgroup per 4096 rows and one per box (thread t takes items t,
//           t + 256, .. in order, then a fixed tree).  Every value is checked for finiteness here;
//   pass 2  d = (double)v - mean: sum d^2, d^3, d^4 per row by the same scheme, then per box; no float atomics, so
//           two calls give the same bits.  The histogram bin is np.digitize((double)v, edges) - 1 (the number of
//           edges <= v, less one), kept when 0 <= bin < n_bins: half-open bins, a value on the last edge is dropped.
//           A workgroup counts a run of rows of one box in LDS (32-bit integer atomics) and adds its non-zero
//           counts to hist[b][bin] with 64-bit integer atomics: integer sums do not depend on their order.
// HBM: 4 B per cell and pass; the row sums are 8 B (pass 1) and 24 B (pass 2) per row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
// rows of one box a pass-2 workgroup takes when it keeps a histogram
constexpr int kRowsPerWgHist = 64;
// row sums one workgroup of the first level of a box's sum takes
constexpr int kChunk = 4096;

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

// rowsum[row] = the fp64 sum of row (b, i, j), lanes strided then a fixed shuffle tree: one wave per row
__global__ __launch_bounds__(kBlock) void moments_rowsum_kernel(const float *__restrict__ in,
                                                                double *__restrict__ rowsum,
                                                                long long rows_per_batch, long long n_rows, int nz,
                                                                long long row_pitch,
                                                                const long long *__restrict__ offsets, int *bad) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // the whole wave
    const long long b = row / rows_per_batch, r = row - b * rows_per_batch;
    const float *src = in + offsets[b] + r * row_pitch;
    double s = 0.0;
    int nonfinite = 0;
    for (int l = lane; l < nz; l += 64) {
        const float v = src[l];
        nonfinite |= !isfinite(v);
        s += (double)v;
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) rowsum[row] = s;
    if (nonfinite) atomicOr(bad, 1);
}

// out[b][v] = scale * the sum over the rows of box b of rowsum[v][b][.], v < NS: one workgroup per box, thread t
// sums rows t, t + 256, .. in order, then a fixed tree.  NS = 1: the mean (out stride 1); NS = 3: m2, m3, m4 behind
// the mean in moments[b][4]
template <int NS>
__global__ __launch_bounds__(kBlock) void moments_boxsum_kernel(const double *__restrict__ rowsum,
                                                                const double *__restrict__ mean,
                                                                double *__restrict__ out, long long rows_per_batch,
                                                                long long n_batch, double scale) {
    __shared__ double red[NS][kBlock];
    const long long b = blockIdx.x;
    double s[NS];
    for (int v = 0; v < NS; ++v) {
        const double *src = rowsum + ((long long)v * n_batch + b) * rows_per_batch;
        s[v] = 0.0;
        for (long long r = threadIdx.x; r < rows_per_batch; r += kBlock) s[v] += src[r];
        red[v][threadIdx.x] = s[v];
    }
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int v = 0; v < NS; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        __syncthreads();
    }
    if (NS == 1) {
        if (threadIdx.x == 0) out[b] = red[0][0] * scale;
    } else {
        if (threadIdx.x == 0) out[b * 4] = mean[b];
        if (threadIdx.x < NS) out[b * 4 + 1 + threadIdx.x] = red[threadIdx.x][0] * scale;
    }
}

// part[v][b][c] = the sum of rowsum[v][b][c kChunk .. (c + 1) kChunk), v < NS: workgroup (c, b), thread t sums
// rows t, t + 256, .. of the chunk in order, then a fixed tree.  One workgroup alone over the 2^18 row sums of a
// 512^3 box took 0.2 ms per array; the chunks bring that to a few microseconds, and the order stays fixed
template <int NS>
__global__ __launch_bounds__(kBlock) void moments_chunksum_kernel(const double *__restrict__ rowsum,
                                                                  double *__restrict__ part,
                                                                  long long rows_per_batch, long long n_chunks) {
    __shared__ double red[NS][kBlock];
    const long long c = blockIdx.x, b = blockIdx.y, n_batch = gridDim.y;
    const long long r0 = c * kChunk;
    long long r1 = r0 + kChunk;
    if (r1 > rows_per_batch) r1 = rows_per_batch;
    for (int v = 0; v < NS; ++v) {
        const double *src = rowsum + ((long long)v * n_batch + b) * rows_per_batch;
        double s = 0.0;
        for (long long r = r0 + threadIdx.x; r < r1; r += kBlock) s += src[r];
        red[v][threadIdx.x] = s;
    }
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int v = 0; v < NS; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < NS) part[((long long)threadIdx.x * n_batch + b) * n_chunks + c] = red[threadIdx.x][0];
}

// workgroup (w, b) takes rows [w rpw, (w + 1) rpw) of box b, wave q of it the rows q, q + 4, ..: the row's sums of
// d^2, d^3, d^4 into rowsum[0..2][b][row], and (HIST) the workgroup's counts into hist[b][.]
template <bool HIST>
__global__ __launch_bounds__(kBlock) void moments_central_kernel(const float *__restrict__ in,
                                                                 double *__restrict__ rowsum,
                                                                 long long rows_per_batch, int rpw, int nz,
                                                                 long long row_pitch,
                                                                 const long long *__restrict__ offsets,
                                                                 const double *__restrict__ mean, int n_bins,
                                                                 const double *__restrict__ edges_g,
                                                                 unsigned long long *__restrict__ hist) {
    extern __shared__ double lds[];
    double *edges = lds;                                 // n_bins + 1
    unsigned *cnt = (unsigned *)(lds + (n_bins + 1));    // n_bins
    if (HIST) {
        for (int q = threadIdx.x; q <= n_bins; q += kBlock) edges[q] = edges_g[q];
        for (int q = threadIdx.x; q < n_bins; q += kBlock) cnt[q] = 0u;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long b = blockIdx.y, n_batch = gridDim.y;
    const long long r0 = (long long)blockIdx.x * rpw;
    long long r1 = r0 + rpw;
    if (r1 > rows_per_batch) r1 = rows_per_batch;
    const double m = mean[b];
    for (long long r = r0 + wave; r < r1; r += kWaves) {
        const float *src = in + offsets[b] + r * row_pitch;
        double s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (int l = lane; l < nz; l += 64) {
            const double x = (double)src[l];
            const double d = x - m, d2 = d * d;
            s2 += d2;
            s3 += d2 * d;
            s4 += d2 * d2;
            if (HIST) {
                int lo = 0, hi = n_bins + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (edges[mid] <= x) lo = mid + 1;
                    else hi = mid;
                }
                const int bin = lo - 1;
                if (bin >= 0 && bin < n_bins) atomicAdd(&cnt[bin], 1u);
            }
        }
        for (int d = 32; d > 0; d >>= 1) {
            s2 += __shfl_down(s2, d, 64);
            s3 += __shfl_down(s3, d, 64);
            s4 += __shfl_down(s4, d, 64);
        }
        if (lane == 0) {
            rowsum[(0 * n_batch + b) * rows_per_batch + r] = s2;
            rowsum[(1 * n_batch + b) * rows_per_batch + r] = s3;
            rowsum[(2 * n_batch + b) * rows_per_batch + r] = s4;
        }
    }
    if (HIST) {
        __syncthreads();
        for (int q = threadIdx.x; q < n_bins; q += kBlock) {
            const unsigned c = cnt[q];
            if (c) atomicAdd(&hist[b * n_bins + q], (unsigned long long)c);
        }
    }
}
// out = scale * the sums over the rows of each box of rowsum[NS][n_batch][per]; boxes of more than one chunk of
// rows go through part[NS][n_batch][chunks] first
template <int NS>
void launch_boxsum(const double *rowsum, double *part, const double *mean, double *out, long long per, int n_batch,
                   double scale, hipStream_t s) {
    const long long chunks = (per + kChunk - 1) / kChunk;
    if (chunks > 1) {
        hipLaunchKernelGGL(moments_chunksum_kernel<NS>, dim3((unsigned)chunks, (unsigned)n_batch), dim3(kBlock), 0, s,
                           rowsum, part, per, chunks);
        hipLaunchKernelGGL(moments_boxsum_kernel<NS>, dim3((unsigned)n_batch), dim3(kBlock), 0, s, part, mean, out,
                           chunks, (long long)n_batch, scale);
    } else {
        hipLaunchKernelGGL(moments_boxsum_kernel<NS>, dim3((unsigned)n_batch), dim3(kBlock), 0, s, rowsum, mean, out,
                           per, (long long)n_batch, scale);
    }
}
}  // namespace

extern "C" size_t c21hip_moments_part_doubles(int nx, int ny, int n_batch) {
    const long long per = (long long)nx * ny;
    return 3 * (size_t)((per + kChunk - 1) / kChunk) * (size_t)n_batch;
}

extern "C" int c21hip_moments_mean(const float *in, int nx, int ny, int nz, long long row_pitch,
                                   const long long *offsets, int n_batch, double *rowsum, double *part, double *mean,
                                   int *bad, void *stream) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || n_batch > 65535 || row_pitch < nz) {
        c21hip_set_error("moments mean: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long per = (long long)nx * ny, rows = per * n_batch;
    const long long blocks = (rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(moments_rowsum_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, in, rowsum,
                       per, rows, nz, row_pitch, offsets, bad);
    launch_boxsum<1>(rowsum, part, nullptr, mean, per, n_batch, 1.0 / ((double)per * (double)nz), (hipStream_t)stream);
    return launch_status("moments mean");
}

extern "C" int c21hip_moments_central(const float *in, int nx, int ny, int nz, long long row_pitch,
                                      const long long *offsets, int n_batch, const double *mean, int n_bins,
                                      const double *edges, double *rowsum, double *part, double *moments,
                                      unsigned long long *hist, void *stream) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || n_batch > 65535 || row_pitch < nz || n_bins < 0 ||
        n_bins > C21HIP_MOMENTS_MAX_BINS || (n_bins > 0 && (!edges || !hist))) {
        c21hip_set_error("moments: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const hipStream_t s = (hipStream_t)stream;
    const long long per = (long long)nx * ny;
    // one row per wave without a histogram; with one, kRowsPerWgHist rows, so that the flush (up to n_bins global
    // atomics on the same few words from every workgroup) stays rare: on the 256^2 x 1536 lightcone with 64 bins,
    // 8 rows per workgroup took 1.4 ms a call and 64 rows 1.1 ms.  A workgroup's 32-bit counts hold its rpw nz cells
    long long rpw = n_bins > 0 ? kRowsPerWgHist : kWaves;
    if (rpw > per) rpw = per;
    while (rpw > 1 && rpw * (long long)nz > 0x7FFFFFFFll) rpw /= 2;
    const long long wgs = (per + rpw - 1) / rpw;
    if (wgs > 0x7FFFFFFFll) {
        c21hip_set_error("moments: too many rows for one launch");
        return C21CM_VALUE_ERROR;
    }
    const dim3 grid((unsigned)wgs, (unsigned)n_batch);
    if (n_bins > 0) {
        hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (size_t)n_batch * (size_t)n_bins, s);
        if (e != hipSuccess) {
            c21hip_set_error("moments: memset failed: %s", hipGetErrorString(e));
            return C21CM_IO_ERROR;
        }
        const size_t lds = sizeof(double) * ((size_t)n_bins + 1) + sizeof(unsigned) * (size_t)n_bins;
        hipLaunchKernelGGL(moments_central_kernel<true>, grid, dim3(kBlock), lds, s, in, rowsum, per, (int)rpw, nz,
                           row_pitch, offsets, mean, n_bins, edges, hist);
    } else {
        hipLaunchKernelGGL(moments_central_kernel<false>, grid, dim3(kBlock), 0, s, in, rowsum, per, (int)rpw, nz,
                           row_pitch, offsets, mean, 0, edges, hist);
    }
    int st = launch_status("moments central");
    if (st) return st;
    launch_boxsum<3>(rowsum, part, mean, moments, per, n_batch, 1.0 / ((double)per * (double)nz), s);
    return launch_status("moments sums");
}
