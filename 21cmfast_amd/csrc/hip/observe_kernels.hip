// observe_kernels.hip -- telescope-resolution smoothing of boxes and lightcones (the definition is
// written down at c21cm_observe_smooth_grids, its spec is tests/observe_reference.py): the mean of every slice in
// fp64, a Gaussian beam across the line of sight whose width differs from slice to slice, a top-hat channel along it.
// The field is (nx, ny, ns) with the line of sight s fastest, and in every kernel the lanes of a wave run along s:
// whichever axis is convolved, a wave reads and writes contiguous segments of rows, and a lane carries the weights
// of its own slice.
//   means      partial sums over (i, j) in fp64, one row of 64 slices per wave; how the rows are dealt out depends
//              on nx ny alone, so the mean of a slice does not depend on the slices beside it.  A non-finite value
//              raises the flag.  A second kernel adds the partials in ascending order and divides.
//   beam       one transverse axis of n cells: a workgroup takes 64 slices of one line, `tile` outputs at a time with
//              a wrapped halo of the largest lw among its 64 slices on either side, into LDS; row q of the LDS tile
//              is one cell of the line for all 64 slices, so a wave reads bank = lane: no conflicts.  The weights of
//              the 64 slices sit beside it.  A lane keeps four outputs in registers and walks d = 1 .. lw once for
//              them: acc = w[0] g[i]; acc = fma(w[d], g[i - d] + g[i + d], acc), d ascending.  The order is a
//              function of the slice alone, so neither the tile, nor the other slices' widths, nor the kernel (LDS
//              or direct) change a bit of the result.  Beams wider than kLdsLw on either side (sigma > 16 cells) go
//              through the direct kernel, which reads its neighbours from global memory: any lw, any n.
//   channel    out = (sum of the slices s - below .. s + above, ascending, clipped or wrapped) / their number.
// The kernel that runs first subtracts the means on load, g = (float)((double)f - m[s]).  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kLanes = 64;
constexpr int kBeamBlock = 512;                          // 8 waves
constexpr int kBeamWaves = kBeamBlock / kLanes;
constexpr int kTileRows = C21HIP_OBSERVE_TILE_ROWS;      // cells of a line, halo included, in LDS at a time
constexpr int kLdsLw = C21HIP_OBSERVE_LDS_LW;            // the widest half kernel of the LDS path
constexpr int kOutputs = 4;                              // outputs a lane keeps in registers
constexpr int kLoads = 8;                                // rows of a tile a wave asks for before it stores one
constexpr int kBlock = 256;
constexpr int kMeanWaves = kBlock / kLanes;
constexpr int kMaxBlocks = 4096;
constexpr int kChannelRows = 4;                          // rows a lane of the channel kernel walks together
// data + weights: (248 + 65) * 256 B = 80128 B, two workgroups of 8 waves per CU
static_assert((kTileRows + kLdsLw + 1) * kLanes * 4 <= 80 * 1024, "two beam workgroups per CU");
static_assert(kTileRows > 2 * kLdsLw, "a tile holds at least one output beside its halo");

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

__device__ inline float centred(float v, const double *__restrict__ means, int s) {
    return means ? (float)((double)v - means[s]) : v;
}

// partial[(p * kMeanWaves + wave) * ns + s] = the sum over the rows p * chunk + wave, + kMeanWaves, ... of part p
__global__ __launch_bounds__(kBlock) void observe_partial_kernel(const float *__restrict__ f, long long rows, int ns,
                                                                 long long chunk, double *__restrict__ partial,
                                                                 int *__restrict__ bad) {
    const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
    const int s = blockIdx.x * kLanes + lane;
    if (s >= ns) return;
    const long long r0 = (long long)blockIdx.y * chunk;
    const long long r1 = r0 + chunk < rows ? r0 + chunk : rows;
    double acc = 0.0;
    bool finite = true;
#pragma unroll 4
    for (long long r = r0 + wave; r < r1; r += kMeanWaves) {
        const float v = f[r * ns + s];
        finite = finite && isfinite(v);
        acc += (double)v;
    }
    partial[((long long)blockIdx.y * kMeanWaves + wave) * ns + s] = acc;
    if (!finite) atomicOr(bad, 1);
}

__global__ __launch_bounds__(kBlock) void observe_mean_kernel(const double *__restrict__ partial, int n_partial,
                                                              int ns, long long rows, double *__restrict__ means) {
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= ns) return;
    double acc = 0.0;
    for (int q = 0; q < n_partial; ++q) acc += partial[(long long)q * ns + s];
    means[s] = acc / (double)rows;
}

struct beam_args {
    const float *in;
    float *out;
    int n;                  // cells of the convolved axis
    long long stride;       // elements between two of them
    int n_lines;            // lines per block of 64 slices
    long long line_stride;  // elements between two lines
    int ns;
    const float *tab;       // [lw_max + 1][ns]: w[d] of every slice, zero beyond its lw
    const int *lw;          // [ns]
    const int *lw_block;    // [ceil(ns / 64)]: the largest lw of 64 slices
    const double *means;    // NULL: nothing to subtract
    int tile;               // outputs of a workgroup: kTileRows - 2 lw_max
    int n_tiles;
};

// i mod n for any int i
__device__ inline int wrap(int i, int n) {
    const int r = i % n;
    return r < 0 ? r + n : r;
}

__global__ __launch_bounds__(kBeamBlock) void observe_beam_lds_kernel(beam_args a) {
    __shared__ float line[kTileRows * kLanes];
    __shared__ float wts[(kLdsLw + 1) * kLanes];
    const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
    const int n_sb = (a.ns + kLanes - 1) / kLanes;
    const int sb = (int)(blockIdx.x % (unsigned)n_sb);
    const unsigned rest = blockIdx.x / (unsigned)n_sb;
    const int t = (int)(rest % (unsigned)a.n_tiles), o = (int)(rest / (unsigned)a.n_tiles);
    const int s = sb * kLanes + lane;
    const bool valid = s < a.ns;
    const int sc = valid ? s : a.ns - 1;  // a lane past the last slice loads that slice and stores nothing
    const int lwb = a.lw_block[sb];       // <= kLdsLw: the launcher looked
    const int i0 = t * a.tile;
    const int cnt = a.n - i0 < a.tile ? a.n - i0 : a.tile;
    const float *src = a.in + (long long)o * a.line_stride + sc;
    const int held = cnt + 2 * lwb;       // <= tile + 2 lw_max = kTileRows
    int idx = wrap(i0 - lwb + wave, a.n);
    const int step = kBeamWaves % a.n;
    for (int q0 = wave; q0 < held; q0 += kBeamWaves * kLoads) {  // kLoads rows in flight per wave
        float v[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            v[u] = src[(long long)idx * a.stride];  // past the tile: a cell of the line all the same, not kept
            idx += step;
            if (idx >= a.n) idx -= a.n;
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int q = q0 + u * kBeamWaves;
            if (q < held) line[q * kLanes + lane] = centred(v[u], a.means, sc);
        }
    }
    for (int d = wave; d <= lwb; d += kBeamWaves) wts[d * kLanes + lane] = a.tab[(long long)d * a.ns + sc];
    __syncthreads();
    const int mine = a.lw[sc];
    float *dst = a.out + (long long)o * a.line_stride + sc;
    for (int k0 = wave; k0 < cnt; k0 += kBeamWaves * kOutputs) {
        int row[kOutputs];
        float acc[kOutputs], centre[kOutputs];
        const float w0 = wts[lane];
#pragma unroll
        for (int u = 0; u < kOutputs; ++u) {
            const int k = k0 + u * kBeamWaves;
            row[u] = ((k < cnt ? k : cnt - 1) + lwb) * kLanes + lane;  // an output past the tile repeats the last
            centre[u] = line[row[u]];
            acc[u] = w0 * centre[u];
        }
        for (int d = 1; d <= lwb; ++d) {
            const float w = wts[d * kLanes + lane];
            const bool in_reach = d <= mine;  // the terms of a slice stop at its own lw, whatever its neighbours'
#pragma unroll
            for (int u = 0; u < kOutputs; ++u) {
                const float pair = line[row[u] - d * kLanes] + line[row[u] + d * kLanes];
                const float next = fmaf(w, pair, acc[u]);
                acc[u] = in_reach ? next : acc[u];
            }
        }
#pragma unroll
        for (int u = 0; u < kOutputs; ++u) {
            const int k = k0 + u * kBeamWaves;
            if (valid && k < cnt) dst[(long long)(i0 + k) * a.stride] = mine ? acc[u] : centre[u];
        }
    }
}

// the same sums for any lw and any n: one thread per cell, its neighbours straight from global memory
__global__ __launch_bounds__(kBlock) void observe_beam_direct_kernel(beam_args a, long long cells) {
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (long long)gridDim.x * kBlock) {
        const int s = (int)(c % a.ns);
        const int i = (int)((c / a.stride) % a.n);
        const float *base = a.in + (c - (long long)i * a.stride);
        const int mine = a.lw[s];
        const float centre = centred(base[(long long)i * a.stride], a.means, s);
        float acc = a.tab[s] * centre;
        int up = i, down = i;
        for (int d = 1; d <= mine; ++d) {
            up = up + 1 == a.n ? 0 : up + 1;
            down = down == 0 ? a.n - 1 : down - 1;
            const float pair = centred(base[(long long)down * a.stride], a.means, s) +
                               centred(base[(long long)up * a.stride], a.means, s);
            acc = fmaf(a.tab[(long long)d * a.ns + s], pair, acc);
        }
        a.out[c] = mine ? acc : centre;
    }
}

// A lane keeps its slice and walks rows blockIdx.y * chunk + wave, + kMeanWaves, ..., kChannelRows of them at a time so
// that as many loads are in flight per step of the window
__global__ __launch_bounds__(kBlock) void observe_channel_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                 long long rows, long long chunk, int ns,
                                                                 const int *__restrict__ below,
                                                                 const int *__restrict__ above, int periodic,
                                                                 const double *__restrict__ means) {
    const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
    const int s = blockIdx.x * kLanes + lane;
    if (s >= ns) return;
    int lo = s - below[s], hi = s + above[s];  // hi - lo + 1 <= ns where the line wraps: the driver looked
    if (!periodic) {
        lo = lo < 0 ? 0 : lo;
        hi = hi > ns - 1 ? ns - 1 : hi;
    }
    const int first = wrap(lo, ns), count = hi - lo + 1;
    const long long r0 = (long long)blockIdx.y * chunk;
    const long long r1 = r0 + chunk < rows ? r0 + chunk : rows;
    for (long long r = r0 + wave; r < r1; r += kMeanWaves * kChannelRows) {
        const float *row[kChannelRows];
        float acc[kChannelRows];
        int j = first;
#pragma unroll
        for (int u = 0; u < kChannelRows; ++u) {  // a row past the end repeats the last one and is not stored
            const long long ru = r + u * kMeanWaves;
            row[u] = in + (ru < r1 ? ru : r1 - 1) * ns;
            acc[u] = centred(row[u][j], means, j);
        }
        for (int q = 1; q < count; ++q) {
            j = j + 1 == ns ? 0 : j + 1;
#pragma unroll
            for (int u = 0; u < kChannelRows; ++u) acc[u] += centred(row[u][j], means, j);
        }
#pragma unroll
        for (int u = 0; u < kChannelRows; ++u) {
            const long long ru = r + u * kMeanWaves;
            if (ru < r1) out[ru * ns + s] = count > 1 ? acc[u] / (float)count : acc[u];
        }
    }
}

unsigned blocks_of(long long cells) {
    const long long blocks = (cells + kBlock - 1) / kBlock;
    return (unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks);
}

bool shape_ok(int nx, int ny, int ns) {
    return nx >= 1 && ny >= 1 && ns >= 1 && (long long)nx * ny * ns <= 0x7FFFFFFFll;
}
}  // namespace

extern "C" void c21hip_observe_geometry(int *tile_rows, int *lds_lw) {
    if (tile_rows) *tile_rows = kTileRows;
    if (lds_lw) *lds_lw = kLdsLw;
}

extern "C" int c21hip_observe_mean_parts(long long rows) {
    const long long parts = rows / (64 * kMeanWaves);  // at least 64 rows for every wave
    return (int)(parts < 1 ? 1 : parts > 64 ? 64 : parts);
}

extern "C" int c21hip_observe_means(const float *field, int nx, int ny, int ns, double *partial, double *means,
                                    int *bad, void *stream) {
    if (!shape_ok(nx, ny, ns) || !field || !partial || !means || !bad) {
        c21hip_set_error("observe means: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long rows = (long long)nx * ny;
    const int parts = c21hip_observe_mean_parts(rows);
    const long long chunk = (rows + parts - 1) / parts;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(observe_partial_kernel, dim3((unsigned)((ns + kLanes - 1) / kLanes), (unsigned)parts),
                       dim3(kBlock), 0, st, field, rows, ns, chunk, partial, bad);
    int status = launch_status("observe partial means");
    if (status) return status;
    hipLaunchKernelGGL(observe_mean_kernel, dim3((unsigned)((ns + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       (const double *)partial, parts * kMeanWaves, ns, rows, means);
    return launch_status("observe means");
}

extern "C" int c21hip_observe_beam(const float *in, float *out, int nx, int ny, int ns, int axis, const float *tab,
                                   const int *lw, const int *lw_block, int lw_max, const double *means,
                                   void *stream) {
    if (!shape_ok(nx, ny, ns) || !in || !out || in == out || axis < 0 || axis > 1 || !tab || !lw || !lw_block ||
        lw_max < 1 || lw_max > C21HIP_OBSERVE_MAX_LW) {
        c21hip_set_error("observe beam: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    beam_args a;
    a.in = in;
    a.out = out;
    a.n = axis == 0 ? nx : ny;
    a.stride = axis == 0 ? (long long)ny * ns : (long long)ns;
    a.n_lines = axis == 0 ? ny : nx;
    a.line_stride = axis == 0 ? (long long)ns : (long long)ny * ns;
    a.ns = ns;
    a.tab = tab;
    a.lw = lw;
    a.lw_block = lw_block;
    a.means = means;
    a.tile = kTileRows - 2 * lw_max;
    a.n_tiles = lw_max <= kLdsLw ? (a.n + a.tile - 1) / a.tile : 0;
    hipStream_t st = (hipStream_t)stream;
    const long long cells = (long long)nx * ny * ns;
    if (lw_max <= kLdsLw) {  // blocks <= cells / 64 + ...: fits an unsigned
        const long long blocks = (long long)((ns + kLanes - 1) / kLanes) * a.n_tiles * a.n_lines;
        hipLaunchKernelGGL(observe_beam_lds_kernel, dim3((unsigned)blocks), dim3(kBeamBlock), 0, st, a);
    } else {
        hipLaunchKernelGGL(observe_beam_direct_kernel, dim3(blocks_of(cells)), dim3(kBlock), 0, st, a, cells);
    }
    return launch_status(axis == 0 ? "observe beam x" : "observe beam y");
}

extern "C" int c21hip_observe_channel(const float *in, float *out, int nx, int ny, int ns, const int *below,
                                      const int *above, int periodic, const double *means, void *stream) {
    if (!shape_ok(nx, ny, ns) || !in || !out || in == out || !below || !above) {
        c21hip_set_error("observe channel: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long rows = (long long)nx * ny;
    long long parts = (rows + kMeanWaves * kChannelRows * 2 - 1) / (kMeanWaves * kChannelRows * 2);
    if (parts > 65535) parts = 65535;
    const long long chunk = (rows + parts - 1) / parts;
    hipLaunchKernelGGL(observe_channel_kernel, dim3((unsigned)((ns + kLanes - 1) / kLanes), (unsigned)parts),
                       dim3(kBlock), 0, (hipStream_t)stream, in, out, rows, chunk, ns, below, above, periodic != 0,
                       means);
    return launch_status("observe channel");
}
