// granulometry_kernels.hip -- exact squared Euclidean distance transforms and granulometry (inscribed-ball) bubble
// sizes of boxes and lightcone chunks (Kakiichi et al. 2017; the estimator is written down at
// c21cm_granulometry_grids, its spec is tests/granulometry_reference.py).  Everything is int32 / int64: no floating
// point anywhere.
//   The core is the separable transform h[i] = opt_j (g[j] -+ d_a(i, j)^2) along one axis of a dense int32 box, one
//   thread per cell, lanes along z in every pass: a wave reads g at distance d as one coalesced row segment whichever
//   axis is walked, so x and y lines need no transpose.  A cell walks outwards, d = 1, 2, ..., both sides at once
//   (minimum image on a periodic axis: d <= n / 2, indices wrapped; d < n with bounds on an open one), and stops at
//   the first d that can no longer win:
//     min-plus (distance transform)  d^2 >= best: every g is >= 0;
//     max-plus (granulometry)        d^2 >= g_max - best, with g_max the box's largest D2: no g exceeds it.
//   So a cell costs 2 sqrt(D2) loads in a distance pass and at most 2 sqrt(max D2) in a granulometry pass, and a line
//   of any length is walked by the cells on it: there is no tile a line has to fit.
//   edt_z    first distance pass straight off the mask of c21hip_bubble_pack: the nearest zero bit of the row from
//            ctz / clz on the inverted words (padding bits masked out), wrapped or not; C21HIP_EDT_NONE for a row of
//            ones;
//   minplus  the y pass, and the x pass, which leaves D2 and with it -- D2 is final there -- the erosion histogram (a
//            cell counts under m = the asked radii below its D2; 32-bit LDS counters flushed with 64-bit atomics), the
//            key (D2, smallest index) of the deepest cell by atomicMax, and level = -1 / 0;
//   finish   one workgroup per box: eroded[k] = the cells with m > k, and the four stats;
//   maxplus  one three-pass transform per radius on G_s = D2 where D2 > s (cut on the fly in the first pass), 0
//            standing for minus infinity: a value <= 0 can never end above 0, so it is clamped.  The last pass writes
//            no box: it counts Q > 0 and bumps level, and stops a cell at the first d that lifts it above 0.  No
//            pass walks an unselected cell: its value is 0 (see the kernel).  A box whose max D2 is <= s leaves every
//            pass at once.
// All boxes of a call go through one launch per kernel (blockIdx.y); at most 2048 workgroups per box, a workgroup
// strides over the rest.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;  // per box: 8 workgroups per CU
constexpr int kNone = C21HIP_EDT_NONE;
constexpr int kLevels = C21HIP_GRAN_MAX_RADII + 1;
constexpr int kAhead = 4;  // steps of a walk whose loads are issued together: the stopping rule is looked at between them

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

// the valid bits of word wi of a row that are zero in the mask, as set bits
__device__ inline unsigned long long zeros_of(const unsigned long long *row, int wi, int W, int nz) {
    unsigned long long inv = ~row[wi];
    if (wi == W - 1 && (nz & 63)) inv &= (1ull << (nz & 63)) - 1ull;
    return inv;
}

// the first zero bit of the row at or after z, or -1
__device__ inline int zero_at_or_after(const unsigned long long *row, int W, int nz, int z) {
    for (int wi = z >> 6; wi < W; ++wi) {
        unsigned long long inv = zeros_of(row, wi, W, nz);
        if (wi == (z >> 6)) inv &= ~0ull << (z & 63);
        if (inv) return wi * 64 + __builtin_ctzll(inv);
    }
    return -1;
}

// the last zero bit of the row at or before z, or -1
__device__ inline int zero_at_or_before(const unsigned long long *row, int W, int nz, int z) {
    for (int wi = z >> 6; wi >= 0; --wi) {
        unsigned long long inv = zeros_of(row, wi, W, nz);
        if (wi == (z >> 6) && (z & 63) != 63) inv &= (1ull << ((z & 63) + 1)) - 1ull;
        if (inv) return wi * 64 + 63 - __builtin_clzll(inv);
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void gran_edt_z_kernel(const unsigned long long *__restrict__ mask, int nz, int W,
                                                            long long rows, int periodic, int *__restrict__ out) {
    const long long cells = rows * nz;
    const unsigned long long *box = mask + (long long)blockIdx.y * rows * W;
    int *dst = out + (long long)blockIdx.y * cells;
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (long long)gridDim.x * kBlock) {
        const long long r = c / nz;
        const int z = (int)(c - r * nz);
        const unsigned long long *row = box + r * W;
        int right = zero_at_or_after(row, W, nz, z), left = zero_at_or_before(row, W, nz, z);
        int d = -1;
        if (right >= 0) d = right - z;
        if (left >= 0 && (d < 0 || z - left < d)) d = z - left;
        if (periodic) {  // a zero found inside the row on one side is nearer than the wrapped one on that side
            if (right < 0) {
                right = zero_at_or_after(row, W, nz, 0);
                if (right >= 0 && (d < 0 || right + nz - z < d)) d = right + nz - z;
            }
            if (left < 0) {
                left = zero_at_or_before(row, W, nz, nz - 1);
                if (left >= 0 && (d < 0 || z + nz - left < d)) d = z + nz - left;
            }
        }
        dst[c] = d < 0 ? kNone : d * d;
    }
}

// The two cells at distance d from cell i of its line (c: the cell's flat index), `neutral` where there is none or
// where !ok.  Both loads are issued whatever the answer -- a missing neighbour reads the cell itself -- so that the
// loads of kAhead steps are in flight together
__device__ inline void two_at(const int *__restrict__ src, long long c, long long ds, long long span, int i, int n,
                              int periodic, int d, bool ok, int neutral, int &a, int &e) {
    bool up = ok, down = ok;
    long long ju = ds, jd = -ds;  // ds = d stride, span = n stride: no multiplication per load
    if (periodic) {
        if (i + d >= n) ju -= span;
        if (i - d < 0) jd += span;
    } else {
        up = ok && i + d < n;
        down = ok && i - d >= 0;
    }
    a = src[up ? c + ju : c];
    e = src[down ? c + jd : c];
    a = up ? a : neutral;
    e = down ? e : neutral;
}

struct edt_final_args {
    int n_radii;
    const long long *radii2;   // device, n_radii
    int *level;                // [n_batch][cells] or NULL
    unsigned long long *hist;  // [n_batch][kLevels], zeroed by the caller
    unsigned long long *key;   // [n_batch], zeroed by the caller
};

// out[c] = min_j (in[j] + d(i, j)^2) along the axis of n cells and the given stride.  in <= kNone and d^2 < 2^30, so
// the sum stays in int32
template <bool FINAL>
__global__ __launch_bounds__(kBlock) void gran_minplus_kernel(const int *__restrict__ in, int *__restrict__ out,
                                                              long long cells, int n, long long stride, int periodic,
                                                              edt_final_args fa) {
    __shared__ long long radii[FINAL ? kLevels : 1];
    __shared__ unsigned int cnt[FINAL ? kLevels : 1];
    __shared__ unsigned long long top;
    if (FINAL) {
        for (int i = threadIdx.x; i < kLevels; i += kBlock) {
            cnt[i] = 0u;
            radii[i] = i < fa.n_radii ? fa.radii2[i] : 0;
        }
        if (threadIdx.x == 0) top = 0ull;
        __syncthreads();
    }
    const long long b = blockIdx.y;
    const int *src = in + b * cells;
    int *dst = out + b * cells;
    const int dmax = periodic ? n / 2 : n - 1;
    const long long span = (long long)n * stride;
    unsigned long long mine = 0ull;
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (long long)gridDim.x * kBlock) {
        const int i = (int)((c / stride) % n);
        int best = src[c];
        long long ds = stride;
        for (int d0 = 1; d0 <= dmax && d0 * d0 < best; d0 += kAhead, ds += kAhead * stride) {
            int a[kAhead], e[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
                two_at(src, c, ds + u * stride, span, i, n, periodic, d0 + u, d0 + u <= dmax, kNone, a[u], e[u]);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {  // a step past the stopping rule is a candidate like any other
                const int d = d0 + u, v = a[u] < e[u] ? a[u] : e[u];
                if (d <= dmax && v + d * d < best) best = v + d * d;
            }
        }
        dst[c] = best;
        if (FINAL) {
            if (fa.level) fa.level[b * cells + c] = best == 0 ? -1 : 0;
            int lo = 0, hi = fa.n_radii;  // m = the radii with s < best: the first k with radii[k] >= best
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (radii[mid] < (long long)best) lo = mid + 1;
                else hi = mid;
            }
            atomicAdd(&cnt[lo], 1u);
            if (best > 0) {
                const unsigned long long k = ((unsigned long long)best << 31) | (unsigned long long)(0x7FFFFFFFll - c);
                if (k > mine) mine = k;
            }
        }
    }
    if (FINAL) {
        if (mine) atomicMax(&top, mine);
        __syncthreads();
        for (int i = threadIdx.x; i < kLevels; i += kBlock)
            if (cnt[i]) atomicAdd(&fa.hist[b * kLevels + i], (unsigned long long)cnt[i]);
        if (threadIdx.x == 0 && top) atomicMax(&fa.key[b], top);
    }
}

// one workgroup per box
__global__ __launch_bounds__(kBlock) void gran_finish_kernel(const unsigned long long *__restrict__ hist,
                                                             const unsigned long long *__restrict__ key,
                                                             long long cells, int n_radii,
                                                             long long *__restrict__ eroded,
                                                             long long *__restrict__ stats) {
    const long long b = blockIdx.x;
    const int k = threadIdx.x;
    if (k < n_radii) {
        unsigned long long s = 0ull;
        for (int m = k + 1; m <= n_radii; ++m) s += hist[b * kLevels + m];
        eroded[b * n_radii + k] = (long long)s;
    }
    if (k == 0) {
        const unsigned long long t = key[b];
        stats[4 * b + 1] = t ? (long long)(t >> 31) : 0;
        stats[4 * b + 2] = t ? 0x7FFFFFFFll - (long long)(t & 0x7FFFFFFFull) : -1;
        stats[4 * b + 3] = cells - stats[4 * b];
    }
}

// out[c] = max(0, max_j (g[j] - d(i, j)^2)); MODE 0: g = in where in > s, else 0 (in = D2); 1: g = in; 2: as 1, but
// nothing is written: the cells with a result > 0 are counted into covered[b * n_radii] and bump level; only the sign
// is asked for, so a cell stops at the first d that lifts it above 0.  An unselected cell x (dist2 = 0) is not walked
// in any pass: sqrt(D2[c]) <= |x - c| + sqrt(D2[x]) = |x - c|, so D2[c] - |x - c|^2 <= 0 for every centre c, and a
// pass takes its maximum over centres that differ from x along the walked axes alone
template <int MODE>
__global__ __launch_bounds__(kBlock) void gran_maxplus_kernel(const int *__restrict__ in, int *__restrict__ out,
                                                              long long cells, int n, long long stride, int periodic,
                                                              const long long *__restrict__ stats, int s,
                                                              unsigned long long *__restrict__ covered, int n_radii,
                                                              int *__restrict__ level, const int *__restrict__ dist2) {
    __shared__ unsigned int count;
    const long long b = blockIdx.y;
    const long long deepest = stats[4 * b + 1];
    if (deepest <= (long long)s) return;  // nothing of this box survives the cut
    const int gmax = (int)deepest;
    if (MODE == 2) {
        if (threadIdx.x == 0) count = 0u;
        __syncthreads();
    }
    const int *src = in + b * cells;
    const int dmax = periodic ? n / 2 : n - 1;
    const long long span = (long long)n * stride;
    unsigned int found = 0u;
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < cells; c += (long long)gridDim.x * kBlock) {
        if (dist2[b * cells + c] == 0) {  // unselected: sqrt(D2) is 1-Lipschitz, so no g[j] - d^2 is above 0 here
            if (MODE < 2) out[b * cells + c] = 0;
            continue;
        }
        const int i = (int)((c / stride) % n);
        int best = src[c];
        if (MODE == 0 && best <= s) best = 0;
        long long ds = stride;
        for (int d0 = 1; d0 <= dmax && d0 * d0 < gmax - best; d0 += kAhead, ds += kAhead * stride) {
            if (MODE == 2 && best > 0) break;  // the last pass asks for the sign alone
            int a[kAhead], e[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u)
                two_at(src, c, ds + u * stride, span, i, n, periodic, d0 + u, d0 + u <= dmax, 0, a[u], e[u]);
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {  // a step past the stopping rule is a candidate like any other
                const int d = d0 + u;
                int v = a[u] > e[u] ? a[u] : e[u];
                if (MODE == 0 && v <= s) v = 0;
                if (d <= dmax && v - d * d > best) best = v - d * d;
            }
        }
        if (MODE < 2) {
            out[b * cells + c] = best;
        } else if (best > 0) {
            ++found;
            if (level) level[b * cells + c] += 1;
        }
    }
    if (MODE == 2) {
        if (found) atomicAdd(&count, found);
        __syncthreads();
        if (threadIdx.x == 0 && count) atomicAdd(&covered[b * n_radii], (unsigned long long)count);
    }
}

bool shape_ok(int nx, int ny, int nz, int n_batch, int periodic_mask) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || n_batch > 65535 || periodic_mask < 0 || periodic_mask > 7)
        return false;
    if ((long long)nx * ny * nz > 0x7FFFFFFFll || (long long)nx * ny > 0x7FFFFFFFll) return false;
    return (long long)nx * nx + (long long)ny * ny + (long long)nz * nz < (long long)kNone;
}

unsigned blocks_of(long long cells) {
    const long long blocks = (cells + kBlock - 1) / kBlock;
    return (unsigned)(blocks > kMaxBlocks ? kMaxBlocks : blocks);
}
}  // namespace

extern "C" int c21hip_gran_edt(const unsigned long long *mask, int nx, int ny, int nz, int n_batch, int periodic_mask,
                               int n_radii, const long long *radii2, int *work_a, int *work_b, int *dist2, int *level,
                               unsigned long long *hist, unsigned long long *key, long long *eroded, long long *stats,
                               void *stream) {
    if (!shape_ok(nx, ny, nz, n_batch, periodic_mask) || n_radii < 0 || n_radii > C21HIP_GRAN_MAX_RADII || !mask ||
        !work_a || !work_b || !dist2 || !hist || !key || !stats || (n_radii > 0 && (!radii2 || !eroded))) {
        c21hip_set_error("granulometry distance transform: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long cells = (long long)nx * ny * nz;
    const dim3 grid(blocks_of(cells), (unsigned)n_batch);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gran_edt_z_kernel, grid, dim3(kBlock), 0, st, mask, nz, (nz + 63) / 64, (long long)nx * ny,
                       (periodic_mask >> 2) & 1, work_a);
    int status = launch_status("granulometry edt z");
    if (status) return status;
    edt_final_args fa = {n_radii, radii2, level, hist, key};
    hipLaunchKernelGGL(gran_minplus_kernel<false>, grid, dim3(kBlock), 0, st, (const int *)work_a, work_b, cells, ny,
                       (long long)nz, (periodic_mask >> 1) & 1, fa);
    if ((status = launch_status("granulometry edt y"))) return status;
    hipLaunchKernelGGL(gran_minplus_kernel<true>, grid, dim3(kBlock), 0, st, (const int *)work_b, dist2, cells, nx,
                       (long long)ny * nz, periodic_mask & 1, fa);
    if ((status = launch_status("granulometry edt x"))) return status;
    hipLaunchKernelGGL(gran_finish_kernel, dim3((unsigned)n_batch), dim3(kBlock), 0, st,
                       (const unsigned long long *)hist, (const unsigned long long *)key, cells, n_radii, eroded, stats);
    return launch_status("granulometry finish");
}

extern "C" int c21hip_gran_cover(const int *dist2, int nx, int ny, int nz, int n_batch, int periodic_mask, int radius2,
                                 int k, int n_radii, const long long *stats, int *work_a, int *work_b,
                                 unsigned long long *covered, int *level, void *stream) {
    if (!shape_ok(nx, ny, nz, n_batch, periodic_mask) || radius2 < 0 || k < 0 || k >= n_radii ||
        n_radii > C21HIP_GRAN_MAX_RADII || !dist2 || !stats || !work_a || !work_b || !covered) {
        c21hip_set_error("granulometry cover: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long cells = (long long)nx * ny * nz;
    const dim3 grid(blocks_of(cells), (unsigned)n_batch);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gran_maxplus_kernel<0>, grid, dim3(kBlock), 0, st, dist2, work_a, cells, nz, 1ll,
                       (periodic_mask >> 2) & 1, stats, radius2, covered + k, n_radii, (int *)nullptr, dist2);
    int status = launch_status("granulometry cover z");
    if (status) return status;
    hipLaunchKernelGGL(gran_maxplus_kernel<1>, grid, dim3(kBlock), 0, st, (const int *)work_a, work_b, cells, ny,
                       (long long)nz, (periodic_mask >> 1) & 1, stats, radius2, covered + k, n_radii, (int *)nullptr,
                       dist2);
    if ((status = launch_status("granulometry cover y"))) return status;
    hipLaunchKernelGGL(gran_maxplus_kernel<2>, grid, dim3(kBlock), 0, st, (const int *)work_b, (int *)nullptr, cells, nx,
                       (long long)ny * nz, periodic_mask & 1, stats, radius2, covered + k, n_radii, level, dist2);
    return launch_status("granulometry cover x");
}
