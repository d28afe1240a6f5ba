// minkowski_kernels.hip -- the element counts behind the Minkowski functionals of boxes and lightcone chunks (DESIGN
// 4.11; the estimator is written down at c21cm_minkowski_grids, its spec is tests/minkowski_reference.py).  Every
// threshold comes out of one read of the field; every launch covers all boxes (blockIdx.y = box).
//   levels   a cell's level is the number of thresholds <= (double)v, found by a branchless search of the thresholds in
//            LDS; with select_below it is n_thresholds less that.  Either way the cell is selected at threshold i iff
//            its level is at least a bound that depends on i alone, so an element of the complex (cube, face, edge,
//            vertex) is in the set iff the LARGEST level of the cells that contain it is.  A cell that does not exist
//            (through an open face, or past the box) has level 0, which no threshold selects.
//   count    site (i, j, k) owns the vertex at its low corner, the three edges and the three faces leaving it and the
//            cube: 8 elements, each with the largest level of its 1 / 2 / 4 / 8 cells.  A wave holds 64 sites along z
//            of kRows + 1 consecutive rows in y and walks x: per step it loads one value per row and lane (and the one
//            cell below the wave's z range per row, on the lanes of a last load), keeps the levels of the step before
//            in registers, and takes the k - 1 levels from the lane below.  The 8 levels of a site go into the
//            workgroup's LDS histogram pre-reduced: per element kind the lanes of a wave that hold the same level add
//            once (a ballot against the first remaining lane's level, a popcount, one lane's atomic), up to kDistinct
//            levels; what is left after that many rounds holds mostly different levels and adds per lane.  A
//            two-valued field takes one round per kind, a field with a level per cell the last route.  (Packing the
//            8 levels of a site into 64 bits and letting the sites that agree in all of them add once was measured
//            and dropped: white noise and smooth fields alike hold too many distinct sites per wave.)  A workgroup
//            runs through tiles a grid stride apart and flushes its histogram once, with 64-bit integer atomics.
//   finish   counts[b][i][kind] = the elements of that kind whose level is at least i + 1 (or n_thresholds - i with
//            select_below): a suffix sum per box and kind.
// Only integer atomics: two calls give the same bytes, and no result depends on the launch shape.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRows = 4;        // site rows in y per wave: kRows + 1 rows of cells are read for them
constexpr int kSegment = 32;    // sites in x a wave walks per tile: one step in kSegment + 1 only loads
constexpr int kKinds = 8;       // n3, n2x, n2y, n2z, n1x, n1y, n1z, n0
constexpr int kLevels = C21HIP_MINKOWSKI_MAX_THRESHOLDS + 1;
constexpr int kDistinct = 3;   // levels per wave and element kind that are added by ballot
constexpr int kMaxBlocks = 2048;  // workgroups per box at the most (8 per CU)
static_assert(kRows + 1 <= 64, "the cells below the wave's z range are loaded by one lane per row");

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

struct mk_geom {
    int nx, ny, nz;
    int sx, sy, sz;     // sites per axis: n on a periodic axis, n + 1 on an open one
    int px, py, pz;     // periodic?
    int n_seg, n_grp, n_chunk;  // tiles per axis: x segments, groups of kWaves * kRows site rows, chunks of 64 sites
    long long tiles;
    long long row_pitch;
    int n_thr, top;     // top: the largest power of two <= n_thr
    int select_below;
};

// the index of cell c on an axis of n cells: -1 wraps where the axis is periodic; no cell otherwise (-1)
__device__ __forceinline__ int cell_index(int c, int n, int periodic) {
    if (c < 0) return periodic ? n - 1 : -1;
    return c < n ? c : -1;
}

// the thresholds <= (double)v; thr is padded with +inf to kLevels entries, so every probe below is in range
__device__ __forceinline__ int level_of(const double *thr, int top, float v) {
    const double d = (double)v;
    int lo = 0;
    for (int s = top; s > 0; s >>= 1)  // uniform
        if (thr[lo + s - 1] <= d) lo += s;
    return lo;
}

// one element kind of one site per lane: hist[m] += 1 where m > 0
__device__ __forceinline__ void tally_kind(unsigned int *hist, int m, int lane) {
    unsigned long long left = __ballot(m > 0);
    for (int round = 0; round < kDistinct && left; ++round) {  // uniform
        const int first = __ffsll((long long)left) - 1;
        const int m0 = __shfl(m, first, 64);
        const unsigned long long same = __ballot(m == m0);
        if (lane == first) atomicAdd(&hist[m0], (unsigned int)__popcll(same));
        left &= ~same;
    }
    if ((left >> lane) & 1ull) atomicAdd(&hist[m], 1u);
}

__device__ __forceinline__ int max4(int a, int b, int c, int d) { return max(max(a, b), max(c, d)); }

__global__ __launch_bounds__(kBlock) void minkowski_count_kernel(mk_geom s, const float *__restrict__ in,
                                                                 const long long *__restrict__ offsets,
                                                                 const double *__restrict__ thresholds,
                                                                 unsigned long long *__restrict__ hist,
                                                                 int *__restrict__ bad) {
    __shared__ double thr[kLevels];
    __shared__ unsigned int h[kKinds * kLevels];
    for (int i = threadIdx.x; i < kLevels; i += kBlock) thr[i] = i < s.n_thr ? thresholds[i] : INFINITY;
    for (int i = threadIdx.x; i < kKinds * kLevels; i += kBlock) h[i] = 0u;
    __syncthreads();

    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *src = in + offsets[b];
    int not_finite = 0;
    for (long long t = blockIdx.x; t < s.tiles; t += gridDim.x) {
        const int chunk = (int)(t % s.n_chunk);
        const long long rest = t / s.n_chunk;
        const int grp = (int)(rest % s.n_grp), seg = (int)(rest / s.n_grp);
        const int j0 = (grp * kWaves + wave) * kRows;
        if (j0 >= s.sy) continue;  // the whole wave
        const int i0 = seg * kSegment, i1 = min(i0 + kSegment, s.sx);
        const int k = chunk * 64 + lane;                               // the lane's site and cell along z
        const int below = cell_index(chunk * 64 - 1, s.nz, s.pz);      // the cell under the wave's first site
        const int row_of_lane = cell_index(j0 - 1 + min(lane, kRows), s.ny, s.py);
        int cy[kRows + 1];
#pragma unroll
        for (int r = 0; r <= kRows; ++r) cy[r] = cell_index(j0 - 1 + r, s.ny, s.py);

        int pk[kRows + 1] = {}, pk1[kRows + 1] = {};  // levels of the column before, at z = k and k - 1
        for (int i = i0 - 1; i < i1; ++i) {
            const int cx = cell_index(i, s.nx, s.px);
            int ck[kRows + 1], ck1[kRows + 1];
            float v[kRows + 1], v_below = 0.0f;
            bool ok[kRows + 1];
#pragma unroll
            for (int r = 0; r <= kRows; ++r) {
                ok[r] = cx >= 0 && cy[r] >= 0 && k < s.nz;
                v[r] = ok[r] ? src[((long long)cx * s.ny + cy[r]) * s.row_pitch + k] : 0.0f;
            }
            const bool ok_below = lane <= kRows && cx >= 0 && row_of_lane >= 0 && below >= 0;
            if (ok_below) v_below = src[((long long)cx * s.ny + row_of_lane) * s.row_pitch + below];
            int l_below = 0;
            if (ok_below) {
                if (!isfinite(v_below)) not_finite = 1;
                l_below = level_of(thr, s.top, v_below);
                if (s.select_below) l_below = s.n_thr - l_below;
            }
#pragma unroll
            for (int r = 0; r <= kRows; ++r) {
                int l = 0;
                if (ok[r]) {
                    if (!isfinite(v[r])) not_finite = 1;
                    l = level_of(thr, s.top, v[r]);
                    if (s.select_below) l = s.n_thr - l;
                }
                ck[r] = l;
                const int up = __shfl_up(l, 1, 64);
                const int first = __shfl(l_below, r, 64);
                ck1[r] = lane ? up : first;
            }
            if (i >= i0) {
#pragma unroll
                for (int q = 0; q < kRows; ++q) {
                    const bool site = j0 + q < s.sy && k < s.sz;
                    // cells: c / p = x at i / i - 1; rows q / q + 1 = y at j - 1 / j; k / k1 = z at k / k - 1
                    const int cube = ck[q + 1];
                    const int ex = max4(ck[q], ck1[q], ck[q + 1], ck1[q + 1]);
                    const int ey = max4(ck[q + 1], ck1[q + 1], pk[q + 1], pk1[q + 1]);
                    const int ez = max4(ck[q], ck[q + 1], pk[q], pk[q + 1]);
                    const int vertex = max(max(ex, ez), max4(pk1[q], pk1[q + 1], pk[q], pk[q + 1]));
                    tally_kind(h + 0 * kLevels, site ? cube : 0, lane);
                    tally_kind(h + 1 * kLevels, site ? max(cube, pk[q + 1]) : 0, lane);
                    tally_kind(h + 2 * kLevels, site ? max(cube, ck[q]) : 0, lane);
                    tally_kind(h + 3 * kLevels, site ? max(cube, ck1[q + 1]) : 0, lane);
                    tally_kind(h + 4 * kLevels, site ? ex : 0, lane);
                    tally_kind(h + 5 * kLevels, site ? ey : 0, lane);
                    tally_kind(h + 6 * kLevels, site ? ez : 0, lane);
                    tally_kind(h + 7 * kLevels, site ? vertex : 0, lane);
                }
            }
#pragma unroll
            for (int r = 0; r <= kRows; ++r) {
                pk[r] = ck[r];
                pk1[r] = ck1[r];
            }
        }
    }
    if (not_finite) atomicOr(bad, 1);
    __syncthreads();
    const int n_lev = s.n_thr + 1;
    unsigned long long *dst = hist + (long long)b * kKinds * n_lev;
    for (int i = threadIdx.x; i < kKinds * n_lev; i += kBlock) {
        const int kind = i / n_lev, m = i - kind * n_lev;
        const unsigned int n = h[kind * kLevels + m];
        if (n) atomicAdd(&dst[i], (unsigned long long)n);
    }
}

// one thread per box and element kind
__global__ void minkowski_finish_kernel(int n_batch, int n_thr, int select_below,
                                        const unsigned long long *__restrict__ hist, long long *__restrict__ counts) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_batch * kKinds) return;
    const int b = g / kKinds, kind = g - b * kKinds;
    const unsigned long long *src = hist + (long long)g * (n_thr + 1);
    long long *dst = counts + (long long)b * n_thr * kKinds + kind;
    long long sum = 0;
    // above: row i takes the levels >= i + 1; below: the levels >= n_thr - i
    for (int m = n_thr; m >= 1; --m) {
        sum += (long long)src[m];
        const int row = select_below ? n_thr - m : m - 1;
        dst[(long long)row * kKinds] = sum;
    }
}
}  // namespace

extern "C" int c21hip_minkowski(const float *in, int nx, int ny, int nz, long long row_pitch, const long long *offsets,
                                int n_batch, int n_thresholds, const double *thresholds, int select_below,
                                int periodic_mask, unsigned long long *hist, long long *counts, int *bad,
                                void *stream) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || n_batch > 65535 || (long long)nx * ny > 0x7FFFFFFFll ||
        (long long)nx * ny * nz > 0x7FFFFFFFll || row_pitch < nz || n_thresholds < 1 ||
        n_thresholds > C21HIP_MINKOWSKI_MAX_THRESHOLDS || periodic_mask < 0 || periodic_mask > 7 || !in || !offsets ||
        !thresholds || !hist || !counts || !bad) {
        c21hip_set_error("minkowski: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    mk_geom s;
    s.nx = nx, s.ny = ny, s.nz = nz;
    s.px = periodic_mask & 1, s.py = (periodic_mask >> 1) & 1, s.pz = (periodic_mask >> 2) & 1;
    s.sx = nx + !s.px, s.sy = ny + !s.py, s.sz = nz + !s.pz;
    s.n_seg = (s.sx + kSegment - 1) / kSegment;
    s.n_grp = (s.sy + kWaves * kRows - 1) / (kWaves * kRows);
    s.n_chunk = (s.sz + 63) / 64;
    s.tiles = (long long)s.n_seg * s.n_grp * s.n_chunk;
    s.row_pitch = row_pitch;
    s.n_thr = n_thresholds;
    s.top = 1;
    while (s.top * 2 <= n_thresholds) s.top *= 2;
    s.select_below = select_below != 0;
    const long long blocks = s.tiles < kMaxBlocks ? s.tiles : kMaxBlocks;
    hipLaunchKernelGGL(minkowski_count_kernel, dim3((unsigned)blocks, (unsigned)n_batch), dim3(kBlock), 0,
                       (hipStream_t)stream, s, in, offsets, thresholds, hist, bad);
    int status = launch_status("minkowski count");
    if (status) return status;
    hipLaunchKernelGGL(minkowski_finish_kernel, dim3((unsigned)((n_batch * kKinds + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, (hipStream_t)stream, n_batch, n_thresholds, s.select_below, hist, counts);
    return launch_status("minkowski finish");
}
