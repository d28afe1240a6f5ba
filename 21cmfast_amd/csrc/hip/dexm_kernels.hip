// dexm_kernels.hip -- the DexM halo finder on the device (reference: HaloCatalog.c:245-358, check_halo
// :460-550, pixel_in_halo :574-620).
//
// The reference decides the candidates of one radius serially in raster order.  Here:
//   * dexm_count / dexm_list: threshold + ordered compaction of the rung's candidates into a raster-ordered
//     list, and the per-cell state grid (0 not a candidate / decided against, 1 undecided, 2 a halo of this
//     rung, 3 / 4 rejected / accepted in the running round);
//   * dexm_decide: one workgroup (a wave for small spheres) per undecided candidate.  Rejected for good when
//     the mask test fails; accepted when it passes and no EARLIER candidate inside the interaction range
//     is still undecided.  States 3 and 4 count as undecided, so a round reads a snapshot and its result
//     does not depend on which workgroup ran first;
//   * dexm_paint: the spheres of the round's accepted halos (plain byte stores, every writer stores 1);
//   * dexm_serial: one workgroup that walks the list in order, path 1 and the tail after the round cap;
//   * dexm_forbid: the DEXM_OPTIMIZE no-go mask of the halos found so far;
//   * dexm_extract: the catalogue in raster order with its Philox deviates;
//   * dexm_mask_float / dexm_downsample: the overlap box.
// check_halo's arithmetic is kept as it is: the radius in cells is a float quotient, its ceiling the search
// range, its double square rounded to float the strict bound on the float squared distance to the nearest
// of the 27 images.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c21hip.h"
#include "c21cm_grid.h"
#include "philox.h"

namespace {
constexpr int kCells = 4;          // cells per thread of the compaction kernels
constexpr int kCBlock = 256;       // their workgroup
constexpr int kTeamSmall = 64;     // one wave per candidate ...
constexpr int kTeamLarge = 256;    // ... or one workgroup, from kLargeCube cells in the search cube
constexpr long long kLargeCube = 4096;
constexpr unsigned kMaxTeams = 8192; // workgroups of a decide / paint launch (grid-stride over the list)

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                       \
            return C21CM_IO_ERROR;                                                      \
        }                                                                               \
    } while (0)

enum { ST_NONE = 0, ST_UNDECIDED = 1, ST_HALO = 2, ST_REJECT_NOW = 3, ST_ACCEPT_NOW = 4 };
enum { CT_DECIDED = 0, CT_ACCEPTED = 1, CT_FOUND = 2, CT_LAST_ROUND = 3 };

struct Sphere {
    int Ri;    // ceil(R / BOX_LEN * DIM)
    float Rsq; // (R / BOX_LEN * DIM)^2, the double square as a float
};

// check_halo :483-484.  BOX_LEN is a float in the reference, so the quotient and the product are float.
__host__ __device__ inline Sphere sphere_of(float R, float box_len, int n) {
    const float q = R / box_len * (float)n;
    Sphere s;
    const double c = ceil((double)q);
    s.Ri = c > 1e9 ? 1000000000 : (c < 0 ? 0 : (int)c);
    s.Rsq = (float)((double)q * (double)q);
    return s;
}

struct Geom {
    int n, nz; // the grid is [n][n][nz], z fastest
};

// the search cube of half-width Ri around (cx, cy, cz): per axis the distinct cells it reaches
struct Cube {
    int bx, by, bz, mx, my, mz; // first coordinate (before wrapping) and count per axis
    long long total;
};

__device__ __forceinline__ Cube cube_of(const Geom &g, int cx, int cy, int cz, int Ri) {
    Cube c;
    const bool wx = 2ll * Ri + 1 >= g.n, wz = 2ll * Ri + 1 >= g.nz;
    c.mx = c.my = wx ? g.n : 2 * Ri + 1;
    c.mz = wz ? g.nz : 2 * Ri + 1;
    c.bx = wx ? 0 : cx - Ri + g.n; // + n: non-negative before the modulo
    c.by = wx ? 0 : cy - Ri + g.n;
    c.bz = wz ? 0 : cz - Ri + g.nz;
    c.total = (long long)c.mx * c.my * c.mz;
    return c;
}

__device__ __forceinline__ float axis_sq(int d, int n) { // the nearest of d, d + n, d - n, squared (float)
    const float a = (float)d * (float)d, b = (float)(d + n) * (float)(d + n), c = (float)(d - n) * (float)(d - n);
    return fminf(a, fminf(b, c));
}

// cell k of the cube: its wrapped coordinates, its index, and pixel_in_halo against Rsq
__device__ __forceinline__ bool cube_cell(const Geom &g, const Cube &c, long long k, int cx, int cy, int cz, float Rsq,
                                          uint32_t *idx) {
    const int iz = (int)(k % c.mz);
    const long long t = k / c.mz;
    const int iy = (int)(t % c.my), ix = (int)(t / c.my);
    const int x = (c.bx + ix) % g.n, y = (c.by + iy) % g.n, z = (c.bz + iz) % g.nz;
    *idx = ((uint32_t)x * (uint32_t)g.n + (uint32_t)y) * (uint32_t)g.nz + (uint32_t)z;
    return Rsq > (axis_sq(cx - x, g.n) + axis_sq(cy - y, g.n)) + axis_sq(cz - z, g.nz);
}

// does any cell of the sphere have mask != 0?  The whole team calls it; *flag is 0 on entry and on return.
__device__ bool team_sphere_hits(const Geom &g, const unsigned char *mask, int cx, int cy, int cz, const Sphere &s,
                                 int *flag) {
    const Cube c = cube_of(g, cx, cy, cz, s.Ri);
    bool found = false;
    int it = 0;
    for (long long k = threadIdx.x; k < c.total; k += blockDim.x, it++) {
        if ((it & 7) == 7 && *(volatile int *)flag) break; // another thread found one
        uint32_t idx;
        if (cube_cell(g, c, k, cx, cy, cz, s.Rsq, &idx) && mask[idx]) {
            found = true;
            *(volatile int *)flag = 1;
            break;
        }
    }
    const bool any = __syncthreads_or(found);
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    return any;
}

// is any candidate EARLIER in raster order and within Chebyshev distance `range` still undecided?
__device__ bool team_earlier_undecided(const Geom &g, const unsigned char *state, uint32_t cell, int cx, int cy, int cz,
                                       int range, int *flag) {
    const Cube c = cube_of(g, cx, cy, cz, range);
    bool found = false;
    int it = 0;
    for (long long k = threadIdx.x; k < c.total; k += blockDim.x, it++) {
        if ((it & 7) == 7 && *(volatile int *)flag) break;
        uint32_t idx;
        (void)cube_cell(g, c, k, cx, cy, cz, 0.f, &idx);
        if (idx < cell) {
            const unsigned char st = state[idx];
            if (st == ST_UNDECIDED || st == ST_REJECT_NOW || st == ST_ACCEPT_NOW) {
                found = true;
                *(volatile int *)flag = 1;
                break;
            }
        }
    }
    const bool any = __syncthreads_or(found);
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    return any;
}

__device__ void team_paint(const Geom &g, unsigned char *mask, int cx, int cy, int cz, const Sphere &s) {
    const Cube c = cube_of(g, cx, cy, cz, s.Ri);
    for (long long k = threadIdx.x; k < c.total; k += blockDim.x) {
        uint32_t idx;
        if (cube_cell(g, c, k, cx, cy, cz, s.Rsq, &idx)) mask[idx] = 1;
    }
}

struct Rung {
    Geom g;
    Sphere paint, test, forbid; // R; R * r_overlap (type 1); (1 + r_overlap) * R (DEXM_OPTIMIZE)
    int range;                  // Chebyshev range inside which a halo of this rung can change a candidate's test
    int optimize;               // the DEXM_OPTIMIZE branch: the test is !forbidden[cell]
    int rung;
    uint32_t n_cells;
};

__device__ __forceinline__ void decode(const Geom &g, uint32_t cell, int *x, int *y, int *z) {
    *z = (int)(cell % (uint32_t)g.nz);
    const uint32_t t = cell / (uint32_t)g.nz;
    *y = (int)(t % (uint32_t)g.n);
    *x = (int)(t / (uint32_t)g.n);
}

// the mask test of one candidate (HaloCatalog.c:263-293): true = it cannot become a halo
__device__ __forceinline__ bool team_mask_test(const Rung &p, const unsigned char *in_halo, const unsigned char *forbidden,
                                               uint32_t cell, int cx, int cy, int cz, int *flag) {
    if (p.optimize) return forbidden[cell] != 0;
    if (in_halo[cell]) return true;
    return team_sphere_hits(p.g, in_halo, cx, cy, cz, p.test, flag);
}

__global__ void dexm_decide_kernel(Rung p, const uint32_t *__restrict__ list, uint32_t n_cand, unsigned char *state,
                                   const unsigned char *in_halo, const unsigned char *forbidden) {
    __shared__ int flag;
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < n_cand; c += gridDim.x) {
        const uint32_t cell = list[c];
        if (state[cell] != ST_UNDECIDED) continue; // only this workgroup writes state[cell] in this kernel
        int cx, cy, cz;
        decode(p.g, cell, &cx, &cy, &cz);
        __syncthreads(); // every thread has read the state before thread 0 may change it
        unsigned char verdict = ST_UNDECIDED;
        if (team_mask_test(p, in_halo, forbidden, cell, cx, cy, cz, &flag))
            verdict = ST_REJECT_NOW;
        else if (!team_earlier_undecided(p.g, state, cell, cx, cy, cz, p.range, &flag))
            verdict = ST_ACCEPT_NOW;
        if (threadIdx.x == 0 && verdict != ST_UNDECIDED) state[cell] = verdict;
    }
}

// bookkeeping of one accepted halo, by one thread
__device__ __forceinline__ void record_halo(const Rung &p, uint32_t cell, unsigned short *rung_grid, uint32_t *found,
                                            unsigned int *ctr) {
    rung_grid[cell] = (unsigned short)(p.rung + 1);
    const uint32_t row = atomicAdd(&ctr[CT_FOUND], 1u); // at most one entry per cell: the list holds N
    if (row < p.n_cells) found[row] = cell;
    atomicAdd(&ctr[CT_ACCEPTED], 1u);
}

__device__ __forceinline__ void team_paint_halo(const Rung &p, unsigned char *in_halo, unsigned char *forbidden, int cx,
                                                int cy, int cz) {
    team_paint(p.g, in_halo, cx, cy, cz, p.paint);
    if (p.optimize) team_paint(p.g, forbidden, cx, cy, cz, p.forbid);
}

__global__ void dexm_paint_kernel(Rung p, const uint32_t *__restrict__ list, uint32_t n_cand, unsigned char *state,
                                  unsigned char *in_halo, unsigned char *forbidden, unsigned short *rung_grid,
                                  uint32_t *found, unsigned int *ctr, unsigned int round) {
    for (uint32_t c = blockIdx.x; c < n_cand; c += gridDim.x) {
        const uint32_t cell = list[c];
        const unsigned char st = state[cell];
        if (st != ST_REJECT_NOW && st != ST_ACCEPT_NOW) continue;
        __syncthreads();
        if (st == ST_ACCEPT_NOW) {
            int cx, cy, cz;
            decode(p.g, cell, &cx, &cy, &cz);
            team_paint_halo(p, in_halo, forbidden, cx, cy, cz);
        }
        if (threadIdx.x == 0) {
            if (st == ST_ACCEPT_NOW) record_halo(p, cell, rung_grid, found, ctr);
            state[cell] = st == ST_ACCEPT_NOW ? ST_HALO : ST_NONE;
            atomicAdd(&ctr[CT_DECIDED], 1u);
            atomicMax(&ctr[CT_LAST_ROUND], round);
        }
    }
}

// one workgroup, the reference's loop: every undecided candidate in list order
__global__ void __launch_bounds__(kTeamLarge)
dexm_serial_kernel(Rung p, const uint32_t *__restrict__ list, uint32_t n_cand, unsigned char *state, unsigned char *in_halo,
                   unsigned char *forbidden, unsigned short *rung_grid, uint32_t *found, unsigned int *ctr) {
    __shared__ int flag;
    if (threadIdx.x == 0) flag = 0;
    __syncthreads();
    for (uint32_t c = 0; c < n_cand; c++) {
        const uint32_t cell = list[c];
        if (state[cell] != ST_UNDECIDED) continue;
        int cx, cy, cz;
        decode(p.g, cell, &cx, &cy, &cz);
        __syncthreads();
        const bool hit = team_mask_test(p, in_halo, forbidden, cell, cx, cy, cz, &flag);
        if (!hit) {
            team_paint_halo(p, in_halo, forbidden, cx, cy, cz);
            if (threadIdx.x == 0) record_halo(p, cell, rung_grid, found, ctr);
            __threadfence(); // the painted bytes are read by other threads of this workgroup next
        }
        if (threadIdx.x == 0) {
            state[cell] = hit ? ST_NONE : ST_HALO;
            atomicAdd(&ctr[CT_DECIDED], 1u);
        }
        __syncthreads();
    }
}

// DEXM_OPTIMIZE (HaloCatalog.c:217-240): the no-go region of every halo found so far, MtoR(M_h) + r_overlap * R
__global__ void dexm_forbid_kernel(Geom g, const uint32_t *__restrict__ found, uint32_t n_found,
                                   const unsigned short *__restrict__ rung_grid, const float *__restrict__ r_of_rung,
                                   double overlap_R, float box_len, unsigned char *forbidden) {
    for (uint32_t h = blockIdx.x; h < n_found; h += gridDim.x) {
        const uint32_t cell = found[h];
        const int r = (int)rung_grid[cell] - 1;
        if (r < 0) continue;
        const float radius = (float)((double)r_of_rung[r] + overlap_R);
        int cx, cy, cz;
        decode(g, cell, &cx, &cy, &cz);
        team_paint(g, forbidden, cx, cy, cz, sphere_of(radius, box_len, g.n));
    }
}

// ---- ordered compaction.  MODE 0: candidates of a rung (delta > crit and the own cell free in `mask`);
// MODE 1: the halos (rung_grid > 0).
template <int MODE>
__device__ __forceinline__ bool selected(size_t cell, const float *delta, float crit, const unsigned char *mask,
                                         const unsigned short *rung_grid) {
    if (MODE == 0) return delta[cell] > crit && !mask[cell];
    return rung_grid[cell] != 0;
}

template <int MODE>
__global__ void __launch_bounds__(kCBlock)
dexm_count_kernel(const float *__restrict__ delta, float crit, const unsigned char *__restrict__ mask,
                  const unsigned short *__restrict__ rung_grid, size_t n, unsigned long long *__restrict__ counts) {
    __shared__ unsigned int part[kCBlock / 64];
    const size_t base = ((size_t)blockIdx.x * kCBlock + threadIdx.x) * kCells;
    unsigned int mine = 0;
    for (int k = 0; k < kCells; k++)
        if (base + k < n && selected<MODE>(base + k, delta, crit, mask, rung_grid)) mine++;
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int s = 0;
        for (int w = 0; w < kCBlock / 64; w++) s += part[w];
        counts[blockIdx.x] = s;
    }
}

// exclusive prefix of `mine` over the workgroup
__device__ __forceinline__ unsigned int block_exclusive(unsigned int mine, unsigned int *scratch) {
    scratch[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kCBlock; d <<= 1) {
        const unsigned int t = threadIdx.x >= (unsigned)d ? scratch[threadIdx.x - d] : 0u;
        __syncthreads();
        scratch[threadIdx.x] += t;
        __syncthreads();
    }
    return scratch[threadIdx.x] - mine;
}

__global__ void __launch_bounds__(kCBlock)
dexm_list_kernel(const float *__restrict__ delta, float crit, const unsigned char *__restrict__ mask, size_t n,
                 const unsigned long long *__restrict__ offsets, uint32_t *__restrict__ list,
                 unsigned char *__restrict__ state) {
    __shared__ unsigned int scratch[kCBlock];
    const size_t base = ((size_t)blockIdx.x * kCBlock + threadIdx.x) * kCells;
    bool sel[kCells];
    unsigned int mine = 0;
    for (int k = 0; k < kCells; k++) {
        sel[k] = base + k < n && selected<0>(base + k, delta, crit, mask, nullptr);
        mine += sel[k];
    }
    unsigned long long row = offsets[blockIdx.x] + block_exclusive(mine, scratch);
    for (int k = 0; k < kCells; k++) {
        if (base + k < n) state[base + k] = sel[k] ? ST_UNDECIDED : ST_NONE;
        if (sel[k]) list[row++] = (uint32_t)(base + k); // row < total <= n
    }
}

struct Rows {
    float *masses, *coords, *star, *sfr, *xray;
};

__global__ void __launch_bounds__(kCBlock)
dexm_extract_kernel(Geom g, const unsigned short *__restrict__ rung_grid, size_t n,
                    const unsigned long long *__restrict__ offsets, const float *__restrict__ mass_of_rung,
                    double cell_length, uint64_t key, Rows o) {
    __shared__ unsigned int scratch[kCBlock];
    const size_t base = ((size_t)blockIdx.x * kCBlock + threadIdx.x) * kCells;
    unsigned short r[kCells];
    unsigned int mine = 0;
    for (int k = 0; k < kCells; k++) {
        r[k] = base + k < n ? rung_grid[base + k] : (unsigned short)0;
        mine += r[k] != 0;
    }
    unsigned long long row = offsets[blockIdx.x] + block_exclusive(mine, scratch);
    for (int k = 0; k < kCells; k++) {
        if (!r[k]) continue;
        const uint64_t cell = base + k;
        int x, y, z;
        decode(g, (uint32_t)cell, &x, &y, &z);
        o.masses[row] = mass_of_rung[r[k] - 1];
        o.coords[3 * row + 0] = (float)(x * cell_length); // HaloCatalog.c:349-351
        o.coords[3 * row + 1] = (float)(y * cell_length);
        o.coords[3 * row + 2] = (float)(z * cell_length);
        // add_properties_cat: three standard normals.  One Philox block, four 32-bit uniforms on (0, 1),
        // Box-Muller on (u0, u1) for the first two and on (u2, u3) for the third.
        uint32_t w[4];
        philox4x32_10_ctr(0u, (uint32_t)C21CM_HS_DRAW_DEXM, (uint32_t)cell, (uint32_t)(cell >> 32), key, w);
        const double u0 = ((double)w[0] + 0.5) * 0x1p-32, u1 = ((double)w[1] + 0.5) * 0x1p-32;
        const double u2 = ((double)w[2] + 0.5) * 0x1p-32, u3 = ((double)w[3] + 0.5) * 0x1p-32;
        const double ra = sqrt(-2.0 * log(u0)), rb = sqrt(-2.0 * log(u2));
        double s, c;
        sincos(2.0 * M_PI * u1, &s, &c);
        o.star[row] = (float)(ra * c);
        o.sfr[row] = (float)(ra * s);
        o.xray[row] = (float)(rb * cos(2.0 * M_PI * u3));
        row++;
    }
}

__global__ void dexm_mask_float_kernel(const unsigned char *__restrict__ mask, float *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mask[i] ? 1.f : 0.f;
}

// HaloCatalog.c:395-417: the smoothed mask at (int)(i * DIM / (float)HII_DIM + 0.5) per axis, clamped to [0, 1]
__global__ void dexm_downsample_kernel(const float *__restrict__ smooth, Geom hi, Geom lo, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)lo.n * lo.n * lo.nz;
    if (i >= n) return;
    const int k = (int)(i % lo.nz), j = (int)((i / lo.nz) % lo.n), l = (int)(i / ((size_t)lo.nz * lo.n));
    const float f = hi.n / (float)lo.n;
    int x = (int)(l * f + 0.5), y = (int)(j * f + 0.5), z = (int)(k * f + 0.5);
    x = x < hi.n ? x : hi.n - 1; // never past the grid, whatever the two z dimensions round to
    y = y < hi.n ? y : hi.n - 1;
    z = z < hi.nz ? z : hi.nz - 1;
    const float v = smooth[((size_t)x * hi.n + y) * hi.nz + z];
    out[i] = (float)fmin(fmax((double)v, 0.), 1.);
}

Rung make_rung(const c21cm_find_halos_spec *s, int r) {
    Rung p;
    p.g.n = s->dim;
    p.g.nz = s->dim_z;
    const float R = s->R[r], box = (float)s->box_len;
    float Rt = R;
    Rt *= s->r_overlap; // check_halo :475, DEXM_R_OVERLAP is a double
    p.paint = sphere_of(R, box, s->dim);
    p.test = sphere_of(Rt, box, s->dim);
    p.forbid = sphere_of((float)((1. + s->r_overlap) * R), box, s->dim);
    p.optimize = s->optimize && s->mass[r] > s->optimize_minmass;
    // a halo accepted at e changes cells within paint.Ri (forbid.Ri) of e per axis; the test of c reads cells
    // within test.Ri of c (its own cell): only |e - c| <= the sum per axis can matter
    p.range = p.optimize ? p.forbid.Ri : p.paint.Ri + p.test.Ri;
    p.rung = r;
    p.n_cells = (uint32_t)((size_t)s->dim * s->dim * s->dim_z);
    return p;
}

// workgroup per candidate: a wave where the larger of the two search cubes is small
int team_of(const Rung &p) {
    const long long side = 2ll * (p.range > p.paint.Ri ? p.range : p.paint.Ri) + 1;
    const long long side_f = 2ll * p.forbid.Ri + 1;
    const long long s = p.optimize && side_f > side ? side_f : side;
    return s * s * s >= kLargeCube ? kTeamLarge : kTeamSmall;
}

unsigned teams_for(uint32_t n) { return n < kMaxTeams ? (n ? n : 1u) : kMaxTeams; }
unsigned cblocks(size_t n) { return (unsigned)((n + (size_t)kCBlock * kCells - 1) / ((size_t)kCBlock * kCells)); }
}  // namespace

extern "C" unsigned long long c21hip_dexm_blocks(size_t n) { return cblocks(n); }

extern "C" int c21hip_dexm_count(int halos, const float *delta, float crit, const unsigned char *mask,
                                 const unsigned short *rung_grid, size_t n, unsigned long long *counts, void *stream) {
    if (halos)
        hipLaunchKernelGGL(dexm_count_kernel<1>, dim3(cblocks(n)), dim3(kCBlock), 0, (hipStream_t)stream, delta, crit, mask,
                           rung_grid, n, counts);
    else
        hipLaunchKernelGGL(dexm_count_kernel<0>, dim3(cblocks(n)), dim3(kCBlock), 0, (hipStream_t)stream, delta, crit, mask,
                           rung_grid, n, counts);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_list(const float *delta, float crit, const unsigned char *mask, size_t n,
                                const unsigned long long *offsets, unsigned int *list, unsigned char *state,
                                void *stream) {
    hipLaunchKernelGGL(dexm_list_kernel, dim3(cblocks(n)), dim3(kCBlock), 0, (hipStream_t)stream, delta, crit, mask, n,
                       offsets, list, state);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_decide(const c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                                  void *stream) {
    const Rung p = make_rung(s, r);
    hipLaunchKernelGGL(dexm_decide_kernel, dim3(teams_for(n_cand)), dim3(team_of(p)), 0, (hipStream_t)stream, p, a->list,
                       n_cand, a->state, a->in_halo, a->forbidden);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_paint(const c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                                 unsigned int round, void *stream) {
    const Rung p = make_rung(s, r);
    hipLaunchKernelGGL(dexm_paint_kernel, dim3(teams_for(n_cand)), dim3(team_of(p)), 0, (hipStream_t)stream, p, a->list,
                       n_cand, a->state, a->in_halo, a->forbidden, a->rung_grid, a->found, a->counters, round);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_serial(const c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                                  void *stream) {
    const Rung p = make_rung(s, r);
    hipLaunchKernelGGL(dexm_serial_kernel, dim3(1), dim3(kTeamLarge), 0, (hipStream_t)stream, p, a->list, n_cand, a->state,
                       a->in_halo, a->forbidden, a->rung_grid, a->found, a->counters);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_forbid(const c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_found,
                                  const float *r_of_rung, void *stream) {
    if (!n_found) return 0;
    Geom g = {s->dim, s->dim_z};
    hipLaunchKernelGGL(dexm_forbid_kernel, dim3(teams_for(n_found)), dim3(kTeamLarge), 0, (hipStream_t)stream, g, a->found,
                       n_found, a->rung_grid, r_of_rung, s->r_overlap * (double)s->R[r], (float)s->box_len, a->forbidden);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_extract(const c21cm_find_halos_spec *s, const c21hip_dexm_arrays *a, size_t n,
                                   const unsigned long long *offsets, const float *mass_of_rung, float *masses,
                                   float *coords, float *star, float *sfr, float *xray, void *stream) {
    Geom g = {s->dim, s->dim_z};
    const Rows o = {masses, coords, star, sfr, xray};
    const uint64_t key = (uint64_t)s->seed + (uint64_t)(s->redshift * 1000);
    hipLaunchKernelGGL(dexm_extract_kernel, dim3(cblocks(n)), dim3(kCBlock), 0, (hipStream_t)stream, g, a->rung_grid, n,
                       offsets, mass_of_rung, (double)((float)s->box_len / (float)s->dim), key, o);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_mask_float(const unsigned char *mask, float *out, size_t n, void *stream) {
    hipLaunchKernelGGL(dexm_mask_float_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask,
                       out, n);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_dexm_downsample(const float *smooth, int dim, int dim_z, int hii_dim, int hii_dim_z, float *out,
                                      void *stream) {
    Geom hi = {dim, dim_z}, lo = {hii_dim, hii_dim_z};
    const size_t n = (size_t)hii_dim * hii_dim * hii_dim_z;
    hipLaunchKernelGGL(dexm_downsample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, smooth,
                       hi, lo, out);
    LAUNCH_CHECK();
    return 0;
}
