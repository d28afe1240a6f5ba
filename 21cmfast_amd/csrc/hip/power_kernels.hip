// power_kernels.hip -- power spectra of boxes and lightcone chunks, binned on the device (the binning of
// powerbox.get_power as oracle/powerbox_power.py restates it; options: tests/power_reference.py).
//
// Three steps around the forward transform (fft.hip, rocFFT):
//   pack    one wave per (batch, x, y) row: the field (or one chunk of a lightcone) into the padded r2c layout
//           float[nx][ny][2(nz/2+1)], every value checked for finiteness, less the box's mean.  An fp32 transform
//           spreads the round-off of its largest mode, the mean's, over the lines through k = 0: with a mean as
//           large as the fluctuations that is a few 1e-5 of the power of the modes beside the axes at 10^7 cells.
//           The mean (fp64 row sums, a fixed tree; rounded to fp32 so that the subtraction is a plain fp32
//           one) goes back onto the k = 0 mode where it is read, N mean, in fp64;
//   bin     one pass over the half spectrum complex[nx][ny][nz/2+1].  A mode with 0 < kz < nz/2 stands for
//           itself and its conjugate (weight 2), the planes kz = 0 and kz = nz/2 (even nz) for themselves, so
//           the counts are those of the full grid.  |k| = sqrt((kx^2 + ky^2) + kz^2) in fp64 from the per-axis
//           tables of the driver (numpy's fftfreq(n, L/n) 2 pi), compiled without FMA contraction (Makefile:
//           -ffp-contract=off).  The bin is found on |k|^2 against thresholds t(e) the driver derives from the
//           edges with the host's correctly rounded sqrt (sqrt(x) >= e exactly when x >= t(e)), so a mode lands
//           in the bin np.digitize gives it whatever the rounding of the device's fp64 square root;
//   reduce  deterministic: along a row of the half spectrum |k| (and |kz|) never decreases, so the 64
//           consecutive modes a wave holds form runs of equal (row, bin).  A segmented shuffle scan sums each
//           run, and the run's last lane adds it to the wave's own LDS row of bins: within a row the runs
//           hit different bins, and the rows a wave holds are flushed one after the other, so every
//           LDS update has one writer in program order.  A workgroup sums its waves' rows in a fixed order
//           into partials[batch][workgroup][bin]; the finish kernels sum the partials of each bin over its
//           workgroups in a fixed order (strided per thread, then a fixed tree).  No float atomics: two calls
//           give the same bits.
// Cylindrical spectra bin k_perp per row on the host (the rows are grouped by k_perp bin, each workgroup
// holds rows of one group) and k_par = |kz| here.
// HBM: 8 B per half-spectrum mode and field, read once; the partials are a few per cent of that.
// Options (c21cm_power_opts; conventions: tests/power_stats_reference.py), each a template parameter so that the
// instantiations without them stay the code they were: a taper in the pack (WIN), mu / wedge cuts in the bin step
// (CUT), and the per-bin variance (VAR), one more accumulator sum(w P^2) through the same scan, rows and finish.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

// one wave per row (b, i, j): in[offsets[b] + (i ny + j) row_pitch + l] - mean[b] -> padded[b][i][j][l], l < nz.
// WIN: times the taper, (v - m) wrow[i ny + j] wz[l] with m the fp64 mean and the difference taken in fp64 (the
// mean does not go back onto k = 0 here, so its fp32 rounding would stay in the modes the window couples to it)
template <bool WIN>
__global__ __launch_bounds__(kBlock) void power_pack_kernel(const float *__restrict__ in, float *__restrict__ padded,
                                                            long long rows_per_batch, long long n_rows, int nz,
                                                            long long row_pitch,
                                                            const long long *__restrict__ offsets,
                                                            const double *__restrict__ mean,
                                                            const float *__restrict__ wrow,
                                                            const float *__restrict__ wz, int *bad) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const long long b = row / rows_per_batch, r = row - b * rows_per_batch;
    const float *src = in + offsets[b] + r * row_pitch;
    float *dst = padded + row * (2 * ((long long)nz / 2 + 1));
    int nonfinite = 0;
    if (WIN) {
        const double m = mean[b];
        const float wr = wrow[r];
        for (int l = lane; l < nz; l += 64) {
            const float v = src[l];
            nonfinite |= !isfinite(v);
            dst[l] = ((float)((double)v - m) * wr) * wz[l];
        }
    } else {
        const float m = (float)mean[b];
        for (int l = lane; l < nz; l += 64) {
            const float v = src[l];
            nonfinite |= !isfinite(v);
            dst[l] = v - m;
        }
    }
    if (nonfinite) atomicOr(bad, 1);
}

// rowsum[row] = the fp64 sum of row (b, i, j), lanes strided then a fixed shuffle tree: one wave per row
__global__ __launch_bounds__(kBlock) void power_rowsum_kernel(const float *__restrict__ in, double *__restrict__ rowsum,
                                                              long long rows_per_batch, long long n_rows, int nz,
                                                              long long row_pitch,
                                                              const long long *__restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // the whole wave
    const long long b = row / rows_per_batch, r = row - b * rows_per_batch;
    const float *src = in + offsets[b] + r * row_pitch;
    double s = 0.0;
    for (int l = lane; l < nz; l += 64) s += (double)src[l];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) rowsum[row] = s;
}

// mean[b] = the mean of box b rounded to fp32 (held as a double; round32 = 0: as it is): one workgroup per box,
// thread t sums rows t, t + 256, .. in order, then a fixed tree
__global__ __launch_bounds__(kBlock) void power_boxmean_kernel(const double *__restrict__ rowsum,
                                                               double *__restrict__ mean, long long rows_per_batch,
                                                               double inv_cells, int round32) {
    __shared__ double red[kBlock];
    const double *src = rowsum + (long long)blockIdx.x * rows_per_batch;
    double s = 0.0;
    for (long long r = threadIdx.x; r < rows_per_batch; r += kBlock) s += src[r];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double md = red[0] * inv_cells;
        const float m = (float)md;
        mean[blockIdx.x] = isfinite(m) ? (round32 ? (double)m : md) : 0.0;  // a non-finite box is reported by the pack
    }
}

// NV accumulators per bin: sum w P, sum w k (|k| or k_perp), [sum w k_par], [sum w P^2], sum w.  VAR adds the
// fourth through the same scan, rows and partials; CUT (spherical) applies the mu / wedge predicates of t: a mode
// they drop stays in its run with weight 0, as one an ignore flag drops
template <bool CYL, bool CROSS, bool VAR, bool CUT>
__global__ __launch_bounds__(kBlock) void power_bin_kernel(const float2 *__restrict__ s1,
                                                           const float2 *__restrict__ s2, long long batch_c,
                                                           int ny, int nz, c21hip_power_tabs t,
                                                           const double *__restrict__ mean1,
                                                           const double *__restrict__ mean2, double n_cells,
                                                           double *__restrict__ partials, int *bad) {
    constexpr int NV = C21HIP_POWER_NV(CYL, VAR);
    extern __shared__ double lds[];
    const int nl = t.n_local, nh = nz / 2 + 1;
    double *edges = lds;             // nl + 1 (|k|^2 thresholds, or k_par edges when cylindrical)
    double *acc = lds + (nl + 1);    // [kWaves][nl][NV]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = threadIdx.x; q <= nl; q += kBlock) edges[q] = t.edges[q];
    for (int q = threadIdx.x; q < kWaves * nl * NV; q += kBlock) acc[q] = 0.0;
    __syncthreads();

    const int w = blockIdx.x;
    const long long b = blockIdx.y;
    const int r0 = t.wg_rows[w], nr = t.wg_rows[w + 1] - r0;
    const long long n_el = (long long)nr * nh;
    const float2 *f1 = s1 + b * batch_c;
    const float2 *f2 = CROSS ? s2 + b * batch_c : nullptr;
    double *mine = acc + wave * nl * NV;
    const int span = 63 / nh + 2;  // rows 64 consecutive modes can touch
    int nonfinite = 0;
    for (long long base = (long long)wave * 64; base < n_el; base += kBlock) {
        const long long e = base + lane;
        const bool active = e < n_el;
        const int rl = active ? (int)(e / nh) : nr;
        const int l = active ? (int)(e - (long long)rl * nh) : 0;
        double p = 0.0, k1 = 0.0, k2 = 0.0, pp = 0.0;
        int wt = 0, key = -1;
        if (active) {
            const int row = t.rows[r0 + rl];
            const int i = row / ny, j = row - i * ny;
            const float2 a = f1[(long long)row * nh + l];
            const bool zero_mode = row == 0 && l == 0;  // the mean the pack took out comes back here
            const double ax = zero_mode ? (double)a.x + mean1[b] * n_cells : (double)a.x;
            double q;
            if (CROSS) {
                const float2 c = f2[(long long)row * nh + l];
                nonfinite |= !(isfinite(c.x) && isfinite(c.y));
                const double cx = zero_mode ? (double)c.x + mean2[b] * n_cells : (double)c.x;
                q = ax * cx + (double)a.y * (double)c.y;
            } else {
                q = ax * ax + (double)a.y * (double)a.y;
            }
            nonfinite |= !(isfinite(a.x) && isfinite(a.y));
            const double kx = t.kx[i], ky = t.ky[j], kz = t.kz[l];
            double x;
            if (CYL) {
                x = fabs(kz);
                k1 = sqrt(kx * kx + ky * ky);
                k2 = x;
            } else {
                // binned on |k|^2 against the driver's thresholds: |k| = sqrt_rn(x) >= e exactly when x >= t(e),
                // so the bin does not depend on how the device rounds its square root
                x = (kx * kx + ky * ky) + kz * kz;
                k1 = sqrt(x);
            }
            // np.digitize (increasing edges): the number of edges <= x, less one
            int lo = 0, hi = nl + 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (edges[mid] <= x) lo = mid + 1;
                else hi = mid;
            }
            const int bin = lo - 1;
            bool use = bin >= 0 && bin < nl;
            if (t.ignore_zero_mode && row == 0 && l == 0) use = false;
            if (t.ignore_kpar_zero && l == 0) use = false;
            if (CUT && !CYL) {
                // fp64 + - x only, in the order the restatement (tests/power_stats_reference.py) writes them
                const double kz2 = kz * kz;
                if (t.use_mu && !(kz2 >= t.mu_min_sq * x && kz2 <= t.mu_max_sq * x)) use = false;
                if (t.use_wedge) {
                    const double a = fabs(kz) - t.wedge_buffer;
                    if (!(a >= 0.0 && a * a >= t.wedge_slope_sq * (kx * kx + ky * ky))) use = false;
                }
            }
            // out-of-range modes join the nearest bin's run with nothing to add: keys stay monotone along a row
            key = bin < 0 ? 0 : (bin >= nl ? nl - 1 : bin);
            if (use) {
                wt = (l == 0 || 2 * l == nz) ? 1 : 2;
                p = q * wt;
                if (VAR) pp = (q * q) * wt;
                k1 *= wt;
                k2 *= wt;
            } else {
                k1 = 0.0;
                k2 = 0.0;
            }
        }
        // segmented inclusive scan over runs of equal (row, key)
        const int comp = active ? rl * nl + key : -1;
        // every lane takes part in every shuffle: a shuffle under a short-circuit reads lanes that are off
        const int comp_prev = __shfl_up(comp, 1, 64), comp_next = __shfl_down(comp, 1, 64);
        int seg = (lane == 0 || comp_prev != comp) ? 1 : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const double po = __shfl_up(p, d, 64), k1o = __shfl_up(k1, d, 64);
            const double k2o = CYL ? __shfl_up(k2, d, 64) : 0.0;
            const double ppo = VAR ? __shfl_up(pp, d, 64) : 0.0;
            const int wo = __shfl_up(wt, d, 64), so = __shfl_up(seg, d, 64);
            if (lane >= d) {
                if (!seg) {
                    p = po + p;
                    k1 = k1o + k1;
                    if (CYL) k2 = k2o + k2;
                    if (VAR) pp = ppo + pp;
                    wt = wo + wt;
                }
                seg |= so;
            }
        }
        const bool last = active && (lane == 63 || comp_next != comp);
        const int rl0 = __shfl(rl, 0, 64);
        for (int rr = 0; rr < span; ++rr) {
            if (last && rl == rl0 + rr) {
                double *c = mine + key * NV;
                c[0] += p;
                c[1] += k1;
                if (CYL) c[2] += k2;
                if (VAR) c[NV - 2] += pp;
                c[NV - 1] += (double)wt;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (nonfinite) atomicOr(bad, 1);
    __syncthreads();
    double *out = partials + ((long long)b * t.n_wg + w) * (long long)(nl * NV);
    for (int q = threadIdx.x; q < nl * NV; q += kBlock) {
        double s = acc[q];
        for (int v = 1; v < kWaves; ++v) s += acc[v * nl * NV + q];
        out[q] = s;
    }
}

// totals[b][g nl + loc][v] = sum over the workgroups of group g of partials[b][w][loc][v]: one workgroup per
// (batch, bin); thread t sums workgroups t, t + 256, .. in order, then a fixed tree over the threads
template <int NV>
__global__ __launch_bounds__(kBlock) void power_sum_kernel(const double *__restrict__ partials,
                                                           double *__restrict__ totals, c21hip_power_tabs t,
                                                           long long n_dest) {
    __shared__ double red[NV][kBlock];
    const long long id = blockIdx.x;  // b * n_dest + d
    const long long b = id / n_dest;
    const int d = (int)(id - b * n_dest);
    const int nl = t.n_local, g = d / nl, loc = d - g * nl;
    double s[NV];
    for (int v = 0; v < NV; ++v) s[v] = 0.0;
    for (int w = t.group_wg[g] + (int)threadIdx.x; w < t.group_wg[g + 1]; w += kBlock) {
        const double *src = partials + (((long long)b * t.n_wg + w) * nl + loc) * NV;
        for (int v = 0; v < NV; ++v) s[v] += src[v];
    }
    for (int v = 0; v < NV; ++v) red[v][threadIdx.x] = s[v];
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
            for (int v = 0; v < NV; ++v) red[v][threadIdx.x] += red[v][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < NV) totals[id * NV + threadIdx.x] = red[threadIdx.x][0];
}

// means: power[b][d] = scale sum(w P) / sum(w), counts[b][d]; kmean[b][.] = |k| per bin, or k_perp per
// k_perp bin followed by k_par per k_par bin (cylindrical).  Empty bins are NaN.  VAR: var[b][d] = scale^2 (sum(w
// P^2) / sum(w) - (sum(w P) / sum(w))^2), the population variance of the per-mode power.
template <bool CYL, bool VAR>
__global__ __launch_bounds__(kBlock) void power_mean_kernel(const double *__restrict__ totals, double scale,
                                                            int n_groups, int nl, long long n_batch,
                                                            double *__restrict__ power, double *__restrict__ kmean,
                                                            double *__restrict__ var,
                                                            long long *__restrict__ counts) {
    constexpr int NV = C21HIP_POWER_NV(CYL, VAR);
    const long long n_dest = (long long)n_groups * nl, n_k = CYL ? n_groups + nl : nl;
    const long long per = n_dest + (CYL ? n_k : 0);
    const long long id = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (id >= per * n_batch) return;
    const long long b = id / per, o = id - b * per;
    const double *tb = totals + b * n_dest * NV;
    const double nan = __builtin_nan("");
    if (o < n_dest) {
        const double c = tb[o * NV + NV - 1];
        power[b * n_dest + o] = c > 0.0 ? tb[o * NV] / c * scale : nan;
        counts[b * n_dest + o] = (long long)c;
        if (VAR) {
            const double m1 = tb[o * NV] / c, m2 = tb[o * NV + NV - 2] / c;
            var[b * n_dest + o] = c > 0.0 ? (m2 - m1 * m1) * (scale * scale) : nan;
        }
        if (!CYL) kmean[b * n_k + o] = c > 0.0 ? tb[o * NV + 1] / c : nan;
        return;
    }
    // cylindrical axis means
    const long long a = o - n_dest;
    double s = 0.0, c = 0.0;
    if (a < n_groups) {
        for (int jj = 0; jj < nl; ++jj) {
            s += tb[(a * nl + jj) * NV + 1];
            c += tb[(a * nl + jj) * NV + NV - 1];
        }
    } else {
        const long long jj = a - n_groups;
        for (int ii = 0; ii < n_groups; ++ii) {
            s += tb[(ii * nl + jj) * NV + 2];
            c += tb[(ii * nl + jj) * NV + NV - 1];
        }
    }
    kmean[b * n_k + a] = c > 0.0 ? s / c : nan;
}
}  // namespace


extern "C" size_t c21hip_power_lds_bytes(int n_local, int cylindrical, int variance) {
    return sizeof(double) *
           ((size_t)n_local + 1 + (size_t)kWaves * (size_t)n_local * C21HIP_POWER_NV(cylindrical, variance));
}

extern "C" int c21hip_power_pack(const float *in, float *padded, int nx, int ny, int nz, long long row_pitch,
                                 const long long *offsets, int n_batch, double *rowsum, double *mean,
                                 const float *wrow, const float *wz, int *bad, void *stream) {
    if (nx < 1 || ny < 1 || nz < 1 || n_batch < 1 || row_pitch < nz || (wrow == nullptr) != (wz == nullptr)) {
        c21hip_set_error("power pack: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const long long per = (long long)nx * ny, rows = per * n_batch;
    const long long blocks = (rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(power_rowsum_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, in, rowsum,
                       per, rows, nz, row_pitch, offsets);
    hipLaunchKernelGGL(power_boxmean_kernel, dim3((unsigned)n_batch), dim3(kBlock), 0, (hipStream_t)stream, rowsum,
                       mean, per, 1.0 / ((double)per * (double)nz), wrow ? 0 : 1);
    if (wrow)
        hipLaunchKernelGGL(power_pack_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, in,
                           padded, per, rows, nz, row_pitch, offsets, mean, wrow, wz, bad);
    else
        hipLaunchKernelGGL(power_pack_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, in,
                           padded, per, rows, nz, row_pitch, offsets, mean, wrow, wz, bad);
    return launch_status("power pack");
}

namespace {
struct bin_args {
    dim3 grid;
    size_t lds;
    hipStream_t stream;
    const float2 *a, *c;
    long long batch_c;
    int ny, nz;
    const c21hip_power_tabs *t;
    const double *mean1, *mean2;
    double n_cells;
    double *partials;
    int *bad;
};

template <bool CYL, bool CROSS, bool VAR, bool CUT>
void launch_bin(const bin_args &g) {
    static bool attr_done = false;  // once per instantiation
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)power_bin_kernel<CYL, CROSS, VAR, CUT>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, C21HIP_POWER_MAX_LDS);
        attr_done = true;
    }
    hipLaunchKernelGGL((power_bin_kernel<CYL, CROSS, VAR, CUT>), g.grid, dim3(kBlock), g.lds, g.stream, g.a, g.c,
                       g.batch_c, g.ny, g.nz, *g.t, g.mean1, g.mean2, g.n_cells, g.partials, g.bad);
}

template <bool CYL, bool VAR, bool CUT>
void launch_bin_cross(const bin_args &g) {
    if (g.c) launch_bin<CYL, true, VAR, CUT>(g);
    else launch_bin<CYL, false, VAR, CUT>(g);
}
}  // namespace

extern "C" int c21hip_power_bin(const float *spec1, const float *spec2, int nx, int ny, int nz, int n_batch,
                                int cylindrical, int variance, const c21hip_power_tabs *t, const double *mean1,
                                const double *mean2, double *partials, int *bad, void *stream) {
    const size_t lds = c21hip_power_lds_bytes(t->n_local, cylindrical, variance);
    const bool cut = t->use_mu || t->use_wedge;
    if (nx < 2 || ny < 2 || nz < 2 || n_batch < 1 || t->n_local < 1 || lds > C21HIP_POWER_MAX_LDS ||
        n_batch > 65535 || (cut && cylindrical)) {
        c21hip_set_error("power bin: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    if (t->n_wg == 0) return 0;
    bin_args g;
    g.grid = dim3((unsigned)t->n_wg, (unsigned)n_batch);
    g.lds = lds;
    g.stream = (hipStream_t)stream;
    g.a = (const float2 *)spec1;
    g.c = (const float2 *)spec2;
    g.batch_c = (long long)nx * ny * (nz / 2 + 1);
    g.ny = ny;
    g.nz = nz;
    g.t = t;
    g.mean1 = mean1;
    g.mean2 = mean2;
    g.n_cells = (double)nx * (double)ny * (double)nz;
    g.partials = partials;
    g.bad = bad;
    if (cylindrical) {
        if (variance) launch_bin_cross<true, true, false>(g);
        else launch_bin_cross<true, false, false>(g);
    } else if (cut) {
        if (variance) launch_bin_cross<false, true, true>(g);
        else launch_bin_cross<false, false, true>(g);
    } else {
        if (variance) launch_bin_cross<false, true, false>(g);
        else launch_bin_cross<false, false, false>(g);
    }
    return launch_status("power bin");
}

extern "C" int c21hip_power_finish(const double *partials, double *totals, int n_batch, int cylindrical,
                                   int variance, const c21hip_power_tabs *t, double scale, double *power,
                                   double *kmean, double *var, long long *counts, void *stream) {
    const long long n_dest = (long long)t->n_groups * t->n_local;
    const hipStream_t s = (hipStream_t)stream;
    long long n = n_dest * n_batch;
    const int nv = C21HIP_POWER_NV(cylindrical, variance);
    if (nv == 5)
        hipLaunchKernelGGL(power_sum_kernel<5>, dim3((unsigned)n), dim3(kBlock), 0, s, partials, totals, *t, n_dest);
    else if (nv == 4)
        hipLaunchKernelGGL(power_sum_kernel<4>, dim3((unsigned)n), dim3(kBlock), 0, s, partials, totals, *t, n_dest);
    else
        hipLaunchKernelGGL(power_sum_kernel<3>, dim3((unsigned)n), dim3(kBlock), 0, s, partials, totals, *t, n_dest);
    int st = launch_status("power sum");
    if (st) return st;
    n = (n_dest + (cylindrical ? t->n_groups + t->n_local : 0)) * n_batch;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (cylindrical) {
        if (variance)
            hipLaunchKernelGGL((power_mean_kernel<true, true>), grid, dim3(kBlock), 0, s, totals, scale, t->n_groups,
                               t->n_local, (long long)n_batch, power, kmean, var, counts);
        else
            hipLaunchKernelGGL((power_mean_kernel<true, false>), grid, dim3(kBlock), 0, s, totals, scale, t->n_groups,
                               t->n_local, (long long)n_batch, power, kmean, var, counts);
    } else {
        if (variance)
            hipLaunchKernelGGL((power_mean_kernel<false, true>), grid, dim3(kBlock), 0, s, totals, scale, t->n_groups,
                               t->n_local, (long long)n_batch, power, kmean, var, counts);
        else
            hipLaunchKernelGGL((power_mean_kernel<false, false>), grid, dim3(kBlock), 0, s, totals, scale,
                               t->n_groups, t->n_local, (long long)n_batch, power, kmean, var, counts);
    }
    return launch_status("power mean");
}
