// bubble_kernels.hip -- mean-free-path bubble size distributions of boxes and lightcone chunks (Mesinger &
// Furlanetto 2007; the estimator is written down at c21cm_bubble_sizes_grids, its spec is
// tests/bubble_reference.py).
//   pack    threshold and pack: one bit per cell, every z-row padded to whole 64-bit words.  A wave reads 64
//           consecutive cells of a row (any offset, any pitch: plain coalesced loads) and its __ballot is the word;
//           the padding lanes vote 0.  One workgroup per chunk of 64 words of a box, which also leaves with the
//           chunk's set bits (a wave issues the loads of its 16 words before the first vote and stores the words
//           with one instruction).  The non-finite check rides along.  A 512^3 mask is 16 MiB: the walk stays in
//           the Infinity Cache;
//   rank    two launches: one workgroup per box scans the chunk counts (tiles of 1024 with a 64-bit carry) and
//           leaves n_sel; then one lane per word, a wave per chunk: a shuffle scan of the popcounts on top of the
//           chunk's offset gives the set bits before every word;
//   walk    one ray per lane at a time; a wave owns a run of rays and hands them to its lanes as they fall idle (see
//           the kernel).  The k-th selected cell is the word found by binary search over `prefix` and a 6-step
//           select inside it: exactly uniform, no rejection.  Then the bounded Amanatides-Woo loop in fp64, one mask
//           word read per step.  The histogram and the three counts go through 32-bit LDS counters flushed with
//           64-bit integer atomics: order-independent, so two calls give the same bytes.  A ray is keyed by (seed,
//           box, ray index) alone, so neither n_rays nor the launch shape moves a result.
// Compiled without FMA contraction (Makefile); plain fp64 + - * /, sqrt and one sincos per ray.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"
#include "philox.h"
#include "wave_bits.h"

namespace {
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = C21HIP_BUBBLE_CHUNK;
constexpr int kScanBlock = 1024;
constexpr int kRaysPerLane = 4;   // rays a walk wave owns, per lane (fewer when there are fewer rays than lanes)
constexpr int kWalkBlocks = 4096;  // longer runs per wave beyond this many workgroups per box (16 per CU)
constexpr int kRefill = 16;        // idle lanes of a wave before they are handed new rays
constexpr int kSteps = 4;          // steps between two looks at the idle lanes
static_assert(kChunk == 64, "the prefix pass gives a lane to every word of a chunk");
static_assert(kChunk % kWaves == 0, "the pack's waves share a chunk evenly");

int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c21hip_set_error("%s launch failed: %s", what, hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}

// workgroup (c, b): words [64 c, 64 c + 64) of box b, 16 per wave
__global__ __launch_bounds__(kBlock) void bubble_pack_kernel(const float *__restrict__ in, int nz, int W,
                                                             long long words_per_box, long long row_pitch,
                                                             const long long *__restrict__ offsets, double threshold,
                                                             int select_below, unsigned long long *__restrict__ mask,
                                                             int *__restrict__ chunk_sum, int n_chunks,
                                                             int *__restrict__ bad) {
    __shared__ int wave_sum[kWaves];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *src = in + offsets[b];
    unsigned long long *dst = mask + (long long)b * words_per_box;
    // the wave's 16 words: every load is issued before the first vote, and lane q stores word q
    constexpr int kPer = kChunk / kWaves;
    const long long g0 = (long long)blockIdx.x * kChunk + wave * kPer;
    long long row = g0 / W;
    int wi = (int)(g0 - row * W);
    float v[kPer];
    bool ok[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int l = wi * 64 + lane;
        ok[q] = g0 + q < words_per_box && l < nz;
        v[q] = ok[q] ? src[row * row_pitch + l] : 0.0f;
        if (++wi == W) {
            wi = 0;
            ++row;
        }
    }
    int count = 0, not_finite = 0;
    unsigned long long mine = 0ull;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        if (!isfinite(v[q])) not_finite = 1;
        const bool sel = ok[q] && (select_below ? (double)v[q] < threshold : (double)v[q] >= threshold);
        const unsigned long long word = __ballot(sel);
        if (lane == q) mine = word;
        count += __popcll(word);
    }
    if (lane < kPer && g0 + lane < words_per_box) dst[g0 + lane] = mine;
    if (not_finite) atomicOr(bad, 1);
    if (lane == 0) wave_sum[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_sum[w];
        chunk_sum[(long long)b * n_chunks + blockIdx.x] = s;
    }
}

// one workgroup per box: chunk_off[b][c] = the set bits of the chunks before c, stats[b][0] = all of them.  A tile
// of 1024 chunks holds at most 1024 x 4096 bits, so the scan inside a tile is in 32 bits and the carry in 64
__global__ __launch_bounds__(kScanBlock) void bubble_scan_kernel(const int *__restrict__ chunk_sum, int n_chunks,
                                                                 long long *__restrict__ chunk_off,
                                                                 long long *__restrict__ stats) {
    __shared__ int wave_tot[kScanBlock / 64];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int *src = chunk_sum + (long long)b * n_chunks;
    long long *dst = chunk_off + (long long)b * n_chunks;
    long long carry = 0;
    for (int base = 0; base < n_chunks; base += kScanBlock) {
        const int c = base + (int)threadIdx.x;
        const int v = c < n_chunks ? src[c] : 0;
        const int incl = wave_inclusive(v, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < kScanBlock / 64; ++w) {
            const int t = wave_tot[w];
            if (w < wave) before += t;
            tile += t;
        }
        if (c < n_chunks) dst[c] = carry + before + (incl - v);
        carry += tile;
        __syncthreads();
    }
    if (threadIdx.x == 0) stats[4 * (long long)b] = carry;
}

// a wave per chunk, a lane per word
__global__ __launch_bounds__(kBlock) void bubble_prefix_kernel(const unsigned long long *__restrict__ mask,
                                                               long long words_per_box,
                                                               const long long *__restrict__ chunk_off, int n_chunks,
                                                               long long *__restrict__ prefix) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * kWaves + wave;
    if (c >= n_chunks) return;
    const long long g = (long long)c * kChunk + lane;
    const bool in = g < words_per_box;
    const int v = in ? __popcll(mask[(long long)b * words_per_box + g]) : 0;
    const int incl = wave_inclusive(v, lane);
    if (in) prefix[(long long)b * words_per_box + g] = chunk_off[(long long)b * n_chunks + c] + (incl - v);
}

// One wave owns a contiguous run of rays and hands them to its lanes as they fall idle: ray lengths differ by orders
// of magnitude inside a wave, and a ray is keyed by its index alone, so which lane walks it, and when, changes no
// result.  Lanes are refilled together once kRefill of them are idle (a start costs about twenty dependent loads of the
// rank search, paid by the whole wave), then every live lane takes kSteps steps.
// dynamic LDS: edges[n_bins + 1] (double) | counters[n_bins + 3] (32 bits): the histogram, then ended, capped, escaped
__global__ __launch_bounds__(kBlock) void bubble_walk_kernel(c21hip_bubble_walk_args a) {
    extern __shared__ double lds[];
    const int nb = a.n_bins;
    double *edges = lds;
    unsigned int *cnt = (unsigned int *)(lds + nb + 1);
    for (int i = threadIdx.x; i <= nb; i += kBlock) edges[i] = a.edges[i];
    for (int i = threadIdx.x; i < nb + 3; i += kBlock) cnt[i] = 0u;
    __syncthreads();

    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int W = (a.nz + 63) / 64;
    const long long words = (long long)a.nx * a.ny * W;
    const unsigned long long *mask = a.mask + (long long)b * words;
    const long long *prefix = a.prefix + (long long)b * words;
    const long long n_sel = a.stats[4 * (long long)b];
    const long long out0 = (long long)b * a.n_rays;

    // the rays of this wave: [next, end)
    const long long n_waves = (long long)gridDim.x * kWaves;
    const long long per_wave = (a.n_rays + n_waves - 1) / n_waves;
    long long next = ((long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * per_wave;
    const long long end = next + per_wave < a.n_rays ? next + per_wave : a.n_rays;

    if (n_sel <= 0) {
        for (long long r = next + lane; r < end; r += 64) {
            if (a.lengths) a.lengths[out0 + r] = __builtin_nan("");
            if (a.flags) a.flags[out0 + r] = 255;
            if (a.starts) a.starts[out0 + r] = -1;
        }
        return;  // the counters stay zero
    }

    // a lane's ray, in scalars: nothing is indexed by the axis at run time
    bool active = false;
    long long r = 0, it = 0;
    int i0 = 0, i1 = 0, i2 = 0, s0 = 1, s1 = 1, s2 = 1;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, e0 = 0.0, e1 = 0.0, e2 = 0.0;
    for (;;) {
        const unsigned long long idle = __ballot(!active);
        if (idle) {  // uniform over the wave from here to the refill
            const bool all_idle = idle == ~0ull;
            if (next < end) {
                if (all_idle || __popcll(idle) >= kRefill) {
                    const long long mine = next + __popcll(idle & ((1ull << lane) - 1ull));
                    next += __popcll(idle);
                    if (!active && mine < end) {
                        r = mine;
                        uint32_t x[4];
                        double u_cell, u[3], u_mu, u_phi;
                        philox4x32_10_ctr((uint32_t)r, 0u, (uint32_t)b, 0u, a.seed, x);
                        philox_uniform_pair(x, &u_cell, &u[0]);
                        philox4x32_10_ctr((uint32_t)r, 1u, (uint32_t)b, 0u, a.seed, x);
                        philox_uniform_pair(x, &u[1], &u[2]);
                        philox4x32_10_ctr((uint32_t)r, 2u, (uint32_t)b, 0u, a.seed, x);
                        philox_uniform_pair(x, &u_mu, &u_phi);

                        // the k-th selected cell: the last word with prefix <= k (its successor's prefix is above k,
                        // so it holds a set bit), then the (k - prefix)-th set bit of it
                        long long k = (long long)(u_cell * (double)n_sel);
                        if (k > n_sel - 1) k = n_sel - 1;
                        long long lo = 0, hi = words;  // the first word with prefix > k lies in (lo, hi]; prefix[0] = 0
                        while (hi - lo > 1) {
                            const long long mid = lo + ((hi - lo) >> 1);
                            if (prefix[mid] <= k) lo = mid;
                            else hi = mid;
                        }
                        const long long row0 = lo / W;
                        int idx[3];
                        idx[0] = (int)(row0 / a.ny);
                        idx[1] = (int)(row0 - (long long)idx[0] * a.ny);
                        idx[2] = (int)(lo - row0 * W) * 64 + select_bit(mask[lo], (int)(k - prefix[lo]));
                        if (a.starts) a.starts[out0 + r] = row0 * a.nz + idx[2];

                        double d[3];
                        if (a.los) {
                            d[0] = 0.0;
                            d[1] = 0.0;
                            d[2] = u_mu >= 0.5 ? 1.0 : -1.0;
                        } else {
                            const double c = 2.0 * u_mu - 1.0;
                            const double s = sqrt(1.0 - c * c);
                            double sn, cs;
                            sincos(6.283185307179586 * u_phi, &sn, &cs);
                            d[0] = s * cs;
                            d[1] = s * sn;
                            d[2] = c;
                        }
                        double tmax[3], tdel[3];
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const double p0 = ((double)idx[q] + u[q]) * a.cell[q];
                            if (d[q] == 0.0) {
                                tmax[q] = INFINITY;
                                tdel[q] = INFINITY;
                            } else {
                                tmax[q] = ((double)(idx[q] + (d[q] > 0.0 ? 1 : 0)) * a.cell[q] - p0) / d[q];
                                tdel[q] = a.cell[q] / fabs(d[q]);
                            }
                        }
                        i0 = idx[0], i1 = idx[1], i2 = idx[2];
                        t0 = tmax[0], t1 = tmax[1], t2 = tmax[2];
                        e0 = tdel[0], e1 = tdel[1], e2 = tdel[2];
                        s0 = d[0] > 0.0 ? 1 : -1, s1 = d[1] > 0.0 ? 1 : -1, s2 = d[2] > 0.0 ? 1 : -1;
                        it = 0;
                        active = true;
                    }
                }
            } else if (all_idle) {
                break;
            }
        }
        for (int q = 0; q < kSteps; ++q) {
            if (!active) continue;
            int flag = -1;  // -1: the ray goes on
            double len = a.max_length;
            int ax = 0;
            double t = t0;
            if (t1 < t) {
                ax = 1;
                t = t1;
            }
            if (t2 < t) {
                ax = 2;
                t = t2;
            }
            if (it >= a.max_steps || !(t < a.max_length)) {
                flag = 1;  // a ray that uses up its steps counts as capped
            } else {
                ++it;
                const int na = ax == 0 ? a.nx : ax == 1 ? a.ny : a.nz;
                const int per = ax == 0 ? a.periodic[0] : ax == 1 ? a.periodic[1] : a.periodic[2];
                int v = ax == 0 ? i0 + s0 : ax == 1 ? i1 + s1 : i2 + s2;
                bool escaped = false;
                if (v < 0 || v >= na) {
                    if (per) v = v < 0 ? na - 1 : 0;
                    else escaped = true;
                }
                if (escaped) {
                    flag = 2;
                    len = t;
                } else {
                    if (ax == 0) i0 = v;
                    else if (ax == 1) i1 = v;
                    else i2 = v;
                    const unsigned long long word = mask[((long long)i0 * a.ny + i1) * W + (i2 >> 6)];
                    if (!((word >> (i2 & 63)) & 1ull)) {
                        flag = 0;
                        len = t;
                    } else if (ax == 0) {
                        t0 = t + e0;
                    } else if (ax == 1) {
                        t1 = t + e1;
                    } else {
                        t2 = t + e2;
                    }
                }
            }
            if (flag < 0) continue;
            active = false;
            if (a.lengths) a.lengths[out0 + r] = len;
            if (a.flags) a.flags[out0 + r] = (unsigned char)flag;
            atomicAdd(&cnt[nb + flag], 1u);
            if (flag == 0) {
                // np.digitize (increasing edges): the number of edges <= len, less one
                int lo_e = 0, hi_e = nb + 1;
                while (lo_e < hi_e) {
                    const int mid = (lo_e + hi_e) >> 1;
                    if (edges[mid] <= len) lo_e = mid + 1;
                    else hi_e = mid;
                }
                const int bin = lo_e - 1;
                if (bin >= 0 && bin < nb) atomicAdd(&cnt[bin], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb + 3; i += kBlock) {
        const unsigned int c = cnt[i];
        if (!c) continue;
        if (i < nb) atomicAdd(&a.hist[(long long)b * nb + i], (unsigned long long)c);
        else atomicAdd((unsigned long long *)&a.stats[4 * (long long)b + 1 + (i - nb)], (unsigned long long)c);
    }
}

bool shape_ok(int nx, int ny, int nz, int n_batch) {
    return nx >= 1 && ny >= 1 && nz >= 1 && (long long)nx * ny <= 0x7FFFFFFFll && n_batch >= 1 && n_batch <= 65535;
}

// chunks of one box, or -1 where they do not fit a launch
long long chunks_of(int nx, int ny, int nz, long long *words_per_box) {
    const long long words = (long long)nx * ny * ((nz + 63) / 64);
    *words_per_box = words;
    const long long chunks = (words + kChunk - 1) / kChunk;
    return chunks > 0x7FFFFFFFll ? -1 : chunks;
}
}  // namespace

extern "C" int c21hip_bubble_pack(const float *in, int nx, int ny, int nz, long long row_pitch,
                                  const long long *offsets, int n_batch, double threshold, int select_below,
                                  unsigned long long *mask, int *chunk_sum, int *bad, void *stream) {
    long long words = 0;
    const long long chunks = shape_ok(nx, ny, nz, n_batch) ? chunks_of(nx, ny, nz, &words) : -1;
    if (chunks < 0 || row_pitch < nz || !in || !offsets || !mask || !chunk_sum || !bad) {
        c21hip_set_error("bubble pack: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    hipLaunchKernelGGL(bubble_pack_kernel, dim3((unsigned)chunks, (unsigned)n_batch), dim3(kBlock), 0,
                       (hipStream_t)stream, in, nz, (nz + 63) / 64, words, row_pitch, offsets, threshold, select_below,
                       mask, chunk_sum, (int)chunks, bad);
    return launch_status("bubble pack");
}

extern "C" int c21hip_bubble_rank(const unsigned long long *mask, const int *chunk_sum, int nx, int ny, int nz,
                                  int n_batch, long long *chunk_off, long long *prefix, long long *stats,
                                  void *stream) {
    long long words = 0;
    const long long chunks = shape_ok(nx, ny, nz, n_batch) ? chunks_of(nx, ny, nz, &words) : -1;
    if (chunks < 0 || !mask || !chunk_sum || !chunk_off || !prefix || !stats) {
        c21hip_set_error("bubble rank: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    hipLaunchKernelGGL(bubble_scan_kernel, dim3((unsigned)n_batch), dim3(kScanBlock), 0, (hipStream_t)stream, chunk_sum,
                       (int)chunks, chunk_off, stats);
    int status = launch_status("bubble scan");
    if (status) return status;
    hipLaunchKernelGGL(bubble_prefix_kernel, dim3((unsigned)((chunks + kWaves - 1) / kWaves), (unsigned)n_batch),
                       dim3(kBlock), 0, (hipStream_t)stream, mask, words, chunk_off, (int)chunks, prefix);
    return launch_status("bubble prefix");
}

extern "C" int c21hip_bubble_walk(const c21hip_bubble_walk_args *a, void *stream) {
    if (!a || !shape_ok(a->nx, a->ny, a->nz, a->n_batch) || a->n_rays < 1 || a->n_rays > 0x7FFFFFFFll ||
        a->n_bins < 1 || a->n_bins > C21HIP_BUBBLE_MAX_BINS || a->max_steps < 1 || !a->mask || !a->prefix || !a->edges ||
        !a->hist || !a->stats) {
        c21hip_set_error("bubble walk: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    long long blocks = (a->n_rays + (long long)kBlock * kRaysPerLane - 1) / ((long long)kBlock * kRaysPerLane);
    if (blocks > kWalkBlocks) blocks = kWalkBlocks;
    const size_t lds = sizeof(double) * ((size_t)a->n_bins + 1) + sizeof(unsigned int) * ((size_t)a->n_bins + 3);
    hipLaunchKernelGGL(bubble_walk_kernel, dim3((unsigned)blocks, (unsigned)a->n_batch), dim3(kBlock), lds,
                       (hipStream_t)stream, *a);
    return launch_status("bubble walk");
}
