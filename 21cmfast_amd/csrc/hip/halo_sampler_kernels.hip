// halo_sampler_kernels.hip -- the halo sampler (SOURCE_MODEL = CHMF-SAMPLER) on MI355X.
//
// reference loops being replaced (src/py21cmfast/src/Stochasticity.c):
//   stoc_set_consts_cond                      :158-207
//   stoc_sample / _halo_sample / _mass_sample :260-276, 374-411, 663-718
//   fix_mass_sample, remove_random_halo       :321-369
//   sample_halo_grids / _progenitors          :761-1113  (with set_prop_rng :210-230 and
//   random_point_in_cell / _sphere, wrap_position, indexing.c:14-86)
//
// The reference walks the conditions serially per OpenMP thread because it consumes GSL streams in a
// data-dependent order and keeps a float[MAX_HALO_CELL] per condition.  Here:
//  * every random number is words of one Philox block whose counter is {draw index, purpose, condition},
//    so draw j of condition i is a pure function of (key, i, j) and can be made again;
//  * pass A samples and keeps four words per condition, pass B makes the same draws again and writes at
//    the condition's offset: no per-condition buffer;
//  * the reference's random removals (uniform, without replacement, until the total falls to the target)
//    remove the draws pi(0), pi(1), ... of a keyed permutation pi of the draw indices (a four-round Feistel
//    network on the next even number of bits, cycle-walked into [0, n)), so "was draw j removed" is
//    pi^-1(j) < r in pass B;
//  * the sums that decide control flow are 64-bit integers of the float-rounded masses in units of 1 Msun
//    (a float >= 2^24 is an integer: exact, associative), so one thread walking a condition and a wave
//    taking 64 draws at a time decide alike, bit for bit.
// Work split: a wave takes 64 consecutive conditions, one per lane; conditions that expect at least
// wave_threshold halos are then taken one after the other by the whole wave.
// Every loop is bounded: draws by the cap, removals by the draws made, the Poisson chunks by 64 uniforms
// each, the cycle walk by kWalkCap steps; a condition that hits a bound reports itself in *bad.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_grid.h"
#include "philox.h"

namespace {
constexpr int kBlock = C21HIP_HS_BLOCK;
constexpr int kWalkCap = 256;       // (3/4)^256: never reached by a working permutation
constexpr double kPoissonChunk = 8.; // Knuth's product method on pieces of the mean
constexpr int kChunkDraws = 64;      // uniforms a piece may use: P(Poisson(8) >= 63) < 1e-33

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                       \
            return C21CM_IO_ERROR;                                                      \
        }                                                                               \
    } while (0)

struct Params {
    c21cm_sample_halos_spec s;
    c21hip_hs_arrays a;
    uint64_t key;
    const double *nhalo, *mcoll, *sigma, *inv;
    float min_mass;
    int cap;
};

enum { K_NONE = 0, K_SINGLE = 1, K_NUMBER = 2, K_MASS = 3, K_BAD = 4 };
struct Cond {
    double M_cond, x, exp_N, exp_M;
    float single_mass;
    int kind;
};

__device__ __forceinline__ double delta_crit(int hmf, double sigma, double growthf) { // hmf.c:151-171
    if (hmf == C21CM_HMF_ST) {
        const double del = 1.686 / growthf;
        return (sqrt(0.73) * del * (1. + 0.34 * pow(sigma * sigma / (0.73 * del * del), 0.81))) * growthf;
    }
    return 1.686;
}

__device__ __forceinline__ double lerp1(const double *y, int n, double x_min, double x_width, double x) {
    int idx = (int)floor((x - x_min) / x_width);
    idx = idx > n - 2 ? n - 2 : idx;
    idx = idx < 0 ? 0 : idx;
    const double t = (x - (x_min + x_width * (double)idx)) / x_width;
    return y[idx] * (1 - t) + y[idx + 1] * t;
}

__device__ Cond cond_setup(const Params &p, uint64_t i) {
    const c21cm_sample_halos_spec &s = p.s;
    Cond c;
    c.kind = K_NONE;
    c.M_cond = c.x = c.exp_N = c.exp_M = 0.;
    c.single_mass = 0.f;
    if (i >= p.a.n_cond) return c;
    double sigma, delta;
    if (s.from_catalog) {
        const double M = (double)p.a.cond_masses[i];
        if (!(M >= s.m_min && M <= s.m_max_tables)) { // Stochasticity.c:1002-1008
            c.kind = K_BAD;
            return c;
        }
        c.M_cond = M;
        c.x = log(M);
        sigma = lerp1(p.sigma, s.n_cond, s.x_min, s.x_width, c.x);
        delta = delta_crit(s.hmf, sigma, s.growth_in) / s.growth_in * s.growth_out;
    } else {
        c.M_cond = s.m_cell;
        sigma = s.sigma_cell;
        delta = p.a.cells_listed ? (double)p.a.density[i] : (double)p.a.density[i] * s.growth_out;
        if (!(fabs(delta) <= 1e30)) {
            c.kind = K_BAD;
            return c;
        }
        c.x = delta;
    }
    const double dcrit = delta_crit(s.hmf, sigma, s.growth_out);
    const double limit = (double)(float)0.99 * dcrit; // MAX_DELTAC_FRAC, hmf.h:8
    if (delta > limit) {
        c.exp_M = c.M_cond;
        c.exp_N = 1.;
    } else if (delta <= -1. || c.M_cond < s.m_min) {
        c.exp_M = c.exp_N = 0.;
    } else {
        c.exp_N = lerp1(p.nhalo, s.n_cond, s.x_min, s.x_width, c.x) * c.M_cond;
        c.exp_M = lerp1(p.mcoll, s.n_cond, s.x_min, s.x_width, c.x) * c.M_cond;
    }
    if (!s.from_catalog && p.a.overlap) {
        const double keep = 1. - (double)p.a.overlap[i];
        c.exp_M *= keep;
        c.exp_N *= keep;
    }
    // stoc_sample, :663-718
    if (delta <= -1.) return c;
    if (delta >= limit) {
        c.kind = K_SINGLE;
        c.single_mass = (float)c.exp_M;
        return c;
    }
    if (s.sample_method == 1 || !s.from_catalog) {
        c.kind = c.exp_N > 0. ? K_NUMBER : K_NONE;
        return c;
    }
    c.exp_M *= s.halomass_correction; // stoc_mass_sample, :374-411
    if (!(c.exp_M > 0.)) return c;
    if (sigma * 7. * s.growth_out < dcrit) {
        c.kind = K_SINGLE;
        c.single_mass = (float)c.exp_M;
        return c;
    }
    c.kind = K_MASS;
    return c;
}

__device__ __forceinline__ void block_of(const Params &p, uint64_t i, int purpose, uint32_t j, uint32_t (&x)[4]) {
    philox4x32_10_ctr(j, (uint32_t)purpose, (uint32_t)i, (uint32_t)(i >> 32), p.key, x);
}

__device__ __forceinline__ double uniform_of(const Params &p, uint64_t i, int purpose, uint32_t j) {
    uint32_t x[4];
    block_of(p, i, purpose, j, x);
    double u1, u2;
    philox_uniform_pair(x, &u1, &u2);
    return u1;
}

// sample_dndM_inverse (:64-74) on draw j: EvaluateNhaloInv (interp_tables.c:1085-1092, the indices
// clamped into the table) times the condition mass, rounded to float as the reference stores it
__device__ float draw_mass(const Params &p, const Cond &c, uint64_t i, uint32_t j) {
    const c21cm_sample_halos_spec &s = p.s;
    double lnp = log(uniform_of(p, i, C21CM_HS_DRAW_MASS, j));
    if (lnp < s.p_min) lnp = s.p_min;
    const int nx = s.n_cond, ny = s.n_prob;
    int xi = (int)floor((c.x - s.x_min) / s.x_width), yi = (int)floor((lnp - s.p_min) / s.p_width);
    xi = xi > nx - 2 ? nx - 2 : xi;
    xi = xi < 0 ? 0 : xi;
    yi = yi > ny - 2 ? ny - 2 : yi;
    yi = yi < 0 ? 0 : yi;
    const double tx = (c.x - (s.x_min + s.x_width * (double)xi)) / s.x_width;
    const double ty = (lnp - (s.p_min + s.p_width * (double)yi)) / s.p_width;
    const double *z = p.inv + (size_t)xi * ny + yi;
    const double left = z[0] * (1 - ty) + z[1] * ty;
    const double right = z[ny] * (1 - ty) + z[ny + 1] * ty;
    double r = left * (1 - tx) + right * tx;
    r = fmin(1., fmax(0., r));
    return (float)(r * c.M_cond);
}

__device__ __forceinline__ long long mass_units(float m) { return llrint((double)m); } // 1 Msun

// ---- the keyed permutation of [0, n)
struct Perm {
    uint32_t k[4];
    uint32_t n, half_bits, mask;
};

__device__ Perm perm_setup(const Params &p, uint64_t i, uint32_t n) {
    Perm q;
    block_of(p, i, C21CM_HS_DRAW_PERMUTE, 0u, q.k);
    q.n = n;
    uint32_t bits = n > 1 ? 32 - __clz(n - 1) : 1;
    q.half_bits = (bits + 1) / 2;
    q.mask = (1u << q.half_bits) - 1u;
    return q;
}

__device__ __forceinline__ uint32_t perm_round(uint32_t v, uint32_t key, uint32_t mask) {
    v = v * 0x9E3779B1u + key;
    v ^= v >> 15;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    return v & mask;
}

__device__ uint32_t perm_forward(const Perm &q, uint32_t x, bool *bad) {
    if (q.n <= 1) return 0;
    for (int walk = 0; walk < kWalkCap; walk++) {
        uint32_t a = x >> q.half_bits, b = x & q.mask;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t t = a ^ perm_round(b, q.k[r], q.mask);
            a = b;
            b = t;
        }
        x = (a << q.half_bits) | b;
        if (x < q.n) return x;
    }
    *bad = true;
    return 0;
}

__device__ uint32_t perm_inverse(const Perm &q, uint32_t x, bool *bad) {
    if (q.n <= 1) return 0;
    for (int walk = 0; walk < kWalkCap; walk++) {
        uint32_t a = x >> q.half_bits, b = x & q.mask;
#pragma unroll
        for (int r = 3; r >= 0; r--) {
            const uint32_t t = b ^ perm_round(a, q.k[r], q.mask);
            b = a;
            a = t;
        }
        x = (a << q.half_bits) | b;
        if (x < q.n) return x;
    }
    *bad = true;
    return 0;
}

// ---- wave helpers (64 lanes)
__device__ __forceinline__ long long shfl_ll(long long v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src);
    return (long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ long long shfl_up_ll(long long v, int d) {
    const int lo = __shfl_up((int)(uint32_t)v, d), hi = __shfl_up((int)(uint32_t)((uint64_t)v >> 32), d);
    return (long long)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ long long wave_inclusive_scan(long long v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = shfl_up_ll(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ unsigned long long lanes_upto(int lane) { // lanes 0 .. lane
    return lane >= 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
}

struct Result {
    uint32_t kept, drawn, removed; // removed carries C21HIP_HS_DROP_LAST
    int bad;
};

// ---- Poisson count: the mean in pieces of kPoissonChunk, Knuth's product of uniforms on each; piece c uses the
// uniforms c * kChunkDraws + k.  Returns the count of one piece.
__device__ int poisson_piece(const Params &p, uint64_t i, uint32_t piece, double mean, int *bad) {
    const double limit = exp(-mean);
    double prod = 1.;
    for (int k = 0; k < kChunkDraws; k++) {
        prod *= uniform_of(p, i, C21CM_HS_DRAW_POISSON, piece * (uint32_t)kChunkDraws + (uint32_t)k);
        if (prod <= limit) return k;
    }
    *bad = C21HIP_HS_BAD_DRAWS;
    return 0;
}
__device__ __forceinline__ uint32_t poisson_pieces(double mean) { return (uint32_t)ceil(mean / kPoissonChunk); }
__device__ __forceinline__ double piece_mean(double mean, uint32_t piece, uint32_t n_pieces) {
    return piece + 1 < n_pieces ? kPoissonChunk : mean - kPoissonChunk * (double)(n_pieces - 1);
}

// ---- pass A, one thread per condition
__device__ Result sample_thread(const Params &p, const Cond &c, uint64_t i) {
    Result r = {0u, 0u, 0u, 0};
    if (c.kind == K_BAD) {
        r.bad = C21HIP_HS_BAD_MASS;
    } else if (c.kind == K_SINGLE) {
        r.drawn = 1;
        r.kept = !(c.single_mass < p.min_mass);
    } else if (c.kind == K_NUMBER) {
        if (!(c.exp_N <= kPoissonChunk * (double)p.cap)) {
            r.bad = C21HIP_HS_BAD_DRAWS;
            return r;
        }
        const uint32_t n_pieces = poisson_pieces(c.exp_N);
        uint32_t nh = 0;
        for (uint32_t piece = 0; piece < n_pieces && !r.bad && nh <= (uint32_t)p.cap; piece++)
            nh += (uint32_t)poisson_piece(p, i, piece, piece_mean(c.exp_N, piece, n_pieces), &r.bad);
        if (!r.bad && nh > (uint32_t)p.cap) r.bad = C21HIP_HS_BAD_DRAWS;
        if (r.bad) return r;
        r.drawn = nh;
        for (uint32_t j = 0; j < nh; j++) r.kept += !(draw_mass(p, c, i, j) < p.min_mass);
    } else if (c.kind == K_MASS) {
        const long long t_ceil = (long long)ceil(c.exp_M), t_floor = (long long)floor(c.exp_M);
        long long tot = 0, q_last = 0;
        uint32_t n = 0;
        bool last_kept = false;
        while (tot < t_ceil) { // M_prog < exp_M on integers
            if (n >= (uint32_t)p.cap) {
                r.bad = C21HIP_HS_BAD_DRAWS;
                return r;
            }
            const float m = draw_mass(p, c, i, n++);
            q_last = mass_units(m);
            tot += q_last;
            last_kept = !(m < p.min_mass);
            r.kept += last_kept;
        }
        r.drawn = n;
        // fix_mass_sample, :341-369
        if (uniform_of(p, i, C21CM_HS_DRAW_SELECT, 0u) >= 0.5) {
            if (fabs((double)(tot - q_last) - c.exp_M) < fabs((double)tot - c.exp_M)) {
                r.removed = C21HIP_HS_DROP_LAST;
                r.kept -= last_kept;
            }
        } else {
            const Perm q = perm_setup(p, i, n);
            bool walk_bad = false;
            uint32_t removed = 0;
            long long q_del = 0;
            bool del_kept = false;
            do {
                const float m = draw_mass(p, c, i, perm_forward(q, removed++, &walk_bad));
                q_del = mass_units(m);
                tot -= q_del;
                del_kept = !(m < p.min_mass);
                r.kept -= del_kept;
            } while (tot > t_floor && removed < n); // M_tot > exp_M on integers
            if (fabs((double)(tot + q_del) - c.exp_M) < fabs((double)tot - c.exp_M)) {
                removed--; // the last one goes back: the removed draws are pi(0 .. removed - 1)
                r.kept += del_kept;
            }
            r.removed = removed;
            if (walk_bad) r.bad = C21HIP_HS_BAD_WALK;
        }
    }
    return r;
}

// ---- pass A, one wave per condition (all 64 lanes call it with the same c, i); every lane returns the result
__device__ Result sample_wave(const Params &p, const Cond &c, uint64_t i, int lane) {
    Result r = {0u, 0u, 0u, 0};
    if (c.kind == K_NUMBER) {
        if (!(c.exp_N <= kPoissonChunk * (double)p.cap)) {
            r.bad = C21HIP_HS_BAD_DRAWS;
            return r;
        }
        const uint32_t n_pieces = poisson_pieces(c.exp_N);
        int bad = 0;
        uint32_t mine = 0;
        for (uint32_t piece = (uint32_t)lane; piece < n_pieces; piece += 64)
            mine += (uint32_t)poisson_piece(p, i, piece, piece_mean(c.exp_N, piece, n_pieces), &bad);
        const uint32_t nh = (uint32_t)shfl_ll(wave_inclusive_scan((long long)mine, lane), 63);
        if (__any(bad) || nh > (uint32_t)p.cap) {
            r.bad = C21HIP_HS_BAD_DRAWS;
            return r;
        }
        r.drawn = nh;
        uint32_t kept = 0;
        for (uint32_t j = (uint32_t)lane; j < nh; j += 64) kept += !(draw_mass(p, c, i, j) < p.min_mass);
        r.kept = (uint32_t)shfl_ll(wave_inclusive_scan((long long)kept, lane), 63);
        return r;
    }
    if (c.kind != K_MASS) return sample_thread(p, c, i); // nothing to share: every lane does the same little
    const long long t_ceil = (long long)ceil(c.exp_M), t_floor = (long long)floor(c.exp_M);
    long long tot = 0, q_last = 0;
    uint32_t n = 0;
    bool last_kept = false;
    for (uint32_t base = 0;; base += 64) {
        if (base >= (uint32_t)p.cap) {
            r.bad = C21HIP_HS_BAD_DRAWS;
            return r;
        }
        const uint32_t j = base + (uint32_t)lane;
        const bool live = j < (uint32_t)p.cap;
        const float m = live ? draw_mass(p, c, i, j) : 0.f;
        const long long q = live ? mass_units(m) : 0;
        const bool keep = live && !(m < p.min_mass);
        const long long run = tot + wave_inclusive_scan(q, lane);
        const unsigned long long over = __ballot(live && run >= t_ceil);
        const unsigned long long keeps = __ballot(keep);
        if (over) {
            const int L = __ffsll((long long)over) - 1;
            n = base + (uint32_t)L + 1;
            tot = shfl_ll(run, L);
            q_last = shfl_ll(q, L);
            last_kept = (keeps >> L) & 1ull;
            r.kept += (uint32_t)__popcll(keeps & lanes_upto(L));
            break;
        }
        if (base + 64 >= (uint32_t)p.cap) { // the cap's last draws did not reach the target
            r.bad = C21HIP_HS_BAD_DRAWS;
            return r;
        }
        tot = shfl_ll(run, 63);
        r.kept += (uint32_t)__popcll(keeps);
    }
    r.drawn = n;
    if (uniform_of(p, i, C21CM_HS_DRAW_SELECT, 0u) >= 0.5) {
        if (fabs((double)(tot - q_last) - c.exp_M) < fabs((double)tot - c.exp_M)) {
            r.removed = C21HIP_HS_DROP_LAST;
            r.kept -= last_kept;
        }
        return r;
    }
    const Perm perm = perm_setup(p, i, n);
    bool walk_bad = false;
    uint32_t removed = 0;
    long long q_del = 0;
    bool del_kept = false;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool live = k < n;
        const float m = live ? draw_mass(p, c, i, perm_forward(perm, k, &walk_bad)) : 0.f;
        const long long q = live ? mass_units(m) : 0;
        const bool keep = live && !(m < p.min_mass);
        const long long run = tot - wave_inclusive_scan(q, lane);
        const unsigned long long done = __ballot(live && !(run > t_floor));
        const unsigned long long keeps = __ballot(keep);
        int L = 63;
        if (done) L = __ffsll((long long)done) - 1;
        else if (base + 64 >= n) L = (int)(n - 1 - base); // every draw removed
        if (done || base + 64 >= n) {
            removed = base + (uint32_t)L + 1;
            tot = shfl_ll(run, L);
            q_del = shfl_ll(q, L);
            del_kept = (keeps >> L) & 1ull;
            r.kept -= (uint32_t)__popcll(keeps & lanes_upto(L));
            break;
        }
        tot = shfl_ll(run, 63);
        r.kept -= (uint32_t)__popcll(keeps);
    }
    if (fabs((double)(tot + q_del) - c.exp_M) < fabs((double)tot - c.exp_M)) {
        removed--;
        r.kept += del_kept;
    }
    r.removed = removed;
    if (__any(walk_bad)) r.bad = C21HIP_HS_BAD_WALK;
    return r;
}

__device__ __forceinline__ bool takes_wave(const Params &p, const Cond &c) {
    return (c.kind == K_NUMBER || c.kind == K_MASS) && c.exp_N >= p.a.wave_threshold;
}

__global__ void __launch_bounds__(kBlock)
hs_pass_a_kernel(Params p, unsigned int *__restrict__ words, unsigned long long *__restrict__ block_sums,
                 unsigned long long *__restrict__ bad) {
    __shared__ unsigned int scan[kBlock];
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const Cond c = cond_setup(p, i);
    const bool wave = takes_wave(p, c);
    Result mine = {0u, 0u, 0u, 0};
    if (!wave) mine = sample_thread(p, c, i);
    unsigned long long heavy = __ballot(wave);
    while (heavy) { // the same for all lanes of the wave
        const int L = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const uint64_t iw = i - (uint64_t)lane + (uint64_t)L;
        const Cond cw = cond_setup(p, iw);
        const Result rw = sample_wave(p, cw, iw, lane);
        if (lane == L) mine = rw;
    }
    if (mine.bad) atomicMin(bad, (unsigned long long)((i << 3) | (uint64_t)mine.bad));
    const unsigned int kept = mine.bad ? 0u : mine.kept;
    // exclusive scan of the block's kept counts: the row of a condition inside its block
    scan[threadIdx.x] = kept;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const unsigned int t = threadIdx.x >= d ? scan[threadIdx.x - d] : 0u;
        __syncthreads();
        scan[threadIdx.x] += t;
        __syncthreads();
    }
    if (i < p.a.n_cond) {
        words[4 * i + 0] = kept;
        words[4 * i + 1] = mine.drawn;
        words[4 * i + 2] = mine.removed;
        words[4 * i + 3] = scan[threadIdx.x] - kept;
    }
    if (threadIdx.x == kBlock - 1) block_sums[blockIdx.x] = scan[kBlock - 1];
}

// exclusive scan of n values by one workgroup, in place; the total to *total
__global__ void __launch_bounds__(1024)
hs_scan_kernel(unsigned long long *__restrict__ v, unsigned long long n, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[1024];
    const unsigned long long per = (n + 1023) / 1024;
    const unsigned long long lo = per * threadIdx.x, hi = lo + per < n ? lo + per : n;
    unsigned long long sum = 0;
    for (unsigned long long k = lo; k < hi; k++) sum += v[k];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long t = threadIdx.x >= d ? part[threadIdx.x - d] : 0ull;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - sum;
    for (unsigned long long k = lo; k < hi; k++) {
        const unsigned long long t = v[k];
        v[k] = run;
        run += t;
    }
    if (threadIdx.x == 1023) *total = part[1023];
}

struct Outputs {
    float *masses, *coords, *star, *sfr, *xray;
};

// one kept halo: draw j of condition i with mass m goes to `row`
__device__ void write_halo(const Params &p, const Cond &c, uint64_t i, uint32_t j, float m, uint64_t row,
                           const Outputs &o) {
    const c21cm_sample_halos_spec &s = p.s;
    uint32_t x[4];
    double u1, u2, u3, u4;
    block_of(p, i, C21CM_HS_DRAW_POSITION, j, x);
    philox_uniform_pair(x, &u1, &u2);
    block_of(p, i, C21CM_HS_DRAW_POSITION2, j, x);
    philox_uniform_pair(x, &u3, &u4);
    double pos[3];
    const double size[3] = {s.box_len, s.box_len, s.box_len_z};
    if (s.from_catalog) { // random_point_in_sphere, indexing.c:60-71
        const double x1 = 2 * u1 - 1, y1 = 2 * u2 - 1, z1 = 2 * u3 - 1;
        const double d1 = sqrt(x1 * x1 + y1 * y1 + z1 * z1);
        const double R2 = pow(c.M_cond / s.rtom_unit, 1. / 3.), R1 = pow((double)m / s.rtom_unit, 1. / 3.);
        const double radius = R2 - R1;
        pos[0] = (double)p.a.cond_coords[3 * i + 0] + (radius * u4 * x1 / d1);
        pos[1] = (double)p.a.cond_coords[3 * i + 1] + (radius * u4 * y1 / d1);
        pos[2] = (double)p.a.cond_coords[3 * i + 2] + (radius * u4 * z1 / d1);
    } else { // random_point_in_cell, indexing.c:73-86
        const uint64_t nz = (uint64_t)s.hii_dim_z, ny = (uint64_t)s.hii_dim;
        const double cell = s.box_len / s.hii_dim;
        double idx[3] = {(double)(i / (nz * ny)), (double)((i / nz) % ny), (double)(i % nz)};
        if (p.a.cells_listed)
            for (int a = 0; a < 3; a++)
                idx[a] = (double)(int)((double)p.a.cond_coords[3 * i + a] / s.box_len * s.hii_dim);
        pos[0] = (idx[0] + (u1 - 0.5)) * cell;
        pos[1] = (idx[1] + (u2 - 0.5)) * cell;
        pos[2] = (idx[2] + (u3 - 0.5)) * cell;
    }
    for (int a = 0; a < 3; a++) { // wrap_position, bounded
        for (int k = 0; k < 4 && pos[a] >= size[a]; k++) pos[a] -= size[a];
        for (int k = 0; k < 4 && pos[a] < 0; k++) pos[a] += size[a];
        // a descendant far outside the box: one modulo brings what the bounded steps left over inside
        if (!(pos[a] >= 0 && pos[a] < size[a])) pos[a] -= size[a] * floor(pos[a] / size[a]);
        float f = (float)pos[a];
        if (!(f >= 0.f && f < (float)size[a])) f = 0.f; // rounded up onto the far face, or not a number
        o.coords[3 * row + a] = f;
    }
    double g0, g1, g2, g3; // set_prop_rng, :210-230
    block_of(p, i, C21CM_HS_DRAW_PROPS, j, x);
    philox_gaussian_pair(x, &g0, &g1);
    block_of(p, i, C21CM_HS_DRAW_PROPS2, j, x);
    philox_gaussian_pair(x, &g2, &g3);
    if (s.from_catalog) {
        g0 = sqrt(1 - s.corr_star * s.corr_star) * g0 + s.corr_star * (double)p.a.cond_star[i];
        g1 = sqrt(1 - s.corr_sfr * s.corr_sfr) * g1 + s.corr_sfr * (double)p.a.cond_sfr[i];
        g2 = sqrt(1 - s.corr_xray * s.corr_xray) * g2 + s.corr_xray * (double)p.a.cond_xray[i];
    }
    o.masses[row] = m;
    o.star[row] = (float)g0;
    o.sfr[row] = (float)g1;
    o.xray[row] = (float)g2;
}

__device__ __forceinline__ bool draw_stays(const Params &p, const Perm &q, uint32_t j, uint32_t drawn,
                                           uint32_t removed, float m) {
    if ((removed & C21HIP_HS_DROP_LAST) && j + 1 == drawn) return false;
    const uint32_t r = removed & ~C21HIP_HS_DROP_LAST;
    bool bad = false;
    if (r && perm_inverse(q, j, &bad) < r) return false;
    return !(m < p.min_mass);
}

__global__ void __launch_bounds__(kBlock)
hs_pass_b_kernel(Params p, const unsigned int *__restrict__ words, const unsigned long long *__restrict__ block_bases,
                 unsigned long long first_row, Outputs o) {
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < p.a.n_cond;
    const Cond c = cond_setup(p, i);
    const uint32_t kept = live ? words[4 * i] : 0u, drawn = live ? words[4 * i + 1] : 0u;
    const uint32_t removed = live ? words[4 * i + 2] : 0u;
    const uint64_t row0 = first_row + block_bases[blockIdx.x] + (live ? words[4 * i + 3] : 0u);
    const bool wave = takes_wave(p, c);
    if (!wave && kept) {
        uint64_t row = row0;
        const uint64_t end = row0 + kept;
        if (c.kind == K_SINGLE) {
            write_halo(p, c, i, 0u, c.single_mass, row, o);
        } else {
            const Perm q = perm_setup(p, i, drawn);
            for (uint32_t j = 0; j < drawn && row < end; j++) {
                const float m = draw_mass(p, c, i, j);
                if (draw_stays(p, q, j, drawn, removed, m)) write_halo(p, c, i, j, m, row++, o);
            }
        }
    }
    unsigned long long heavy = __ballot(wave && kept);
    while (heavy) {
        const int L = __ffsll((long long)heavy) - 1;
        heavy &= heavy - 1;
        const uint64_t iw = i - (uint64_t)lane + (uint64_t)L;
        const Cond cw = cond_setup(p, iw);
        const uint32_t drawn_w = (uint32_t)__shfl((int)drawn, L), removed_w = (uint32_t)__shfl((int)removed, L);
        const uint32_t kept_w = (uint32_t)__shfl((int)kept, L);
        uint64_t row = (uint64_t)shfl_ll((long long)row0, L);
        const uint64_t end = row + kept_w;
        const Perm q = perm_setup(p, iw, drawn_w);
        for (uint32_t base = 0; base < drawn_w; base += 64) {
            const uint32_t j = base + (uint32_t)lane;
            const float m = j < drawn_w ? draw_mass(p, cw, iw, j) : 0.f;
            const bool stays = j < drawn_w && draw_stays(p, q, j, drawn_w, removed_w, m);
            const unsigned long long mask = __ballot(stays);
            const uint64_t mine = row + (uint64_t)__popcll(mask & (lanes_upto(lane) >> 1));
            if (stays && mine < end) write_halo(p, cw, iw, j, m, mine, o);
            row += (uint64_t)__popcll(mask);
        }
    }
}

Params make_params(const c21cm_sample_halos_spec *s, const c21hip_hs_arrays *a) {
    Params p;
    p.s = *s;
    p.a = *a;
    p.key = (uint64_t)s->seed + (uint64_t)(s->redshift * 1000);
    const size_t nx = (size_t)s->n_cond;
    p.nhalo = a->tables;
    p.mcoll = a->tables + nx;
    p.sigma = a->tables + 2 * nx;
    p.inv = a->tables + 3 * nx;
    p.min_mass = (float)s->sampler_min_mass;
    p.cap = s->max_halo_cell > 0 && s->max_halo_cell < C21CM_MAX_HALO_CELL ? s->max_halo_cell : C21CM_MAX_HALO_CELL;
    return p;
}
}  // namespace

extern "C" int c21hip_hs_pass_a(const c21cm_sample_halos_spec *s, const c21hip_hs_arrays *a, unsigned int *words,
                                unsigned long long *block_sums, unsigned long long *bad, void *stream) {
    if (!a->n_cond) return 0;
    const unsigned long long nb = (a->n_cond + kBlock - 1) / kBlock;
    if (nb > 0x7fffffffull) {
        c21hip_set_error("halo sampler: %llu conditions are more than one launch takes", a->n_cond);
        return C21CM_VALUE_ERROR;
    }
    hipLaunchKernelGGL(hs_pass_a_kernel, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, make_params(s, a),
                       words, block_sums, bad);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_hs_scan(unsigned long long *block_sums, unsigned long long n_blocks, unsigned long long *total,
                              void *stream) {
    hipLaunchKernelGGL(hs_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, block_sums, n_blocks, total);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_hs_pass_b(const c21cm_sample_halos_spec *s, const c21hip_hs_arrays *a, const unsigned int *words,
                                const unsigned long long *block_bases, unsigned long long first_row, float *masses,
                                float *coords, float *star, float *sfr, float *xray, void *stream) {
    if (!a->n_cond) return 0;
    const unsigned long long nb = (a->n_cond + kBlock - 1) / kBlock;
    const Outputs o = {masses, coords, star, sfr, xray};
    hipLaunchKernelGGL(hs_pass_b_kernel, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)stream, make_params(s, a),
                       words, block_bases, first_row, o);
    LAUNCH_CHECK();
    return 0;
}
