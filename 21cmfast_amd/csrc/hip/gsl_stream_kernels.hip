// gsl_stream_kernels.hip -- the reference's initial-condition random streams drawn on the device
// (host restatement and layouts: csrc/host/gsl_stream.c; reference: rng.c:31-90 seed_rng_threads,
// InitialConditions.c:103-139 two gsl_ran_ugaussian per mode).
//
// What looks serial in a stream is the polar method's acceptance loop, and that is a stream compaction:
// drop the zero words, pair the survivors, keep the pairs with 0 < x^2 + y^2 <= 1; deviate i comes from
// the i-th kept pair.  One workgroup of 256 lanes owns one stream and works tile by tile:
//   fill     the word source writes the next tile of raw outputs into LDS
//              mt19937   the 624-word state in LDS, twice over; a block is three dependent sub-steps of
//                        227, 227 and 170 words from the old copy into the new one; tempering on the way out
//              gfsr4     the 2^14-word ring in LDS; the 471 words of a step only read older ones
//              cmrg, mrg, taus2   lane t owns C21_GSL_RUN consecutive outputs of a tile and keeps the state at
//                        the start of its run; the next tile's is that state times A^(256 RUN) (a 3x3 or 5x5
//                        matrix modulo the prime, three 32x32 matrices over GF(2): tables from the host)
//              memory    caller-supplied words (c21cm_gsl_accept_pairs)
//   compact  a lane takes E consecutive words; a prefix over the non-zero counts gives every survivor its
//            index behind the word the tile before left unpaired; a lane then takes EP consecutive pairs,
//            computes r2 with the host's fp64 operations and a second prefix over the keep flags gives the
//            output index.  Only accepted pairs reach HBM, 8 B per deviate.
// The accepted count, the carry word and the stop position live in LDS, so every branch of the tile loop
// is uniform over the workgroup.  A launch ends at the stream's count, after max_pairs accepted pairs
// (then the pair that reaches the limit names the word behind it, and the state saved is the one after
// exactly that word: results do not depend on max_pairs) or at the tile cap, which is an error.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRun = C21_GSL_RUN;
constexpr int kTileJump = kBlock * kRun;  // words per tile of cmrg, mrg, taus2 and of words in memory
constexpr int kTileMax = kTileJump;
constexpr int kGenLds = 16384;  // words of generator state in LDS: the gfsr4 ring is the largest
constexpr int kCtlWords = 16;
constexpr int kLdsWords = kGenLds + kTileMax + 2 * (kTileMax + 1) + kCtlWords;

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                       \
            return C21CM_IO_ERROR;                                                      \
        }                                                                               \
    } while (0)

struct Ctl {
    unsigned long long accepted;
    uint32_t carry_has, carry_word;
    int stop_m;  // words of the tile consumed when the limit was reached, -1 otherwise
    int pad;
    int ws_a[kWaves], ws_b[kWaves];
};
static_assert(sizeof(Ctl) <= kCtlWords * 4, "Ctl");

// exclusive prefix of v over the workgroup; `ws` is one of Ctl's wave-sum arrays (one barrier)
__device__ inline int block_scan(int v, int *ws, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(inc, d, 64);
        if (lane >= d) inc += n;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const int x = ws[w];
        if (w < wave) off += x;
        total += x;
    }
    return off + inc - v;
}

// ---- word sources ----------------------------------------------------------------------------------
// load(state, lds, jump)  take the stream's generator state
// fill(s_w)               the next tile into LDS, returns its length (uniform); ends with a barrier
// next(nw)                the stream consumed the whole tile
// save(state, m)          store the state after m words of the tile filled last
// last()                  no tile follows (words in memory only)

struct MtSource {
    static constexpr int kTile = 624;
    static constexpr bool kDiv31 = false;
    uint32_t *x;
    int cur, pos;
    __device__ void load(const uint32_t *st, uint32_t *lds, const uint32_t *) {
        x = lds;
        cur = 0;
        pos = __builtin_amdgcn_readfirstlane((int)st[0]);
        for (int i = threadIdx.x; i < 624; i += kBlock) x[i] = st[1 + i];
        __syncthreads();
    }
    static __device__ uint32_t twist(uint32_t a, uint32_t b, uint32_t far) {
        const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
        return far ^ (y >> 1) ^ (0x9908b0dfu & (0u - (y & 1u)));
    }
    __device__ int fill(uint32_t *s_w) {
        if (pos == 624) {
            // mt_refill: x[i] = x[(i + 397) % 624] ^ f(x[i], x[(i + 1) % 624]) for i = 0 .. 623 in turn, so
            // i < 227 reads old words only, 227 <= i < 454 reads the new words [0, 227), the rest the new
            // words [227, 397), and i = 623 the new x[0]
            const uint32_t *o = x + cur * 624;
            uint32_t *n = x + (cur ^ 1) * 624;
            for (int i = threadIdx.x; i < 227; i += kBlock) n[i] = twist(o[i], o[i + 1], o[i + 397]);
            __syncthreads();
            for (int i = 227 + threadIdx.x; i < 454; i += kBlock) n[i] = twist(o[i], o[i + 1], n[i - 227]);
            __syncthreads();
            for (int i = 454 + threadIdx.x; i < 624; i += kBlock)
                n[i] = twist(o[i], i == 623 ? n[0] : o[i + 1], n[i - 227]);
            __syncthreads();
            cur ^= 1;
            pos = 0;
        }
        const int nw = 624 - pos;
        const uint32_t *s = x + cur * 624 + pos;
        for (int i = threadIdx.x; i < nw; i += kBlock) {
            uint32_t k = s[i];
            k ^= k >> 11;
            k ^= (k << 7) & 0x9d2c5680u;
            k ^= (k << 15) & 0xefc60000u;
            k ^= k >> 18;
            s_w[i] = k;
        }
        __syncthreads();
        return nw;
    }
    __device__ void next(int nw) { pos += nw; }
    __device__ bool last() const { return false; }
    __device__ void save(uint32_t *st, int m) {
        if (threadIdx.x == 0) st[0] = (uint32_t)(pos + m);
        for (int i = threadIdx.x; i < 624; i += kBlock) st[1 + i] = x[cur * 624 + i];
    }
};

struct GfsrSource {
    static constexpr int kTile = 471;
    static constexpr bool kDiv31 = false;
    uint32_t *r;
    int nd;
    __device__ void load(const uint32_t *st, uint32_t *lds, const uint32_t *) {
        r = lds;
        nd = __builtin_amdgcn_readfirstlane((int)st[0]) & 16383;
        for (int i = threadIdx.x; i < 16384; i += kBlock) r[i] = st[1 + i];
        __syncthreads();
    }
    __device__ int fill(uint32_t *s_w) {
        // word nd + 1 + i reads the words 471, 1586, 6988 and 9689 behind it: for i < 471 all of them are at or
        // before nd, and no slot written here is one that is read (the ring is longer than 9689 + 471)
        for (int i = threadIdx.x; i < 471; i += kBlock) {
            const int p = nd + 1 + i;
            const uint32_t v = r[(p - 471) & 16383] ^ r[(p - 1586) & 16383] ^ r[(p - 6988) & 16383] ^
                               r[(p - 9689) & 16383];
            r[p & 16383] = v;
            s_w[i] = v;
        }
        __syncthreads();
        return 471;
    }
    __device__ void next(int nw) { nd = (nd + nw) & 16383; }
    __device__ bool last() const { return false; }
    // the words written beyond nd + m are the ones the next launch computes there again
    __device__ void save(uint32_t *st, int m) {
        if (threadIdx.x == 0) st[0] = (uint32_t)((nd + m) & 16383);
        for (int i = threadIdx.x; i < 16384; i += kBlock) st[1 + i] = r[i];
    }
};

// (sum over j of a[j] s[j]) mod m; every product is reduced before it is added (5 products of 2^62 overflow)
template <int N>
__device__ inline uint32_t row_mod(const uint32_t *a, const uint32_t *s, uint64_t m) {
    uint64_t acc = 0;
#pragma unroll
    for (int j = 0; j < N; j++) acc += ((uint64_t)a[j] * s[j]) % m;
    return (uint32_t)(acc % m);
}

struct CmrgGen {
    static constexpr int kWords = 6, kJump = C21_GSL_JUMP_CMRG, kMat = 18;
    static constexpr bool kDiv31 = true;
    static __device__ uint32_t step(uint32_t *s) {  // cmrg_get
        const int64_t m1 = 2147483647, m2 = 2145483479;
        int64_t t = (63308 * (int64_t)s[1] - 183326 * (int64_t)s[2]) % m1;
        if (t < 0) t += m1;
        s[2] = s[1], s[1] = s[0], s[0] = (uint32_t)t;
        t = (86098 * (int64_t)s[3] - 539608 * (int64_t)s[5]) % m2;
        if (t < 0) t += m2;
        s[5] = s[4], s[4] = s[3], s[3] = (uint32_t)t;
        return s[0] < s[3] ? (uint32_t)(s[0] - s[3] + 2147483647u) : s[0] - s[3];
    }
    static __device__ void apply(const uint32_t *mat, uint32_t *s) {
        uint32_t r[6];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r[i] = row_mod<3>(mat + 3 * i, s, 2147483647u);
            r[3 + i] = row_mod<3>(mat + 9 + 3 * i, s + 3, 2145483479u);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) s[i] = r[i];
    }
};

struct MrgGen {
    static constexpr int kWords = 5, kJump = C21_GSL_JUMP_MRG, kMat = 25;
    static constexpr bool kDiv31 = true;
    static __device__ uint32_t step(uint32_t *s) {  // mrg_get
        const int64_t m = 2147483647;
        const int64_t t = (107374182 * (int64_t)s[0] + 104480 * (int64_t)s[4]) % m;
        s[4] = s[3], s[3] = s[2], s[2] = s[1], s[1] = s[0], s[0] = (uint32_t)t;
        return s[0];
    }
    static __device__ void apply(const uint32_t *mat, uint32_t *s) {
        uint32_t r[5];
#pragma unroll
        for (int i = 0; i < 5; i++) r[i] = row_mod<5>(mat + 5 * i, s, 2147483647u);
#pragma unroll
        for (int i = 0; i < 5; i++) s[i] = r[i];
    }
};

struct Taus2Gen {
    static constexpr int kWords = 3, kJump = C21_GSL_JUMP_TAUS2, kMat = 96;
    static constexpr bool kDiv31 = false;
    static __device__ uint32_t step(uint32_t *s) {  // taus2_get
#define TAUSWORTHE(s, a, b, c, d) ((((s) & (c)) << (d)) ^ ((((s) << (a)) ^ (s)) >> (b)))
        s[0] = TAUSWORTHE(s[0], 13, 19, 4294967294u, 12);
        s[1] = TAUSWORTHE(s[1], 2, 25, 4294967288u, 4);
        s[2] = TAUSWORTHE(s[2], 3, 11, 4294967280u, 17);
#undef TAUSWORTHE
        return s[0] ^ s[1] ^ s[2];
    }
    static __device__ void apply(const uint32_t *mat, uint32_t *s) {  // column c of a component's matrix: image of bit c
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint32_t r = 0;
            for (int c = 0; c < 32; c++) r ^= mat[32 * k + c] & (0u - ((s[k] >> c) & 1u));
            s[k] = r;
        }
    }
};

template <class G>
struct JumpSource {
    static constexpr int kTile = kTileJump;
    static constexpr bool kDiv31 = G::kDiv31;
    uint32_t s0[G::kWords];  // the state before this lane's run of the current tile
    const uint32_t *jump;
    __device__ void load(const uint32_t *st, uint32_t *, const uint32_t *jump_all) {
        jump = jump_all + G::kJump;
#pragma unroll
        for (int i = 0; i < G::kWords; i++) s0[i] = st[i];
        // lane t starts t runs into the tile: A^(RUN 2^j) for every bit j of t
        for (int j = 0; j < 8; j++)
            if ((threadIdx.x >> j) & 1) G::apply(jump + j * G::kMat, s0);
    }
    __device__ int fill(uint32_t *s_w) {
        uint32_t s[G::kWords];
#pragma unroll
        for (int i = 0; i < G::kWords; i++) s[i] = s0[i];
#pragma unroll
        for (int k = 0; k < kRun; k++) s_w[threadIdx.x * kRun + k] = G::step(s);
        __syncthreads();
        return kTile;
    }
    __device__ void next(int) { G::apply(jump + 8 * G::kMat, s0); }
    __device__ bool last() const { return false; }
    __device__ void save(uint32_t *st, int m) {
        if (m == kTile) {
            if (threadIdx.x == 0) {
                G::apply(jump + 8 * G::kMat, s0);
                for (int i = 0; i < G::kWords; i++) st[i] = s0[i];
            }
        } else if ((int)threadIdx.x == m / kRun) {
            for (int k = 0; k < m % kRun; k++) (void)G::step(s0);
            for (int i = 0; i < G::kWords; i++) st[i] = s0[i];
        }
    }
};

template <bool DIV31>
struct MemSource {
    static constexpr int kTile = kTileMax;
    static constexpr bool kDiv31 = DIV31;
    const uint32_t *words;
    size_t n_words, base;
    int nw_last;
    __device__ int fill(uint32_t *s_w) {
        const size_t left = n_words - base;
        const int nw = left < (size_t)kTile ? (int)left : kTile;
        for (int i = threadIdx.x; i < nw; i += kBlock) s_w[i] = words[base + i];
        __syncthreads();
        nw_last = nw;
        return nw;
    }
    __device__ void next(int nw) { base += nw; }
    __device__ bool last() const { return base + nw_last >= n_words; }
};

// ---- one tile through the polar method --------------------------------------------------------------
template <int TILE, bool DIV31>
__device__ inline void compact_tile(const uint32_t *s_w, int nw, uint32_t *surv, uint32_t *spos, Ctl *ctl,
                                    unsigned long long *out, unsigned long long limit) {
    constexpr int E = (TILE + kBlock - 1) / kBlock;
    constexpr int EP = ((TILE + 1) / 2 + kBlock - 1) / kBlock;
    const int t = threadIdx.x;
    const unsigned long long acc = ctl->accepted;
    const uint32_t carry_has = ctl->carry_has, carry_word = ctl->carry_word;

    uint32_t w[E];
    int nz = 0;
#pragma unroll
    for (int k = 0; k < E; k++) {
        const int i = t * E + k;
        w[k] = i < nw ? s_w[i] : 0u;
        nz += w[k] != 0u;
    }
    int total;
    int s = (int)carry_has + block_scan(nz, ctl->ws_a, total);
#pragma unroll
    for (int k = 0; k < E; k++)
        if (w[k]) {
            surv[s] = w[k];
            spos[s] = (uint32_t)(t * E + k);
            ++s;
        }
    if (t == 0 && carry_has) surv[0] = carry_word;
    const int n_surv = (int)carry_has + total;
    __syncthreads();

    const int n_pairs = n_surv >> 1;
    uint32_t pa[EP], pc[EP];
    unsigned keep = 0;
    int n_keep = 0;
#pragma unroll
    for (int k = 0; k < EP; k++) {
        const int p = t * EP + k;
        pa[k] = pc[k] = 0;
        if (p < n_pairs) {
            pa[k] = surv[2 * p];
            pc[k] = surv[2 * p + 1];
            // raw_to_uniform, x = 2 u - 1, r2 = x x + y y: the host's operations one by one
            const double ua = DIV31 ? (double)pa[k] / 2147483647.0 : __dmul_rn((double)pa[k], 1.0 / 4294967296.0);
            const double uc = DIV31 ? (double)pc[k] / 2147483647.0 : __dmul_rn((double)pc[k], 1.0 / 4294967296.0);
            const double x = __dadd_rn(__dmul_rn(2.0, ua), -1.0), y = __dadd_rn(__dmul_rn(2.0, uc), -1.0);
            const double r2 = __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
            if (!(r2 > 1.0 || r2 == 0)) {
                keep |= 1u << k;
                ++n_keep;
            }
        }
    }
    int kept;
    unsigned long long idx = acc + (unsigned long long)block_scan(n_keep, ctl->ws_b, kept);
#pragma unroll
    for (int k = 0; k < EP; k++)
        if ((keep >> k) & 1u) {
            if (idx < limit) {
                out[idx] = (unsigned long long)pa[k] | ((unsigned long long)pc[k] << 32);
                if (idx + 1 == limit) ctl->stop_m = (int)spos[2 * (t * EP + k) + 1] + 1;
            }
            ++idx;
        }
    if (t == 0) {
        if (acc + (unsigned long long)kept >= limit) {
            ctl->accepted = limit;  // the pairs behind the limit are drawn again by the next launch
            ctl->carry_has = 0;
        } else {
            ctl->accepted = acc + (unsigned long long)kept;
            ctl->carry_has = (uint32_t)(n_surv & 1);
            if (n_surv & 1) ctl->carry_word = surv[n_surv - 1];
        }
    }
    __syncthreads();
}

struct TileLds {
    uint32_t *s_w, *surv, *spos;
    Ctl *ctl;
};
__device__ inline TileLds carve(uint32_t *tile_lds) {  // behind the generator's words, if any
    TileLds l;
    l.s_w = tile_lds;
    l.surv = l.s_w + kTileMax;
    l.spos = l.surv + kTileMax + 1;
    l.ctl = reinterpret_cast<Ctl *>(l.spos + kTileMax + 1);
    return l;
}

// The tile loop.  Returns 1 when it ended at the tile cap.  m_out: words of the last tile the stream consumed.
template <class Src>
__device__ inline int tile_loop(Src &src, const TileLds &l, unsigned long long *out, unsigned long long limit,
                                long cap, int &m_out) {
    for (long tiles = 1;; ++tiles) {
        const int nw = src.fill(l.s_w);
        compact_tile<Src::kTile, Src::kDiv31>(l.s_w, nw, l.surv, l.spos, l.ctl, out, limit);
        const bool done = l.ctl->accepted >= limit;
        if (done || tiles >= cap || src.last()) {
            m_out = done ? l.ctl->stop_m : nw;
            return !done && !src.last();
        }
        src.next(nw);
    }
}

template <class Src>
__device__ inline void draw_stream(uint32_t *lds, uint32_t *rec, const uint32_t *jump, unsigned long long *out,
                                   unsigned long long count, unsigned long long max_pairs, long tile_cap,
                                   int *flag) {
    const TileLds l = carve(lds + kGenLds);
    const unsigned long long acc0 = (unsigned long long)rec[0] | ((unsigned long long)rec[1] << 32);
    if (acc0 >= count || rec[4]) return;  // done, or failed in an earlier launch
    const unsigned long long limit = count - acc0 < max_pairs ? count : acc0 + max_pairs;
    // expected 2 * 4 / pi = 2.55 words per pair: four times that, and four tiles for short ones
    const long cap = tile_cap > 0 ? tile_cap : (long)((limit - acc0) * 11 / Src::kTile) + 4;
    if (threadIdx.x == 0) {
        l.ctl->accepted = acc0;
        l.ctl->carry_has = rec[2];
        l.ctl->carry_word = rec[3];
        l.ctl->stop_m = -1;
    }
    Src src;
    src.load(rec + C21_GSL_HDR, lds, jump);
    __syncthreads();
    int m;
    const int capped = tile_loop(src, l, out, limit, cap, m);
    src.save(rec + C21_GSL_HDR, m);
    if (threadIdx.x == 0) {
        const unsigned long long acc = l.ctl->accepted;
        rec[0] = (uint32_t)acc;
        rec[1] = (uint32_t)(acc >> 32);
        rec[2] = l.ctl->carry_has;
        rec[3] = l.ctl->carry_word;
        if (capped) {
            rec[4] = 1;
            *flag = 1;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
gsl_stream_draw_kernel(const c21_gsl_stream_desc *__restrict__ desc, uint32_t *state, const uint32_t *jump,
                       unsigned long long *out, unsigned long long max_pairs, long tile_cap, int *flag) {
    __shared__ alignas(16) uint32_t lds[kLdsWords];
    const c21_gsl_stream_desc d = desc[blockIdx.x];
    uint32_t *rec = state + d.state_offset;
    unsigned long long *o = out + d.out_offset;
    switch (d.kind) {  // uniform over the workgroup
        case 0: draw_stream<MtSource>(lds, rec, jump, o, d.count, max_pairs, tile_cap, flag); break;
        case 1: draw_stream<GfsrSource>(lds, rec, jump, o, d.count, max_pairs, tile_cap, flag); break;
        case 2: draw_stream<JumpSource<CmrgGen>>(lds, rec, jump, o, d.count, max_pairs, tile_cap, flag); break;
        case 3: draw_stream<JumpSource<MrgGen>>(lds, rec, jump, o, d.count, max_pairs, tile_cap, flag); break;
        default: draw_stream<JumpSource<Taus2Gen>>(lds, rec, jump, o, d.count, max_pairs, tile_cap, flag); break;
    }
}

// the compaction alone: the same tile loop over words in memory, one workgroup
template <bool DIV31>
__global__ void __launch_bounds__(kBlock)
gsl_accept_kernel(const uint32_t *__restrict__ words, size_t n_words, unsigned long long want,
                  unsigned long long *out, unsigned long long *result) {
    __shared__ alignas(16) uint32_t lds[kLdsWords - kGenLds];
    const TileLds l = carve(lds);
    if (threadIdx.x == 0) {
        l.ctl->accepted = 0;
        l.ctl->carry_has = 0;
        l.ctl->carry_word = 0;
        l.ctl->stop_m = -1;
    }
    __syncthreads();
    unsigned long long found = 0, used = 0;
    if (want > 0 && n_words > 0) {
        MemSource<DIV31> src;
        src.words = words;
        src.n_words = n_words;
        src.base = 0;
        src.nw_last = 0;
        int m;
        (void)tile_loop(src, l, out, want, (long)(n_words / kTileMax) + 2, m);
        found = l.ctl->accepted;
        used = found >= want ? src.base + (size_t)m : n_words;
    }
    if (threadIdx.x == 0) {
        result[0] = found;
        result[1] = used;
    }
}

template <class Src>
__device__ inline void raw_words(uint32_t *lds, const uint32_t *st, const uint32_t *jump, size_t n, uint32_t *out) {
    uint32_t *s_w = lds + kGenLds;
    Src src;
    src.load(st, lds, jump);
    __syncthreads();
    for (size_t done = 0; done < n;) {
        const int nw = src.fill(s_w);
        for (int i = threadIdx.x; i < nw && done + i < n; i += kBlock) out[done + i] = s_w[i];
        __syncthreads();
        src.next(nw);
        done += nw;
    }
}

__global__ void __launch_bounds__(kBlock)
gsl_raw_words_kernel(int kind, const uint32_t *__restrict__ st, const uint32_t *__restrict__ jump, size_t n,
                     uint32_t *out) {
    __shared__ alignas(16) uint32_t lds[kGenLds + kTileMax];
    switch (kind) {
        case 0: raw_words<MtSource>(lds, st, jump, n, out); break;
        case 1: raw_words<GfsrSource>(lds, st, jump, n, out); break;
        case 2: raw_words<JumpSource<CmrgGen>>(lds, st, jump, n, out); break;
        case 3: raw_words<JumpSource<MrgGen>>(lds, st, jump, n, out); break;
        default: raw_words<JumpSource<Taus2Gen>>(lds, st, jump, n, out); break;
    }
}

}  // namespace

extern "C" int c21hip_gsl_tile_words(int kind) {
    return kind == 0 ? MtSource::kTile : kind == 1 ? GfsrSource::kTile : kTileJump;
}

extern "C" int c21hip_gsl_stream_draw(const void *desc_dev, int n_streams, unsigned int *state_dev,
                                      const unsigned int *jump_dev, unsigned long long *pairs_dev,
                                      unsigned long long max_pairs, long tile_cap, int *flag_dev, void *stream) {
    if (n_streams < 1) return 0;
    hipLaunchKernelGGL(gsl_stream_draw_kernel, dim3(n_streams), dim3(kBlock), 0, (hipStream_t)stream,
                       (const c21_gsl_stream_desc *)desc_dev, state_dev, jump_dev, pairs_dev, max_pairs, tile_cap,
                       flag_dev);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_gsl_accept_pairs(int kind, const unsigned int *words_dev, size_t n_words, size_t want,
                                       unsigned long long *pairs_dev, unsigned long long *result_dev, void *stream) {
    if (kind == 2 || kind == 3)
        hipLaunchKernelGGL(gsl_accept_kernel<true>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, words_dev, n_words,
                           (unsigned long long)want, pairs_dev, result_dev);
    else
        hipLaunchKernelGGL(gsl_accept_kernel<false>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, words_dev, n_words,
                           (unsigned long long)want, pairs_dev, result_dev);
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_gsl_raw_words(int kind, const unsigned int *state_dev, const unsigned int *jump_dev, size_t n,
                                    unsigned int *out_dev, void *stream) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(gsl_raw_words_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, kind, state_dev, jump_dev,
                       n, out_dev);
    LAUNCH_CHECK();
    return 0;
}
