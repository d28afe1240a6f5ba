/*
 * gsl_stream.c -- the reference's initial-condition random stream, for "same seed, same universe".
 *
 * reference call sites:
 *   src/py21cmfast/src/rng.c:31-90                  seed_rng_threads(r, random_seed)
 *   src/py21cmfast/src/InitialConditions.c:103-139  sample_ic_modes: per mode two
 *       gsl_ran_ugaussian(r[omp_get_thread_num()]) inside `#pragma omp for` over n_x
 *
 * The generators are GSL's, a dependency of the reference that is neither in its tree nor in
 * this image; they are written here from their published definitions:
 *   mt19937  Matsumoto & Nishimura (1998) with the 2002 seeding recurrence
 *            x_i = 1812433253 (x_{i-1} ^ (x_{i-1} >> 30)) + i, seed 0 meaning 4357
 *   gfsr4    Ziff (1998): x_n = x_{n-471} ^ x_{n-1586} ^ x_{n-6988} ^ x_{n-9689} on 2^14 words,
 *            filled bit by bit from the top bit of the LCG x -> 69069 x (mod 2^32), 32 words
 *            forced to a unit upper-triangular pattern, first output at position 33
 *   uniform = word / 2^32; uniform_pos rejects 0; uniform_int(n) = word / (0xffffffff / n),
 *            rejecting values >= n
 *   choose   selection sampling: item i of n is taken with probability (k - taken)/(n - i)
 *   shuffle  Fisher-Yates from the last element down, swapping with uniform_int(i + 1)
 *   ugaussian  polar method: (x, y) = 2 u_pos - 1 until 0 < x^2 + y^2 <= 1, value
 *            y sqrt(-2 ln r2 / r2); the pair's other value is discarded
 *   cmrg     L'Ecuyer (1996) combined multiple recursive generator: two order-3 recurrences
 *            modulo 2147483647 and 2145483479 (multipliers 63308, -183326 / 86098, -539608, each
 *            step by Schrage's decomposition), output (x - y) mod m1; seeded from the LCG
 *            x -> 69069 x (mod 2^32), seven warm-up steps; uniform = value / 2147483647
 *   mrg      L'Ecuyer, Blouin & Couture (1993) order-5 recurrence modulo 2147483647
 *            (multipliers 107374182 and 104480), same seeding, six warm-up steps
 *   taus2    L'Ecuyer (1996/1999) three-component Tausworthe generator with the 1999 seeding
 *            (components forced >= 2, 8, 16), six warm-up steps; uniform = value / 2^32
 *   GSL's own self-test values (rng/test.c: the 10000th output for seed 1 is 719452880 for cmrg,
 *   2064828650 for mrg, 2733957125 for taus2) are reproduced (the generator tests under tests/).
 * Thread t of seed_rng_threads cycles through mt19937, gfsr4, cmrg, mrg, taus2 (rng.c:58-85), so
 * any N_THREADS reproduces upstream; the reference's fixtures pin the first two
 * (tests/produce_integration_test_data.py:62,213-220), the other three rest on GSL's self-test
 * values.  A mode belongs to the
 * thread that owns its n_x under the default static OpenMP schedule (contiguous blocks, the
 * first DIM % N_THREADS threads one row longer).
 *
 * The number of words a deviate consumes depends on the words themselves, but that does not make a
 * thread's stream serial: the polar method is a stream compaction (drop the zero words, pair the
 * survivors, keep the pairs with 0 < r2 <= 1; deviate i is the i-th kept pair), and all five generators
 * have parallel structure (227 / 471 independent words per step of mt19937 / gfsr4, matrix powers for
 * the three linear recurrences).  Three ways to draw the streams follow from that:
 *   c21_gsl_mode_deviates            everything on the host, one OpenMP thread per stream
 *   c21_gsl_mode_deviates_device     the acceptance loop on the host, its accepted raw pairs staged over
 *                                    PCIe, ln and sqrt on the device (the default of C21CM_RNG_GSL)
 *   c21_gsl_mode_deviates_ondevice   the streams drawn on the device, one workgroup per stream
 *                                    (gsl_stream_kernels.hip; C21CM_RNG_GSL_DEVICE): the same accepted
 *                                    pairs, then the same ln / sqrt kernel
 * The device then applies sqrt(V P(k) / 2) and the Hermitian constraints (ics_kernels.hip:
 * sample_modes_kernel).
 * Parity: bit-identical deviates to the CPU oracle's independent restatement
 * (tests/test_gpu_ics.py), which the reference's own HDF5 fixtures pin
 * (tests/test_reference_fixtures.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"

/* ---- word sources: both fill a block of raw 32-bit outputs at a time ------------------- */
typedef struct word_source {
    uint32_t *buf;
    int pos, len;
    void (*refill)(struct word_source *);
    /* mt19937 */
    uint32_t mt[624];
    /* gfsr4 */
    uint32_t *ring;
    int nd;
    /* cmrg (x1..x3, y1..y3), mrg (x1..x5), taus2 (s1..s3) */
    int kind; /* which generator steps: -1 for caller-supplied words */
    int unit; /* whose raw-to-uniform scale applies (= kind for a generator) */
    int eof;  /* caller-supplied words: they ran out */
    long int lx[6];
    uint32_t ts[3];
} word_source;

/* ---- the three generators without a block structure ------------------------------------ */
/* (Both recurrences in 64-bit arithmetic: the products stay below 2^59, and the reductions by the
 * constant moduli compile to multiplications.  GSL steps them by Schrage's decomposition in 32-bit
 * longs; the residues are the same numbers -- GSL's self-test values and the oracle's independent
 * restatement pin them -- at a third of the time: 22 -> 7 ns per output, which matters because the
 * slowest of the N_THREADS streams sets the wall time of the IC draw.) */
static unsigned long cmrg_get(word_source *w) {
    const int64_t m1 = 2147483647, m2 = 2145483479;
    long int *x = w->lx, *y = w->lx + 3;
    { /* component 1: x_n = 63308 x_{n-2} - 183326 x_{n-3} (mod m1) */
        int64_t t = (63308 * (int64_t)x[1] - 183326 * (int64_t)x[2]) % m1;
        if (t < 0) t += m1;
        x[2] = x[1], x[1] = x[0], x[0] = (long int)t;
    }
    { /* component 2: y_n = 86098 y_{n-1} - 539608 y_{n-3} (mod m2) */
        int64_t t = (86098 * (int64_t)y[0] - 539608 * (int64_t)y[2]) % m2;
        if (t < 0) t += m2;
        y[2] = y[1], y[1] = y[0], y[0] = (long int)t;
    }
    return x[0] < y[0] ? (unsigned long)(x[0] - y[0] + m1) : (unsigned long)(x[0] - y[0]);
}

static unsigned long mrg_get(word_source *w) {
    /* x_n = 107374182 x_{n-1} + 104480 x_{n-5} (mod 2^31 - 1) */
    const int64_t m = 2147483647;
    long int *x = w->lx;
    const int64_t t = (107374182 * (int64_t)x[0] + 104480 * (int64_t)x[4]) % m;
    x[4] = x[3], x[3] = x[2], x[2] = x[1], x[1] = x[0], x[0] = (long int)t;
    return (unsigned long)x[0];
}

static unsigned long taus2_get(word_source *w) {
#define TAUSWORTHE(s, a, b, c, d) ((((s) & (c)) << (d)) ^ ((((s) << (a)) ^ (s)) >> (b)))
    uint32_t *s = w->ts;
    s[0] = TAUSWORTHE(s[0], 13, 19, 4294967294u, 12);
    s[1] = TAUSWORTHE(s[1], 2, 25, 4294967288u, 4);
    s[2] = TAUSWORTHE(s[2], 3, 11, 4294967280u, 17);
#undef TAUSWORTHE
    return s[0] ^ s[1] ^ s[2];
}



static void mt_refill(word_source *w) {
    uint32_t *x = w->mt;
    for (int i = 0; i < 624; i++) {
        const uint32_t y = (x[i] & 0x80000000u) | (x[(i + 1) % 624] & 0x7fffffffu);
        x[i] = x[(i + 397) % 624] ^ (y >> 1) ^ (0x9908b0dfu & (0u - (y & 1u)));
    }
    for (int i = 0; i < 624; i++) { /* tempering */
        uint32_t k = x[i];
        k ^= k >> 11;
        k ^= (k << 7) & 0x9d2c5680u;
        k ^= (k << 15) & 0xefc60000u;
        k ^= k >> 18;
        w->buf[i] = k;
    }
    w->pos = 0;
    w->len = 624;
}

static void gfsr4_refill(word_source *w) {
    uint32_t *r = w->ring;
    int nd = w->nd;
    for (int i = 0; i < 624; i++) {
        nd = (nd + 1) & 16383;
        r[nd] = r[(nd + 16384 - 471) & 16383] ^ r[(nd + 16384 - 1586) & 16383] ^
                r[(nd + 16384 - 6988) & 16383] ^ r[(nd + 16384 - 9689) & 16383];
        w->buf[i] = r[nd];
    }
    w->nd = nd;
    w->pos = 0;
    w->len = 624;
}

static int source_open(word_source *w, int kind, unsigned long seed) {
    memset(w, 0, sizeof(*w));
    w->buf = (uint32_t *)malloc(624 * sizeof(uint32_t));
    if (!w->buf) return C21CM_MEMORY_ALLOC_ERROR;
    w->kind = w->unit = kind;
    if (kind >= 2) { /* cmrg, mrg, taus2: seeded through the LCG x -> 69069 x mod 2^32; 0 means 1 */
        uint32_t x = seed == 0 ? 1u : (uint32_t)seed;
#define LCG(n) ((uint32_t)(69069u * (n)))
        if (kind == 2) {
            for (int i = 0; i < 6; i++) {
                x = LCG(x);
                w->lx[i] = (long int)(x % (i < 3 ? 2147483647u : 2145483479u));
            }
            for (int i = 0; i < 7; i++) (void)cmrg_get(w);
        } else if (kind == 3) {
            for (int i = 0; i < 5; i++) {
                x = LCG(x);
                w->lx[i] = (long int)(x % 2147483647u);
            }
            for (int i = 0; i < 6; i++) (void)mrg_get(w);
        } else {
            w->ts[0] = LCG(x);
            if (w->ts[0] < 2) w->ts[0] += 2u;
            w->ts[1] = LCG(w->ts[0]);
            if (w->ts[1] < 8) w->ts[1] += 8u;
            w->ts[2] = LCG(w->ts[1]);
            if (w->ts[2] < 16) w->ts[2] += 16u;
            for (int i = 0; i < 6; i++) (void)taus2_get(w);
        }
#undef LCG
        return 0;
    }
    if (seed == 0) seed = 4357;
    if (kind == 0) {
        w->mt[0] = (uint32_t)seed;
        for (uint32_t i = 1; i < 624; i++)
            w->mt[i] = 1812433253u * (w->mt[i - 1] ^ (w->mt[i - 1] >> 30)) + i;
        w->refill = mt_refill;
    } else {
        w->ring = (uint32_t *)malloc(16384 * sizeof(uint32_t));
        if (!w->ring) return C21CM_MEMORY_ALLOC_ERROR;
        uint32_t x = (uint32_t)seed;
        for (int i = 0; i < 16384; i++) {
            uint32_t word = 0;
            for (int b = 31; b >= 0; b--) {
                x *= 69069u;
                word |= (x >> 31) << b;
            }
            w->ring[i] = word;
        }
        for (int i = 0; i < 32; i++) { /* rows 7, 10, 13, ...: zero left of the diagonal, one on it */
            const uint32_t diag = 0x80000000u >> i;
            w->ring[7 + 3 * i] = (w->ring[7 + 3 * i] & (0xffffffffu >> i)) | diag;
        }
        w->nd = 32;
        w->refill = gfsr4_refill;
    }
    w->pos = w->len = 0;
    return 0;
}

static void source_close(word_source *w) {
    free(w->buf);
    free(w->ring);
    w->buf = w->ring = NULL;
}

static inline uint32_t next_word(word_source *w) {
    if (w->pos == w->len) w->refill(w);
    return w->buf[w->pos++];
}

static inline double next_uniform_pos(word_source *w) {
    if (w->kind >= 2) { /* gsl_rng_uniform_pos: the generator's get_double until it is non-zero */
        double u;
        do {
            if (w->kind == 2)
                u = cmrg_get(w) / 2147483647.0;
            else if (w->kind == 3)
                u = mrg_get(w) / 2147483647.0;
            else
                u = taus2_get(w) / 4294967296.0;
        } while (u == 0);
        return u;
    }
    uint32_t v;
    do v = next_word(w);
    while (v == 0);
    return v * (1.0 / 4294967296.0);
}

static inline double next_ugaussian(word_source *w) {
    double x, y, r2;
    do {
        x = 2 * next_uniform_pos(w) - 1;
        y = 2 * next_uniform_pos(w) - 1;
        r2 = x * x + y * y;
    } while (r2 > 1.0 || r2 == 0);
    return y * sqrt(-2.0 * log(r2) / r2);
}

/* rng.c:31-56 with src[i] = i: the per-thread seeds */
int c21_gsl_thread_seeds(unsigned long long seed, int n_threads, unsigned int *seeds) {
    if (n_threads < 1 || !seeds) return C21CM_VALUE_ERROR;
    word_source w;
    int st = source_open(&w, 0, (unsigned long)seed);
    if (st) return st;
    const uint64_t n = 2147483647 / 16;
    uint64_t taken = 0;
    for (uint64_t i = 0; i < n && taken < (uint64_t)n_threads; i++) {
        const double u = next_word(&w) * (1.0 / 4294967296.0);
        if ((double)(n - i) * u < (double)((uint64_t)n_threads - taken)) seeds[taken++] = (unsigned int)i;
    }
    for (int i = n_threads - 1; i > 0; i--) {
        const uint32_t scale = 0xffffffffu / (uint32_t)(i + 1);
        uint32_t j;
        do j = next_word(&w) / scale;
        while (j >= (uint32_t)(i + 1));
        const unsigned int t = seeds[i];
        seeds[i] = seeds[j];
        seeds[j] = t;
    }
    source_close(&w);
    return 0;
}

int c21_gsl_stream_supported(int n_threads) { return n_threads >= 1 && n_threads <= 4096; }

/* the n-th raw output of generator `kind` (0 mt19937, 1 gfsr4, 2 cmrg, 3 mrg, 4 taus2) after
 * gsl_rng_set(seed): what GSL's own self-test compares (rng/test.c) */
unsigned long c21_gsl_nth_output(int kind, unsigned long seed, int n) {
    word_source w;
    if (kind < 0 || kind > 4 || n < 1 || source_open(&w, kind, seed)) return 0;
    unsigned long v = 0;
    for (int i = 0; i < n; i++)
        v = kind == 2 ? cmrg_get(&w) : kind == 3 ? mrg_get(&w) : kind == 4 ? taus2_get(&w) : next_word(&w);
    source_close(&w);
    return v;
}

/* The (a, b) deviates of all nx * ny * nzc modes in grid order: ab[2 * mode + {0, 1}]. */
int c21_gsl_mode_deviates(unsigned long long seed, int n_threads, int nx, int ny, int nzc,
                          double *ab) {
    if (!c21_gsl_stream_supported(n_threads)) {
        c21hip_set_error("ics: N_THREADS = %d is outside 1..4096", n_threads);
        return C21CM_VALUE_ERROR;
    }
    unsigned int *seeds = (unsigned int *)malloc(sizeof(unsigned int) * (size_t)n_threads);
    if (!seeds) return C21CM_MEMORY_ALLOC_ERROR;
    int st = c21_gsl_thread_seeds(seed, n_threads, seeds);
    if (st) {
        free(seeds);
        return st;
    }
    const int q = nx / n_threads, rem = nx % n_threads;
    /* the threads' streams are independent of each other: draw them concurrently, as upstream's
     * OpenMP loop does (each stream stays serial) */
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads > 64 ? 64 : n_threads) reduction(| : failed)
    for (int t = 0; t < n_threads; t++) {
        const int lo = t * q + (t < rem ? t : rem), rows = q + (t < rem ? 1 : 0);
        word_source w;
        if (source_open(&w, t % 5, seeds[t])) { /* rng.c:58-85: the five kinds in turn */
            failed |= 1;
            continue;
        }
        double *p = ab + 2 * (size_t)lo * ny * nzc;
        const size_t count = 2 * (size_t)rows * ny * nzc;
        for (size_t m = 0; m < count; m++) p[m] = next_ugaussian(&w);
        source_close(&w);
    }
    if (failed) {
        free(seeds);
        return C21CM_MEMORY_ALLOC_ERROR;
    }
    free(seeds);
    return 0;
}

/* ---- the same stream with the transcendental half on the device (round 4) ------------------------
 * This path keeps the acceptance loop on the host and moves the logarithm: the host draws words
 * until a pair is accepted (0 < x^2 + y^2 <= 1) and keeps the two RAW outputs of the accepted pair --
 * eight bytes per deviate, the size of the deviate itself -- and the device turns them into
 * y sqrt(-2 ln r2 / r2) in place (ics_kernels.hip: gsl_words_kernel).  Every thread stages its words
 * through two pinned chunks on its own stream while it keeps drawing, so the copy over PCIe and the
 * page faults of an 8.6 GB host array (DIM = 1024) are off the critical path as well.  5.8 -> ~1.5 s
 * at DIM = 1024 with 16 streams.  dev_ab: device array of 2 nx ny nzc doubles, filled in grid order. */
static inline uint32_t next_raw_pos(word_source *w) { /* the raw output behind gsl_rng_uniform_pos */
    if (w->kind >= 2) {
        unsigned long v;
        do v = w->kind == 2 ? cmrg_get(w) : w->kind == 3 ? mrg_get(w) : taus2_get(w);
        while (v == 0);
        return (uint32_t)v;
    }
    uint32_t v;
    do v = next_word(w);
    while (v == 0);
    return v;
}
static inline double raw_to_uniform(int kind, uint32_t v) {
    return (kind == 2 || kind == 3) ? v / 2147483647.0 : v * (1.0 / 4294967296.0);
}

/* The acceptance loop: the next n accepted pairs of the source, packed a | c << 32.  Returns how many it
 * filled: n, or fewer when caller-supplied words ran out (mem_refill). */
static size_t accept_fill(word_source *w, uint64_t *p, size_t n) {
    const int unit = w->unit;
    for (size_t m = 0; m < n; m++) {
        uint32_t a, c;
        double x, y, r2;
        do {
            a = next_raw_pos(w);
            c = next_raw_pos(w);
            x = 2 * raw_to_uniform(unit, a) - 1;
            y = 2 * raw_to_uniform(unit, c) - 1;
            r2 = x * x + y * y;
        } while ((r2 > 1.0 || r2 == 0) && !w->eof);
        if (w->eof) return m;
        p[m] = (uint64_t)a | ((uint64_t)c << 32);
    }
    return n;
}

/* caller-supplied words as a source: when they run out the source says so and hands out a non-zero
 * word for ever, which ends the loops above */
static void mem_refill(word_source *w) {
    static uint32_t one = 1;
    w->eof = 1;
    w->buf = &one;
    w->pos = 0;
    w->len = 1;
}

/* the generator kind of every row, then raw pairs -> deviates in place on the caller's stream */
static int rows_to_deviates(const unsigned char *row_kind, int nx, size_t per_row, double *dev_ab, void *stream) {
    unsigned char *kind_dev = (unsigned char *)c21hip_ws(WS_GSL_ROW_KIND, (size_t)nx);
    if (!kind_dev) return C21CM_MEMORY_ALLOC_ERROR;
    int st = c21hip_h2d(kind_dev, row_kind, (size_t)nx, stream);
    if (!st) st = c21hip_sync(stream); /* the caller frees `row_kind` */
    if (st) return st;
    return c21hip_gsl_words_to_deviates(dev_ab, (size_t)nx * per_row, kind_dev, per_row, stream);
}

int c21_gsl_mode_deviates_device(unsigned long long seed, int n_threads, int nx, int ny, int nzc,
                                 double *dev_ab, void *stream) {
    if (!c21_gsl_stream_supported(n_threads)) {
        c21hip_set_error("ics: N_THREADS = %d is outside 1..4096", n_threads);
        return C21CM_VALUE_ERROR;
    }
    unsigned int *seeds = (unsigned int *)malloc(sizeof(unsigned int) * (size_t)n_threads);
    unsigned char *row_kind = (unsigned char *)malloc((size_t)nx);
    if (!seeds || !row_kind) {
        free(seeds);
        free(row_kind);
        return C21CM_MEMORY_ALLOC_ERROR;
    }
    int st = c21_gsl_thread_seeds(seed, n_threads, seeds);
    if (st) {
        free(seeds);
        free(row_kind);
        return st;
    }
    const int q = nx / n_threads, rem = nx % n_threads;
    const size_t per_row = 2 * (size_t)ny * nzc; /* deviates per x-row */
    const int device = c21hip_current_device();
    /* deviates per staging chunk: 32 MB each, two per stream -- but no more than 512 MB of pinned memory
     * over all concurrently drawing streams (64 streams of 2 x 32 MB were 4 GB: ADVICE r4) */
    size_t CH = (size_t)1 << 22;
    {
        const int streams = n_threads > 64 ? 64 : n_threads;
        while (CH > ((size_t)1 << 16) && 2 * CH * sizeof(uint64_t) * (size_t)streams > ((size_t)512 << 20)) CH >>= 1;
    }
    int failed = 0;
    /* everything queued on the caller's stream before this call has to be done with dev_ab */
    if ((st = c21hip_sync(stream))) {
        free(seeds);
        free(row_kind);
        return st;
    }
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads > 64 ? 64 : n_threads) reduction(| : failed)
    for (int t = 0; t < n_threads; t++) {
        const int lo = t * q + (t < rem ? t : rem), rows = q + (t < rem ? 1 : 0);
        for (int r = 0; r < rows; r++) row_kind[lo + r] = (unsigned char)(t % 5);
        if (rows == 0) continue;
        word_source w;
        uint64_t *chunk[2] = {NULL, NULL};
        void *ev[2] = {NULL, NULL}, *cs = NULL;
        int ok = device < 0 || c21hip_use_device(device) == 0;
        if (ok && source_open(&w, t % 5, seeds[t])) ok = 0; /* rng.c:58-85: the five kinds in turn */
        if (!ok) {
            failed |= 1;
            continue;
        }
        const size_t count = (size_t)rows * per_row;
        const size_t ch = count < CH ? count : CH;
        chunk[0] = (uint64_t *)c21hip_pinned_alloc(ch * sizeof(uint64_t));
        chunk[1] = (uint64_t *)c21hip_pinned_alloc(ch * sizeof(uint64_t));
        ev[0] = c21hip_event_create();
        ev[1] = c21hip_event_create();
        cs = c21hip_stream_create();
        if (!chunk[0] || !chunk[1] || !ev[0] || !ev[1] || !cs) {
            failed |= 1;
        } else {
            uint64_t *dst = (uint64_t *)dev_ab + (size_t)lo * per_row;
            int used[2] = {0, 0};
            size_t done = 0;
            for (int b = 0; done < count && !failed; b ^= 1) {
                const size_t n = count - done < ch ? count - done : ch;
                if (used[b] && c21hip_event_synchronize(ev[b])) failed |= 1; /* the chunk's last copy has left it */
                uint64_t *p = chunk[b];
                (void)accept_fill(&w, p, n);
                if (c21hip_h2d(dst + done, p, n * sizeof(uint64_t), cs) || c21hip_event_record(ev[b], cs))
                    failed |= 1;
                used[b] = 1;
                done += n;
            }
            if (c21hip_sync(cs)) failed |= 1;
        }
        c21hip_pinned_free(chunk[0]);
        c21hip_pinned_free(chunk[1]);
        c21hip_event_destroy(ev[0]);
        c21hip_event_destroy(ev[1]);
        c21hip_stream_destroy(cs);
        source_close(&w);
    }
    free(seeds);
    if (failed) {
        free(row_kind);
        c21hip_set_error("ics: staging the random stream failed (pinned memory / stream / copy)");
        return C21CM_MEMORY_ALLOC_ERROR;
    }
    st = rows_to_deviates(row_kind, nx, per_row, dev_ab, stream);
    free(row_kind);
    return st;
}

/* ---- the streams drawn on the device (gsl_stream_kernels.hip) ---------------------------------------------
 * State of a generator as 32-bit words, the form the device loads and saves:
 *   mt19937  [0] words of the current block already handed out (624: refill first), [1 ..] the 624 state words
 *   gfsr4    [0] ring position of the last output, [1 ..] the 2^14 ring words
 *   cmrg     x1 x2 x3 y1 y2 y3;  mrg  x1 .. x5;  taus2  s1 s2 s3 */
static size_t state_words(int kind) {
    return kind == 0 ? 625 : kind == 1 ? 16385 : kind == 2 ? 6 : kind == 3 ? 5 : 3;
}

int c21_gsl_export_state(int kind, unsigned long seed, unsigned int *state) {
    word_source w;
    if (kind < 0 || kind > 4 || !state) return C21CM_VALUE_ERROR;
    int st = source_open(&w, kind, seed);
    if (st) {
        source_close(&w);
        return st;
    }
    if (kind == 0) {
        state[0] = 624;
        memcpy(state + 1, w.mt, sizeof(w.mt));
    } else if (kind == 1) {
        state[0] = (unsigned int)w.nd;
        memcpy(state + 1, w.ring, 16384 * sizeof(uint32_t));
    } else if (kind == 4) {
        for (int i = 0; i < 3; i++) state[i] = w.ts[i];
    } else {
        for (int i = 0; i < (kind == 2 ? 6 : 5); i++) state[i] = (unsigned int)w.lx[i];
    }
    source_close(&w);
    return 0;
}

/* one step of cmrg, mrg or taus2 on an exported state */
unsigned int c21_gsl_step(int kind, unsigned int *state) {
    word_source w;
    memset(&w, 0, sizeof(w));
    unsigned long v;
    if (kind == 4) {
        memcpy(w.ts, state, sizeof(w.ts));
        v = taus2_get(&w);
        memcpy(state, w.ts, sizeof(w.ts));
        return (unsigned int)v;
    }
    if (kind != 2 && kind != 3) return 0;
    const int n = kind == 2 ? 6 : 5;
    for (int i = 0; i < n; i++) w.lx[i] = (long int)state[i];
    v = kind == 2 ? cmrg_get(&w) : mrg_get(&w);
    for (int i = 0; i < n; i++) state[i] = (unsigned int)w.lx[i];
    return (unsigned int)v;
}

/* Jumping ahead.  A step of cmrg or mrg multiplies the state by a companion matrix modulo the prime (a negative
 * multiplier -a enters as m - a: the same residue), a step of a taus2 component is a linear map of GF(2)^32,
 * held as the images of the 32 unit vectors.  One matrix set: cmrg 9 + 9 words (row major), mrg 25, taus2 3 x 32
 * columns -- the layout of the device's tables (c21hip.h). */
#define JUMP_MAT_MAX 96
static int jump_mat_words(int kind) { return kind == 2 ? 18 : kind == 3 ? 25 : 96; }

static void modmat_mul(const uint32_t *a, const uint32_t *b, uint32_t *c, int n, uint64_t m) {
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            uint64_t acc = 0;
            for (int k = 0; k < n; k++) acc += ((uint64_t)a[i * n + k] * b[k * n + j]) % m;
            c[i * n + j] = (uint32_t)(acc % m);
        }
}
static void modmat_vec(const uint32_t *a, uint32_t *s, int n, uint64_t m) {
    uint32_t r[5];
    for (int i = 0; i < n; i++) {
        uint64_t acc = 0;
        for (int k = 0; k < n; k++) acc += ((uint64_t)a[i * n + k] * s[k]) % m;
        r[i] = (uint32_t)(acc % m);
    }
    memcpy(s, r, sizeof(uint32_t) * (size_t)n);
}
static uint32_t gf2_vec(const uint32_t *cols, uint32_t s) {
    uint32_t r = 0;
    for (int c = 0; c < 32; c++)
        if ((s >> c) & 1u) r ^= cols[c];
    return r;
}
static void jump_mat_one_step(int kind, uint32_t *mat) {
    memset(mat, 0, sizeof(uint32_t) * JUMP_MAT_MAX);
    if (kind == 2) {
        mat[1] = 63308, mat[2] = 2147483647u - 183326u, mat[3] = 1, mat[7] = 1;
        mat[9] = 86098, mat[11] = 2145483479u - 539608u, mat[12] = 1, mat[16] = 1;
    } else if (kind == 3) {
        mat[0] = 107374182, mat[4] = 104480;
        for (int i = 1; i < 5; i++) mat[5 * i + i - 1] = 1;
    } else {
        for (int c = 0; c < 32; c++) {
            word_source w;
            for (int k = 0; k < 3; k++) {
                /* the three components do not mix: step the unit vector in one of them at a time */
                w.ts[0] = w.ts[1] = w.ts[2] = 0;
                w.ts[k] = 1u << c;
                (void)taus2_get(&w);
                mat[32 * k + c] = w.ts[k];
            }
        }
    }
}
static void jump_mat_mul(int kind, const uint32_t *a, const uint32_t *b, uint32_t *c) { /* c = a b; c is neither */
    if (kind == 2) {
        modmat_mul(a, b, c, 3, 2147483647u);
        modmat_mul(a + 9, b + 9, c + 9, 3, 2145483479u);
    } else if (kind == 3) {
        modmat_mul(a, b, c, 5, 2147483647u);
    } else {
        for (int k = 0; k < 3; k++)
            for (int col = 0; col < 32; col++) c[32 * k + col] = gf2_vec(a + 32 * k, b[32 * k + col]);
    }
}
static void jump_mat_apply(int kind, const uint32_t *mat, uint32_t *state) {
    if (kind == 2) {
        modmat_vec(mat, state, 3, 2147483647u);
        modmat_vec(mat + 9, state + 3, 3, 2145483479u);
    } else if (kind == 3) {
        modmat_vec(mat, state, 5, 2147483647u);
    } else {
        for (int k = 0; k < 3; k++) state[k] = gf2_vec(mat + 32 * k, state[k]);
    }
}

/* the state n steps on: A^n by squaring */
int c21_gsl_jump(int kind, unsigned int *state, unsigned long long n) {
    if (kind < 2 || kind > 4 || !state) return C21CM_VALUE_ERROR;
    uint32_t sq[JUMP_MAT_MAX], tmp[JUMP_MAT_MAX];
    jump_mat_one_step(kind, sq);
    for (; n; n >>= 1) {
        if (n & 1) jump_mat_apply(kind, sq, state);
        jump_mat_mul(kind, sq, sq, tmp);
        memcpy(sq, tmp, sizeof(sq));
    }
    return 0;
}

/* the device's tables: A^(C21_GSL_RUN 2^j), j = 0 .. C21_GSL_JUMPS - 1, for the three kinds back to back */
static void jump_tables(uint32_t *out) {
    const int offset[3] = {C21_GSL_JUMP_CMRG, C21_GSL_JUMP_MRG, C21_GSL_JUMP_TAUS2};
    for (int kind = 2; kind <= 4; kind++) {
        uint32_t sq[JUMP_MAT_MAX], tmp[JUMP_MAT_MAX];
        const int words = jump_mat_words(kind);
        jump_mat_one_step(kind, sq);
        for (int run = C21_GSL_RUN; run > 1; run >>= 1) {
            jump_mat_mul(kind, sq, sq, tmp);
            memcpy(sq, tmp, sizeof(sq));
        }
        for (int j = 0; j < C21_GSL_JUMPS; j++) {
            memcpy(out + offset[kind - 2] + j * words, sq, sizeof(uint32_t) * (size_t)words);
            jump_mat_mul(kind, sq, sq, tmp);
            memcpy(sq, tmp, sizeof(sq));
        }
    }
}
_Static_assert((C21_GSL_RUN & (C21_GSL_RUN - 1)) == 0, "gsl stream: the run length is a power of two");

static const uint32_t *jump_tables_dev(void *stream, int *status) {
    uint32_t host[C21_GSL_JUMP_WORDS];
    uint32_t *dev = (uint32_t *)c21hip_ws(WS_GSL_JUMP, sizeof(host));
    if (!dev) {
        *status = C21CM_MEMORY_ALLOC_ERROR;
        return NULL;
    }
    jump_tables(host);
    *status = c21hip_h2d(dev, host, sizeof(host), stream);
    if (!*status) *status = c21hip_sync(stream); /* `host` is on this stack */
    return dev;
}

/* A launch of the device draw accepts at most this many pairs per stream: 2^22 pairs are 32 MB of output per
 * stream and keep a launch in the tens of milliseconds (DESIGN 4.5 has the measured time). */
#define GSL_PAIRS_PER_LAUNCH ((long long)1 << 22)
long long c21cm_gsl_default_pairs_per_launch(void) { return GSL_PAIRS_PER_LAUNCH; }
int c21cm_gsl_tile_words(int kind) { return c21hip_gsl_tile_words(kind); }

/* the rows of thread t under the static schedule: first row, number of rows */
static inline void thread_rows(int t, int nx, int n_threads, int *lo, int *rows) {
    const int q = nx / n_threads, rem = nx % n_threads;
    *lo = t * q + (t < rem ? t : rem);
    *rows = q + (t < rem ? 1 : 0);
}

/* The packed accepted pairs of all modes in grid order into dev_pairs (device, 2 nx ny nzc entries): one workgroup
 * per stream that owns rows, launched again until every stream has its count.  row_kind (host, nx entries, or NULL)
 * receives the generator kind per row. */
static int stream_pairs_device(unsigned long long seed, int n_threads, int nx, int ny, int nzc, long long max_pairs,
                               long tile_cap, uint64_t *dev_pairs, unsigned char *row_kind, void *stream) {
    if (!c21_gsl_stream_supported(n_threads)) {
        c21hip_set_error("ics: N_THREADS = %d is outside 1..4096", n_threads);
        return C21CM_VALUE_ERROR;
    }
    if (nx < 1 || ny < 1 || nzc < 1 || !dev_pairs) {
        c21hip_set_error("gsl stream: nx, ny, nzc must be positive and the output is required");
        return C21CM_VALUE_ERROR;
    }
    if (max_pairs <= 0) max_pairs = GSL_PAIRS_PER_LAUNCH;
    const size_t per_row = 2 * (size_t)ny * nzc;
    unsigned int *seeds = (unsigned int *)malloc(sizeof(unsigned int) * (size_t)n_threads);
    c21_gsl_stream_desc *desc = (c21_gsl_stream_desc *)malloc(sizeof(c21_gsl_stream_desc) * (size_t)n_threads);
    uint32_t *state = NULL;
    int status = seeds && desc ? c21_gsl_thread_seeds(seed, n_threads, seeds) : C21CM_MEMORY_ALLOC_ERROR;
    int n_streams = 0;
    size_t words = 0;
    unsigned long long longest = 0;
    if (!status) {
        for (int t = 0; t < n_threads; t++) {
            int lo, rows;
            thread_rows(t, nx, n_threads, &lo, &rows);
            if (rows == 0) continue; /* upstream's surplus threads get no iterations */
            if (row_kind)
                for (int r = 0; r < rows; r++) row_kind[lo + r] = (unsigned char)(t % 5);
            c21_gsl_stream_desc *d = &desc[n_streams++];
            d->out_offset = (unsigned long long)lo * per_row;
            d->count = (unsigned long long)rows * per_row;
            d->kind = (unsigned int)(t % 5); /* rng.c:58-85: the five kinds in turn */
            d->state_offset = (unsigned int)words;
            words += C21_GSL_HDR + state_words(t % 5);
            if (d->count > longest) longest = d->count;
        }
        state = (uint32_t *)calloc(words, sizeof(uint32_t));
        if (!state) status = C21CM_MEMORY_ALLOC_ERROR;
    }
    for (int i = 0, t = 0; !status && t < n_threads; t++) {
        int lo, rows;
        thread_rows(t, nx, n_threads, &lo, &rows);
        if (rows == 0) continue;
        status = c21_gsl_export_state(t % 5, seeds[t], state + desc[i++].state_offset + C21_GSL_HDR);
    }
    void *desc_dev = NULL;
    uint32_t *state_dev = NULL;
    int *flag_dev = NULL;
    const uint32_t *jump_dev = NULL;
    if (!status) {
        desc_dev = c21hip_ws(WS_GSL_DESC, sizeof(c21_gsl_stream_desc) * (size_t)n_streams);
        state_dev = (uint32_t *)c21hip_ws(WS_GSL_STATE, words * sizeof(uint32_t));
        flag_dev = (int *)c21hip_ws(WS_GSL_FLAG, 2 * sizeof(unsigned long long));
        if (!desc_dev || !state_dev || !flag_dev) status = C21CM_MEMORY_ALLOC_ERROR;
    }
    if (!status) jump_dev = jump_tables_dev(stream, &status);
    if (!status) status = c21hip_h2d(desc_dev, desc, sizeof(c21_gsl_stream_desc) * (size_t)n_streams, stream);
    if (!status) status = c21hip_h2d(state_dev, state, words * sizeof(uint32_t), stream);
    if (!status) status = c21hip_memset(flag_dev, 0, sizeof(int), stream);
    /* every launch hands each unfinished stream exactly min(max_pairs, what it still owes), or fails at the tile
     * cap: the number of launches follows from the longest stream, and nothing is read back in between */
    const unsigned long long launches = (longest + (unsigned long long)max_pairs - 1) / (unsigned long long)max_pairs;
    for (unsigned long long l = 0; !status && l < launches; l++)
        status = c21hip_gsl_stream_draw(desc_dev, n_streams, state_dev, jump_dev, (unsigned long long *)dev_pairs,
                                        (unsigned long long)max_pairs, tile_cap, flag_dev, stream);
    int flag = 0;
    if (!status) status = c21hip_d2h(&flag, flag_dev, sizeof(int), stream);
    /* also before the host copies of the descriptors and states are freed */
    const int sync_status = c21hip_sync(stream);
    if (!status) status = sync_status;
    if (!status && flag) {
        c21hip_set_error("gsl stream: a launch reached its tile cap before it had its pairs");
        status = C21CM_VALUE_ERROR;
    }
    free(seeds);
    free(desc);
    free(state);
    return status;
}

/* dev_ab: device array of 2 nx ny nzc doubles, filled in grid order (as c21_gsl_mode_deviates_device) */
int c21_gsl_mode_deviates_ondevice(unsigned long long seed, int n_threads, int nx, int ny, int nzc, double *dev_ab,
                                   long long max_pairs_per_launch, void *stream) {
    if (nx < 1) return C21CM_VALUE_ERROR;
    unsigned char *row_kind = (unsigned char *)malloc((size_t)nx);
    if (!row_kind) return C21CM_MEMORY_ALLOC_ERROR;
    int st = stream_pairs_device(seed, n_threads, nx, ny, nzc, max_pairs_per_launch, 0, (uint64_t *)dev_ab, row_kind,
                                 stream);
    if (!st) st = rows_to_deviates(row_kind, nx, 2 * (size_t)ny * nzc, dev_ab, stream);
    free(row_kind);
    return st;
}

/* ---- the pieces, on the host or on the device (c21cm_grid.h) ---------------------------------------------- */
static int gsl_fail(const char *msg) {
    c21hip_set_error("gsl stream: %s", msg);
    return C21CM_VALUE_ERROR;
}

/* a host result on its way to `out`, which may be a device array; frees `host` */
static int deliver_host(void *out, void *host, size_t bytes, void *stream) {
    int st = 0;
    if (c21hip_is_device_ptr(out)) {
        st = c21hip_h2d(out, host, bytes, stream);
        if (!st) st = c21hip_sync(stream);
    } else {
        memcpy(out, host, bytes);
    }
    free(host);
    return st;
}

int c21cm_gsl_raw_words(int kind, unsigned long long seed, size_t n, int on_device, unsigned int *out_u32) {
    if (kind < 0 || kind > 4) return gsl_fail("kind must be 0 .. 4");
    if (!out_u32 && n) return gsl_fail("the output is required");
    if (n == 0) return 0;
    if (!on_device) {
        word_source w;
        uint32_t *host = (uint32_t *)malloc(n * sizeof(uint32_t));
        int st = host ? source_open(&w, kind, (unsigned long)seed) : C21CM_MEMORY_ALLOC_ERROR;
        if (st) {
            free(host);
            return st;
        }
        for (size_t i = 0; i < n; i++)
            host[i] = (uint32_t)(kind == 2 ? cmrg_get(&w) : kind == 3 ? mrg_get(&w) : kind == 4 ? taus2_get(&w) : next_word(&w));
        source_close(&w);
        return deliver_host(out_u32, host, n * sizeof(uint32_t), NULL);
    }
    int st = 0;
    const size_t words = state_words(kind);
    uint32_t *state = (uint32_t *)malloc(words * sizeof(uint32_t));
    uint32_t *state_dev = (uint32_t *)c21hip_ws(WS_GSL_STATE, words * sizeof(uint32_t));
    const int host_out = !c21hip_is_device_ptr(out_u32);
    uint32_t *out_dev = host_out ? (uint32_t *)c21hip_ws(WS_GSL_OUT, n * sizeof(uint32_t)) : out_u32;
    if (!state || !state_dev || !out_dev) st = C21CM_MEMORY_ALLOC_ERROR;
    if (!st) st = c21_gsl_export_state(kind, (unsigned long)seed, state);
    const uint32_t *jump_dev = st ? NULL : jump_tables_dev(NULL, &st);
    if (!st) st = c21hip_h2d(state_dev, state, words * sizeof(uint32_t), NULL);
    if (!st) st = c21hip_gsl_raw_words(kind, state_dev, jump_dev, n, out_dev, NULL);
    if (!st && host_out) st = c21hip_d2h(out_u32, out_dev, n * sizeof(uint32_t), NULL);
    const int sync_status = c21hip_sync(NULL);
    free(state);
    return st ? st : sync_status;
}

int c21cm_gsl_accept_pairs(int kind, const unsigned int *words, size_t n_words, size_t want, int on_device,
                           unsigned long long *pairs_out, size_t *n_pairs, size_t *n_words_used) {
    if (kind < 0 || kind > 4) return gsl_fail("kind must be 0 .. 4");
    if (!n_pairs || !n_words_used || (n_words && !words)) return gsl_fail("words and both counts are required");
    const size_t room = want < n_words / 2 ? want : n_words / 2;
    if (room && !pairs_out) return gsl_fail("the output is required");
    *n_pairs = *n_words_used = 0;
    if (!on_device) {
        uint32_t *copy = NULL;
        if (n_words && c21hip_is_device_ptr(words)) {
            copy = (uint32_t *)malloc(n_words * sizeof(uint32_t));
            if (!copy) return C21CM_MEMORY_ALLOC_ERROR;
            int st = c21hip_d2h(copy, words, n_words * sizeof(uint32_t), NULL);
            if (!st) st = c21hip_sync(NULL);
            if (st) {
                free(copy);
                return st;
            }
        }
        uint64_t *host = (uint64_t *)malloc((room + 1) * sizeof(uint64_t));
        if (!host) {
            free(copy);
            return C21CM_MEMORY_ALLOC_ERROR;
        }
        word_source w;
        memset(&w, 0, sizeof(w));
        w.kind = -1;
        w.unit = kind;
        w.refill = mem_refill;
        w.buf = copy ? copy : (uint32_t *)words;
        w.len = (int)n_words;
        if ((size_t)w.len != n_words) {
            free(copy);
            free(host);
            return gsl_fail("too many words");
        }
        /* n_words / 2 pairs are all the words can give, so the loop never writes beyond `room` entries: it
         * runs out of words first */
        *n_pairs = accept_fill(&w, host, want);
        *n_words_used = w.eof ? n_words : (size_t)w.pos;
        free(copy);
        return room ? deliver_host(pairs_out, host, room * sizeof(uint64_t), NULL) : (free(host), 0);
    }
    int st = 0;
    if (n_words == 0 || want == 0) return 0;
    const uint32_t *words_dev = (const uint32_t *)c21_stage_in(WS_GSL_IN, words, n_words * sizeof(uint32_t), NULL, &st);
    unsigned long long *result_dev = (unsigned long long *)c21hip_ws(WS_GSL_FLAG, 2 * sizeof(unsigned long long));
    const int host_out = !c21hip_is_device_ptr(pairs_out);
    unsigned long long *pairs_dev =
        host_out ? (unsigned long long *)c21hip_ws(WS_GSL_OUT, (room ? room : 1) * sizeof(uint64_t)) : pairs_out;
    if (!st && (!result_dev || !pairs_dev)) st = C21CM_MEMORY_ALLOC_ERROR;
    if (!st) st = c21hip_gsl_accept_pairs(kind, words_dev, n_words, want, pairs_dev, result_dev, NULL);
    unsigned long long result[2] = {0, 0};
    if (!st) st = c21hip_d2h(result, result_dev, sizeof(result), NULL);
    if (!st) st = c21hip_sync(NULL);
    if (!st && host_out && result[0]) st = c21hip_d2h(pairs_out, pairs_dev, result[0] * sizeof(uint64_t), NULL);
    if (!st) st = c21hip_sync(NULL);
    if (st) return st;
    *n_pairs = (size_t)result[0];
    *n_words_used = (size_t)result[1];
    return 0;
}

int c21cm_gsl_stream_pairs(unsigned long long seed, int n_threads, int nx, int ny, int nzc, int on_device,
                           long long max_pairs_per_launch, long tile_cap, unsigned long long *pairs_out,
                           void *stream) {
    if (nx < 1 || ny < 1 || nzc < 1 || !pairs_out) return gsl_fail("nx, ny, nzc must be positive and the output is required");
    const size_t per_row = 2 * (size_t)ny * nzc, bytes = (size_t)nx * per_row * sizeof(uint64_t);
    if (on_device) {
        const int host_out = !c21hip_is_device_ptr(pairs_out);
        uint64_t *dev = host_out ? (uint64_t *)c21hip_ws(WS_GSL_OUT, bytes) : (uint64_t *)pairs_out;
        if (!dev) return C21CM_MEMORY_ALLOC_ERROR;
        int st = stream_pairs_device(seed, n_threads, nx, ny, nzc, max_pairs_per_launch, tile_cap, dev, NULL, stream);
        if (!st && host_out) {
            st = c21hip_d2h(pairs_out, dev, bytes, stream);
            if (!st) st = c21hip_sync(stream);
        }
        return st;
    }
    if (!c21_gsl_stream_supported(n_threads)) {
        c21hip_set_error("ics: N_THREADS = %d is outside 1..4096", n_threads);
        return C21CM_VALUE_ERROR;
    }
    unsigned int *seeds = (unsigned int *)malloc(sizeof(unsigned int) * (size_t)n_threads);
    uint64_t *host = (uint64_t *)malloc(bytes);
    int st = seeds && host ? c21_gsl_thread_seeds(seed, n_threads, seeds) : C21CM_MEMORY_ALLOC_ERROR;
    int failed = 0;
    if (!st) {
#pragma omp parallel for schedule(dynamic, 1) num_threads(n_threads > 64 ? 64 : n_threads) reduction(| : failed)
        for (int t = 0; t < n_threads; t++) {
            int lo, rows;
            thread_rows(t, nx, n_threads, &lo, &rows);
            if (rows == 0) continue;
            word_source w;
            if (source_open(&w, t % 5, seeds[t])) {
                failed |= 1;
                source_close(&w);
                continue;
            }
            (void)accept_fill(&w, host + (size_t)lo * per_row, (size_t)rows * per_row);
            source_close(&w);
        }
        if (failed) st = C21CM_MEMORY_ALLOC_ERROR;
    }
    free(seeds);
    if (st) {
        free(host);
        return st;
    }
    return deliver_host(pairs_out, host, bytes, stream);
}
