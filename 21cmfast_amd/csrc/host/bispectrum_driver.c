/*
 * bispectrum_driver.c -- C host driver of the bispectrum of boxes and lightcone chunks (the spec is
 * tests/bispectrum_reference.py): pack -> batched r2c for all chunks (the power spectrum's), then per chunk shell
 * fill -> batched c2r over the stack of shells -> triple products, and one fixed-order finish for all chunks
 * (csrc/hip/bispectrum_kernels.hip).  The host builds the per-axis wavenumbers and the |k|^2 thresholds as
 * power_driver.c does, so a shell is exactly a get_power bin, and sorts the triangles into groups of one (b1, b2)
 * pair and up to C21HIP_BISPEC_GROUP third shells.
 *
 * The number of closed mode triplets of a triangle depends on the geometry alone (shape, lengths, edges).  It comes
 * from fp64 transforms of the shell indicators (an fp32 transform is off by 5e-5 relative at 64^3 for sparsely
 * populated triangles, and worse with N), rounded to integers, for every triangle whose shells can close, and is
 * kept in a one-entry cache: the next call with the same geometry -- every chunk of a lightcone, every sample of an
 * inference run -- skips the indicator pass.  The cache, like the workspace, is not guarded against concurrent calls.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"

#define TRY(expr)         \
    do {                  \
        int st_ = (expr); \
        if (st_) {        \
            status = st_; \
            goto done;    \
        }                 \
    } while (0)

#define BS_G C21HIP_BISPEC_GROUP
#define BS_GI C21HIP_BISPEC_GROUP_INTS
#define BS_MAXB C21HIP_BISPEC_MAX_BINS

static int bs_fail(const char *msg) {
    c21hip_set_error("bispectrum: %s", msg);
    return C21CM_VALUE_ERROR;
}

/* numpy: fftfreq(n, d) = [0, 1, .., (n-1)/2, -(n/2), .., -1] * (1.0 / (n * d)), then * 2.0 * pi, d = L / n */
static void k_axis(double *k, int n, int count, double L) {
    const double d = L / (double)n, val = 1.0 / ((double)n * d);
    const int npos = (n - 1) / 2 + 1;
    for (int i = 0; i < count; ++i) {
        const long long f = i < npos ? i : (long long)i - n;
        k[i] = (double)f * val * 2.0 * 3.141592653589793;
    }
}

/* the smallest x with sqrt(x) >= e > 0 (sqrt correctly rounded, as numpy's): the fill kernel bins |k|^2 on these */
static double sq_threshold(double e) {
    double x = e * e;
    while (sqrt(x) < e) x = nextafter(x, INFINITY);
    while (x > 0 && sqrt(nextafter(x, -INFINITY)) >= e) x = nextafter(x, -INFINITY);
    return x;
}

static int cmp_u64(const void *a, const void *b) {
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

/* Triangles sorted by (b1, b2, b3) and cut into groups: groups[g] = {b1, b2, count, b3 x BS_G (unused places: b2)},
 * slot[t] = g BS_G + j where triangle t sits.  Returns the number of groups, or -1 out of memory. */
static int build_groups(const int *tri, int n, int **groups_out, int *slot) {
    uint64_t *key = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    int *groups = (int *)malloc(sizeof(int) * (size_t)n * BS_GI); /* at most one group per triangle */
    if (!key || !groups) {
        free(key);
        free(groups);
        return -1;
    }
    for (int t = 0; t < n; ++t)
        key[t] = ((uint64_t)((tri[3 * t] * BS_MAXB + tri[3 * t + 1]) * BS_MAXB + tri[3 * t + 2]) << 32) | (uint32_t)t;
    qsort(key, (size_t)n, sizeof(uint64_t), cmp_u64);
    int ng = 0, fill = BS_G, pair = -1;
    for (int q = 0; q < n; ++q) {
        const int t = (int)(uint32_t)key[q];
        const int p = tri[3 * t] * BS_MAXB + tri[3 * t + 1];
        if (p != pair || fill == BS_G) {
            int *g = groups + (size_t)ng++ * BS_GI;
            g[0] = tri[3 * t];
            g[1] = tri[3 * t + 1];
            for (int j = 0; j < BS_G; ++j) g[3 + j] = g[1];
            pair = p;
            fill = 0;
        }
        groups[(size_t)(ng - 1) * BS_GI + 3 + fill] = tri[3 * t + 2];
        slot[t] = (ng - 1) * BS_G + fill++;
        groups[(size_t)(ng - 1) * BS_GI + 2] = fill;
    }
    free(key);
    *groups_out = groups;
    return ng;
}

/* ---- the triangle counts of the last geometry ---- */
static struct {
    int valid, nx, ny, nz, n_bins;
    double L[3], edges[BS_MAXB + 1];
    long long *counts; /* [n_bins][n_bins][n_bins], b1 <= b2 <= b3 filled */
} g_cache;

static int cache_hit(int nx, int ny, int nz, const double *L, int n_bins, const double *edges) {
    return g_cache.valid && g_cache.nx == nx && g_cache.ny == ny && g_cache.nz == nz && g_cache.n_bins == n_bins &&
           !memcmp(g_cache.L, L, sizeof(double) * 3) && !memcmp(g_cache.edges, edges, sizeof(double) * ((size_t)n_bins + 1));
}

/* the k tables of a geometry on the host: kx ky kz thr (doubles) */
static size_t fill_ktab(double *hd, int nx, int ny, int nz, const double *L, int n_bins, const double *edges) {
    const int nh = nz / 2 + 1;
    k_axis(hd, nx, nx, L[0]);
    k_axis(hd + nx, ny, ny, L[1]);
    k_axis(hd + nx + ny, nz, nh, L[2]);
    for (int q = 0; q <= n_bins; ++q) hd[nx + ny + nh + q] = sq_threshold(edges[q]);
    return (size_t)nx + ny + nh + (size_t)n_bins + 1;
}

static void set_tabs(c21hip_bispec_tabs *t, const double *dd, int nx, int ny, int nz, int n_bins) {
    t->kx = dd;
    t->ky = dd + nx;
    t->kz = dd + nx + ny;
    t->thr = dd + nx + ny + (nz / 2 + 1);
    t->n_bins = n_bins;
}

/* The indicator pass: n_tri of every triangle whose shells can close (e[b3] < e[b1+1] + e[b2+1]; the others hold no
 * closed triplet), from fp64 transforms, into the cache.  Synchronises the stream. */
static int count_pass(int nx, int ny, int nz, const double *L, int n_bins, const double *edges, void *stream) {
    int status = 0;
    int *tri = NULL, *groups = NULL, *slot = NULL;
    unsigned char *host_tab = NULL;
    long long *counts = NULL, *table = NULL;
    g_cache.valid = 0;
    const size_t n_all = (size_t)n_bins * (n_bins + 1) * (n_bins + 2) / 6;
    tri = (int *)malloc(sizeof(int) * 3 * n_all);
    slot = (int *)malloc(sizeof(int) * n_all);
    table = (long long *)calloc((size_t)n_bins * n_bins * n_bins, sizeof(long long));
    if (!tri || !slot || !table) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    int n = 0;
    for (int a = 0; a < n_bins; ++a)
        for (int b = a; b < n_bins; ++b)
            for (int c = b; c < n_bins; ++c)
                if (edges[c] < edges[a + 1] + edges[b + 1]) {
                    tri[3 * n] = a;
                    tri[3 * n + 1] = b;
                    tri[3 * n + 2] = c;
                    ++n;
                }
    /* (0, 0, 0) always passes: n >= 1 */
    const int ng = build_groups(tri, n, &groups, slot);
    if (ng < 0) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const int nh = nz / 2 + 1;
    const size_t n_dbl = (size_t)nx + ny + nh + (size_t)n_bins + 1;
    const size_t n_int = (size_t)ng * BS_GI + (size_t)n;
    const size_t tab_bytes = sizeof(double) * n_dbl + sizeof(int) * n_int;
    host_tab = (unsigned char *)malloc(tab_bytes);
    counts = (long long *)malloc(sizeof(long long) * (size_t)n);
    if (!host_tab || !counts) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    fill_ktab((double *)host_tab, nx, ny, nz, L, n_bins, edges);
    int *hi = (int *)(host_tab + sizeof(double) * n_dbl);
    memcpy(hi, groups, sizeof(int) * (size_t)ng * BS_GI);
    memcpy(hi + (size_t)ng * BS_GI, slot, sizeof(int) * (size_t)n);

    const int n_slabs = c21hip_bispec_slabs(nx, ny, nz, NULL);
    const size_t plane = (size_t)nx * ny * 2 * (size_t)nh;
    const size_t part_dbl = (size_t)n_slabs * ng * BS_G;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_BS_TAB, tab_bytes);
    double *d_stack = (double *)c21hip_ws(WS_BS_STACK, sizeof(double) * plane * (size_t)n_bins);
    double *d_sums = (double *)c21hip_ws(WS_BS_SUMS, sizeof(double) * (part_dbl + (size_t)n));
    if (!d_tab || !d_stack || !d_sums) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    c21hip_bispec_tabs t;
    set_tabs(&t, (const double *)d_tab, nx, ny, nz, n_bins);
    const int *d_groups = (const int *)(d_tab + sizeof(double) * n_dbl), *d_slot = d_groups + (size_t)ng * BS_GI;
    long long *d_counts = (long long *)(d_sums + part_dbl);
    TRY(c21hip_bispec_fill(NULL, d_stack, 1, nx, ny, nz, &t, stream));
    TRY(c21hip_fft_c2r_batched_f64(d_stack, nx, ny, nz, n_bins, stream));
    TRY(c21hip_bispec_products(d_stack, 1, nx, ny, nz, d_groups, ng, d_sums, stream));
    TRY(c21hip_bispec_finish(d_sums, 1, n_slabs, ng * BS_G, d_slot, n, 0.0, (double)nx * (double)ny * (double)nz, NULL,
                             NULL, d_counts, stream));
    TRY(c21hip_d2h(counts, d_counts, sizeof(long long) * (size_t)n, stream));
    TRY(c21hip_sync(stream));
    for (int q = 0; q < n; ++q)
        table[((size_t)tri[3 * q] * n_bins + tri[3 * q + 1]) * n_bins + tri[3 * q + 2]] = counts[q];
    free(g_cache.counts);
    g_cache.counts = table;
    table = NULL;
    g_cache.nx = nx;
    g_cache.ny = ny;
    g_cache.nz = nz;
    g_cache.n_bins = n_bins;
    memcpy(g_cache.L, L, sizeof(double) * 3);
    memcpy(g_cache.edges, edges, sizeof(double) * ((size_t)n_bins + 1));
    g_cache.valid = 1;
done:
    free(tri);
    free(groups);
    free(slot);
    free(host_tab);
    free(counts);
    free(table);
    return status;
}

int c21cm_bispectrum_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                           const long long *batch_offsets, double Lx, double Ly, double Lz,
                           const c21cm_bispec_bins *bins, double *bispectrum, long long *n_triangles, void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    int *groups = NULL, *slot = NULL;
    if (!bins) return bs_fail("bins are required");
    if (!field || !bispectrum || !n_triangles || !batch_offsets) return bs_fail("a required pointer is NULL");
    if (nx < 2 || ny < 2 || nz < 2) return bs_fail("every axis needs at least 2 cells");
    if ((long long)nx * ny > 0x7FFFFFFFll) return bs_fail("nx * ny must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return bs_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return bs_fail("row_pitch must be >= nz");
    if (!(isfinite(Lx) && isfinite(Ly) && isfinite(Lz) && Lx > 0 && Ly > 0 && Lz > 0))
        return bs_fail("box lengths must be positive and finite");
    const int n_bins = bins->n_bins, n_tri = bins->n_triangles;
    if (n_bins < 1 || n_bins > BS_MAXB) {
        c21hip_set_error("bispectrum: n_bins must be in [1, %d], got %d", BS_MAXB, n_bins);
        return C21CM_VALUE_ERROR;
    }
    const double *e = bins->edges;
    if (!e) return bs_fail("edges are required");
    for (int i = 0; i <= n_bins; ++i)
        if (!isfinite(e[i]) || (i && !(e[i] > e[i - 1]))) return bs_fail("bin edges must be finite and increasing");
    if (!(e[0] > 0)) return bs_fail("the first edge must be > 0 (k = 0 is in no shell)");
    /* beyond this a triplet could close modulo the grid, or a Nyquist mode sit in a shell */
    const double L[3] = {Lx, Ly, Lz};
    double kny = 3.141592653589793 * (double)nx / Lx;
    if (3.141592653589793 * (double)ny / Ly < kny) kny = 3.141592653589793 * (double)ny / Ly;
    if (3.141592653589793 * (double)nz / Lz < kny) kny = 3.141592653589793 * (double)nz / Lz;
    const double kmax = (2.0 / 3.0) * kny;
    if (e[n_bins] > kmax) {
        c21hip_set_error("bispectrum: the last edge %.17g exceeds k_max = (2/3) min(pi n / L) = %.17g", e[n_bins], kmax);
        return C21CM_VALUE_ERROR;
    }
    if (n_tri < 1 || !bins->triangles) return bs_fail("at least one triangle is needed");
    for (int t = 0; t < n_tri; ++t) {
        const int *q = bins->triangles + 3 * (size_t)t;
        if (!(0 <= q[0] && q[0] <= q[1] && q[1] <= q[2] && q[2] < n_bins))
            return bs_fail("a triangle needs 0 <= b1 <= b2 <= b3 < n_bins");
    }
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return bs_fail("batch offsets must be >= 0");

    if (!cache_hit(nx, ny, nz, L, n_bins, e)) TRY(count_pass(nx, ny, nz, L, n_bins, e, stream));

    slot = (int *)malloc(sizeof(int) * (size_t)n_tri);
    if (!slot) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const int ng = build_groups(bins->triangles, n_tri, &groups, slot);
    if (ng < 0) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    /* one table buffer: kx ky kz thresholds (double) | offsets, counts (int64) | groups, slots (int) */
    const int nh = nz / 2 + 1;
    const size_t n_rows = (size_t)nx * ny;
    const size_t n_dbl = (size_t)nx + ny + nh + (size_t)n_bins + 1;
    const size_t n_i64 = (size_t)n_batch + (size_t)n_tri;
    const size_t n_int = (size_t)ng * BS_GI + (size_t)n_tri;
    const size_t tab_bytes = sizeof(double) * n_dbl + sizeof(long long) * n_i64 + sizeof(int) * n_int;
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    fill_ktab((double *)host_tab, nx, ny, nz, L, n_bins, e);
    long long *ho = (long long *)(host_tab + sizeof(double) * n_dbl), *hc = ho + n_batch;
    memcpy(ho, batch_offsets, sizeof(long long) * (size_t)n_batch);
    for (int t = 0; t < n_tri; ++t) {
        const int *q = bins->triangles + 3 * (size_t)t;
        hc[t] = g_cache.counts[((size_t)q[0] * n_bins + q[1]) * n_bins + q[2]];
    }
    int *hi = (int *)(hc + n_tri);
    memcpy(hi, groups, sizeof(int) * (size_t)ng * BS_GI);
    memcpy(hi + (size_t)ng * BS_GI, slot, sizeof(int) * (size_t)n_tri);

    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;
    const size_t plane = n_rows * 2 * (size_t)nh;
    const int n_slabs = c21hip_bispec_slabs(nx, ny, nz, NULL);
    const size_t part_dbl = (size_t)n_batch * n_slabs * ng * BS_G;
    const size_t rowsum_dbl = n_rows * (size_t)n_batch, out_dbl = (size_t)n_batch * n_tri;

    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_BS_TAB, tab_bytes);
    float *d_pad = (float *)c21hip_ws(WS_BS_PAD, sizeof(float) * plane * (size_t)n_batch);
    float *d_stack = (float *)c21hip_ws(WS_BS_STACK, sizeof(float) * plane * (size_t)n_bins);
    double *d_sums = (double *)c21hip_ws(WS_BS_SUMS, sizeof(double) * (part_dbl + rowsum_dbl + n_batch + out_dbl));
    int *d_bad = (int *)c21hip_ws(WS_BS_FLAG, sizeof(int));
    if (!d_tab || !d_pad || !d_stack || !d_sums || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_BS_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    c21hip_bispec_tabs t;
    set_tabs(&t, (const double *)d_tab, nx, ny, nz, n_bins);
    const long long *d_off = (const long long *)(d_tab + sizeof(double) * n_dbl), *d_counts = d_off + n_batch;
    const int *d_groups = (const int *)(d_counts + n_tri), *d_slot = d_groups + (size_t)ng * BS_GI;
    double *d_part = d_sums, *d_rowsum = d_part + part_dbl, *d_mean = d_rowsum + rowsum_dbl, *d_out = d_mean + n_batch;

    /* k = 0 is in no shell, so the mean the pack takes out is never missed */
    TRY(c21hip_power_pack(in, d_pad, nx, ny, nz, row_pitch, d_off, n_batch, d_rowsum, d_mean, NULL, NULL, d_bad, stream));
    TRY(c21hip_fft_r2c_batched(d_pad, nx, ny, nz, n_batch, stream));
    for (int b = 0; b < n_batch; ++b) {
        TRY(c21hip_bispec_fill(d_pad + (size_t)b * plane, d_stack, 0, nx, ny, nz, &t, stream));
        TRY(c21hip_fft_c2r_batched(d_stack, nx, ny, nz, n_bins, stream));
        TRY(c21hip_bispec_products(d_stack, 0, nx, ny, nz, d_groups, ng, d_part + (size_t)b * n_slabs * ng * BS_G,
                                   stream));
    }
    /* B = (V^2 / N^3) S / (N n_tri) */
    const double vol = Lx * Ly * Lz, n_cells = (double)nx * (double)ny * (double)nz;
    TRY(c21hip_bispec_finish(d_part, n_batch, n_slabs, ng * BS_G, d_slot, n_tri, vol * vol / (n_cells * n_cells * n_cells),
                             n_cells, d_counts, d_out, NULL, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("bispectrum: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    void *dst[2] = {bispectrum, n_triangles};
    const void *from[2] = {d_out, d_counts};
    const size_t nb[2] = {sizeof(double) * out_dbl, sizeof(long long) * (size_t)n_tri};
    for (int q = 0; q < 2; ++q) {
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    free(groups);
    free(slot);
    return status;
}
