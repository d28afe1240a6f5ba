/*
 * bubble_driver.c -- C host driver of the mean-free-path bubble size distribution of boxes and lightcone chunks
 * (the estimator is written down at c21cm_bubble_sizes_grids, include/c21cm_grid.h, and its spec is
 * tests/bubble_reference.py): threshold and pack -> counts and rank tables -> ray walk
 * (csrc/hip/bubble_kernels.hip).  All boxes of a call go through one launch per kernel.
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

static int bu_fail(const char *msg) {
    c21hip_set_error("bubble sizes: %s", msg);
    return C21CM_VALUE_ERROR;
}

static size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

int c21cm_bubble_sizes_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                             const long long *batch_offsets, double Lx, double Ly, double Lz, double threshold,
                             int select_below, long long n_rays, unsigned long long seed, int directions,
                             int periodic_mask, double max_length, int n_bins, const double *edges, long long *hist,
                             long long *stats, double *lengths, unsigned char *flags, long long *starts,
                             void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    if (!field || !batch_offsets || !edges || !hist || !stats) return bu_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || nz < 1) return bu_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll) return bu_fail("nx * ny must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return bu_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return bu_fail("row_pitch must be >= nz");
    if (!(isfinite(Lx) && isfinite(Ly) && isfinite(Lz) && Lx > 0 && Ly > 0 && Lz > 0))
        return bu_fail("box lengths must be positive and finite");
    if (!isfinite(threshold)) return bu_fail("the threshold must be finite");
    if (n_rays < 1 || n_rays > 0x7FFFFFFFll) return bu_fail("n_rays must be in [1, 2^31 - 1]");
    if (directions != 0 && directions != 1) return bu_fail("directions must be 0 (isotropic) or 1 (line of sight)");
    if (periodic_mask < 0 || periodic_mask > 7) return bu_fail("periodic_mask must be in [0, 7]");
    if (!(isfinite(max_length) && max_length > 0)) return bu_fail("max_length must be positive and finite");
    if (n_bins < 1 || n_bins > C21HIP_BUBBLE_MAX_BINS) {
        c21hip_set_error("bubble sizes: n_bins must be in [1, %d] (the LDS of one workgroup), got %d",
                         C21HIP_BUBBLE_MAX_BINS, n_bins);
        return C21CM_VALUE_ERROR;
    }
    for (int i = 0; i <= n_bins; ++i)
        if (!isfinite(edges[i]) || (i && !(edges[i] > edges[i - 1])))
            return bu_fail("bin edges must be finite and increasing");
    if (edges[0] < 0) return bu_fail("the first edge must be >= 0");
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return bu_fail("batch offsets must be >= 0");
    const double cell[3] = {Lx / (double)nx, Ly / (double)ny, Lz / (double)nz};
    const double steps = ceil(max_length / cell[0]) + ceil(max_length / cell[1]) + ceil(max_length / cell[2]) + 3.0;
    if (!(steps < 2147483648.0)) return bu_fail("max_length spans 2^31 cells or more");

    const size_t n_rows = (size_t)nx * ny;
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;
    const size_t words = n_rows * (size_t)((nz + 63) / 64);
    const size_t chunks = (words + C21HIP_BUBBLE_CHUNK - 1) / C21HIP_BUBBLE_CHUNK;
    if (chunks > 0x7FFFFFFFull) return bu_fail("the box is too large for one launch");

    /* one table buffer: edges (double) | offsets (int64) */
    const size_t n_edges = (size_t)n_bins + 1;
    const size_t tab_bytes = sizeof(double) * n_edges + sizeof(long long) * (size_t)n_batch;
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) return C21CM_MEMORY_ALLOC_ERROR;
    memcpy(host_tab, edges, sizeof(double) * n_edges);
    memcpy(host_tab + sizeof(double) * n_edges, batch_offsets, sizeof(long long) * (size_t)n_batch);

    /* prefix: set bits before every word (int64) | chunk offsets (int64) | chunk counts (int)
     * out: stats [n_batch][4] | hist [n_batch][n_bins] | lengths | starts | flags, the last three where asked for */
    const size_t n_out = (size_t)n_batch * (size_t)n_rays;
    const size_t stats_b = sizeof(long long) * 4 * (size_t)n_batch, hist_b = sizeof(long long) * (size_t)n_batch * n_bins;
    const size_t len_b = lengths ? sizeof(double) * n_out : 0, start_b = starts ? sizeof(long long) * n_out : 0;
    const size_t flag_b = flags ? round8(n_out) : 0;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_BU_TAB, tab_bytes);
    unsigned long long *d_mask =
        (unsigned long long *)c21hip_ws(WS_BU_MASK, sizeof(unsigned long long) * words * (size_t)n_batch);
    long long *d_prefix = (long long *)c21hip_ws(
        WS_BU_PREFIX, (sizeof(long long) * (words + chunks) + round8(sizeof(int) * chunks)) * (size_t)n_batch);
    unsigned char *d_out = (unsigned char *)c21hip_ws(WS_BU_OUT, stats_b + hist_b + len_b + start_b + flag_b);
    int *d_bad = (int *)c21hip_ws(WS_BU_FLAG, sizeof(int));
    if (!d_tab || !d_mask || !d_prefix || !d_out || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_BU_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    TRY(c21hip_memset(d_out, 0, stats_b + hist_b, stream));
    const double *d_edges = (const double *)d_tab;
    const long long *d_off = (const long long *)(d_tab + sizeof(double) * n_edges);
    long long *d_chunk_off = d_prefix + words * (size_t)n_batch;
    int *d_chunk_sum = (int *)(d_chunk_off + chunks * (size_t)n_batch);
    long long *d_stats = (long long *)d_out;
    unsigned long long *d_hist = (unsigned long long *)(d_out + stats_b);
    double *d_len = lengths ? (double *)(d_out + stats_b + hist_b) : NULL;
    long long *d_start = starts ? (long long *)(d_out + stats_b + hist_b + len_b) : NULL;
    unsigned char *d_flags = flags ? d_out + stats_b + hist_b + len_b + start_b : NULL;

    TRY(c21hip_bubble_pack(in, nx, ny, nz, row_pitch, d_off, n_batch, threshold, select_below != 0, d_mask, d_chunk_sum,
                           d_bad, stream));
    TRY(c21hip_bubble_rank(d_mask, d_chunk_sum, nx, ny, nz, n_batch, d_chunk_off, d_prefix, d_stats, stream));
    c21hip_bubble_walk_args a;
    memset(&a, 0, sizeof(a));
    a.mask = d_mask;
    a.prefix = d_prefix;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.n_batch = n_batch;
    for (int q = 0; q < 3; ++q) {
        a.cell[q] = cell[q];
        a.periodic[q] = (periodic_mask >> q) & 1;
    }
    a.max_length = max_length;
    a.los = directions;
    a.n_rays = n_rays;
    a.max_steps = (long long)steps;
    a.seed = seed;
    a.n_bins = n_bins;
    a.edges = d_edges;
    a.hist = d_hist;
    a.stats = d_stats;
    a.lengths = d_len;
    a.flags = d_flags;
    a.starts = d_start;
    TRY(c21hip_bubble_walk(&a, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("bubble sizes: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    void *dst[5] = {stats, hist, lengths, starts, flags};
    const void *from[5] = {d_stats, d_hist, d_len, d_start, d_flags};
    const size_t nb[5] = {stats_b, hist_b, len_b, start_b, flags ? n_out : 0};
    for (int q = 0; q < 5; ++q) {
        if (!dst[q]) continue;
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    return status;
}
