/*
 * cluster_driver.c -- C host driver of the friends-of-friends clusters of boxes and lightcone chunks (DESIGN 4.11;
 * the estimator is written down at c21cm_bubble_clusters_grids, include/c21cm_grid.h, and its spec is
 * tests/cluster_reference.py): threshold and pack (bubble_kernels.hip) -> labels and sizes -> root mask and its
 * rank tables -> cluster lists, histograms and stats (csrc/hip/cluster_kernels.hip).  All boxes of a call go through
 * one launch per kernel.
 *
 * Device memory per box of N = nx ny nz cells in rows of W = ceil(nz / 64) words, M = nx ny W, C = ceil(M / 64):
 * 4 N (labels) + 4 N (sizes) + 2 x 8 M (the two masks) + 8 (M + C) + 4 C (rank tables) bytes: 8.4 N for rows of
 * whole words, 1.03 GiB at 512^3.
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

static int bc_fail(const char *msg) {
    c21hip_set_error("bubble clusters: %s", msg);
    return C21CM_VALUE_ERROR;
}

static size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

int c21cm_bubble_clusters_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                                const long long *batch_offsets, double threshold, int select_below,
                                int connectivity, int periodic_mask, int n_bins, const long long *edges,
                                long long *hist_n, long long *hist_cells, long long *stats, int *labels,
                                long long max_clusters, long long *cluster_roots, long long *cluster_sizes,
                                void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    if (!field || !batch_offsets || !edges || !hist_n || !hist_cells || !stats)
        return bc_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || nz < 1) return bc_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll || (long long)nx * ny * nz > 0x7FFFFFFFll)
        return bc_fail("nx * ny * nz must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return bc_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return bc_fail("row_pitch must be >= nz");
    if (!isfinite(threshold)) return bc_fail("the threshold must be finite");
    if (connectivity < 1 || connectivity > 3)
        return bc_fail("connectivity must be 1 (faces), 2 (and edges) or 3 (and corners)");
    if (periodic_mask < 0 || periodic_mask > 7) return bc_fail("periodic_mask must be in [0, 7]");
    if (n_bins < 1 || n_bins > C21HIP_BUBBLE_MAX_BINS) {
        c21hip_set_error("bubble clusters: n_bins must be in [1, %d] (the LDS of one workgroup), got %d",
                         C21HIP_BUBBLE_MAX_BINS, n_bins);
        return C21CM_VALUE_ERROR;
    }
    for (int i = 1; i <= n_bins; ++i)
        if (!(edges[i] > edges[i - 1])) return bc_fail("bin edges must be increasing");
    if (edges[0] < 1) return bc_fail("the first edge must be >= 1");
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return bc_fail("batch offsets must be >= 0");
    if ((cluster_roots != NULL) != (cluster_sizes != NULL))
        return bc_fail("cluster_roots and cluster_sizes are given as both or neither");
    if (cluster_roots && max_clusters < 1) return bc_fail("max_clusters must be >= 1 with the cluster arrays");
    if (!cluster_roots) max_clusters = 0;

    const size_t n_rows = (size_t)nx * ny, cells = n_rows * (size_t)nz;
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;
    const size_t words = n_rows * (size_t)((nz + 63) / 64);
    const size_t chunks = (words + C21HIP_BUBBLE_CHUNK - 1) / C21HIP_BUBBLE_CHUNK;

    /* one table buffer: edges (int64) | offsets (int64) */
    const size_t n_edges = (size_t)n_bins + 1;
    const size_t tab_bytes = sizeof(long long) * (n_edges + (size_t)n_batch);
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) return C21CM_MEMORY_ALLOC_ERROR;
    memcpy(host_tab, edges, sizeof(long long) * n_edges);
    memcpy(host_tab + sizeof(long long) * n_edges, batch_offsets, sizeof(long long) * (size_t)n_batch);

    /* mask: selection | roots
     * prefix: set bits before every word (int64) | chunk offsets (int64) | chunk counts (int)
     * out: stats [n_batch][4] | hist_n | hist_cells | root counts [n_batch][4] | keys [n_batch] | roots | sizes */
    const size_t nbt = (size_t)n_batch;
    const size_t stats_b = sizeof(long long) * 4 * nbt, hist_b = sizeof(long long) * nbt * (size_t)n_bins;
    const size_t key_b = sizeof(long long) * nbt, list_b = sizeof(long long) * nbt * (size_t)max_clusters;
    const size_t zero_b = 2 * stats_b + 2 * hist_b + key_b; /* everything before the lists; stats sits twice in it */
    const size_t label_b = sizeof(int) * cells * nbt;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_BC_TAB, tab_bytes);
    unsigned long long *d_mask =
        (unsigned long long *)c21hip_ws(WS_BC_MASK, 2 * sizeof(unsigned long long) * words * nbt);
    long long *d_prefix =
        (long long *)c21hip_ws(WS_BC_PREFIX, (sizeof(long long) * (words + chunks) + round8(sizeof(int) * chunks)) * nbt);
    int *d_label = (int *)c21hip_ws(WS_BC_LABEL, label_b);
    int *d_size = (int *)c21hip_ws(WS_BC_SIZE, label_b);
    unsigned char *d_out = (unsigned char *)c21hip_ws(WS_BC_OUT, zero_b + 2 * list_b);
    int *d_bad = (int *)c21hip_ws(WS_BC_FLAG, sizeof(int));
    if (!d_tab || !d_mask || !d_prefix || !d_label || !d_size || !d_out || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_BC_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    TRY(c21hip_memset(d_out, 0, zero_b + 2 * list_b, stream));
    const long long *d_edges = (const long long *)d_tab;
    const long long *d_off = d_edges + n_edges;
    unsigned long long *d_root_mask = d_mask + words * nbt;
    long long *d_chunk_off = d_prefix + words * nbt;
    int *d_chunk_sum = (int *)(d_chunk_off + chunks * nbt);
    long long *d_stats = (long long *)d_out;
    unsigned long long *d_hist_n = (unsigned long long *)(d_out + stats_b);
    unsigned long long *d_hist_cells = (unsigned long long *)(d_out + stats_b + hist_b);
    long long *d_n_clusters = (long long *)(d_out + stats_b + 2 * hist_b);
    unsigned long long *d_best = (unsigned long long *)(d_out + 2 * stats_b + 2 * hist_b);
    long long *d_roots = cluster_roots ? (long long *)(d_out + zero_b) : NULL;
    long long *d_sizes = cluster_roots ? (long long *)(d_out + zero_b + list_b) : NULL;
    if (d_roots) TRY(c21hip_memset(d_roots, 0xFF, list_b, stream)); /* -1: no cluster */

    TRY(c21hip_bubble_pack(in, nx, ny, nz, row_pitch, d_off, n_batch, threshold, select_below != 0, d_mask, d_chunk_sum,
                           d_bad, stream));
    /* n_selected; the rank tables of the selection are not used and are overwritten by those of the roots */
    TRY(c21hip_bubble_rank(d_mask, d_chunk_sum, nx, ny, nz, n_batch, d_chunk_off, d_prefix, d_stats, stream));
    TRY(c21hip_cluster_label(d_mask, nx, ny, nz, n_batch, connectivity, periodic_mask, d_label, d_size, stream));
    TRY(c21hip_cluster_roots(d_label, nx, ny, nz, n_batch, d_root_mask, d_chunk_sum, stream));
    TRY(c21hip_bubble_rank(d_root_mask, d_chunk_sum, nx, ny, nz, n_batch, d_chunk_off, d_prefix, d_n_clusters, stream));
    c21hip_cluster_emit_args a;
    memset(&a, 0, sizeof(a));
    a.root_mask = d_root_mask;
    a.prefix = d_prefix;
    a.n_clusters = d_n_clusters;
    a.size = d_size;
    a.nx = nx;
    a.ny = ny;
    a.nz = nz;
    a.n_batch = n_batch;
    a.n_bins = n_bins;
    a.edges = d_edges;
    a.hist_n = d_hist_n;
    a.hist_cells = d_hist_cells;
    a.best = d_best;
    a.stats = d_stats;
    a.max_clusters = max_clusters;
    a.roots = d_roots;
    a.sizes = d_sizes;
    TRY(c21hip_cluster_emit(&a, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("bubble clusters: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    void *dst[6] = {stats, hist_n, hist_cells, labels, cluster_roots, cluster_sizes};
    const void *from[6] = {d_stats, d_hist_n, d_hist_cells, d_label, d_roots, d_sizes};
    const size_t nb[6] = {stats_b, hist_b, hist_b, label_b, list_b, list_b};
    for (int q = 0; q < 6; ++q) {
        if (!dst[q]) continue;
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    return status;
}
