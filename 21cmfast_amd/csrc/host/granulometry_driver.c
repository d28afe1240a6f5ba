/*
 * granulometry_driver.c -- C host driver of the squared distance transforms and granulometry bubble sizes of boxes
 * and lightcone chunks (the estimator is written down at c21cm_granulometry_grids,
 * include/c21cm_grid.h, and its spec is tests/granulometry_reference.py): threshold and pack, n_selected
 * (bubble_kernels.hip) -> D2, erosion counts and stats -> one read-back (the non-finite flag and max D2) -> one
 * three-pass transform per radius below max D2 (csrc/hip/granulometry_kernels.hip).  All boxes of a call go through
 * one launch per kernel.
 *
 * Device memory per box of N = nx ny nz cells in rows of W = ceil(nz / 64) words, M = nx ny W, C = ceil(M / 64):
 * 4 N (D2) + 2 x 4 N (the two work boxes) + 4 N (level, where asked for) + 8 M (mask) + 8 (M + C) + 4 C (rank
 * scratch) bytes: 12.3 N, or 16.3 N with level, for rows of whole words; 1.5 / 2.0 GiB at 512^3.  A host field is
 * staged in 4 N more.
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

static int gr_fail(const char *msg) {
    c21hip_set_error("granulometry: %s", msg);
    return C21CM_VALUE_ERROR;
}

static size_t round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

int c21cm_granulometry_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                             const long long *batch_offsets, double threshold, int select_below, int periodic_mask,
                             int n_radii, const long long *radii2, long long *covered, long long *eroded,
                             long long *stats, int *dist2, int *level, void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    long long *host_stats = NULL;
    if (!field || !batch_offsets || !stats) return gr_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || nz < 1) return gr_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll || (long long)nx * ny * nz > 0x7FFFFFFFll)
        return gr_fail("nx * ny * nz must be below 2^31");
    if ((long long)nx * nx + (long long)ny * ny + (long long)nz * nz >= (long long)C21CM_EDT_NONE)
        return gr_fail("nx^2 + ny^2 + nz^2 must be below 2^30");
    if (n_batch < 1 || n_batch > 65535) return gr_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return gr_fail("row_pitch must be >= nz");
    if (!isfinite(threshold)) return gr_fail("the threshold must be finite");
    if (periodic_mask < 0 || periodic_mask > 7) return gr_fail("periodic_mask must be in [0, 7]");
    if (n_radii < 0 || n_radii > C21HIP_GRAN_MAX_RADII) {
        c21hip_set_error("granulometry: n_radii must be in [0, %d], got %d", C21HIP_GRAN_MAX_RADII, n_radii);
        return C21CM_VALUE_ERROR;
    }
    if (n_radii > 0 && (!radii2 || !covered || !eroded))
        return gr_fail("radii2, covered and eroded are required with n_radii >= 1");
    for (int k = 0; k < n_radii; ++k)
        if (radii2[k] < 0 || (k > 0 && !(radii2[k] > radii2[k - 1])))
            return gr_fail("squared radii must be >= 0 and strictly increasing");
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return gr_fail("batch offsets must be >= 0");

    const size_t n_rows = (size_t)nx * ny, cells = n_rows * (size_t)nz;
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;
    const size_t words = n_rows * (size_t)((nz + 63) / 64);
    const size_t chunks = (words + C21HIP_BUBBLE_CHUNK - 1) / C21HIP_BUBBLE_CHUNK;

    /* one table buffer: radii (int64, at least one entry) | offsets (int64) */
    const size_t nbt = (size_t)n_batch, n_tab = n_radii > 0 ? (size_t)n_radii : 1;
    const size_t tab_bytes = sizeof(long long) * (n_tab + nbt);
    const size_t stats_b = sizeof(long long) * 4 * nbt;
    host_tab = (unsigned char *)calloc(1, tab_bytes);
    host_stats = (long long *)malloc(stats_b);
    if (!host_tab || !host_stats) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    if (n_radii > 0) memcpy(host_tab, radii2, sizeof(long long) * (size_t)n_radii);
    memcpy(host_tab + sizeof(long long) * n_tab, batch_offsets, sizeof(long long) * nbt);

    /* out: stats [n_batch][4] | covered | eroded | erosion histogram [n_batch][256] | keys [n_batch] */
    const size_t rad_b = sizeof(long long) * nbt * (size_t)n_radii;
    const size_t hist_b = sizeof(long long) * nbt * (C21HIP_GRAN_MAX_RADII + 1), key_b = sizeof(long long) * nbt;
    const size_t out_b = stats_b + 2 * rad_b + hist_b + key_b;
    const size_t box_b = sizeof(int) * cells * nbt;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_GR_TAB, tab_bytes);
    unsigned long long *d_mask = (unsigned long long *)c21hip_ws(WS_GR_MASK, sizeof(unsigned long long) * words * nbt);
    long long *d_prefix =
        (long long *)c21hip_ws(WS_GR_PREFIX, (sizeof(long long) * (words + chunks) + round8(sizeof(int) * chunks)) * nbt);
    int *d_d2 = (int *)c21hip_ws(WS_GR_D2, box_b);
    int *d_a = (int *)c21hip_ws(WS_GR_WORK_A, box_b);
    int *d_b = (int *)c21hip_ws(WS_GR_WORK_B, box_b);
    int *d_level = level ? (int *)c21hip_ws(WS_GR_LEVEL, box_b) : NULL;
    unsigned char *d_out = (unsigned char *)c21hip_ws(WS_GR_OUT, out_b);
    int *d_bad = (int *)c21hip_ws(WS_GR_FLAG, sizeof(int));
    if (!d_tab || !d_mask || !d_prefix || !d_d2 || !d_a || !d_b || (level && !d_level) || !d_out || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_GR_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    TRY(c21hip_memset(d_out, 0, out_b, stream));
    const long long *d_radii = (const long long *)d_tab;
    const long long *d_off = d_radii + n_tab;
    long long *d_chunk_off = d_prefix + words * nbt;
    int *d_chunk_sum = (int *)(d_chunk_off + chunks * nbt);
    long long *d_stats = (long long *)d_out;
    unsigned long long *d_covered = (unsigned long long *)(d_out + stats_b);
    long long *d_eroded = (long long *)(d_out + stats_b + rad_b);
    unsigned long long *d_hist = (unsigned long long *)(d_out + stats_b + 2 * rad_b);
    unsigned long long *d_key = (unsigned long long *)(d_out + stats_b + 2 * rad_b + hist_b);

    TRY(c21hip_bubble_pack(in, nx, ny, nz, row_pitch, d_off, n_batch, threshold, select_below != 0, d_mask, d_chunk_sum,
                           d_bad, stream));
    TRY(c21hip_bubble_rank(d_mask, d_chunk_sum, nx, ny, nz, n_batch, d_chunk_off, d_prefix, d_stats, stream)); /* n_selected */
    TRY(c21hip_gran_edt(d_mask, nx, ny, nz, n_batch, periodic_mask, n_radii, d_radii, d_a, d_b, d_d2, d_level, d_hist,
                        d_key, d_eroded, d_stats, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_d2h(host_stats, d_stats, stats_b, stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("granulometry: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    /* a radius at or above the largest D2 of the call covers nothing: its row stays zero without a launch */
    long long deepest = 0;
    for (int b = 0; b < n_batch; ++b)
        if (host_stats[4 * b + 1] > deepest) deepest = host_stats[4 * b + 1];
    for (int k = 0; k < n_radii && radii2[k] < deepest; ++k)
        TRY(c21hip_gran_cover(d_d2, nx, ny, nz, n_batch, periodic_mask, (int)radii2[k], k, n_radii, d_stats, d_a, d_b,
                              d_covered, d_level, stream));
    void *dst[5] = {stats, covered, eroded, dist2, level};
    const void *from[5] = {d_stats, d_covered, d_eroded, d_d2, d_level};
    const size_t nb[5] = {stats_b, rad_b, rad_b, box_b, box_b};
    for (int q = 0; q < 5; ++q) {
        if (!dst[q] || !nb[q]) continue;
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    free(host_stats);
    return status;
}
