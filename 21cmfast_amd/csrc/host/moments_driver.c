/*
 * moments_driver.c -- C host driver of the one-point statistics of boxes and lightcone chunks:
 * pass 1 the fp64 mean, pass 2 the central moments and the histogram (csrc/hip/moments_kernels.hip).  All boxes
 * of a call go through one launch per pass.
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

static int mo_fail(const char *msg) {
    c21hip_set_error("field moments: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_field_moments_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                              const long long *batch_offsets, int n_bins, const double *edges, double *moments,
                              long long *hist, void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    if (!field || !moments || !batch_offsets) return mo_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || nz < 1) return mo_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll) return mo_fail("nx * ny must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return mo_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return mo_fail("row_pitch must be >= nz");
    if (n_bins < 0) return mo_fail("n_bins must be >= 0");
    if (n_bins > C21HIP_MOMENTS_MAX_BINS) {
        c21hip_set_error("field moments: %d histogram bins do not fit the LDS of one workgroup (at most %d)", n_bins,
                         C21HIP_MOMENTS_MAX_BINS);
        return C21CM_VALUE_ERROR;
    }
    if (n_bins > 0) {
        if (!edges || !hist) return mo_fail("a histogram needs edges and an output array");
        for (int i = 0; i <= n_bins; ++i)
            if (!isfinite(edges[i]) || (i && !(edges[i] > edges[i - 1])))
                return mo_fail("bin edges must be finite and increasing");
    }
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return mo_fail("batch offsets must be >= 0");

    const size_t n_rows = (size_t)nx * ny;
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;

    /* one table buffer: edges (double) | offsets (int64) */
    const size_t n_edges = n_bins > 0 ? (size_t)n_bins + 1 : 0;
    const size_t tab_bytes = sizeof(double) * n_edges + sizeof(long long) * (size_t)n_batch;
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) return C21CM_MEMORY_ALLOC_ERROR;
    if (n_edges) memcpy(host_tab, edges, sizeof(double) * n_edges);
    memcpy(host_tab + sizeof(double) * n_edges, batch_offsets, sizeof(long long) * (size_t)n_batch);

    /* sums: row sums [3][n_batch][rows] | their first-level sums | mean [n_batch] | moments [n_batch][4] | hist
     * [n_batch][n_bins] (int64) */
    const size_t part_dbl = c21hip_moments_part_doubles(nx, ny, n_batch);
    const size_t rowsum_dbl = 3 * n_rows * (size_t)n_batch, mom_dbl = 4 * (size_t)n_batch;
    const size_t hist_n = (size_t)n_batch * (size_t)n_bins;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_MO_TAB, tab_bytes);
    double *d_sums = (double *)c21hip_ws(WS_MO_SUMS, sizeof(double) * (rowsum_dbl + part_dbl + n_batch + mom_dbl + hist_n));
    int *d_bad = (int *)c21hip_ws(WS_MO_FLAG, sizeof(int));
    if (!d_tab || !d_sums || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_MO_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    const double *d_edges = n_edges ? (const double *)d_tab : NULL;
    const long long *d_off = (const long long *)(d_tab + sizeof(double) * n_edges);
    double *d_part = d_sums + rowsum_dbl, *d_mean = d_part + part_dbl, *d_mom = d_mean + n_batch;
    unsigned long long *d_hist = (unsigned long long *)(d_mom + mom_dbl);

    TRY(c21hip_moments_mean(in, nx, ny, nz, row_pitch, d_off, n_batch, d_sums, d_part, d_mean, d_bad, stream));
    TRY(c21hip_moments_central(in, nx, ny, nz, row_pitch, d_off, n_batch, d_mean, n_bins, d_edges, d_sums, d_part, d_mom,
                               n_bins > 0 ? d_hist : NULL, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("field moments: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    void *dst[2] = {moments, hist};
    const void *from[2] = {d_mom, d_hist};
    const size_t nb[2] = {sizeof(double) * mom_dbl, sizeof(long long) * hist_n};
    for (int q = 0; q < (n_bins > 0 ? 2 : 1); ++q) {
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    return status;
}
