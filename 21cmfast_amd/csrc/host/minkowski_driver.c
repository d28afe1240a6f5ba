/*
 * minkowski_driver.c -- C host driver of the Minkowski functionals of boxes and lightcone chunks (the
 * estimator is written down at c21cm_minkowski_grids, include/c21cm_grid.h, and its spec is
 * tests/minkowski_reference.py): one pass over the field histograms the 8 element kinds of the cubical complex over
 * the level at which they enter the excursion set, and a finish kernel sums the histograms into the counts of every
 * threshold (csrc/hip/minkowski_kernels.hip).  All boxes of a call go through one launch per kernel.
 *
 * Device memory beyond the field: 8 (n_thresholds + 1) + 8 n_thresholds counters of 8 bytes per box.
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

static int mk_fail(const char *msg) {
    c21hip_set_error("minkowski: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_minkowski_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                          const long long *batch_offsets, int n_thresholds, const double *thresholds,
                          int select_below, int periodic_mask, long long *counts, void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    if (!field || !batch_offsets || !thresholds || !counts) return mk_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || nz < 1) return mk_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll || (long long)nx * ny * nz > 0x7FFFFFFFll)
        return mk_fail("nx * ny * nz must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return mk_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return mk_fail("row_pitch must be >= nz");
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return mk_fail("batch offsets must be >= 0");
    if (n_thresholds < 1 || n_thresholds > C21HIP_MINKOWSKI_MAX_THRESHOLDS) {
        c21hip_set_error("minkowski: n_thresholds must be in [1, %d] (a level fits a byte), got %d",
                         C21HIP_MINKOWSKI_MAX_THRESHOLDS, n_thresholds);
        return C21CM_VALUE_ERROR;
    }
    for (int i = 0; i < n_thresholds; ++i) {
        if (!isfinite(thresholds[i])) return mk_fail("thresholds must be finite");
        if (i && !(thresholds[i] > thresholds[i - 1])) return mk_fail("thresholds must be strictly increasing");
    }
    if (periodic_mask < 0 || periodic_mask > 7) return mk_fail("periodic_mask must be in [0, 7]");

    const size_t n_rows = (size_t)nx * ny;
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (n_rows - 1) * (size_t)row_pitch + (size_t)nz;

    /* one table buffer: thresholds (fp64) | offsets (int64) */
    const size_t nbt = (size_t)n_batch, nt = (size_t)n_thresholds;
    const size_t tab_bytes = sizeof(double) * nt + sizeof(long long) * nbt;
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) return C21CM_MEMORY_ALLOC_ERROR;
    memcpy(host_tab, thresholds, sizeof(double) * nt);
    memcpy(host_tab + sizeof(double) * nt, batch_offsets, sizeof(long long) * nbt);

    /* out: level histograms [n_batch][8][n_thresholds + 1] | counts [n_batch][n_thresholds][8] */
    const size_t hist_b = sizeof(long long) * nbt * 8 * (nt + 1), counts_b = sizeof(long long) * nbt * nt * 8;
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_MK_TAB, tab_bytes);
    unsigned char *d_out = (unsigned char *)c21hip_ws(WS_MK_OUT, hist_b + counts_b);
    int *d_bad = (int *)c21hip_ws(WS_MK_FLAG, sizeof(int));
    if (!d_tab || !d_out || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_MK_IN, field, sizeof(float) * extent, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    TRY(c21hip_memset(d_out, 0, hist_b + counts_b, stream));
    const double *d_thr = (const double *)d_tab;
    const long long *d_off = (const long long *)(d_tab + sizeof(double) * nt);
    unsigned long long *d_hist = (unsigned long long *)d_out;
    long long *d_counts = (long long *)(d_out + hist_b);

    TRY(c21hip_minkowski(in, nx, ny, nz, row_pitch, d_off, n_batch, n_thresholds, d_thr, select_below != 0,
                         periodic_mask, d_hist, d_counts, d_bad, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("minkowski: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    if (c21hip_is_device_ptr(counts)) TRY(c21hip_d2d(counts, d_counts, counts_b, stream));
    else TRY(c21hip_d2h(counts, d_counts, counts_b, stream));
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    return status;
}
