/*
 * observe_driver.c -- C host driver of the telescope-resolution smoothing of boxes and lightcones (the
 * definition is written down at c21cm_observe_smooth_grids, include/c21cm_grid.h, and its spec is
 * tests/observe_reference.py): slice means and the non-finite flag -> one read-back -> beam along x -> beam along y
 * -> channel along the line of sight (csrc/hip/observe_kernels.hip).  A pass that would change nothing is not
 * launched: the beam passes where every slice has lw = 0, the channel pass where every count is 0.  The pass that
 * runs first subtracts the means as it loads; the pass that runs last writes the result.
 *
 * The weight table is built here in fp64 as the spec says and rounded to fp32.  It is uploaded with the half-kernel
 * index d as its slow axis, tab[d][s], zero beyond a slice's lw, so that the 64 lanes of a wave -- 64 slices -- read
 * one contiguous segment per d.
 *
 * Device memory for N = nx ny ns cells: 4 N per pass but the last (at most two work boxes), 4 N for a host result,
 * 4 N for a staged host field, 8 (4 parts + 1) ns for the means, 4 (lw_max + 4) ns for the tables.
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

static int ob_fail(const char *msg) {
    c21hip_set_error("observe: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_observe_smooth_grids(const float *field, int nx, int ny, int ns, const double *sigma_cells,
                               const int *los_below, const int *los_above, int periodic_los, int subtract_mean,
                               float *out, double *slice_means, void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    if (!field || !sigma_cells || !los_below || !los_above || !out) return ob_fail("a required pointer is NULL");
    if (nx < 1 || ny < 1 || ns < 1) return ob_fail("every axis needs at least 1 cell");
    if ((long long)nx * ny > 0x7FFFFFFFll || (long long)nx * ny * ns > 0x7FFFFFFFll)
        return ob_fail("nx * ny * ns must be below 2^31");
    int lw_max = 0, any_channel = 0;
    for (int s = 0; s < ns; ++s) {
        const double sg = sigma_cells[s];
        if (!isfinite(sg) || sg < 0.0) {
            c21hip_set_error("observe: sigma_cells[%d] = %g must be finite and >= 0", s, sg);
            return C21CM_VALUE_ERROR;
        }
        if (sg > (double)C21HIP_OBSERVE_MAX_LW / 4.0) {
            c21hip_set_error("observe: sigma_cells[%d] = %g is above the limit of %d cells", s, sg,
                             C21HIP_OBSERVE_MAX_LW / 4);
            return C21CM_VALUE_ERROR;
        }
        const int lw = (int)(4.0 * sg + 0.5);
        if (lw > lw_max) lw_max = lw;
        if (los_below[s] < 0 || los_above[s] < 0) {
            c21hip_set_error("observe: the channel counts of slice %d are (%d, %d), must be >= 0", s, los_below[s],
                             los_above[s]);
            return C21CM_VALUE_ERROR;
        }
        if (periodic_los && (long long)los_below[s] + los_above[s] + 1 > (long long)ns) {
            c21hip_set_error("observe: the periodic channel of slice %d spans %lld slices of %d", s,
                             (long long)los_below[s] + los_above[s] + 1, ns);
            return C21CM_VALUE_ERROR;
        }
        any_channel |= los_below[s] > 0 || los_above[s] > 0;
    }
    const size_t cells = (size_t)nx * ny * (size_t)ns, box_b = sizeof(float) * cells;
    {
        const uintptr_t a = (uintptr_t)field, b = (uintptr_t)out;
        if (a < b + box_b && b < a + box_b) return ob_fail("out must not overlap field");
    }

    /* tab[lw_max + 1][ns] | lw[ns] | lw_block[n_sb] | below[ns] | above[ns], 4 bytes each */
    const size_t n_sb = ((size_t)ns + 63) / 64, nsz = (size_t)ns;
    const size_t tab_n = ((size_t)lw_max + 1) * nsz;
    const size_t tab_bytes = 4 * (tab_n + 3 * nsz + n_sb);
    host_tab = (unsigned char *)calloc(1, tab_bytes);
    double *half = (double *)malloc(sizeof(double) * ((size_t)lw_max + 1));
    if (!host_tab || !half) {
        free(half);
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    float *h_tab = (float *)host_tab;
    int *h_lw = (int *)(h_tab + tab_n), *h_lwb = h_lw + nsz, *h_below = h_lwb + n_sb, *h_above = h_below + nsz;
    for (int s = 0; s < ns; ++s) {
        const double sg = sigma_cells[s];
        const int lw = (int)(4.0 * sg + 0.5);
        h_lw[s] = lw;
        if (lw > h_lwb[s / 64]) h_lwb[s / 64] = lw;
        h_below[s] = los_below[s];
        h_above[s] = los_above[s];
        if (lw == 0) {
            h_tab[s] = 1.0f;
            continue;
        }
        double tail = 0.0;
        for (int d = 0; d <= lw; ++d) {
            half[d] = exp(-(double)d * (double)d / (2.0 * sg * sg));
            if (d) tail += half[d];
        }
        const double norm = half[0] + 2.0 * tail;
        for (int d = 0; d <= lw; ++d) h_tab[(size_t)d * nsz + (size_t)s] = (float)(half[d] / norm);
    }
    free(half);

    const int run_beam = lw_max > 0;
    /* with nothing else to run, the channel pass with its counts all 0 is what subtracts the means */
    const int run_channel = any_channel || (!run_beam && subtract_mean);
    const int n_pass = 2 * run_beam + run_channel;
    const int parts = c21hip_observe_mean_parts((long long)nx * ny);
    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_OB_TAB, tab_bytes);
    double *d_partial = (double *)c21hip_ws(WS_OB_MEANS, sizeof(double) * ((size_t)parts * 4 + 1) * nsz);
    int *d_bad = (int *)c21hip_ws(WS_OB_FLAG, sizeof(int));
    float *d_a = n_pass > 1 ? (float *)c21hip_ws(WS_OB_WORK_A, box_b) : NULL;
    float *d_b = n_pass > 2 ? (float *)c21hip_ws(WS_OB_WORK_B, box_b) : NULL;
    const int out_on_device = c21hip_is_device_ptr(out);
    float *d_out = out_on_device ? out : (float *)c21hip_ws(WS_OB_OUT, box_b);
    if (!d_tab || !d_partial || !d_bad || (n_pass > 1 && !d_a) || (n_pass > 2 && !d_b) || !d_out) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    const float *in = (const float *)c21_stage_in(WS_OB_IN, field, box_b, stream, &status);
    if (status) goto done;
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    const float *t_tab = (const float *)d_tab;
    const int *t_lw = (const int *)(t_tab + tab_n), *t_lwb = t_lw + nsz, *t_below = t_lwb + n_sb;
    const int *t_above = t_below + nsz;
    double *d_means = d_partial + (size_t)parts * 4 * nsz;

    TRY(c21hip_observe_means(in, nx, ny, ns, d_partial, d_means, d_bad, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) { /* before any output is touched */
        c21hip_set_error("observe: a field value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }

    const float *src = in;
    const double *sub = subtract_mean ? d_means : NULL; /* handed to the first pass alone */
    float *spare[2] = {d_a, d_b};
    int done_passes = 0;
    if (run_beam)
        for (int axis = 0; axis < 2; ++axis) {
            float *dst = ++done_passes == n_pass ? d_out : spare[axis];
            TRY(c21hip_observe_beam(src, dst, nx, ny, ns, axis, t_tab, t_lw, t_lwb, lw_max, sub, stream));
            src = dst;
            sub = NULL;
        }
    if (run_channel)
        TRY(c21hip_observe_channel(src, d_out, nx, ny, ns, t_below, t_above, periodic_los != 0, sub, stream));
    if (n_pass == 0) TRY(c21hip_d2d(d_out, in, box_b, stream));
    if (!out_on_device) TRY(c21hip_d2h(out, d_out, box_b, stream));
    if (slice_means) {
        if (c21hip_is_device_ptr(slice_means)) TRY(c21hip_d2d(slice_means, d_means, sizeof(double) * nsz, stream));
        else TRY(c21hip_d2h(slice_means, d_means, sizeof(double) * nsz, stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    return status;
}
