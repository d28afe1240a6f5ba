/*
 * angular_driver.c -- C host driver of the angular lightcone: the slices of one node pair
 * (src/py21cmfast/lightconers.py:162-287 make_lightcone_slices with AngularLightconer :541-701, as the
 * node loop of drivers/lightcone.py:544-575 calls it) and the periodic B-spline prefilter of the node
 * boxes for interpolation orders 3 and 5.  Host arrays are staged through workspace slots, device
 * arrays are used in place; a host lightcone receives only the slices of the call, as one 2-D copy per
 * field.  Non-finite inputs are reported once, after the launch.
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

static int ang_fail(const char *msg) {
    c21hip_set_error("angular lightcone: %s", msg);
    return C21CM_VALUE_ERROR;
}

static int popcount16(unsigned v) {
    int n = 0;
    for (int q = 0; q < C21CM_LC_MAX_FIELDS; ++q) n += (v >> q) & 1u;
    return n;
}

int c21cm_lightcone_angular_grids(const c21cm_angular_spec *s, const float *const *box_lo,
                                  const float *const *box_hi, float *const *lightcone, void *stream) {
    int status = 0;
    c21hip_ang_slice *tab = NULL;
    if (!s) return ang_fail("spec is required");
    if (s->hii_dim < 1 || s->hii_d_para < 1) return ang_fail("hii_dim and hii_d_para must be positive");
    if (s->n_pix < 0) return ang_fail("n_pix must be >= 0");
    if (s->n_slices < 1) return ang_fail("the lightcone has zero slices");
    if (s->i0 < 0 || s->i1 <= s->i0 || s->i1 > s->n_slices)
        return ang_fail("slice range [i0, i1) is empty or outside the lightcone");
    if (s->n_fields < 1 || s->n_fields > C21CM_LC_MAX_FIELDS) return ang_fail("n_fields outside 1 .. 16");
    if (s->order != 0 && s->order != 1 && s->order != 3 && s->order != 5)
        return ang_fail("order must be 0, 1, 3 or 5");
    const unsigned used = (unsigned)((1u << s->n_fields) - 1u);
    if ((s->mean_max | s->vector) & ~used) return ang_fail("mean_max / vector bits beyond n_fields");
    if (s->mean_max & s->vector) return ang_fail("a vector field cannot interpolate with mean_max");
    if (s->order >= 3 && s->mean_max)
        return ang_fail("mean_max needs interpolation order 0 or 1 (the spline coefficients are those of "
                        "the node boxes, not of the interpolated box)");
    if (!s->nhat || !s->distance || !s->w_lo || !s->w_hi)
        return ang_fail("nhat, distance, w_lo and w_hi are required");
    if (!(s->w_norm > 0.0) || !isfinite(s->w_norm)) return ang_fail("w_norm must be positive and finite");
    for (int k = 0; k < 3; ++k)
        if (!isfinite(s->origin[k])) return ang_fail("origin must be finite");
    if (!box_lo || !box_hi || !lightcone) return ang_fail("field pointer arrays are required");
    const int run = s->i1 - s->i0;
    /* |d| and |origin| below 1e12 cells: floor() and the tap indices stay exact */
    for (int j = 0; j < run; ++j) {
        if (!isfinite(s->distance[j]) || !isfinite(s->w_lo[j]) || !isfinite(s->w_hi[j]))
            return ang_fail("non-finite slice distance or weight");
        if (fabs(s->distance[j]) > 1e12) return ang_fail("slice distance beyond 1e12 cells");
    }
    for (int k = 0; k < 3; ++k)
        if (fabs(s->origin[k]) > 1e12) return ang_fail("origin beyond 1e12 cells");
    const int n_boxes = s->n_fields + 2 * popcount16(s->vector);
    for (int b = 0; b < n_boxes; ++b)
        if (!box_lo[b] || !box_hi[b]) return ang_fail("a node box pointer is NULL");
    for (int q = 0; q < s->n_fields; ++q)
        if (!lightcone[q]) return ang_fail("a lightcone pointer is NULL");
    if (s->n_pix == 0) return 0;

    const size_t n_pix = (size_t)s->n_pix;
    const size_t box_elems = (size_t)s->hii_dim * (size_t)s->hii_dim * (size_t)s->hii_d_para;
    const size_t slab_elems = n_pix * (size_t)run;

    /* directions: a host array is copied (and checked) on every call */
    const double *d_nhat = s->nhat;
    if (!c21hip_is_device_ptr(s->nhat)) {
        for (size_t i = 0; i < 3 * n_pix; ++i)
            if (!isfinite(s->nhat[i]) || fabs(s->nhat[i]) > 1.0 + 1e-9) return ang_fail("nhat must hold unit vectors");
        double *d = (double *)c21hip_ws(WS_ANG_NHAT, 3 * n_pix * sizeof(double));
        if (!d) return C21CM_MEMORY_ALLOC_ERROR;
        TRY(c21hip_h2d(d, s->nhat, 3 * n_pix * sizeof(double), stream));
        d_nhat = d;
    }

    /* per-slice table */
    tab = (c21hip_ang_slice *)malloc(sizeof(c21hip_ang_slice) * (size_t)run);
    if (!tab) return C21CM_MEMORY_ALLOC_ERROR;
    for (int j = 0; j < run; ++j) {
        tab[j].d = s->distance[j];
        tab[j].w_lo = s->w_lo[j];
        tab[j].w_hi = s->w_hi[j];
    }
    c21hip_ang_slice *d_tab = (c21hip_ang_slice *)c21hip_ws(WS_ANG_TAB, sizeof(c21hip_ang_slice) * (size_t)run);
    int *d_bad = (int *)c21hip_ws(WS_ANG_FLAG, sizeof(int));
    if (!d_tab || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    TRY(c21hip_h2d(d_tab, tab, sizeof(c21hip_ang_slice) * (size_t)run, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));

    /* node boxes: host ones staged into one slot, device ones used in place */
    int n_host_in = 0, n_host_out = 0;
    for (int b = 0; b < n_boxes; ++b)
        n_host_in += !c21hip_is_device_ptr(box_lo[b]) + !c21hip_is_device_ptr(box_hi[b]);
    for (int q = 0; q < s->n_fields; ++q) n_host_out += !c21hip_is_device_ptr(lightcone[q]);
    float *stage_in = NULL, *stage_out = NULL;
    if (n_host_in) {
        stage_in = (float *)c21hip_ws(WS_ANG_BOXES, (size_t)n_host_in * box_elems * sizeof(float));
        if (!stage_in) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    if (n_host_out) {
        stage_out = (float *)c21hip_ws(WS_ANG_SLAB, (size_t)n_host_out * slab_elems * sizeof(float));
        if (!stage_out) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    const float *lo[C21HIP_ANG_MAX_BOXES], *hi[C21HIP_ANG_MAX_BOXES];
    float *dst[C21CM_LC_MAX_FIELDS];
    long stride[C21CM_LC_MAX_FIELDS], off[C21CM_LC_MAX_FIELDS];
    int in_i = 0, out_i = 0;
    for (int b = 0; b < n_boxes; ++b) {
        const float *src[2] = {box_lo[b], box_hi[b]};
        const float **dev[2] = {&lo[b], &hi[b]};
        for (int k = 0; k < 2; ++k) {
            if (c21hip_is_device_ptr(src[k])) {
                *dev[k] = src[k];
            } else {
                float *d = stage_in + (size_t)in_i++ * box_elems;
                TRY(c21hip_h2d(d, src[k], box_elems * sizeof(float), stream));
                *dev[k] = d;
            }
        }
    }
    /* device lightcones are written in place, host ones into a packed slab of the run */
    for (int q = 0; q < s->n_fields; ++q) {
        if (c21hip_is_device_ptr(lightcone[q])) {
            dst[q] = lightcone[q], stride[q] = s->n_slices, off[q] = s->i0;
        } else {
            dst[q] = stage_out + (size_t)out_i++ * slab_elems, stride[q] = run, off[q] = 0;
        }
    }
    TRY(c21hip_angular_sample(lo, hi, dst, stride, off, s->n_fields, s->mean_max, s->vector, s->order, n_pix, run,
                              s->hii_dim, s->hii_dim, s->hii_d_para, d_nhat, s->origin, d_tab, s->w_norm, d_bad,
                              stream));
    for (int q = 0; q < s->n_fields; ++q) {
        if (c21hip_is_device_ptr(lightcone[q])) continue;
        TRY(c21hip_d2h_2d(lightcone[q] + s->i0, (size_t)s->n_slices * sizeof(float), dst[q],
                          (size_t)run * sizeof(float), (size_t)run * sizeof(float), n_pix, stream));
    }
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    /* the host tables and host outputs must outlive the copies */
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("angular lightcone: a node box value read by the interpolation is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
    }
done:
    free(tab);
    return status;
}

int c21cm_spline_prefilter_grids(int n0, int n1, int n2, int order, int n_fields, const float *const *boxes,
                                 float *const *coefs, void *stream) {
    int status = 0;
    if (n0 < 1 || n1 < 1 || n2 < 1) {
        c21hip_set_error("spline prefilter: the box dimensions must be positive");
        return C21CM_VALUE_ERROR;
    }
    if (order != 3 && order != 5) {
        c21hip_set_error("spline prefilter: order must be 3 or 5");
        return C21CM_VALUE_ERROR;
    }
    if (n_fields < 1 || !boxes || !coefs) {
        c21hip_set_error("spline prefilter: n_fields >= 1 and the pointer arrays are required");
        return C21CM_VALUE_ERROR;
    }
    for (int q = 0; q < n_fields; ++q)
        if (!boxes[q] || !coefs[q]) {
            c21hip_set_error("spline prefilter: a box pointer is NULL");
            return C21CM_VALUE_ERROR;
        }
    const size_t elems = (size_t)n0 * (size_t)n1 * (size_t)n2, bytes = elems * sizeof(float);
    int *d_bad = (int *)c21hip_ws(WS_ANG_FLAG, sizeof(int));
    if (!d_bad) return C21CM_MEMORY_ALLOC_ERROR;
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    for (int q = 0; q < n_fields; ++q) {
        const int host_in = !c21hip_is_device_ptr(boxes[q]), host_out = !c21hip_is_device_ptr(coefs[q]);
        const float *src = boxes[q];
        float *dst = coefs[q];
        if (host_in) {
            float *d = (float *)c21hip_ws(WS_PREFILTER_IN, bytes);
            if (!d) {
                status = C21CM_MEMORY_ALLOC_ERROR;
                goto done;
            }
            TRY(c21hip_h2d(d, boxes[q], bytes, stream));
            src = d;
        }
        if (host_out) {
            dst = (float *)c21hip_ws(WS_PREFILTER_OUT, bytes);
            if (!dst) {
                status = C21CM_MEMORY_ALLOC_ERROR;
                goto done;
            }
        }
        TRY(c21hip_spline_prefilter(src, dst, n0, n1, n2, order, d_bad, stream));
        if (host_out) {
            TRY(c21hip_d2h(coefs[q], dst, bytes, stream));
            /* the next field reuses the staging slots */
            TRY(c21hip_sync(stream));
        }
    }
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("spline prefilter: a box value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
    }
done:
    return status;
}
