/*
 * lightcone_driver.c -- C host driver of the rectilinear lightcone: the slab of one node pair
 * (src/py21cmfast/lightconers.py:162-319 make_lightcone_slices / redshift_interpolation, as the node
 * loop of drivers/lightcone.py:544-575 calls it) and the dv/dr correction of the brightness
 * temperature at the last node (drivers/lightcone.py:249-277, rsds.py:16-103).
 * Host arrays are staged through workspace slots, device arrays are used in place; a host lightcone
 * receives only the slices of the call, as one 2-D copy per field.
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

static int lc_fail(const char *msg) {
    c21hip_set_error("lightcone: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_lightcone_slab_grids(const c21cm_lightcone_spec *s, const float *const *box_lo,
                               const float *const *box_hi, float *const *lightcone, void *stream) {
    int status = 0;
    c21hip_lc_slice *tab = NULL;
    if (!s) return lc_fail("spec is required");
    if (s->hii_dim < 1 || s->hii_d_para < 1) return lc_fail("hii_dim and hii_d_para must be positive");
    if (s->n_slices < 1) return lc_fail("the lightcone has zero slices");
    if (s->i0 < 0 || s->i1 <= s->i0 || s->i1 > s->n_slices)
        return lc_fail("slice range [i0, i1) is empty or outside the lightcone");
    if (s->n_fields < 1 || s->n_fields > C21CM_LC_MAX_FIELDS) return lc_fail("n_fields outside 1 .. 16");
    if (!s->plane || !s->w_lo || !s->w_hi) return lc_fail("plane, w_lo and w_hi tables are required");
    if (!(s->w_norm > 0.0) || !isfinite(s->w_norm)) return lc_fail("w_norm must be positive and finite");
    if (!box_lo || !box_hi || !lightcone) return lc_fail("field pointer arrays are required");
    const int run = s->i1 - s->i0;
    for (int j = 0; j < run; ++j) {
        if (s->plane[j] < 0 || s->plane[j] >= s->hii_d_para) {
            c21hip_set_error("lightcone: plane index %d of slice %d outside [0, %d)", s->plane[j],
                             s->i0 + j, s->hii_d_para);
            return C21CM_VALUE_ERROR;
        }
        if (!isfinite(s->w_lo[j]) || !isfinite(s->w_hi[j])) return lc_fail("non-finite slice weight");
    }
    for (int q = 0; q < s->n_fields; ++q)
        if (!box_lo[q] || !box_hi[q] || !lightcone[q]) return lc_fail("a field pointer is NULL");

    const size_t n_cols = (size_t)s->hii_dim * (size_t)s->hii_dim;
    const size_t box_elems = n_cols * (size_t)s->hii_d_para;
    const size_t slab_elems = n_cols * (size_t)run;

    /* per-slice table */
    tab = (c21hip_lc_slice *)malloc(sizeof(c21hip_lc_slice) * (size_t)run);
    if (!tab) return C21CM_MEMORY_ALLOC_ERROR;
    for (int j = 0; j < run; ++j) {
        tab[j].plane = s->plane[j];
        tab[j].pad_ = 0;
        tab[j].w_lo = s->w_lo[j];
        tab[j].w_hi = s->w_hi[j];
    }
    c21hip_lc_slice *d_tab = (c21hip_lc_slice *)c21hip_ws(WS_LC_TAB, sizeof(c21hip_lc_slice) * (size_t)run);
    if (!d_tab) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    TRY(c21hip_h2d(d_tab, tab, sizeof(c21hip_lc_slice) * (size_t)run, stream));

    /* node boxes: host ones staged into one slot, device ones used in place */
    int n_host_in = 0, n_host_out = 0;
    for (int q = 0; q < s->n_fields; ++q) {
        n_host_in += !c21hip_is_device_ptr(box_lo[q]) + !c21hip_is_device_ptr(box_hi[q]);
        n_host_out += !c21hip_is_device_ptr(lightcone[q]);
    }
    float *stage_in = NULL, *stage_out = NULL;
    if (n_host_in) {
        stage_in = (float *)c21hip_ws(WS_LC_BOXES, (size_t)n_host_in * box_elems * sizeof(float));
        if (!stage_in) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    if (n_host_out) {
        stage_out = (float *)c21hip_ws(WS_LC_SLAB, (size_t)n_host_out * slab_elems * sizeof(float));
        if (!stage_out) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    const float *lo[C21CM_LC_MAX_FIELDS], *hi[C21CM_LC_MAX_FIELDS];
    float *dst[C21CM_LC_MAX_FIELDS];
    int in_i = 0, out_i = 0, any_host_out = 0, all_host_out = 1;
    for (int q = 0; q < s->n_fields; ++q) {
        const float *src[2] = {box_lo[q], box_hi[q]};
        const float **dev[2] = {&lo[q], &hi[q]};
        for (int b = 0; b < 2; ++b) {
            if (c21hip_is_device_ptr(src[b])) {
                *dev[b] = src[b];
            } else {
                float *d = stage_in + (size_t)in_i++ * box_elems;
                TRY(c21hip_h2d(d, src[b], box_elems * sizeof(float), stream));
                *dev[b] = d;
            }
        }
        if (c21hip_is_device_ptr(lightcone[q])) {
            dst[q] = lightcone[q];
            all_host_out = 0;
        } else {
            dst[q] = stage_out + (size_t)out_i++ * slab_elems;
            any_host_out = 1;
        }
    }
    /* one launch when every output lives in the same kind of memory; else one per kind */
    if (!any_host_out || all_host_out) {
        const long stride = all_host_out ? run : s->n_slices, off = all_host_out ? 0 : s->i0;
        TRY(c21hip_lightcone_slab(lo, hi, dst, s->n_fields, s->mean_max, n_cols, run, s->hii_d_para, stride,
                                  off, d_tab, s->w_norm, stream));
    } else {
        for (int host_pass = 0; host_pass < 2; ++host_pass) {
            const float *l2[C21CM_LC_MAX_FIELDS], *h2[C21CM_LC_MAX_FIELDS];
            float *d2[C21CM_LC_MAX_FIELDS];
            unsigned mm = 0;
            int n = 0;
            for (int q = 0; q < s->n_fields; ++q) {
                if ((!c21hip_is_device_ptr(lightcone[q])) != host_pass) continue;
                l2[n] = lo[q], h2[n] = hi[q], d2[n] = dst[q];
                mm |= ((s->mean_max >> q) & 1u) << n;
                ++n;
            }
            TRY(c21hip_lightcone_slab(l2, h2, d2, n, mm, n_cols, run, s->hii_d_para,
                                      host_pass ? run : s->n_slices, host_pass ? 0 : s->i0, d_tab, s->w_norm,
                                      stream));
        }
    }
    for (int q = 0; q < s->n_fields; ++q) {
        if (c21hip_is_device_ptr(lightcone[q])) continue;
        TRY(c21hip_d2h_2d(lightcone[q] + s->i0, (size_t)s->n_slices * sizeof(float), dst[q],
                          (size_t)run * sizeof(float), (size_t)run * sizeof(float), n_cols, stream));
    }
    /* the host tables and host outputs must outlive the copies */
    TRY(c21hip_sync(stream));
done:
    free(tab);
    return status;
}

static int dvdr_columns(const c21cm_dvdr_spec *s, size_t n_cols, float *brightness_temp,
                        const float *los_velocity, const float *tau_21, void *stream);

int c21cm_lightcone_dvdr_grids(const c21cm_dvdr_spec *s, float *brightness_temp, const float *los_velocity,
                               const float *tau_21, void *stream) {
    if (!s) return lc_fail("spec is required");
    if (s->hii_dim < 1) return lc_fail("hii_dim must be positive");
    return dvdr_columns(s, (size_t)s->hii_dim * (size_t)s->hii_dim, brightness_temp, los_velocity, tau_21,
                        stream);
}

/* the same correction on n_cols columns (an angular lightcone: one per pixel) */
int c21cm_lightcone_dvdr_columns_grids(const c21cm_dvdr_spec *s, long long n_cols, float *brightness_temp,
                                       const float *los_velocity, const float *tau_21, void *stream) {
    if (!s) return lc_fail("spec is required");
    if (n_cols < 0) return lc_fail("n_cols must be >= 0");
    return dvdr_columns(s, (size_t)n_cols, brightness_temp, los_velocity, tau_21, stream);
}

static int dvdr_columns(const c21cm_dvdr_spec *s, size_t n_cols, float *brightness_temp,
                        const float *los_velocity, const float *tau_21, void *stream) {
    int status = 0;
    if (s->n_slices < 3)
        return lc_fail("dv/dr needs at least 3 slices (second-order one-sided differences at both ends)");
    if (!brightness_temp || !los_velocity) return lc_fail("brightness_temp and los_velocity are required");
    if (s->use_ts_fluct && !tau_21) return lc_fail("USE_TS_FLUCT needs the tau_21 lightcone");
    if (!(s->dx > 0.0) || !isfinite(s->dx)) return lc_fail("dx must be positive and finite");
    if (!(s->max_dvdr >= 0.0) || !isfinite(s->max_dvdr)) return lc_fail("max_dvdr must be >= 0 and finite");
    if (!s->hubble) return lc_fail("the H(z) table is required");
    for (int k = 0; k < s->n_slices; ++k)
        if (!(s->hubble[k] > 0.0) || !isfinite(s->hubble[k])) return lc_fail("H(z) must be positive and finite");

    const size_t elems = n_cols * (size_t)s->n_slices, bytes = elems * sizeof(float);
    if (elems == 0) return 0;
    double *d_h = (double *)c21hip_ws(WS_LC_HUBBLE, sizeof(double) * (size_t)s->n_slices);
    if (!d_h) return C21CM_MEMORY_ALLOC_ERROR;
    TRY(c21hip_h2d(d_h, s->hubble, sizeof(double) * (size_t)s->n_slices, stream));
    const int host_bt = !c21hip_is_device_ptr(brightness_temp);
    const int host_v = !c21hip_is_device_ptr(los_velocity);
    const int host_tau = s->use_ts_fluct && !c21hip_is_device_ptr(tau_21);
    const int n_stage = host_bt + host_v + host_tau;
    float *stage = NULL;
    if (n_stage) {
        stage = (float *)c21hip_ws(WS_LC_DVDR, (size_t)n_stage * bytes);
        if (!stage) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    float *d_bt = brightness_temp;
    const float *d_v = los_velocity, *d_tau = s->use_ts_fluct ? tau_21 : NULL;
    int i = 0;
    if (host_bt) {
        d_bt = stage + (size_t)i++ * elems;
        TRY(c21hip_h2d(d_bt, brightness_temp, bytes, stream));
    }
    if (host_v) {
        float *d = stage + (size_t)i++ * elems;
        TRY(c21hip_h2d(d, los_velocity, bytes, stream));
        d_v = d;
    }
    if (host_tau) {
        float *d = stage + (size_t)i++ * elems;
        TRY(c21hip_h2d(d, tau_21, bytes, stream));
        d_tau = d;
    }
    TRY(c21hip_lightcone_dvdr(d_bt, d_v, d_tau, d_h, n_cols, s->n_slices, s->dx, s->max_dvdr,
                              s->use_ts_fluct, stream));
    if (host_bt) TRY(c21hip_d2h(brightness_temp, d_bt, bytes, stream));
    TRY(c21hip_sync(stream));
done:
    return status;
}
