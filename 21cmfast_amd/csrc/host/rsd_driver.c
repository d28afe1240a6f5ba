/*
 * rsd_driver.c -- C host driver of the redshift-space shift along the line of sight
 * (src/py21cmfast/rsds.py:106-255 apply_rsds / rsds_shift, as drivers/lightcone.py:279-303 calls it
 * for every lightcone and as a caller does for a coeval box).  Host arrays are staged through
 * workspace slots, device arrays are used in place; the fields are launched in groups that fit the
 * LDS (csrc/hip/rsd_kernels.hip) and a non-finite input is reported once, after the last launch.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"

/* LDS a launch aims for: two workgroups per CU */
#define RSD_LDS_TARGET (80 * 1024)

#define TRY(expr)         \
    do {                  \
        int st_ = (expr); \
        if (st_) {        \
            status = st_; \
            goto done;    \
        }                 \
    } while (0)

static int rsd_fail(const char *msg) {
    c21hip_set_error("rsd shift: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_rsd_shift_grids(const c21cm_rsd_spec *s, const float *const *fields, float *const *out,
                          const float *los_velocity, void *stream) {
    int status = 0;
    const float **in_d = NULL;
    float **out_d = NULL;
    if (!s) return rsd_fail("spec is required");
    if (s->n_cols < 0) return rsd_fail("n_cols must be >= 0");
    if (s->n_slices < 2) return rsd_fail("a column needs at least 2 slices");
    if (s->n_sub < 1) return rsd_fail("n_sub (n_rsd_subcells) must be >= 1");
    if ((long long)s->n_slices * s->n_sub > 0x7FFFFFFFll) return rsd_fail("n_slices * n_sub must be below 2^31");
    if (s->n_fields < 1) return rsd_fail("n_fields must be >= 1");
    if (!s->disp_scale) return rsd_fail("the disp_scale table is required");
    for (int j = 0; j < s->n_slices; ++j)
        if (!isfinite(s->disp_scale[j])) return rsd_fail("disp_scale must be finite");
    if (!fields || !out || !los_velocity) return rsd_fail("field, output and velocity pointers are required");
    for (int q = 0; q < s->n_fields; ++q)
        if (!fields[q] || !out[q]) return rsd_fail("a field pointer is NULL");
    int cpb = 1;
    const size_t per_field = c21hip_rsd_lds_bytes(s->n_slices, 1, &cpb);
    if (per_field > C21HIP_RSD_MAX_LDS) {
        c21hip_set_error("rsd shift: a column of %d slices needs %zu bytes of LDS accumulators, more than %d",
                         s->n_slices, per_field, C21HIP_RSD_MAX_LDS);
        return C21CM_VALUE_ERROR;
    }
    if (s->n_cols == 0) return 0;
    int per_pass = (int)(RSD_LDS_TARGET / per_field);
    if (per_pass < 1) per_pass = 1;
    if (per_pass > C21HIP_RSD_MAX_FIELDS) per_pass = C21HIP_RSD_MAX_FIELDS;

    const int nf = s->n_fields, n = s->n_slices;
    const size_t n_cols = (size_t)s->n_cols;
    const size_t elems = n_cols * (size_t)n, bytes = elems * sizeof(float);
    in_d = (const float **)calloc((size_t)nf, sizeof(*in_d));
    out_d = (float **)calloc((size_t)nf, sizeof(*out_d));
    if (!in_d || !out_d) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    double *d_scale = (double *)c21hip_ws(WS_RSD_SCALE, sizeof(double) * (size_t)n);
    int *d_bad = (int *)c21hip_ws(WS_RSD_FLAG, sizeof(int));
    if (!d_scale || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    TRY(c21hip_h2d(d_scale, s->disp_scale, sizeof(double) * (size_t)n, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));

    /* host inputs (and the host velocity) share one slot; a host output that is its own input is
     * shifted in place there, other host outputs get a slot of their own */
    const int host_v = !c21hip_is_device_ptr(los_velocity);
    int n_host_in = host_v, n_host_out = 0;
    for (int q = 0; q < nf; ++q) {
        const int hin = !c21hip_is_device_ptr(fields[q]), hout = !c21hip_is_device_ptr(out[q]);
        n_host_in += hin;
        n_host_out += hout && !(hin && (const float *)out[q] == fields[q]);
    }
    float *stage_in = NULL, *stage_out = NULL;
    if (n_host_in) {
        stage_in = (float *)c21hip_ws(WS_RSD_IN, (size_t)n_host_in * bytes);
        if (!stage_in) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    if (n_host_out) {
        stage_out = (float *)c21hip_ws(WS_RSD_OUT, (size_t)n_host_out * bytes);
        if (!stage_out) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    int in_i = 0, out_i = 0;
    const float *d_v = los_velocity;
    if (host_v) {
        float *d = stage_in + (size_t)in_i++ * elems;
        TRY(c21hip_h2d(d, los_velocity, bytes, stream));
        d_v = d;
    }
    int v_overwritten = 0;
    for (int q = 0; q < nf; ++q) {
        const int hin = !c21hip_is_device_ptr(fields[q]);
        if (hin) {
            float *d = stage_in + (size_t)in_i++ * elems;
            TRY(c21hip_h2d(d, fields[q], bytes, stream));
            in_d[q] = d;
        } else {
            in_d[q] = fields[q];
        }
        if (c21hip_is_device_ptr(out[q])) {
            out_d[q] = out[q];
            v_overwritten |= (const float *)out[q] == d_v;
        } else if (hin && (const float *)out[q] == fields[q]) {
            out_d[q] = (float *)in_d[q];
        } else {
            out_d[q] = stage_out + (size_t)out_i++ * elems;
        }
    }
    /* a device velocity that is also an output would change under the later launches: shift a copy */
    if (v_overwritten) {
        float *d = (float *)c21hip_ws(WS_RSD_VEL, bytes);
        if (!d) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
        TRY(c21hip_d2d(d, d_v, bytes, stream));
        d_v = d;
    }
    for (int q0 = 0; q0 < nf; q0 += per_pass) {
        const int cnt = nf - q0 < per_pass ? nf - q0 : per_pass;
        TRY(c21hip_rsd_shift(in_d + q0, out_d + q0, cnt, d_v, d_scale, n_cols, n, s->n_sub, s->periodic != 0,
                             d_bad, stream));
    }
    for (int q = 0; q < nf; ++q)
        if (!c21hip_is_device_ptr(out[q])) TRY(c21hip_d2h(out[q], out_d[q], bytes, stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("rsd shift: a field or los_velocity value is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
    }
done:
    free(in_d);
    free(out_d);
    return status;
}
