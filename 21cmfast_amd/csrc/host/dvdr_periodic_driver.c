/*
 * dvdr_periodic_driver.c -- C host driver of the dv/dr correction of a coeval box with a periodic line
 * of sight (src/py21cmfast/rsds.py:16-103 include_dvdr_in_tau21 with periodic = True, as
 * drivers/coeval.py:242-278 calls it).  Host arrays are staged through workspace slots, device arrays
 * are used in place; the correction itself is one launch (csrc/hip/dvdr_periodic_kernels.hip).
 */
#include <math.h>
#include <stddef.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"

static int dvp_fail(const char *msg) {
    c21hip_set_error("periodic dvdr: %s", msg);
    return C21CM_VALUE_ERROR;
}

int c21cm_dvdr_periodic_grids(const c21cm_dvdr_periodic_spec *s, const float *brightness_temp,
                              const float *los_velocity, const float *tau_21, float *out, void *stream) {
    int status = 0;
    if (!s) return dvp_fail("spec is required");
    if (s->n_cols < 0) return dvp_fail("n_cols must be >= 0");
    if (s->n_slices < 2) return dvp_fail("a periodic line of sight needs at least 2 slices");
    if (!brightness_temp || !los_velocity || !out)
        return dvp_fail("brightness_temp, los_velocity and out are required");
    if (s->use_ts_fluct && !tau_21) return dvp_fail("USE_TS_FLUCT needs the tau_21 box");
    if (out == los_velocity || (s->use_ts_fluct && out == tau_21))
        return dvp_fail("out may alias brightness_temp only");
    if (!(s->dx > 0.0) || !isfinite(s->dx)) return dvp_fail("dx must be positive and finite");
    if (!(s->max_dvdr >= 0.0) || !isfinite(s->max_dvdr)) return dvp_fail("max_dvdr must be >= 0 and finite");
    if (s->method < 0 || s->method > 2) return dvp_fail("method must be 0 (automatic), 1 (transform) or 2 (direct)");
    if (!s->hubble) return dvp_fail("the H(z) table is required");
    for (int k = 0; k < s->n_slices; ++k)
        if (!(s->hubble[k] > 0.0) || !isfinite(s->hubble[k])) return dvp_fail("H(z) must be positive and finite");
    if (s->n_cols == 0) return 0;

    const size_t n_cols = (size_t)s->n_cols;
    const size_t bytes = n_cols * (size_t)s->n_slices * sizeof(float);
    const double *d_h = (const double *)c21_stage_in(WS_DVP_HUBBLE, s->hubble, sizeof(double) * (size_t)s->n_slices,
                                                     stream, &status);
    const float *d_bt = (const float *)c21_stage_in(WS_DVP_BT, brightness_temp, bytes, stream, &status);
    const float *d_v = (const float *)c21_stage_in(WS_DVP_VEL, los_velocity, bytes, stream, &status);
    const float *d_tau = s->use_ts_fluct ? (const float *)c21_stage_in(WS_DVP_TAU, tau_21, bytes, stream, &status) : NULL;
    if (status) return status;
    /* a host out that is brightness_temp is corrected in place in its staged copy */
    const int host_out = !c21hip_is_device_ptr(out);
    float *d_out = out;
    if (host_out) {
        d_out = out == brightness_temp ? (float *)d_bt : (float *)c21hip_ws(WS_DVP_OUT, bytes);
        if (!d_out) return C21CM_MEMORY_ALLOC_ERROR;
    }
    status = c21hip_dvdr_periodic(d_out, d_bt, d_v, d_tau, d_h, n_cols, s->n_slices, s->dx, s->max_dvdr,
                                  s->use_ts_fluct != 0, s->method, stream);
    if (status) return status;
    if (host_out) {
        status = c21hip_d2h(out, d_out, bytes, stream);
        if (status) return status;
    }
    /* the host table and a host output must outlive the copies */
    return c21hip_sync(stream);
}
