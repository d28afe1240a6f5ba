/*
 * tsfilter.h -- the transform machinery of tsfilter_driver.c for the other host drivers that filter one
 * field at many radii (dexm_driver.c): one forward transform kept as a spectrum, then per window the
 * multiply and the inverse.  Native sizes use the split layout, other sizes rocFFT.  Internal to the library.
 */
#ifndef C21_TSFILTER_H
#define C21_TSFILTER_H

#include <stddef.h>

typedef struct {
    int nx, ny, nz, native;
    size_t ntot, npad;
    double box_len, box_len_z;
    float *unf, *work;
    double *partials, *stats; /* stats: 3 doubles per window, device */
    void *stream;
} tf_ctx;

#define TF_HIDDEN __attribute__((visibility("hidden")))
/* workspace slots WS_TF_UNF / WS_TF_WORK / WS_TF_PART sized for [hii_dim][hii_dim][hii_dim_z] and n_stats windows */
TF_HIDDEN int tf_setup(tf_ctx *c, int hii_dim, int hii_dim_z, double box_len, double box_len_z, int n_stats,
                       void *stream);
/* dense real input -> c->unf = spectrum / N */
TF_HIDDEN int tf_forward(tf_ctx *c, const float *d_in);
/* c->unf x W -> real space -> max(v, min_value) * const_factor -> d_out (dense), {min, max, sum} to stats3 */
TF_HIDDEN int tf_window(tf_ctx *c, int filter_type, float R, float R_param, int apply, double min_value,
                        double const_factor, float *d_out, double *stats3);

#endif
