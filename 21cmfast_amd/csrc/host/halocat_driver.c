/*
 * halocat_driver.c -- C host driver of ComputePerturbedHaloCatalog with convert_halo_props
 * (src/py21cmfast/src/PerturbedHaloCatalog.c:25-149, src/py21cmfast/src/HaloBox.c:781-880): the
 * halo catalogue moved to its Eulerian positions and converted to galaxy properties, one row per
 * halo in input order.  Host arrays are staged into three workspace slots (inputs, outputs, grids);
 * device arrays are used where they are.
 */
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

/* a float array of `count` values for the kernel: the caller's when it is in HBM, else the next piece
 * of `pool` (copied in when `upload`); *cursor counts floats, pieces start on 64-float boundaries */
static float *stage(float *pool, size_t *cursor, const float *p, size_t count, int upload,
                    void *stream, int *status) {
    if (!p || *status) return NULL;
    if (c21hip_is_device_ptr(p)) return (float *)p;
    float *d = pool + *cursor;
    *cursor += (count + 63) & ~(size_t)63;
    if (upload) *status = c21hip_h2d(d, p, count * sizeof(float), stream);
    return d;
}

static size_t piece(const float *p, size_t count) {
    return p && !c21hip_is_device_ptr(p) ? (count + 63) & ~(size_t)63 : 0;
}

int c21cm_perturb_halos_grids(const c21cm_perturb_halos_spec *s, const c21cm_halo_consts *c,
                              const InitialConditions *ics, const float *log10_mturn_acg,
                              const float *log10_mturn_mcg, const HaloCatalog *halos,
                              PerturbedHaloCatalog *out, void *stream) {
    int status = 0;
    if (!s || !c || !ics || !halos || !out) {
        c21hip_set_error("perturbed halos: NULL spec / constants / ics / catalogue / output");
        return C21CM_VALUE_ERROR;
    }
    const unsigned long long nh = halos->n_halos;
    if (out->buffer_size < nh) {
        c21hip_set_error("perturbed halos: the output holds %llu rows, the catalogue has %llu halos",
                         out->buffer_size, nh);
        return C21CM_VALUE_ERROR;
    }
    if (!(s->box_len > 0) || !(s->box_len_z > 0) || s->dim < 1 || s->dim_z < 1 || s->hii_dim < 1 ||
        s->hii_dim_z < 1) {
        c21hip_set_error("perturbed halos: grid dimensions and box lengths must be positive");
        return C21CM_VALUE_ERROR;
    }
    if (!nh) {
        out->n_halos = 0;
        return 0;
    }
    const int hires = s->perturb_on_high_res, mini = c->use_mini_halos;
    const float *vel_h[3] = {hires ? ics->hires_vx : ics->lowres_vx, hires ? ics->hires_vy : ics->lowres_vy,
                             hires ? ics->hires_vz : ics->lowres_vz};
    const float *vel2_h[3] = {hires ? ics->hires_vx_2LPT : ics->lowres_vx_2LPT,
                              hires ? ics->hires_vy_2LPT : ics->lowres_vy_2LPT,
                              hires ? ics->hires_vz_2LPT : ics->lowres_vz_2LPT};
    if (!vel_h[0] || !vel_h[1] || !vel_h[2] || (s->lpt2 && (!vel2_h[0] || !vel2_h[1] || !vel2_h[2]))) {
        c21hip_set_error("perturbed halos: the velocity grids of InitialConditions are missing");
        return C21CM_VALUE_ERROR;
    }
    if (!halos->halo_masses || !halos->halo_coords || !halos->star_rng || !halos->sfr_rng ||
        (c->use_xray && !halos->xray_rng)) {
        c21hip_set_error("perturbed halos: the catalogue needs masses, coordinates and the random "
                         "deviates of the scaling relations");
        return C21CM_VALUE_ERROR;
    }
    if (!out->halo_coords || !out->halo_masses || !out->stellar_masses || !out->sfr ||
        !out->ion_emissivity) {
        c21hip_set_error("perturbed halos: the output needs halo_coords, halo_masses, stellar_masses, "
                         "sfr and ion_emissivity");
        return C21CM_VALUE_ERROR;
    }
    if (mini && (!log10_mturn_acg || !log10_mturn_mcg)) {
        c21hip_set_error("perturbed halos: USE_MINI_HALOS needs the two log10 turnover grids");
        return C21CM_VALUE_ERROR;
    }
    const int vel_dim[3] = {hires ? s->dim : s->hii_dim, hires ? s->dim : s->hii_dim,
                            hires ? s->dim_z : s->hii_dim_z};
    const int lo_dim[3] = {s->hii_dim, s->hii_dim, s->hii_dim_z};
    const size_t n_vel = (size_t)vel_dim[0] * vel_dim[1] * vel_dim[2];
    const size_t n_lo = (size_t)lo_dim[0] * lo_dim[1] * lo_dim[2];
    const size_t n = (size_t)nh;

    /* inputs */
    const float *cat_h[5] = {halos->halo_masses, halos->halo_coords, halos->star_rng, halos->sfr_rng,
                             c->use_xray ? halos->xray_rng : NULL};
    size_t need = 0, cursor = 0;
    for (int k = 0; k < 5; k++) need += piece(cat_h[k], k == 1 ? 3 * n : n);
    float *pool = need ? (float *)c21hip_ws(WS_PH_IN, need * sizeof(float)) : NULL;
    if (need && !pool) return C21CM_MEMORY_ALLOC_ERROR;
    const float *cat[5];
    for (int k = 0; k < 5; k++)
        cat[k] = stage(pool, &cursor, cat_h[k], k == 1 ? 3 * n : n, 1, stream, &status);
    if (status) return status;

    /* grids */
    need = 0, cursor = 0;
    for (int a = 0; a < 3; a++) need += piece(vel_h[a], n_vel) + (s->lpt2 ? piece(vel2_h[a], n_vel) : 0);
    if (mini) need += piece(log10_mturn_acg, n_lo) + piece(log10_mturn_mcg, n_lo);
    pool = need ? (float *)c21hip_ws(WS_PH_GRIDS, need * sizeof(float)) : NULL;
    if (need && !pool) return C21CM_MEMORY_ALLOC_ERROR;
    const float *vel[3], *vel2[3] = {NULL, NULL, NULL};
    for (int a = 0; a < 3; a++) {
        vel[a] = stage(pool, &cursor, vel_h[a], n_vel, 1, stream, &status);
        if (s->lpt2) vel2[a] = stage(pool, &cursor, vel2_h[a], n_vel, 1, stream, &status);
    }
    const float *mta = mini ? stage(pool, &cursor, log10_mturn_acg, n_lo, 1, stream, &status) : NULL;
    const float *mtm = mini ? stage(pool, &cursor, log10_mturn_mcg, n_lo, 1, stream, &status) : NULL;
    if (status) return status;

    /* outputs: host property arrays are copied in first, so that the rows of cut halos come back as
     * they were */
    float *out_h[9] = {out->halo_coords, out->halo_masses, out->stellar_masses, out->sfr,
                       out->ion_emissivity, c->use_xray ? out->xray_emissivity : NULL, out->fesc_sfr,
                       mini ? out->stellar_mini : NULL, mini ? out->sfr_mini : NULL};
    need = 0, cursor = 0;
    for (int k = 0; k < 9; k++) need += piece(out_h[k], k == 0 ? 3 * n : n);
    pool = need ? (float *)c21hip_ws(WS_PH_OUT, need * sizeof(float)) : NULL;
    if (need && !pool) return C21CM_MEMORY_ALLOC_ERROR;
    float *dev[9];
    for (int k = 0; k < 9; k++)
        dev[k] = stage(pool, &cursor, out_h[k], k == 0 ? 3 * n : n, k != 0, stream, &status);
    if (status) return status;

    TRY(c21hip_halo_catalog(c, nh, cat[0], cat[1], cat[2], cat[3], cat[4], vel, vel2, vel_dim, lo_dim,
                            s->box_len, s->box_len_z, s->velocity_displacement_factor,
                            s->velocity_displacement_factor_2lpt, s->lpt2,
                            s->hii_dim / (double)s->dim, mta, mtm, dev, stream));
    for (int k = 0; k < 9; k++)
        if (out_h[k] && dev[k] != out_h[k])
            TRY(c21hip_d2h(out_h[k], dev[k], (k == 0 ? 3 * n : n) * sizeof(float), stream));
    TRY(c21hip_sync(stream));
    out->n_halos = nh;
done:
    return status;
}
