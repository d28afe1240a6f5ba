/*
 * dexm_driver.c -- C host driver of the DexM halo finder (ComputeHaloCatalog, src/py21cmfast/src/
 * HaloCatalog.c:38-456): one forward transform of the hi-res density kept as a spectrum, then per rung of
 * the radius ladder the window and the inverse transform (tsfilter_driver.c's machinery), the threshold
 * with ordered compaction, the rounds that decide the candidates with the serial tail,
 * and at the end the catalogue in raster order and the overlap box.  Host arrays are staged through
 * workspace slots; device arrays are used where they are.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"
#include "cosmology.h"
#include "tsfilter.h"

#define TRY(expr)         \
    do {                  \
        int st_ = (expr); \
        if (st_) {        \
            status = st_; \
            goto done;    \
        }                 \
    } while (0)

static c21cm_find_halos_report g_report;

/* C21CM_DEXM_TIMING=1: the stream is drained around every phase and its wall-clock time goes to the report
 * (tools/time_dexm.py); otherwise nothing waits */
static int g_timing;
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}
#define PHASE(k, expr)                                     \
    do {                                                   \
        double t0_ = 0;                                    \
        if (g_timing) {                                    \
            TRY(c21hip_sync(stream));                      \
            t0_ = now_ms();                                \
        }                                                  \
        TRY(expr);                                         \
        if (g_timing) {                                    \
            TRY(c21hip_sync(stream));                      \
            g_report.ms[k] += now_ms() - t0_;              \
        }                                                  \
    } while (0)

void c21cm_find_halos_last_report(c21cm_find_halos_report *report) {
    if (report) *report = g_report;
}

static int catalogue_complete(const HaloCatalog *c) {
    return c->halo_masses && c->halo_coords && c->star_rng && c->sfr_rng && c->xray_rng;
}

/* the candidates of rung r decided: rounds (path 0, 2), the serial workgroup (path 1, or the tail of path 0) */
static int decide_rung(const c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                       void *stream) {
    int status = 0;
    unsigned int ctr[4] = {0, 0, 0, 0};
    TRY(c21hip_memset(a->counters, 0, 2 * sizeof(unsigned int), stream)); /* decided, accepted */
    TRY(c21hip_memset(a->counters + 3, 0, sizeof(unsigned int), stream)); /* last round */
    unsigned int round = 0;
    while (s->path != 1 && ctr[0] < n_cand && (s->path == 2 || round < C21CM_DEXM_ROUND_CAP)) {
        /* a round over nothing undecided is a no-op, so the count is read once per batch */
        for (int k = 0; k < C21CM_DEXM_ROUND_BATCH; k++) {
            PHASE(C21CM_DEXM_MS_DECIDE, c21hip_dexm_decide(s, r, a, n_cand, stream));
            PHASE(C21CM_DEXM_MS_PAINT, c21hip_dexm_paint(s, r, a, n_cand, ++round, stream));
        }
        TRY(c21hip_d2h(ctr, a->counters, sizeof(ctr), stream));
        TRY(c21hip_sync(stream));
    }
    g_report.rounds[r] = (int)ctr[3];
    if (ctr[0] < n_cand) {
        g_report.tail[r] = 1;
        PHASE(C21CM_DEXM_MS_SERIAL, c21hip_dexm_serial(s, r, a, n_cand, stream));
        TRY(c21hip_d2h(ctr, a->counters, sizeof(ctr), stream));
        TRY(c21hip_sync(stream));
        if (ctr[0] != n_cand) {
            c21hip_set_error("DexM: %u of %u candidates of radius %d were decided", ctr[0], n_cand, r);
            return C21CM_VALUE_ERROR;
        }
    }
    g_report.accepted[r] = ctr[1];
done:
    return status;
}

int c21cm_find_halos_grids(const c21cm_find_halos_spec *s, const float *hires_density, float *filtered,
                           HaloCatalog *out, unsigned char *in_halo, float *overlap, void *stream) {
    int status = 0;
    memset(&g_report, 0, sizeof(g_report));
    {
        const char *e = getenv("C21CM_DEXM_TIMING");
        g_timing = e && e[0] == '1';
    }
    if (!s || !out) {
        c21hip_set_error("DexM: NULL spec / output");
        return C21CM_VALUE_ERROR;
    }
    if (s->dim < 2 || s->dim_z < 2 || !(s->box_len > 0) || !(s->box_len_z > 0) || !(s->growth > 0) ||
        !(s->r_overlap >= 0) || !isfinite(s->r_overlap) || !(s->rtom_unit > 0)) {
        c21hip_set_error("DexM: grid dimensions, box lengths, growth factor and rtom_unit must be positive, "
                         "DEXM_R_OVERLAP not negative");
        return C21CM_VALUE_ERROR;
    }
    if (s->n_R < 0 || s->n_R > C21CM_MAX_DEXM_RADII) {
        c21hip_set_error("DexM: 0 <= n_R <= %d", C21CM_MAX_DEXM_RADII);
        return C21CM_VALUE_ERROR;
    }
    if (s->halo_filter < 0 || s->halo_filter > 2) {
        c21hip_set_error("DexM: HALO_FILTER must be 0 (top-hat), 1 (sharp-k) or 2 (Gaussian)");
        return C21CM_VALUE_ERROR;
    }
    if (s->filtered_mode < 0 || s->filtered_mode > 2 || s->path < 0 || s->path > 2) {
        c21hip_set_error("DexM: filtered_mode and path are 0, 1 or 2");
        return C21CM_VALUE_ERROR;
    }
    for (int r = 0; r < s->n_R; r++)
        if (!(s->R[r] > 0) || !isfinite(s->R[r]) || !(s->mass[r] > 0) || !isfinite(s->mass[r]) ||
            !isfinite(s->delta_crit[r])) {
            c21hip_set_error("DexM: radius %d of the ladder is not a finite positive radius, mass and barrier", r);
            return C21CM_VALUE_ERROR;
        }
    const size_t n = (size_t)s->dim * s->dim * s->dim_z;
    if (n > 0xfffff000ull) { /* cell indices are 32-bit words */
        c21hip_set_error("DexM: %zu cells are more than the candidate lists index", n);
        return C21CM_VALUE_ERROR;
    }
    if (s->filtered_mode && !filtered) {
        c21hip_set_error("DexM: filtered_mode %d needs the `filtered` array", s->filtered_mode);
        return C21CM_VALUE_ERROR;
    }
    if (s->filtered_mode != 1 && s->n_R && !hires_density) {
        c21hip_set_error("DexM halo finder: the hi-res density (InitialConditions.hires_density) is missing");
        return C21CM_VALUE_ERROR;
    }
    const int want_overlap = s->hii_dim > 0;
    if (want_overlap && (!overlap || s->hii_dim_z < 1 || s->hii_dim > s->dim || s->hii_dim_z > s->dim_z)) {
        c21hip_set_error("DexM: the overlap box needs its array and 1 <= hii_dim <= dim");
        return C21CM_VALUE_ERROR;
    }
    if (!catalogue_complete(out) && out->buffer_size) {
        c21hip_set_error("DexM: the output needs halo_masses, halo_coords, star_rng, sfr_rng and xray_rng");
        return C21CM_VALUE_ERROR;
    }

    const size_t bytes = n * sizeof(float);
    const unsigned long long nb = c21hip_dexm_blocks(n);
    c21hip_dexm_arrays a;
    memset(&a, 0, sizeof(a));
    a.in_halo = (unsigned char *)c21hip_ws(WS_DX_MASK, n);
    a.forbidden = s->optimize ? (unsigned char *)c21hip_ws(WS_DX_FORBID, n) : NULL;
    a.state = (unsigned char *)c21hip_ws(WS_DX_STATE, n);
    a.rung_grid = (unsigned short *)c21hip_ws(WS_DX_RUNG, n * sizeof(unsigned short));
    a.list = (unsigned int *)c21hip_ws(WS_DX_LIST, n * sizeof(unsigned int));
    a.found = (unsigned int *)c21hip_ws(WS_DX_FOUND, n * sizeof(unsigned int));
    a.counters = (unsigned int *)c21hip_ws(WS_DX_COUNTERS, 4 * sizeof(unsigned int));
    unsigned long long *counts = (unsigned long long *)c21hip_ws(WS_DX_COUNTS, (size_t)(nb + 1) * sizeof(*counts));
    float *tables = (float *)c21hip_ws(WS_DX_TABLES, 2 * C21CM_MAX_DEXM_RADII * sizeof(float));
    float *delta = (float *)c21hip_ws(WS_DX_DELTA, bytes);
    if (!a.in_halo || (s->optimize && !a.forbidden) || !a.state || !a.rung_grid || !a.list || !a.found ||
        !a.counters || !counts || !tables || !delta)
        return C21CM_MEMORY_ALLOC_ERROR;
    TRY(c21hip_memset(a.in_halo, 0, n, stream));
    TRY(c21hip_memset(a.rung_grid, 0, n * sizeof(unsigned short), stream));
    TRY(c21hip_memset(a.counters, 0, 4 * sizeof(unsigned int), stream));
    {
        float host_tab[2 * C21CM_MAX_DEXM_RADII];
        memset(host_tab, 0, sizeof(host_tab));
        for (int r = 0; r < s->n_R; r++) {
            host_tab[r] = s->mass[r];
            /* MtoR as a float variable (R_temp, HaloCatalog.c:231) */
            host_tab[C21CM_MAX_DEXM_RADII + r] = (float)pow((double)s->mass[r] / s->rtom_unit, 1. / 3.);
        }
        TRY(c21hip_h2d(tables, host_tab, sizeof(host_tab), stream));
        TRY(c21hip_sync(stream)); /* host_tab leaves scope */
    }

    tf_ctx c;
    const int transforms = s->filtered_mode != 1 && s->n_R > 0;
    if (transforms || want_overlap) TRY(tf_setup(&c, s->dim, s->dim_z, s->box_len, s->box_len_z, 1, stream));
    if (transforms) {
        const float *d_in = (const float *)c21_stage_in(WS_DX_IN, hires_density, bytes, stream, &status);
        if (status) return status;
        PHASE(C21CM_DEXM_MS_TRANSFORMS, tf_forward(&c, d_in));
    }
    const int filtered_dev = filtered && c21hip_is_device_ptr(filtered);
    unsigned long long n_found = 0;
    g_report.n_R = s->n_R;
    for (int r = 0; r < s->n_R; r++) {
        const float *d = delta;
        float *slice = filtered ? filtered + (size_t)r * n : NULL;
        if (s->filtered_mode == 1) {
            if (filtered_dev) d = slice;
            else TRY(c21hip_h2d(delta, slice, bytes, stream));
        } else {
            /* delta_m = filtered density * growth (HaloCatalog.c:259-260); no floor */
            float *d_out = s->filtered_mode == 2 && filtered_dev ? slice : delta;
            PHASE(C21CM_DEXM_MS_TRANSFORMS,
                  tf_window(&c, s->halo_filter, s->R[r], 0.f, 1, -INFINITY, s->growth, d_out, c.stats));
            if (s->filtered_mode == 2 && !filtered_dev) TRY(c21hip_d2h(slice, delta, bytes, stream));
            d = d_out;
        }
        const int opt = s->optimize && s->mass[r] > s->optimize_minmass;
        if (opt) { /* HaloCatalog.c:215-241 */
            TRY(c21hip_memset(a.forbidden, 0, n, stream));
            PHASE(C21CM_DEXM_MS_PAINT,
                  c21hip_dexm_forbid(s, r, &a, (unsigned int)n_found, tables + C21CM_MAX_DEXM_RADII, stream));
        }
        const unsigned char *mask = opt ? a.forbidden : a.in_halo;
        unsigned long long total = 0;
        PHASE(C21CM_DEXM_MS_COMPACTION, c21hip_dexm_count(0, d, s->delta_crit[r], mask, NULL, n, counts + 1, stream));
        PHASE(C21CM_DEXM_MS_COMPACTION, c21hip_hs_scan(counts + 1, nb, counts, stream));
        TRY(c21hip_d2h(&total, counts, sizeof(total), stream));
        TRY(c21hip_sync(stream));
        g_report.candidates[r] = (unsigned int)total;
        if (!total) continue;
        PHASE(C21CM_DEXM_MS_COMPACTION,
              c21hip_dexm_list(d, s->delta_crit[r], mask, n, counts + 1, a.list, a.state, stream));
        TRY(decide_rung(s, r, &a, (unsigned int)total, stream));
        n_found += g_report.accepted[r];
    }
    g_report.n_halos = n_found;

    const unsigned long long buffer = out->buffer_size;
    if (n_found > buffer) { /* HaloCatalog.c:310-327 */
        const double mem = config_settings.HALO_CATALOG_MEM_FACTOR;
        const double expected = expected_nhalo(s->redshift);
        c21hip_set_error("DexM: %llu halos were found and the halo catalog holds %llu.  Try raising "
                         "HALO_CATALOG_MEM_FACTOR from %.2f to %.2f.", n_found, buffer, mem,
                         (double)n_found / (expected + 1) * 1.15);
        return C21CM_VALUE_ERROR;
    }
    float *out_h[5] = {out->halo_masses, out->halo_coords, out->star_rng, out->sfr_rng, out->xray_rng};
    const size_t width[5] = {1, 3, 1, 1, 1};
    if (n_found) {
        unsigned long long total = 0;
        float *dev[5];
        for (int k = 0; k < 5; k++) {
            dev[k] = c21hip_is_device_ptr(out_h[k]) ? out_h[k]
                                                    : (float *)c21hip_ws(WS_DX_OUT0 + k, (size_t)n_found * width[k] * sizeof(float));
            if (!dev[k]) return C21CM_MEMORY_ALLOC_ERROR;
        }
        TRY(c21hip_dexm_count(1, NULL, 0.f, NULL, a.rung_grid, n, counts + 1, stream));
        TRY(c21hip_hs_scan(counts + 1, nb, counts, stream));
        TRY(c21hip_d2h(&total, counts, sizeof(total), stream));
        TRY(c21hip_sync(stream));
        if (total != n_found) { /* the rows written below are exactly the halos counted above */
            c21hip_set_error("DexM: %llu halo cells for %llu accepted halos", total, n_found);
            return C21CM_VALUE_ERROR;
        }
        TRY(c21hip_dexm_extract(s, &a, n, counts + 1, tables, dev[0], dev[1], dev[2], dev[3], dev[4], stream));
        for (int k = 0; k < 5; k++)
            if (dev[k] != out_h[k]) TRY(c21hip_d2h(out_h[k], dev[k], (size_t)n_found * width[k] * sizeof(float), stream));
    }
    for (int k = 0; k < 5 && buffer > n_found; k++) { /* zeros from n_halos to buffer_size, as the sampler leaves them */
        const size_t tail = (size_t)(buffer - n_found) * width[k] * sizeof(float);
        if (c21hip_is_device_ptr(out_h[k]))
            TRY(c21hip_memset(out_h[k] + n_found * width[k], 0, tail, stream));
        else
            memset(out_h[k] + n_found * width[k], 0, tail);
    }
    if (in_halo)
        TRY(c21hip_is_device_ptr(in_halo) ? c21hip_d2d(in_halo, a.in_halo, n, stream)
                                          : c21hip_d2h(in_halo, a.in_halo, n, stream));
    if (want_overlap) { /* HaloCatalog.c:361-420 */
        const size_t n_lo = (size_t)s->hii_dim * s->hii_dim * s->hii_dim_z;
        const int ov_dev = c21hip_is_device_ptr(overlap);
        float *d_ov = ov_dev ? overlap : (float *)c21hip_ws(WS_DX_OVERLAP, n_lo * sizeof(float));
        if (!d_ov) return C21CM_MEMORY_ALLOC_ERROR;
        TRY(c21hip_dexm_mask_float(a.in_halo, delta, n, stream));
        TRY(tf_forward(&c, delta)); /* spectrum / N: the reference divides after the inverse */
        const float R_lo = (float)(0.620350491 * (double)(float)s->box_len / (s->hii_dim + 0.0));
        TRY(tf_window(&c, 0, R_lo, 0.f, s->dim != s->hii_dim, -INFINITY, 1.0, delta, c.stats));
        TRY(c21hip_dexm_downsample(delta, s->dim, s->dim_z, s->hii_dim, s->hii_dim_z, d_ov, stream));
        if (!ov_dev) TRY(c21hip_d2h(overlap, d_ov, n_lo * sizeof(float), stream));
    }
    TRY(c21hip_sync(stream));
    out->n_halos = n_found;
done:
    return status;
}
