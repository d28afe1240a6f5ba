/*
 * halo_sampler_driver.c -- C host driver of the halo sampler (sample_halo_grids / sample_halo_progenitors,
 * src/py21cmfast/src/Stochasticity.c:761-1113): pass A, the scan of the kept counts, the checks that need
 * the total (a condition that hit a bound, the size of the output), pass B, the zeroed tail.  Host arrays
 * are staged into workspace slots; device arrays are used where they are.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"
#include "cosmology.h"

#define TRY(expr)         \
    do {                  \
        int st_ = (expr); \
        if (st_) {        \
            status = st_; \
            goto done;    \
        }                 \
    } while (0)

/* expected halos from which a whole wave takes a condition (spec->path) */
static double wave_threshold(int path) { return path == 1 ? INFINITY : path == 2 ? 0. : 64.; }

/* what c21cm_sample_halos_last_counts may report: the conditions of the last call that succeeded and the
 * workspace generation it ran in; cleared when a call starts */
static unsigned long long g_last_n;
static unsigned long g_last_generation;

static int catalogue_complete(const HaloCatalog *c) {
    return c->halo_masses && c->halo_coords && c->star_rng && c->sfr_rng && c->xray_rng;
}

/* listed: single_test_sample's form -- grid mode takes `density` as n_listed overdensities at the redshift
 * itself with cell positions in cell_crd; the output needs masses and coordinates only and is trusted
 * to be large enough (as the reference trusts it), so nothing is zeroed behind the halos */
static int sample_impl(const c21cm_sample_halos_spec *s, const float *density, const float *overlap,
                       const HaloCatalog *large, const HaloCatalog *desc, HaloCatalog *out, void *stream,
                       unsigned long long n_listed, const float *cell_crd) {
    int status = 0;
    const int listed = n_listed > 0;
    if (!s || !out || !s->tables) {
        c21hip_set_error("halo sampler: NULL spec / tables / output");
        return C21CM_VALUE_ERROR;
    }
    if (s->n_cond < 2 || s->n_prob < 3 || !(s->x_width > 0) || !(s->p_width > 0) || !(s->box_len > 0) ||
        !(s->box_len_z > 0) || !(s->rtom_unit > 0) || !(s->growth_out > 0) || !(s->m_min > 0)) {
        c21hip_set_error("halo sampler: table sizes, table steps, box lengths, growth factor and masses "
                         "must be positive");
        return C21CM_VALUE_ERROR;
    }
    if (s->hmf != C21CM_HMF_PS && s->hmf != C21CM_HMF_ST) {
        c21hip_set_error("halo sampler: an HMF other than PS / ST is not implemented in this backend yet");
        return C21CM_VALUE_ERROR;
    }
    if (s->sample_method != 0 && s->sample_method != 1) {
        c21hip_set_error("halo sampler: SAMPLE_METHOD = %s is not implemented in this backend yet",
                         s->sample_method == 2 ? "PARTITION" : "BINARY-SPLIT");
        return C21CM_VALUE_ERROR;
    }
    if (!listed && !catalogue_complete(out) && out->buffer_size) {
        c21hip_set_error("halo sampler: the output needs halo_masses, halo_coords, star_rng, sfr_rng and "
                         "xray_rng");
        return C21CM_VALUE_ERROR;
    }
    c21hip_hs_arrays a;
    memset(&a, 0, sizeof(a));
    a.wave_threshold = wave_threshold(s->path);
    g_last_n = 0;
    unsigned long long n_large = 0;
    if (s->from_catalog) {
        if (!desc || (desc->n_halos && !catalogue_complete(desc))) {
            c21hip_set_error("halo sampler: the descendant catalogue needs masses, coordinates and the "
                             "three deviates");
            return C21CM_VALUE_ERROR;
        }
        if (!(s->growth_in > 0) || s->redshift < s->redshift_desc) {
            c21hip_set_error("halo sampler: the descendant redshift %g lies above the progenitor redshift %g",
                             s->redshift_desc, s->redshift);
            return C21CM_VALUE_ERROR;
        }
        a.n_cond = desc->n_halos;
    } else {
        if (!density || s->hii_dim < 1 || s->hii_dim_z < 1 || !(s->m_cell > 0)) {
            c21hip_set_error("halo sampler: grid mode needs the density field, its dimensions and the cell mass");
            return C21CM_VALUE_ERROR;
        }
        a.n_cond = listed ? n_listed : (unsigned long long)s->hii_dim * s->hii_dim * s->hii_dim_z;
        a.cells_listed = listed && !s->from_catalog;
        if (large && large->n_halos) {
            if (!catalogue_complete(large)) {
                c21hip_set_error("halo sampler: the catalogue of large halos needs all five arrays");
                return C21CM_VALUE_ERROR;
            }
            n_large = large->n_halos;
        }
    }
    const unsigned long long buffer = out->buffer_size;
    float *out_h[5] = {out->halo_masses, out->halo_coords, out->star_rng, out->sfr_rng, out->xray_rng};
    const size_t width[5] = {1, 3, 1, 1, 1};
    unsigned long long total = 0;

    if (a.n_cond) {
        const size_t n = (size_t)a.n_cond, nx = (size_t)s->n_cond;
        a.tables = (const double *)c21_stage_in(WS_HS_TABLES, s->tables, nx * (3 + (size_t)s->n_prob) * sizeof(double),
                                                stream, &status);
        if (s->from_catalog) {
            a.cond_masses = (const float *)c21_stage_in(WS_HS_IN0, desc->halo_masses, n * sizeof(float), stream, &status);
            a.cond_coords = (const float *)c21_stage_in(WS_HS_IN0 + 1, desc->halo_coords, 3 * n * sizeof(float), stream, &status);
            a.cond_star = (const float *)c21_stage_in(WS_HS_IN0 + 2, desc->star_rng, n * sizeof(float), stream, &status);
            a.cond_sfr = (const float *)c21_stage_in(WS_HS_IN0 + 3, desc->sfr_rng, n * sizeof(float), stream, &status);
            a.cond_xray = (const float *)c21_stage_in(WS_HS_IN0 + 4, desc->xray_rng, n * sizeof(float), stream, &status);
        } else {
            a.density = (const float *)c21_stage_in(WS_HS_IN0, density, n * sizeof(float), stream, &status);
            a.overlap = (const float *)c21_stage_in(WS_HS_IN0 + 1, overlap, n * sizeof(float), stream, &status);
            if (a.cells_listed)
                a.cond_coords = (const float *)c21_stage_in(WS_HS_IN0 + 2, cell_crd, 3 * n * sizeof(float), stream, &status);
        }
        if (status) return status;
        const unsigned long long nb = (a.n_cond + C21HIP_HS_BLOCK - 1) / C21HIP_HS_BLOCK;
        unsigned int *words = (unsigned int *)c21hip_ws(WS_HS_WORDS, 4 * n * sizeof(unsigned int));
        unsigned long long *sums = (unsigned long long *)c21hip_ws(WS_HS_SUMS, (size_t)(nb + 2) * sizeof(*sums));
        if (!words || !sums) return C21CM_MEMORY_ALLOC_ERROR;
        unsigned long long head[2] = {0ull, ~0ull}; /* total, first failing condition */
        TRY(c21hip_h2d(sums, head, sizeof(head), stream));
        TRY(c21hip_hs_pass_a(s, &a, words, sums + 2, sums + 1, stream));
        TRY(c21hip_hs_scan(sums + 2, nb, sums, stream));
        TRY(c21hip_d2h(head, sums, sizeof(head), stream));
        TRY(c21hip_sync(stream));
        if (head[1] != ~0ull) {
            const unsigned long long idx = head[1] >> 3;
            const int code = (int)(head[1] & 7);
            if (code == C21HIP_HS_BAD_MASS)
                c21hip_set_error("halo sampler: condition %llu of %llu lies outside the tables (a descendant mass "
                                 "outside [%.3e, %.3e] or a non-finite density)", idx, a.n_cond, s->m_min,
                                 s->m_max_tables);
            else if (code == C21HIP_HS_BAD_WALK)
                c21hip_set_error("halo sampler: the removal permutation of condition %llu did not close", idx);
            else
                c21hip_set_error("halo sampler: too many halos in condition %llu (more than %d draws)", idx,
                                 s->max_halo_cell > 0 && s->max_halo_cell < C21CM_MAX_HALO_CELL
                                     ? s->max_halo_cell : C21CM_MAX_HALO_CELL);
            return C21CM_VALUE_ERROR;
        }
        total = head[0];
        if (n_large + total > buffer) {
            /* Stochasticity.c:918-933 with one share instead of N_THREADS */
            const double mem = config_settings.HALO_CATALOG_MEM_FACTOR;
            const double expected = expected_nhalo(s->redshift);
            c21hip_set_error("halo sampler: %llu halos were found and the halo catalog holds %llu.  Try raising "
                             "HALO_CATALOG_MEM_FACTOR from %.2f to %.2f.", n_large + total, buffer, mem,
                             (double)(n_large + total) / (expected + 1) * 1.15);
            return C21CM_VALUE_ERROR;
        }
        float *dev[5];
        for (int k = 0; k < 5; k++) {
            const size_t rows = (size_t)(n_large + total);
            dev[k] = out_h[k] && c21hip_is_device_ptr(out_h[k]) ? out_h[k]
                                                    : (float *)c21hip_ws(WS_HS_OUT0 + k, (rows ? rows : 1) * width[k] * sizeof(float));
            if (!dev[k]) return C21CM_MEMORY_ALLOC_ERROR;
        }
        if (n_large) {
            const float *src[5] = {large->halo_masses, large->halo_coords, large->star_rng, large->sfr_rng,
                                   large->xray_rng};
            for (int k = 0; k < 5; k++) {
                const size_t bytes = (size_t)n_large * width[k] * sizeof(float);
                TRY(c21hip_is_device_ptr(src[k]) ? c21hip_d2d(dev[k], src[k], bytes, stream)
                                                 : c21hip_h2d(dev[k], src[k], bytes, stream));
            }
        }
        if (total)
            TRY(c21hip_hs_pass_b(s, &a, words, sums + 2, n_large, dev[0], dev[1], dev[2], dev[3], dev[4], stream));
        for (int k = 0; k < 5; k++)
            if (out_h[k] && dev[k] != out_h[k] && n_large + total)
                TRY(c21hip_d2h(out_h[k], dev[k], (size_t)(n_large + total) * width[k] * sizeof(float), stream));
    }
    /* condense_sparse_halolist, :745-755: zeros from n_halos to buffer_size */
    const unsigned long long n_out = n_large + total;
    for (int k = 0; k < 5 && buffer > n_out && !listed; k++) {
        const size_t bytes = (size_t)(buffer - n_out) * width[k] * sizeof(float);
        if (c21hip_is_device_ptr(out_h[k]))
            TRY(c21hip_memset(out_h[k] + n_out * width[k], 0, bytes, stream));
        else
            memset(out_h[k] + n_out * width[k], 0, bytes);
    }
    TRY(c21hip_sync(stream));
    out->n_halos = n_out;
    g_last_n = a.n_cond;
    g_last_generation = c21hip_ws_generation();
done:
    return status;
}

int c21cm_sample_halos_grids(const c21cm_sample_halos_spec *s, const float *density, const float *overlap,
                             const HaloCatalog *large, const HaloCatalog *desc, HaloCatalog *out,
                             void *stream) {
    return sample_impl(s, density, overlap, large, desc, out, stream, 0, NULL);
}

/* halos kept per condition by the last c21cm_sample_halos_grids call of n conditions (pass A's first
 * word), into a host array: what single_test_sample reports per condition, and what a test needs to cut
 * a catalogue into its conditions */
int c21cm_sample_halos_last_counts(unsigned long long n, int *counts) {
    size_t bytes = 0;
    const unsigned int *words = (const unsigned int *)c21hip_ws_peek(WS_HS_WORDS, &bytes);
    if (!counts || !words || !n || n != g_last_n || g_last_generation != c21hip_ws_generation() ||
        bytes < 4 * (size_t)n * sizeof(unsigned int)) {
        c21hip_set_error("halo sampler: the last call that succeeded sampled %llu conditions, %llu asked for", g_last_n, n);
        return C21CM_VALUE_ERROR;
    }
    unsigned int *host = (unsigned int *)malloc(4 * (size_t)n * sizeof(unsigned int));
    if (!host) return C21CM_MEMORY_ALLOC_ERROR;
    int status = c21hip_d2h(host, words, 4 * (size_t)n * sizeof(unsigned int), NULL);
    if (!status) status = c21hip_sync(NULL);
    for (size_t i = 0; i < (size_t)n && !status; i++) counts[i] = (int)host[4 * i];
    free(host);
    return status;
}

/* single_test_sample (Stochasticity.c:1164-1306): n_condition conditions (descendant masses at z_in > 0,
 * else overdensities of cells at z_out) sampled by the same kernels; per condition the halos kept above
 * SAMPLER_MIN_MASS and their mass, and what the conditional mass function expects above SAMPLER_MIN_MASS
 * (the reference rebuilds its tables from that limit and interpolates; here the integral itself); the
 * catalogue's masses and coordinates in condition order.  Host arrays; the two catalogue arrays are
 * trusted to hold every halo, as in the reference. */
int single_test_sample(unsigned long long int seed, int n_condition, float *conditions, float *cond_crd,
                       double z_out, double z_in, int *out_n_tot, int *out_n_cell, double *out_n_exp,
                       double *out_m_cell, double *out_m_exp, float *out_halo_masses, float *out_halo_coords) {
    if (n_condition < 1 || !conditions || !cond_crd || !out_n_tot || !out_n_cell || !out_n_exp || !out_m_cell ||
        !out_m_exp || !out_halo_masses || !out_halo_coords) {
        c21hip_set_error("single_test_sample: NULL array or no condition");
        return C21CM_VALUE_ERROR;
    }
    if (z_in > 0 && z_out <= z_in) {
        c21hip_set_error("single_test_sample: progenitor sampling must go back in time (z_out = %g, z_in = %g)",
                         z_out, z_in);
        return C21CM_VALUE_ERROR;
    }
    c21cm_sample_halos_spec s;
    int status = c21cm_sampler_setup(z_out, z_in, seed, &s);
    if (status) return status;
    const size_t n = (size_t)n_condition;
    HaloCatalog out, desc;
    memset(&out, 0, sizeof(out));
    memset(&desc, 0, sizeof(desc));
    out.buffer_size = ~0ull;
    out.halo_masses = out_halo_masses;
    out.halo_coords = out_halo_coords;
    float *zeros = NULL;
    if (s.from_catalog) {
        zeros = (float *)calloc(n, sizeof(float)); /* the descendants' deviates: not reported */
        if (!zeros) return C21CM_MEMORY_ALLOC_ERROR;
        desc.n_halos = desc.buffer_size = n;
        desc.halo_masses = conditions;
        desc.halo_coords = cond_crd;
        desc.star_rng = desc.sfr_rng = desc.xray_rng = zeros;
    }
    status = sample_impl(&s, conditions, NULL, NULL, &desc, &out, NULL, n, cond_crd);
    free(zeros);
    if (status) return status;
    if ((status = c21cm_sample_halos_last_counts(n, out_n_cell))) return status;
    out_n_tot[0] = (int)out.n_halos;
    size_t row = 0;
    const double lnM_lo = log(s.sampler_min_mass);
    for (size_t j = 0; j < n; j++) {
        double mass = 0.;
        for (int k = 0; k < out_n_cell[j]; k++) mass += out_halo_masses[row++];
        out_m_cell[j] = mass;
        if (j && conditions[j] == conditions[j - 1]) {
            out_n_exp[j] = out_n_exp[j - 1];
            out_m_exp[j] = out_m_exp[j - 1];
        } else {
            c21_sampler_expected(&s, conditions[j], lnM_lo, &out_n_exp[j], &out_m_exp[j]);
        }
    }
    return 0;
}
