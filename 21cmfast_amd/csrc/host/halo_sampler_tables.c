/*
 * halo_sampler_tables.c -- the halo sampler's per-snapshot constants and tables on the host
 * (stoc_set_consts_z / stoc_set_consts_cond, Stochasticity.c:77-207; initialise_dNdM_tables and
 * initialise_dNdM_inverse_table, interp_tables.c:580-801; EvaluateNhalo / Mcoll / NhaloInv, :1046-1092) and
 * the helpers exported with the reference's names (integral_wrappers.c:26-97, Stochasticity.c:43-62).
 *
 * One sweep per condition node builds all three tables.  The conditional mass function of a condition has
 * its structure next to the condition mass (a peak whose distance from ln M_cond shrinks with the barrier
 * difference), so the sweep walks DOWN from ln M_cond in panels whose width grows geometrically with the
 * distance t = ln M_cond - ln M (PANEL_RATIO per panel from PANEL_T0), 15-point Gauss-Kronrod on each,
 * and keeps the running integrals N(> M) and M_coll(> M) at the panel edges.  The inverse table's node
 * (condition, ln p) is then the root of ln(N(> M) / N(> M_min)) = ln p inside the panel where the running
 * integral crosses, found by a bracketed Newton iteration on the edge value plus one more Gauss-Kronrod
 * sum over the part of the panel above M -- no root search over a fresh adaptive integral per node, which
 * is what costs the reference seconds per snapshot.  The iteration stops at |step| < 1e-9 in ln M, far
 * inside the reference's own root tolerance (rf_tol_abs = 1e-4, interp_tables.c:676).
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"
#include "cosmology.h"

#define MAX_DELTAC_FRAC ((float)0.99) /* hmf.h:8 */
#define DELTA_MIN (-1.)               /* hmf.h:9 */
#define M_MAX_INTEGRAL 1e16           /* hmf.h:11 */
#define FRACT_FLOAT_ERR 1e-7
#define PANEL_T0 1e-7
#define PANEL_RATIO 1.04
#define MAX_PANELS 1024

static const double gk_x[8] = {0.991455371120812639206854697526329, 0.949107912342758524526189684047851,
                               0.864864423359769072789712788640926, 0.741531185599394439863864773280788,
                               0.586087235467691130294144838258730, 0.405845151377397166906606412076961,
                               0.207784955007898467600689403773245, 0.0};
static const double gk_wk[8] = {0.022935322010529224963732008058970, 0.063092092629978553290700663189204,
                                0.104790010322250183839876322541518, 0.140653259715525918745189590510238,
                                0.169004726639267902826583426598550, 0.190350578064785409913256402421014,
                                0.204432940075298892414161999234649, 0.209482141084727828012999174891714};

struct cond {
    double growthf, lnM_cond, sigma, delta;
    int hmf;
};

/* integrals of the conditional mass function and of M times it over [a, b] (15-point Kronrod rule) */
static void gk15_pair(const struct cond *c, double a, double b, double *n_out, double *m_out) {
    const double mid = 0.5 * (a + b), h = 0.5 * (b - a);
    double f = conditional_hmf(c->growthf, mid, c->delta, c->sigma, c->hmf);
    double sn = gk_wk[7] * f, sm = gk_wk[7] * f * exp(mid);
    for (int j = 0; j < 7; j++) {
        const double dx = h * gk_x[j];
        const double f1 = conditional_hmf(c->growthf, mid - dx, c->delta, c->sigma, c->hmf);
        const double f2 = conditional_hmf(c->growthf, mid + dx, c->delta, c->sigma, c->hmf);
        sn += gk_wk[j] * (f1 + f2);
        sm += gk_wk[j] * (f1 * exp(mid - dx) + f2 * exp(mid + dx));
    }
    *n_out = sn * h;
    *m_out = sm * h;
}

/* the panel edges ln M_cond - t_k between `hi` (<= ln M_cond) and `lo`, from the top down: edges[0] = hi,
 * edges[n] = lo; returns n (0 when the interval is empty) */
static int panel_edges(double lnM_cond, double lo, double hi, double *edges) {
    if (hi > lnM_cond) hi = lnM_cond;
    if (!(lo < hi)) return 0;
    int n = 0;
    edges[0] = hi;
    double t = lnM_cond - hi;
    t = t < PANEL_T0 ? PANEL_T0 : t * PANEL_RATIO;
    while (lnM_cond - t > lo && n < MAX_PANELS - 2) {
        edges[++n] = lnM_cond - t;
        t *= PANEL_RATIO;
    }
    edges[++n] = lo;
    return n;
}

/* Nhalo_Conditional and Mcoll_Conditional (hmf.c:1019-1064), per unit condition mass */
static void conditional_integrals(const struct cond *c, double lnM1, double lnM2, double *n_out, double *m_out) {
    *n_out = *m_out = 0.;
    if (lnM1 >= c->lnM_cond) return;
    if (c->delta > MAX_DELTAC_FRAC * get_delta_crit(c->hmf, c->sigma, c->growthf)) {
        if (c->lnM_cond * (1 - FRACT_FLOAT_ERR) <= lnM2) {
            *n_out = 1. / exp(c->lnM_cond);
            *m_out = 1.;
        }
        return;
    }
    double edges[MAX_PANELS];
    const int n = panel_edges(c->lnM_cond, lnM1, lnM2, edges);
    for (int k = 0; k < n; k++) {
        double pn, pm;
        gk15_pair(c, edges[k + 1], edges[k], &pn, &pm);
        *n_out += pn;
        *m_out += pm;
    }
}

/* ---------------------------------------------------------------- the tables of one snapshot */
static struct {
    int ready;
    double key[20];
    c21cm_sample_halos_spec spec;
    double *tables;
    size_t n_doubles;
} tb;
static pthread_mutex_t tb_lock = PTHREAD_MUTEX_INITIALIZER; /* the cache is looked up and replaced under it */

static double lerp1(const double *y, int n, double x_min, double x_width, double x) { /* EvaluateRGTable1D */
    int idx = (int)floor((x - x_min) / x_width);
    if (idx > n - 2) idx = n - 2; /* the reference reads past its table at the upper edge */
    if (idx < 0) idx = 0;
    const double t = (x - (x_min + x_width * (double)idx)) / x_width;
    return y[idx] * (1 - t) + y[idx + 1] * t;
}

static double lerp2(const double *z, int nx, int ny, double x_min, double x_width, double y_min, double y_width,
                    double x, double y) { /* EvaluateRGTable2D */
    int xi = (int)floor((x - x_min) / x_width), yi = (int)floor((y - y_min) / y_width);
    if (xi > nx - 2) xi = nx - 2;
    if (xi < 0) xi = 0;
    if (yi > ny - 2) yi = ny - 2;
    if (yi < 0) yi = 0;
    const double tx = (x - (x_min + x_width * (double)xi)) / x_width;
    const double ty = (y - (y_min + y_width * (double)yi)) / y_width;
    const double left = z[(size_t)xi * ny + yi] * (1 - ty) + z[(size_t)xi * ny + yi + 1] * ty;
    const double right = z[(size_t)(xi + 1) * ny + yi] * (1 - ty) + z[(size_t)(xi + 1) * ny + yi + 1] * ty;
    return left * (1 - tx) + right * tx;
}

/* one row of the three tables: condition node i */
static void build_row(const c21cm_sample_halos_spec *s, int i, double x, double lnM_lo_sample, double lnM_lo_int,
                      double lnM_hi_int, double *nhalo, double *mcoll, double *sigma_tab, double *inv) {
    const int np = s->n_prob;
    struct cond c;
    c.growthf = s->growth_out;
    c.hmf = s->hmf;
    if (s->from_catalog) {
        c.lnM_cond = x;
        c.sigma = c21_sigma_fast(exp(x));
        c.delta = get_delta_crit(s->hmf, c.sigma, s->growth_in) / s->growth_in * s->growth_out;
        sigma_tab[i] = c.sigma;
    } else {
        c.lnM_cond = log(s->m_cell);
        c.sigma = s->sigma_cell;
        c.delta = x;
        sigma_tab[i] = 0.;
    }
    conditional_integrals(&c, lnM_lo_int, lnM_hi_int, &nhalo[i], &mcoll[i]);

    double *row = inv + (size_t)i * np;
    const double M_cond = exp(c.lnM_cond);
    if (!s->from_catalog && c.delta > MAX_DELTAC_FRAC * get_delta_crit(s->hmf, c.sigma, s->growth_out)) {
        for (int k = 1; k < np; k++) row[k] = 1.; /* interp_tables.c:739-743 */
        return;
    }
    /* running N(> M) at the panel edges from ln M_cond down to the sampling minimum */
    double edges[MAX_PANELS], cum[MAX_PANELS];
    const int n = panel_edges(c.lnM_cond, lnM_lo_sample, c.lnM_cond, edges);
    cum[0] = 0.;
    for (int k = 0; k < n; k++) {
        double pn, pm;
        gk15_pair(&c, edges[k + 1], edges[k], &pn, &pm);
        cum[k + 1] = cum[k] + pn;
    }
    const double norm = n ? cum[n] : 0.;
    if (!(norm > 0.)) {
        for (int k = 1; k < np - 1; k++) row[k] = exp(lnM_lo_sample) / M_cond; /* :761-764 */
        return;
    }
    row[np - 1] = exp(lnM_lo_sample) / M_cond;
    int panel = n - 1; /* the targets fall from ln p = 0: the roots climb towards ln M_cond */
    for (int k = np - 2; k >= 0; k--) {
        const double target = s->p_min + s->p_width * k + log(norm); /* ln N(> M) wanted */
        while (panel > 0 && cum[panel] > 0. && log(cum[panel]) > target) panel--;
        /* the root lies in [edges[panel + 1], edges[panel]]: cum rises from cum[panel] to cum[panel + 1] */
        double lo = edges[panel + 1], hi = edges[panel], xr = 0.5 * (lo + hi);
        for (int it = 0; it < 60; it++) {
            double pn, pm;
            gk15_pair(&c, xr, edges[panel], &pn, &pm);
            const double F = cum[panel] + pn;
            const double g = F > 0. ? log(F) - target : -1e300;
            if (g > 0.) lo = xr; else hi = xr; /* N(> M) too large: M must rise */
            const double f = conditional_hmf(c.growthf, xr, c.delta, c.sigma, c.hmf);
            double step = (F > 0. && f > 0.) ? g * F / f : 0.; /* Newton on ln F, d ln F / dx = -f / F */
            double xn = xr + step;
            if (!(step != 0.) || !(xn > lo && xn < hi)) xn = 0.5 * (lo + hi);
            const double moved = fabs(xn - xr);
            xr = xn;
            if (moved < 1e-9 || hi - lo < 1e-9) break;
        }
        row[k] = exp(xr) / M_cond;
    }
}

const char *c21_sampler_unsupported_options(void) {
    const MatterOptions *mo = matter_options_global;
    if (mo->HMF != C21CM_HMF_PS && mo->HMF != C21CM_HMF_ST) return "an HMF other than PS / ST";
    if (mo->USE_INTERPOLATION_TABLES != C21CM_INTERP_HMF)
        return "USE_INTERPOLATION_TABLES other than hmf-interpolation";
    if (mo->SAMPLE_METHOD == 2) return "SAMPLE_METHOD = PARTITION";
    if (mo->SAMPLE_METHOD == 3) return "SAMPLE_METHOD = BINARY-SPLIT";
    if (mo->SAMPLE_METHOD < 0 || mo->SAMPLE_METHOD > 3) return "an unknown SAMPLE_METHOD";
    if (astro_options_global && astro_options_global->PHOTON_CONS_TYPE != C21CM_PHOTONCONS_NONE)
        return "PHOTON_CONS_TYPE != none";
    return NULL;
}

int c21cm_sampler_setup(double redshift, double redshift_desc, unsigned long long seed,
                        c21cm_sample_halos_spec *spec) {
    if (!spec) return C21CM_VALUE_ERROR;
    if (!simulation_options_global || !matter_options_global || !cosmo_params_global) {
        c21hip_set_error("halo sampler: Broadcast_struct_global_all has not been called");
        return C21CM_VALUE_ERROR;
    }
    const char *why = c21_sampler_unsupported_options();
    if (why) {
        c21hip_set_error("halo sampler: %s is not implemented in this backend yet", why);
        return C21CM_VALUE_ERROR;
    }
    if (redshift_desc > 0 && redshift < redshift_desc) {
        c21hip_set_error("halo sampler: the descendant redshift %g lies above the progenitor redshift %g",
                         redshift_desc, redshift);
        return C21CM_VALUE_ERROR;
    }
    if (!c21_ps_ready()) init_ps();
    if (!c21_ps_ready()) return C21CM_VALUE_ERROR;
    const SimulationOptions *so = simulation_options_global;
    const int nx = so->N_COND_INTERP, np = so->N_PROB_INTERP;
    if (nx < 2 || np < 3 || !(so->MIN_LOGPROB < 0) || !(so->SAMPLER_MIN_MASS > 0) ||
        !(so->SAMPLER_BUFFER_FACTOR >= 1)) {
        c21hip_set_error("halo sampler: N_COND_INTERP >= 2, N_PROB_INTERP >= 3, MIN_LOGPROB < 0, "
                         "SAMPLER_MIN_MASS > 0 and SAMPLER_BUFFER_FACTOR >= 1 are required");
        return C21CM_VALUE_ERROR;
    }
    c21cm_sample_halos_spec s;
    memset(&s, 0, sizeof(s));
    s.from_catalog = redshift_desc > 0;
    s.sample_method = matter_options_global->SAMPLE_METHOD;
    s.hmf = matter_options_global->HMF;
    s.hii_dim = so->HII_DIM;
    s.hii_dim_z = (int)(so->NON_CUBIC_FACTOR * so->HII_DIM);
    s.n_cond = nx;
    s.n_prob = np;
    s.max_halo_cell = C21CM_MAX_HALO_CELL;
    s.seed = seed;
    s.redshift = redshift;
    s.redshift_desc = redshift_desc;
    s.box_len = (double)so->BOX_LEN;
    s.box_len_z = (double)(so->BOX_LEN * so->NON_CUBIC_FACTOR);
    s.growth_out = dicke(redshift);
    s.m_min = so->SAMPLER_MIN_MASS / so->SAMPLER_BUFFER_FACTOR;
    s.m_max_tables = M_MAX_INTEGRAL;
    s.sampler_min_mass = so->SAMPLER_MIN_MASS;
    s.halomass_correction = so->HALOMASS_CORRECTION;
    s.rtom_unit = c21_RtoM(1.0);
    s.p_min = so->MIN_LOGPROB;
    s.p_width = -so->MIN_LOGPROB / (double)(np - 1);
    const double lnM_min = log(s.m_min), lnM_max = log(s.m_max_tables);
    double xmax;
    if (s.from_catalog) {
        s.growth_in = dicke(redshift_desc);
        const double dz = redshift - redshift_desc;
        s.corr_star = so->CORR_STAR > 0 ? exp(-dz / so->CORR_STAR) : 0.;
        s.corr_sfr = so->CORR_SFR > 0 ? exp(-dz / so->CORR_SFR) : 0.;
        s.corr_xray = so->CORR_LX > 0 ? exp(-dz / so->CORR_LX) : 0.;
        s.x_min = log((double)so->SAMPLER_MIN_MASS);
        xmax = lnM_max;
    } else {
        const double volume = s.box_len * s.box_len * s.box_len_z;
        s.m_cell = c21_rhocrit() * cosmo_params_global->OMm * volume /
                   ((double)s.hii_dim * s.hii_dim * s.hii_dim_z);
        s.sigma_cell = c21_sigma_fast(s.m_cell);
        s.x_min = DELTA_MIN;
        xmax = MAX_DELTAC_FRAC * get_delta_crit(s.hmf, s.sigma_cell, s.growth_out);
    }
    s.x_width = (xmax - s.x_min) / ((double)nx - 1);

    /* everything the tables depend on: the snapshot, the table shape, and the cosmology through its
     * parameters and sigma(M) at three masses (the power spectrum's options and normalisation) */
    const CosmoParams *cp = cosmo_params_global;
    const double key[20] = {redshift, redshift_desc, s.m_min, (double)nx, (double)np, s.p_min, (double)s.hmf,
                            s.growth_out, s.growth_in, s.m_cell, s.sampler_min_mass, c21_sigma_fast(1e8),
                            c21_sigma_fast(1e10), c21_sigma_fast(1e13), cp->hlittle, cp->OMm, cp->OMb,
                            cp->POWER_INDEX, (double)matter_options_global->POWER_SPECTRUM, c21_rhocrit()};
    pthread_mutex_lock(&tb_lock);
    const size_t n_doubles = (size_t)nx * (3 + (size_t)np);
    if (!tb.ready || memcmp(key, tb.key, sizeof(key)) || tb.n_doubles != n_doubles) {
        double *t = (double *)calloc(n_doubles, sizeof(double));
        if (!t) {
            pthread_mutex_unlock(&tb_lock);
            return C21CM_MEMORY_ALLOC_ERROR;
        }
        (void)c21_sigma_fast(1e10); /* the sigma(M) table is built outside the parallel loop */
        double *nhalo = t, *mcoll = t + nx, *sigma_tab = t + 2 * (size_t)nx, *inv = t + 3 * (size_t)nx;
#pragma omp parallel for schedule(dynamic, 1)
        for (int i = 0; i < nx; i++) {
            /* the last node sits exactly on the upper limit (interp_tables.c:690-691) */
            const double x = i == nx - 1 ? xmax : s.x_min + (xmax - s.x_min) * (double)i / ((double)nx - 1);
            build_row(&s, i, x, lnM_min, lnM_min, lnM_max, nhalo, mcoll, sigma_tab, inv);
        }
        free(tb.tables);
        tb.tables = t;
        tb.n_doubles = n_doubles;
        memcpy(tb.key, key, sizeof(key));
        tb.ready = 1;
    }
    s.tables = tb.tables;
    tb.spec = s;
    pthread_mutex_unlock(&tb_lock);
    *spec = s;
    return 0;
}

/* ---------------------------------------------------------------- per-condition constants on the host */
struct cond_consts {
    double M_cond, lnM_cond, sigma_cond, delta, cond_val, delta_crit, expected_N, expected_M;
};

/* stoc_set_consts_cond (Stochasticity.c:158-207) */
static void set_consts_cond(const c21cm_sample_halos_spec *s, double cond_val, struct cond_consts *c) {
    const int nx = s->n_cond;
    if (s->from_catalog) {
        c->M_cond = cond_val;
        c->lnM_cond = log(cond_val);
        /* sigma(M) as the kernel takes it: linear on the condition nodes, so that the helpers report the
         * delta, the barrier and the expectations of exactly what is sampled */
        c->sigma_cond = lerp1(s->tables + 2 * (size_t)nx, nx, s->x_min, s->x_width, c->lnM_cond);
        c->cond_val = c->lnM_cond;
        c->delta = get_delta_crit(s->hmf, c->sigma_cond, s->growth_in) / s->growth_in * s->growth_out;
    } else {
        c->M_cond = s->m_cell;
        c->lnM_cond = log(s->m_cell);
        c->sigma_cond = s->sigma_cell;
        c->delta = c->cond_val = cond_val;
    }
    c->delta_crit = get_delta_crit(s->hmf, c->sigma_cond, s->growth_out);
    if (c->delta > MAX_DELTAC_FRAC * c->delta_crit) {
        c->expected_M = c->M_cond;
        c->expected_N = 1;
    } else if (c->delta <= DELTA_MIN || c->M_cond < s->m_min) {
        c->expected_M = c->expected_N = 0;
    } else {
        c->expected_N = lerp1(s->tables, nx, s->x_min, s->x_width, c->cond_val) * c->M_cond;
        c->expected_M = lerp1(s->tables + nx, nx, s->x_min, s->x_width, c->cond_val) * c->M_cond;
    }
}

/* expected N and M of one condition above exp(lnM_lo): stoc_set_consts_cond with the integrals themselves
 * in place of the tables (single_test_sample, Stochasticity.c:1269-1296) */
void c21_sampler_expected(const c21cm_sample_halos_spec *s, double cond_val, double lnM_lo, double *n_exp,
                          double *m_exp) {
    struct cond_consts c;
    set_consts_cond(s, cond_val, &c);
    *n_exp = c.expected_N;
    *m_exp = c.expected_M;
    if (c.delta > MAX_DELTAC_FRAC * c.delta_crit || c.delta <= DELTA_MIN || c.M_cond < s->m_min) return;
    const struct cond q = {s->growth_out, c.lnM_cond, c.sigma_cond, c.delta, s->hmf};
    conditional_integrals(&q, lnM_lo, log(s->m_max_tables), n_exp, m_exp);
    *n_exp *= c.M_cond;
    *m_exp *= c.M_cond;
}

static int out_of_bounds(const c21cm_sample_halos_spec *s, const struct cond_consts *c) { /* :28-33 */
    return c->M_cond < s->sampler_min_mass || c->M_cond > s->m_max_tables || c->delta < -1 ||
           c->delta > MAX_DELTAC_FRAC * get_delta_crit(s->hmf, c->sigma_cond, s->growth_out);
}

void get_condition_integrals(double redshift, double z_prev, int n_conditions, double *cond_values,
                             double *out_n_exp, double *out_m_exp) {
    c21cm_sample_halos_spec s;
    if (c21cm_sampler_setup(redshift, z_prev, 0, &s)) {
        for (int i = 0; i < n_conditions; i++) out_n_exp[i] = out_m_exp[i] = NAN;
        return;
    }
    for (int i = 0; i < n_conditions; i++) {
        struct cond_consts c;
        set_consts_cond(&s, cond_values[i], &c);
        if (out_of_bounds(&s, &c)) {
            out_n_exp[i] = -1.;
            continue;
        }
        out_n_exp[i] = c.expected_N;
        out_m_exp[i] = c.expected_M;
    }
}

void get_halo_chmf_interval(double redshift, double z_prev, int n_conditions, double *cond_values,
                            int n_masslim, double *lnM_lo, double *lnM_hi, double *out_n) {
    c21cm_sample_halos_spec s;
    if (c21cm_sampler_setup(redshift, z_prev, 0, &s)) {
        for (int i = 0; i < n_conditions * n_masslim; i++) out_n[i] = NAN;
        return;
    }
    for (int i = 0; i < n_conditions; i++) {
        struct cond_consts c;
        set_consts_cond(&s, cond_values[i], &c);
        const struct cond q = {s.growth_out, c.lnM_cond, c.sigma_cond, c.delta, s.hmf};
        for (int j = 0; j < n_masslim; j++) {
            double n, m;
            conditional_integrals(&q, lnM_lo[j], lnM_hi[j], &n, &m);
            out_n[i * n_masslim + j] = n * c.M_cond;
        }
    }
}

void get_halomass_at_probability(double redshift, double z_prev, int n_conditions, double *cond_values,
                                 double *probabilities, double *out_mass) {
    c21cm_sample_halos_spec s;
    if (c21cm_sampler_setup(redshift, z_prev, 0, &s)) {
        for (int i = 0; i < n_conditions; i++) out_mass[i] = NAN;
        return;
    }
    const double *inv = s.tables + 3 * (size_t)s.n_cond;
    for (int i = 0; i < n_conditions; i++) {
        struct cond_consts c;
        set_consts_cond(&s, cond_values[i], &c);
        const double p = probabilities[i];
        if (out_of_bounds(&s, &c) || p < 0 || p > 1) {
            out_mass[i] = -1;
            continue;
        }
        double lnp = log(p); /* EvaluateNhaloInv, interp_tables.c:1085-1092 */
        if (p == 0 || lnp < s.p_min) lnp = s.p_min;
        out_mass[i] = lerp2(inv, s.n_cond, s.n_prob, s.x_min, s.x_width, s.p_min, s.p_width, c.cond_val, lnp) *
                      c.M_cond;
    }
}

/* Stochasticity.c:43-62 */
double expected_nhalo(double redshift) {
    if (!simulation_options_global || !matter_options_global || !cosmo_params_global) return NAN;
    if (!c21_ps_ready()) init_ps();
    const SimulationOptions *so = simulation_options_global;
    const double box_z = (double)(so->BOX_LEN * so->NON_CUBIC_FACTOR);
    const double volume = (double)so->BOX_LEN * so->BOX_LEN * box_z;
    const double hii_tot = (double)so->HII_DIM * so->HII_DIM * (int)(so->NON_CUBIC_FACTOR * so->HII_DIM);
    double M_min;
    if (matter_options_global->SOURCE_MODEL == C21CM_SOURCE_CHMF_SAMPLER)
        M_min = so->SAMPLER_MIN_MASS;
    else
        M_min = c21_RtoM(0.620350491 * so->BOX_LEN / so->DIM);
    const double rho_m = c21_rhocrit() * cosmo_params_global->OMm;
    const double M_max = rho_m * volume / hii_tot;
    /* the adaptive quadrature does not return for limits that are not finite */
    if (!(M_min > 0) || !(M_max > 0) || !isfinite(M_min) || !isfinite(M_max) || !isfinite(redshift) ||
        !isfinite(volume * rho_m))
        return NAN;
    if (M_min >= M_max) return 0.;
    return c21_Nhalo_General(redshift, log(M_min), log(M_max)) * volume * rho_m;
}

/* HaloCatalog.c:81-200: the radii DexM filters at, each skipped when a halo of its mass is rarer than
 * 7 sigma under the DexM barrier (sheth_delc_dexm, hmf.c:143-146).  One walk serves both callers: with
 * spec == NULL it stops at the first kept rung (c21cm_dexm_is_empty), else it stores every kept rung.
 * Returns the number of kept rungs (1 for "at least one" without a spec), -1 for parameters that describe
 * no box, -2 for more rungs than the spec holds. */
static int dexm_walk(double redshift, c21cm_find_halos_spec *spec) {
    const SimulationOptions *so = simulation_options_global;
    const double l_factor = 0.620350491;
    const float growth = dicke(redshift);
    const double dim = matter_options_global->SOURCE_MODEL == C21CM_SOURCE_CHMF_SAMPLER ? so->HII_DIM : so->DIM;
    const float M_MIN = c21_RtoM(l_factor * so->BOX_LEN / dim);
    const float Delta_R = l_factor * 2. * so->BOX_LEN / (so->DIM + 0.0);
    /* Nothing non-finite may reach sigma_z0: its adaptive quadrature does not return for a mass that is
     * not a finite positive number.  Parameters that cannot describe a box (a non-finite or absurd box
     * length, a step factor next to 1, a mass that overflows a float) answer "no box", which makes
     * c21cm_dexm_is_empty say "not empty" and ComputeHaloCatalog refuse.  Both walks are bounded. */
    if (!(so->DELTA_R_FACTOR >= 1.0001) || !(so->DELTA_R_FACTOR <= 1e3) || !(so->BOX_LEN > 0) ||
        !(so->BOX_LEN <= 1e6) || dim < 1 || so->DIM < 1 || !(growth > 0) || !isfinite(growth) ||
        !(M_MIN > 0) || !isfinite(M_MIN))
        return -1;
    float R = c21_MtoR(M_MIN * 1.01);
    if (!(R > 0) || !isfinite(R)) return -1;
    int steps = 0, kept = 0;
    while (R < l_factor * so->BOX_LEN && steps++ < 4096) R *= so->DELTA_R_FACTOR;
    if (!(R >= l_factor * so->BOX_LEN) || !isfinite(R)) return -1;
    steps = 0;
    while (R > 0.5 * Delta_R && c21_RtoM(R) >= M_MIN) {
        if (steps++ >= 4096) return -1;
        const float M = c21_RtoM(R);
        if (!(M > 0) || !isfinite(M)) return -1;
        const double sig = sigma_z0(M), del = 1.686 / growth;
        const float delta_crit = growth * (sqrt(0.73) * del * (1. + 0.15 * pow(sig * sig / (0.73 * del * del), 0.05)));
        if (!(sig * growth * 7. < delta_crit)) {
            if (!spec) return 1;
            if (kept >= C21CM_MAX_DEXM_RADII) return -2;
            spec->R[kept] = R;
            spec->mass[kept] = M;
            spec->delta_crit[kept] = delta_crit;
            kept++;
        }
        R /= so->DELTA_R_FACTOR;
    }
    return kept;
}

int c21cm_dexm_is_empty(double redshift) {
    if (!simulation_options_global || !matter_options_global || !cosmo_params_global) return 0;
    if (!c21_ps_ready()) init_ps();
    return dexm_walk(redshift, NULL) == 0;
}

int c21cm_dexm_ladder(double redshift, c21cm_find_halos_spec *spec) {
    if (!spec) return C21CM_VALUE_ERROR;
    if (!simulation_options_global || !matter_options_global || !cosmo_params_global) {
        c21hip_set_error("DexM ladder: Broadcast_struct_global_all has not been called");
        return C21CM_VALUE_ERROR;
    }
    if (!c21_ps_ready()) init_ps();
    if (!c21_ps_ready()) return C21CM_VALUE_ERROR;
    const SimulationOptions *so = simulation_options_global;
    const MatterOptions *mo = matter_options_global;
    memset(spec, 0, sizeof(*spec));
    const int n = dexm_walk(redshift, spec);
    if (n == -1) {
        c21hip_set_error("DexM ladder: BOX_LEN, DIM, HII_DIM, DELTA_R_FACTOR and the cosmology describe no box");
        return C21CM_VALUE_ERROR;
    }
    if (n == -2) {
        c21hip_set_error("DexM ladder: more than %d radii; raise DELTA_R_FACTOR", C21CM_MAX_DEXM_RADII);
        return C21CM_VALUE_ERROR;
    }
    spec->n_R = n;
    spec->dim = so->DIM;
    spec->dim_z = (int)(so->NON_CUBIC_FACTOR * so->DIM);
    if (mo->SOURCE_MODEL == C21CM_SOURCE_CHMF_SAMPLER) {
        spec->hii_dim = so->HII_DIM;
        spec->hii_dim_z = (int)(so->NON_CUBIC_FACTOR * so->HII_DIM);
    }
    spec->halo_filter = mo->HALO_FILTER;
    spec->optimize = mo->DEXM_OPTIMIZE ? 1 : 0;
    spec->redshift = redshift;
    spec->box_len = (double)so->BOX_LEN;
    spec->box_len_z = (double)(so->BOX_LEN * so->NON_CUBIC_FACTOR);
    spec->growth = (double)(float)dicke(redshift);
    spec->r_overlap = so->DEXM_R_OVERLAP;
    spec->optimize_minmass = so->DEXM_OPTIMIZE_MINMASS;
    spec->rtom_unit = c21_RtoM(1.0);
    return 0;
}
