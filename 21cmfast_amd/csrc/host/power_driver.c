/*
 * power_driver.c -- C host driver of the binned power spectrum: pack -> batched r2c (rocFFT)
 * -> one binning launch -> fixed-order sums (csrc/hip/power_kernels.hip).  The host builds what is cheap and
 * must match numpy bit for bit: the per-axis wavenumbers (fftfreq(n, L/n) 2 pi) and, for cylindrical spectra,
 * the k_perp bin of every (x, y) row; the workgroups' row lists follow from them.  The options of
 * c21cm_power_opts (taper, mu / wedge cuts, variance) select other instantiations of the same kernels; without
 * them every launch and every value is what c21cm_power_spectrum_grids always did.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../hip/c21hip.h"
#include "c21cm_grid.h"

/* half-spectrum modes one workgroup aims for (at most), and workgroups a launch aims for (at least) */
#define PW_MODES_PER_WG 32768
#define PW_MIN_WGS 1024

#define TRY(expr)         \
    do {                  \
        int st_ = (expr); \
        if (st_) {        \
            status = st_; \
            goto done;    \
        }                 \
    } while (0)

static int pw_fail(const char *msg) {
    c21hip_set_error("power spectrum: %s", msg);
    return C21CM_VALUE_ERROR;
}

/* numpy: fftfreq(n, d) = [0, 1, .., (n-1)/2, -(n/2), .., -1] * (1.0 / (n * d)), then * 2.0 * pi, d = L / n */
static void k_axis(double *k, int n, int count, double L) {
    const double d = L / (double)n, val = 1.0 / ((double)n * d);
    const int npos = (n - 1) / 2 + 1;
    for (int i = 0; i < count; ++i) {
        const long long f = i < npos ? i : (long long)i - n;
        k[i] = (double)f * val * 2.0 * 3.141592653589793;
    }
}

static int edges_ok(const double *e, int n) {
    if (!e) return 0;
    for (int i = 0; i <= n; ++i)
        if (!isfinite(e[i]) || (i && !(e[i] > e[i - 1]))) return 0;
    return 1;
}

/* the smallest x with sqrt(x) >= e (sqrt correctly rounded, as numpy's): the kernel bins |k|^2 on these */
static double sq_threshold(double e) {
    if (e < 0) return -INFINITY;
    if (e == 0) return 0.0;
    double x = e * e;
    while (sqrt(x) < e) x = nextafter(x, INFINITY);
    while (x > 0 && sqrt(nextafter(x, -INFINITY)) >= e) x = nextafter(x, -INFINITY);
    return x;
}

/* np.digitize on increasing edges, less one: -1 below, n at or above the last edge */
static int digitize(const double *e, int n, double x) {
    int lo = 0, hi = n + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

static int window_ok(const double *w, int n) {
    int nonzero = 0;
    for (int i = 0; w && i < n; ++i) {
        if (!isfinite(w[i])) return 0;
        nonzero |= w[i] != 0.0;
    }
    return !w || nonzero;
}

int c21cm_power_spectrum_grids(const float *field, const float *field2, int nx, int ny, int nz, int n_batch,
                               long long row_pitch, const long long *batch_offsets, double Lx, double Ly,
                               double Lz, const c21cm_power_bins *bins, double *power, double *kmean,
                               long long *counts, void *stream) {
    return c21cm_power_spectrum_ex_grids(field, field2, nx, ny, nz, n_batch, row_pitch, batch_offsets, Lx, Ly, Lz,
                                         bins, NULL, power, kmean, NULL, counts, stream);
}

int c21cm_power_spectrum_ex_grids(const float *field, const float *field2, int nx, int ny, int nz, int n_batch,
                                  long long row_pitch, const long long *batch_offsets, double Lx, double Ly,
                                  double Lz, const c21cm_power_bins *bins, const c21cm_power_opts *opts,
                                  double *power, double *kmean, double *variance, long long *counts,
                                  void *stream) {
    int status = 0;
    unsigned char *host_tab = NULL;
    int *row_bin = NULL;
    if (!bins) return pw_fail("bins are required");
    if (!field || !power || !kmean || !counts || !batch_offsets) return pw_fail("a required pointer is NULL");
    if (nx < 2 || ny < 2 || nz < 2) return pw_fail("every axis needs at least 2 cells");
    if ((long long)nx * ny > 0x7FFFFFFFll) return pw_fail("nx * ny must be below 2^31");
    if (n_batch < 1 || n_batch > 65535) return pw_fail("n_batch must be in [1, 65535]");
    if (row_pitch < nz) return pw_fail("row_pitch must be >= nz");
    if (!(isfinite(Lx) && isfinite(Ly) && isfinite(Lz) && Lx > 0 && Ly > 0 && Lz > 0))
        return pw_fail("box lengths must be positive and finite");
    const int cyl = bins->cylindrical != 0;
    if (bins->n_bins < 1 || (cyl && bins->n_bins_par < 1)) return pw_fail("at least one bin per axis is needed");
    if (!edges_ok(bins->edges, bins->n_bins) || (cyl && !edges_ok(bins->edges_par, bins->n_bins_par)))
        return pw_fail("bin edges must be finite and increasing");
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] < 0) return pw_fail("batch offsets must be >= 0");
    const int n_local = cyl ? bins->n_bins_par : bins->n_bins;
    const int n_groups = cyl ? bins->n_bins : 1;
    const int want_var = opts && opts->want_variance;
    const int use_mu = opts && opts->use_mu, use_wedge = opts && opts->use_wedge;
    const int windowed = opts && (opts->window_x || opts->window_y || opts->window_z);
    if (want_var && !variance) return pw_fail("want_variance needs a variance array");
    if ((use_mu || use_wedge) && cyl) return pw_fail("mu and wedge cuts apply to spherical bins only");
    if (use_mu) {
        if (!(opts->mu_min_sq >= 0 && opts->mu_min_sq <= 1 && opts->mu_max_sq >= 0 && opts->mu_max_sq <= 1))
            return pw_fail("mu_min and mu_max must lie in [0, 1]");
        if (opts->mu_min_sq > opts->mu_max_sq) return pw_fail("mu_min must not exceed mu_max");
    }
    if (use_wedge && !(opts->wedge_slope_sq >= 0 && isfinite(opts->wedge_slope_sq) && opts->wedge_buffer >= 0 &&
                       isfinite(opts->wedge_buffer)))
        return pw_fail("wedge_slope and wedge_buffer must be finite and >= 0");
    if (windowed) {
        if (!window_ok(opts->window_x, nx) || !window_ok(opts->window_y, ny) || !window_ok(opts->window_z, nz))
            return pw_fail("a window must be finite and not all zero");
        if (!(isfinite(opts->inv_mean_w2) && opts->inv_mean_w2 > 0))
            return pw_fail("inv_mean_w2 must be positive and finite");
    }
    if (c21hip_power_lds_bytes(n_local, cyl, want_var) > C21HIP_POWER_MAX_LDS) {
        c21hip_set_error("power spectrum: %d %s bins%s do not fit the LDS of one workgroup", n_local,
                         cyl ? "k_par" : "|k|", want_var ? " with the variance" : "");
        return C21CM_VALUE_ERROR;
    }

    const int nh = nz / 2 + 1, n_rows = nx * ny;
    double *kx = NULL, *ky = NULL, *kz = NULL;
    /* host wavenumbers (also for the k_perp bins of the rows) */
    double *ktab = (double *)malloc(sizeof(double) * ((size_t)nx + ny + nh));
    row_bin = (int *)malloc(sizeof(int) * (size_t)n_rows);
    if (!ktab || !row_bin) {
        free(ktab);
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    kx = ktab;
    ky = kx + nx;
    kz = ky + ny;
    k_axis(kx, nx, nx, Lx);
    k_axis(ky, ny, ny, Ly);
    k_axis(kz, nz, nh, Lz);

    /* the rows each group bins, in row order; cylindrical rows outside the k_perp edges are left out */
    int *group_rows = (int *)calloc((size_t)n_groups + 1, sizeof(int));
    if (!group_rows) {
        free(ktab);
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    for (int r = 0; r < n_rows; ++r) {
        int g = 0;
        if (r == 0 && bins->ignore_kperp_zero) g = -1;
        else if (cyl) {
            const double kxv = kx[r / ny], kyv = ky[r % ny];
            g = digitize(bins->edges, bins->n_bins, sqrt(kxv * kxv + kyv * kyv));
            if (g >= bins->n_bins) g = -1;
        }
        row_bin[r] = g;
        if (g >= 0) group_rows[g + 1]++;
    }
    for (int g = 0; g < n_groups; ++g) group_rows[g + 1] += group_rows[g];
    const int n_used = group_rows[n_groups];
    long long want = ((long long)n_used * n_batch + PW_MIN_WGS - 1) / PW_MIN_WGS;
    int rpw = PW_MODES_PER_WG / nh;
    if (want < rpw) rpw = (int)want;
    if (rpw < 1) rpw = 1;
    int n_wg = 0;
    for (int g = 0; g < n_groups; ++g) n_wg += (group_rows[g + 1] - group_rows[g] + rpw - 1) / rpw;

    /* one table buffer: kx ky kz edges (double) | offsets (int64) | rows wg_rows group_wg (int) | with a window:
     * its row factors wx[i] wy[j] and wz (float) */
    const size_t n_dbl = (size_t)nx + ny + nh + (size_t)n_local + 1;
    const size_t n_int = (size_t)n_used + (size_t)n_wg + 1 + (size_t)n_groups + 1;
    const size_t n_flt = windowed ? (size_t)n_rows + (size_t)nz : 0;
    const size_t tab_bytes =
        sizeof(double) * n_dbl + sizeof(long long) * (size_t)n_batch + sizeof(int) * n_int + sizeof(float) * n_flt;
    host_tab = (unsigned char *)malloc(tab_bytes);
    if (!host_tab) {
        free(ktab);
        free(group_rows);
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    double *hd = (double *)host_tab;
    memcpy(hd, ktab, sizeof(double) * ((size_t)nx + ny + nh));
    if (cyl) memcpy(hd + nx + ny + nh, bins->edges_par, sizeof(double) * ((size_t)n_local + 1));
    else
        for (int q = 0; q <= n_local; ++q) hd[nx + ny + nh + q] = sq_threshold(bins->edges[q]);
    long long *ho = (long long *)(hd + n_dbl);
    memcpy(ho, batch_offsets, sizeof(long long) * (size_t)n_batch);
    int *hrows = (int *)(ho + n_batch), *hwg = hrows + n_used, *hgw = hwg + n_wg + 1;
    {
        int *fill = (int *)malloc(sizeof(int) * (size_t)n_groups);
        if (!fill) {
            free(ktab);
            free(group_rows);
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
        memcpy(fill, group_rows, sizeof(int) * (size_t)n_groups);
        for (int r = 0; r < n_rows; ++r)
            if (row_bin[r] >= 0) hrows[fill[row_bin[r]]++] = r;
        free(fill);
        int w = 0;
        for (int g = 0; g < n_groups; ++g) {
            hgw[g] = w;
            for (int r = group_rows[g]; r < group_rows[g + 1]; r += rpw) hwg[w++] = r;
        }
        hgw[n_groups] = w;
        hwg[w] = n_used;
    }
    if (windowed) {
        /* the row factor is formed in fp64 and rounded once */
        float *hw = (float *)(hgw + n_groups + 1);
        const double *wx = opts->window_x, *wy = opts->window_y, *wz = opts->window_z;
        for (int r = 0; r < n_rows; ++r) hw[r] = (float)((wx ? wx[r / ny] : 1.0) * (wy ? wy[r % ny] : 1.0));
        for (int l = 0; l < nz; ++l) hw[n_rows + l] = (float)(wz ? wz[l] : 1.0);
    }
    free(group_rows);
    free(ktab);

    /* what the inputs span, per field */
    long long max_off = 0;
    for (int b = 0; b < n_batch; ++b)
        if (batch_offsets[b] > max_off) max_off = batch_offsets[b];
    const size_t extent = (size_t)max_off + (size_t)(n_rows - 1) * (size_t)row_pitch + (size_t)nz;
    const size_t pad_floats = (size_t)n_rows * 2 * (size_t)nh * (size_t)n_batch;
    const int n_fields = field2 ? 2 : 1;
    const int NV = C21HIP_POWER_NV(cyl, want_var);
    const size_t n_dest = (size_t)n_groups * n_local, n_k = cyl ? (size_t)n_groups + n_local : (size_t)n_local;
    const size_t part_dbl = (size_t)n_batch * n_wg * n_local * NV, tot_dbl = (size_t)n_batch * n_dest * NV;
    /* power, counts (int64), kmean, variance */
    const size_t out_dbl = (size_t)n_batch * ((want_var ? 3 : 2) * n_dest + n_k);
    /* the box means the pack takes out (per field; behind them as many zeros: what goes back onto k = 0 with a
     * window), and the row sums they come from */
    const size_t mean_dbl = (size_t)(windowed ? 2 : 1) * n_fields * (size_t)n_batch;
    const size_t rowsum_dbl = (size_t)n_rows * (size_t)n_batch;

    unsigned char *d_tab = (unsigned char *)c21hip_ws(WS_PW_TAB, tab_bytes);
    float *d_pad = (float *)c21hip_ws(WS_PW_PAD, sizeof(float) * pad_floats * n_fields);
    double *d_sums = (double *)c21hip_ws(WS_PW_SUMS, sizeof(double) * (part_dbl + tot_dbl + out_dbl + mean_dbl + rowsum_dbl));
    int *d_bad = (int *)c21hip_ws(WS_PW_FLAG, sizeof(int));
    if (!d_tab || !d_pad || !d_sums || !d_bad) {
        status = C21CM_MEMORY_ALLOC_ERROR;
        goto done;
    }
    TRY(c21hip_h2d(d_tab, host_tab, tab_bytes, stream));
    TRY(c21hip_memset(d_bad, 0, sizeof(int), stream));
    const double *dd = (const double *)d_tab;
    c21hip_power_tabs t;
    t.kx = dd;
    t.ky = dd + nx;
    t.kz = dd + nx + ny;
    t.edges = dd + nx + ny + nh;
    const long long *d_off = (const long long *)(dd + n_dbl);
    t.rows = (const int *)(d_off + n_batch);
    t.wg_rows = t.rows + n_used;
    t.group_wg = t.wg_rows + n_wg + 1;
    t.n_wg = n_wg;
    t.n_groups = n_groups;
    t.n_local = n_local;
    t.ignore_zero_mode = bins->ignore_zero_mode != 0;
    t.ignore_kpar_zero = bins->ignore_kpar_zero != 0;
    t.use_mu = use_mu;
    t.use_wedge = use_wedge;
    t.mu_min_sq = use_mu ? opts->mu_min_sq : 0.0;
    t.mu_max_sq = use_mu ? opts->mu_max_sq : 1.0;
    t.wedge_slope_sq = use_wedge ? opts->wedge_slope_sq : 0.0;
    t.wedge_buffer = use_wedge ? opts->wedge_buffer : 0.0;
    const float *d_wrow = windowed ? (const float *)(t.group_wg + n_groups + 1) : NULL;
    const float *d_wz = windowed ? d_wrow + n_rows : NULL;

    double *d_mean = d_sums + part_dbl + tot_dbl + out_dbl, *d_rowsum = d_mean + mean_dbl;
    /* what the bin kernel adds to the k = 0 mode */
    const double *d_back = d_mean;
    if (windowed) {
        d_back = d_mean + (size_t)n_fields * n_batch;
        TRY(c21hip_memset((void *)d_back, 0, sizeof(double) * (size_t)n_fields * n_batch, stream));
    }
    const float *src[2] = {field, field2};
    int n_host = 0;
    for (int q = 0; q < n_fields; ++q) n_host += !c21hip_is_device_ptr(src[q]);
    float *stage = NULL;
    if (n_host) {
        stage = (float *)c21hip_ws(WS_PW_IN, sizeof(float) * extent * (size_t)n_host);
        if (!stage) {
            status = C21CM_MEMORY_ALLOC_ERROR;
            goto done;
        }
    }
    for (int q = 0, h = 0; q < n_fields; ++q) {
        const float *in = src[q];
        if (!c21hip_is_device_ptr(in)) {
            float *d = stage + (size_t)h++ * extent;
            TRY(c21hip_h2d(d, in, sizeof(float) * extent, stream));
            in = d;
        }
        float *pad = d_pad + (size_t)q * pad_floats;
        TRY(c21hip_power_pack(in, pad, nx, ny, nz, row_pitch, d_off, n_batch, d_rowsum, d_mean + (size_t)q * n_batch,
                              d_wrow, d_wz, d_bad, stream));
        TRY(c21hip_fft_r2c_batched(pad, nx, ny, nz, n_batch, stream));
    }
    double *d_part = d_sums, *d_tot = d_part + part_dbl, *d_power = d_tot + tot_dbl;
    long long *d_counts = (long long *)(d_power + (size_t)n_batch * n_dest);
    double *d_kmean = (double *)(d_counts + (size_t)n_batch * n_dest);
    double *d_var = want_var ? d_kmean + (size_t)n_batch * n_k : NULL;
    TRY(c21hip_power_bin(d_pad, field2 ? d_pad + pad_floats : NULL, nx, ny, nz, n_batch, cyl, want_var, &t, d_back,
                         field2 ? d_back + n_batch : NULL, d_part, d_bad, stream));
    /* F = (V/N) DFT: P = |F|^2 / V = (V/N)^2 |DFT|^2 / V; with a window over its mean square */
    const double vol = Lx * Ly * Lz, c = vol / ((double)nx * (double)ny * (double)nz);
    const double scale = windowed ? c * c / vol * opts->inv_mean_w2 : c * c / vol;
    TRY(c21hip_power_finish(d_part, d_tot, n_batch, cyl, want_var, &t, scale, d_power, d_kmean, d_var, d_counts,
                            stream));
    int bad = 0;
    TRY(c21hip_d2h(&bad, d_bad, sizeof(int), stream));
    TRY(c21hip_sync(stream));
    if (bad) {
        c21hip_set_error("power spectrum: a field value (or its transform) is not finite");
        status = C21CM_INFINITY_OR_NAN_ERROR;
        goto done;
    }
    void *dst[4] = {power, counts, kmean, variance};
    const void *from[4] = {d_power, d_counts, d_kmean, d_var};
    const size_t nb[4] = {sizeof(double) * n_batch * n_dest, sizeof(long long) * n_batch * n_dest,
                          sizeof(double) * n_batch * n_k, sizeof(double) * n_batch * n_dest};
    for (int q = 0; q < (want_var ? 4 : 3); ++q) {
        if (c21hip_is_device_ptr(dst[q])) TRY(c21hip_d2d(dst[q], from[q], nb[q], stream));
        else TRY(c21hip_d2h(dst[q], from[q], nb[q], stream));
    }
    TRY(c21hip_sync(stream));
done:
    free(host_tab);
    free(row_bin);
    return status;
}
