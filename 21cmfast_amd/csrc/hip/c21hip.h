/*
 * c21hip.h -- the thin C layer between the C host drivers (csrc/host/ *.c) and the
 * hand-written CDNA4 kernels (csrc/hip/ *.hip).  Plain pointers and sizes only.
 * Every function enqueues work on `stream` (a hipStream_t carried as void*) and
 * returns 0 or a c21cm_status code; nothing here synchronises unless it says so.
 *
 * Grid layouts (reference: src/py21cmfast/src/indexing.h:84-100):
 *   dense  float[nx][ny][nz]
 *   padded float[nx][ny][2*(nz/2+1)]  == complex float2[nx][ny][nz/2+1]
 */
#ifndef C21HIP_H
#define C21HIP_H

#include <stddef.h>

#include "ws_slots.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime.hip : memory, residency, workspace, timing ---- */
int c21hip_device_count(void);
int c21hip_current_device(void);     /* -1 when there is none */
int c21hip_use_device(int device);   /* per-thread: for helper threads of the host drivers */
int c21hip_is_device_ptr(const void *p);     /* 1 = MI355X HBM, 0 = host          */
void *c21hip_ws(int slot, size_t bytes);     /* cached device scratch, NULL = OOM */
/* host/stage.c: the device copy of an input array.  A device pointer comes back as it is; a host array is
 * uploaded into `slot` on `stream`.  NULL in, or *status already set: NULL, and *status stays as it was.
 * (Internal to the library: not exported.) */
__attribute__((visibility("hidden"))) const void *c21_stage_in(int slot, const void *p, size_t bytes, void *stream, int *status);
/* placement shopping (ionize_driver.c: place_work_partner): what a slot holds, a buffer handed to a slot, plain
 * allocations outside the workspace, free device memory; the timed two-grid pass Y that tells whether two work
 * spectra sit well together (fft_native.hip) */
void *c21hip_ws_peek(int slot, size_t *bytes);
int c21hip_ws_adopt(int slot, void *ptr, size_t bytes);
void *c21hip_raw_alloc(size_t bytes);
/* physical memory with only its head mapped (placement walk); the workspace adopts a fully mapped one */
void *c21hip_vmm_chunk(size_t phys_bytes, size_t map_bytes, void **va_out);
void c21hip_vmm_chunk_free(void *chunk);
int c21hip_ws_adopt_vmm(int slot, void *chunk, size_t bytes);
void c21hip_raw_free(void *p);
size_t c21hip_free_bytes(void);
size_t c21hip_total_bytes(void);
/* processes holding memory on the current device, this one included (KFD sysfs); -1: unknown */
int c21hip_device_tenants(void);
int c21hip_probe_pass_y2(float *work_a, float *work_b, int nx, int ny, int nz, int reps, float *ms, void *stream);
/* host/placement.c: the workspace slot `slot_new` (bytes) filled with a buffer that sits well with the one in
 * `slot_partner` for two-grid launches; plain c21hip_ws where the walk does not apply */
float *c21_place_work_partner(int slot_partner, int slot_new, size_t bytes, int nx, int ny, int nz, void *stream);
void c21hip_ws_release(void);
unsigned long c21hip_ws_generation(void); /* counts c21hip_ws_release calls */
int c21hip_h2d(void *dst, const void *src, size_t bytes, void *stream);
int c21hip_d2h(void *dst, const void *src, size_t bytes, void *stream);
int c21hip_d2d(void *dst, const void *src, size_t bytes, void *stream);
int c21hip_memset(void *dst, int byte, size_t bytes, void *stream);
int c21hip_sync(void *stream);
int c21hip_device_sync(void);
void *c21hip_event_create(void);
void c21hip_event_destroy(void *ev);
int c21hip_event_record(void *ev, void *stream);
int c21hip_stream_wait_event(void *stream, void *ev);
int c21hip_event_synchronize(void *ev); /* host waits for the event */
void *c21hip_pinned_host(size_t bytes);  /* library-owned pinned staging buffer (one, reused) */
void *c21hip_pinned_alloc(size_t bytes); /* caller-owned pinned blocks (c21hip_pinned_free) */
void c21hip_pinned_free(void *p);
void *c21hip_stream_create(void);        /* caller-owned non-blocking stream */
void c21hip_stream_destroy(void *s);
void *c21hip_aux_stream(void); /* library-owned non-blocking side stream, NULL on failure */
float c21hip_event_elapsed_ms(void *start, void *stop); /* synchronises on stop */
void c21hip_set_error(const char *fmt, ...);
const char *c21hip_get_error(void);

/* ---- fft.hip : in-place padded real 3-D transforms (reference: dft.c:18-72) ---- */
int c21hip_fft_r2c(float *padded, int nx, int ny, int nz, void *stream);
int c21hip_fft_c2r(float *padded, int nx, int ny, int nz, void *stream);
/* n_batch padded boxes back to back (rocFFT, one batched plan) */
int c21hip_fft_r2c_batched(float *padded, int nx, int ny, int nz, int n_batch, void *stream);
/* the inverse of n_batch padded boxes back to back, unnormalised as c21hip_fft_c2r (rocFFT, one batched plan),
 * and its double-precision twin on double[n_batch][nx][ny][2(nz/2+1)] */
int c21hip_fft_c2r_batched(float *padded, int nx, int ny, int nz, int n_batch, void *stream);
int c21hip_fft_c2r_batched_f64(double *padded, int nx, int ny, int nz, int n_batch, void *stream);
void c21hip_fft_release(void);
/* 1 when the hand-written power-of-two transform is used, 0 for rocFFT */
int c21hip_fft_is_native(int nx, int ny, int nz);
int c21hip_pair_sweep_supported(int nx); /* two line tiles of nx points fit in LDS */
/* Pass Y's epilogue over the Nyquist plane: 1 unless the process runs with C21CM_YNYQ_SPLIT=0 (one (tile, grid)
 * per workgroup, moved in 16-byte vectors along y, against two grids per workgroup and 8-byte accesses).  Read
 * once per process; results do not depend on it. */
int c21hip_ynyq_split_enabled(void);

/* ---- fft_native.hip : power-of-two transform on the split k-space layout ----
 * split layout: complex main[nx][ny][nz/2] followed by the Nyquist plane nyq[nx][ny]. */
size_t c21hip_split_floats(int nx, int ny, int nz);
int c21hip_padded_to_split(const float *padded_c, float *split, int nx, int ny, int nz,
                           void *stream);
/* [W(kR) x] inverse transform: split_src -> (split_work) -> real rows of out_zstride floats.
 * Fuses memcpy + filter_box + dft_c2r_cube (IonisationBox.c:577-663). */
int c21hip_split_filter_c2r(const float *split_src, float *split_work, float *real_out,
                            long out_zstride, int nx, int ny, int nz, double box_len,
                            double box_len_z, int filter_type, float R, float R_param, int apply,
                            void *stream);

/* forward transform of real rows into the split layout, scale-and-clip fused into the load
 * (lo > hi disables the clip), result times out_scale: IonisationBox.c:323-360 in 3 sweeps */
int c21hip_split_r2c(const float *real_in, long in_zstride, float *split_out, int nx, int ny,
                     int nz, double factor, double lo, double hi, float out_scale, void *stream);
int c21hip_split_filter_xy(const float *split_src, float *split_work, int nx, int ny, int nz,
                           double box_len, double box_len_z, int filter_type, float R,
                           float R_param, int apply, void *stream);
/* two grids (density, emissivity) of one radius in one sweep, each with its own window;
 * tables_ready: the W(kR) tables were prebuilt into buffer table_slot (0/1) */
int c21hip_split_filter_xy2(const float *src_a, float *work_a, int filter_a, float R_param_a,
                            const float *src_b, float *work_b, int filter_b, float R_param_b,
                            int nx, int ny, int nz, double box_len, double box_len_z, float R,
                            int apply, int table_slot, int tables_ready, void *stream);
/* one or two grids of one shell (windows 4 = spherical shell / 5 = multiple scattering between
 * R_inner and R_outer; SpinTemperatureBox.c:698-700) */
int c21hip_split_filter_shell(const float *src_a, float *work_a, int filter_a, const float *src_b,
                              float *work_b, int filter_b, int n_grids, int nx, int ny, int nz,
                              double box_len, double box_len_z, float R_inner, float R_outer,
                              float R_star, int apply, void *stream);
/* the same for two radii out of one pass-X sweep (nx < 1024); table slots 0..3;
 * phases: 1 build the tables, 2 pass X, 4 / 8 pass Y of the first / second radius */
int c21hip_split_filter_xy2_pair(const float *src_a, float *work_a, float *work_a2, int filter_a,
                                 float R_param_a, const float *src_b, float *work_b,
                                 float *work_b2, int filter_b, float R_param_b, int nx, int ny,
                                 int nz, double box_len, double box_len_z, float R, float R2,
                                 int table_slot, int table_slot2, int phases, void *stream);
/* one grid, two radii, windows evaluated in the kernel (the Eulerian loops' filtered density; phases 2 / 4 / 8 as
 * above, calls without 2 run the pass Y alone); C21CM_VALUE_ERROR when the evaluated set does not cover it */
int c21hip_split_filter_x_pair1(const float *src, float *work, float *work2, int filter_type, int nx, int ny,
                                int nz, double box_len, double box_len_z, float R, float R2, int phases,
                                void *stream);
/* ... two grids (delta and x_e of a spin-temperature run's Eulerian loop), same rules */
int c21hip_split_filter_xy2_pair_eval(const float *src_a, float *work_a, float *work_a2, int filter_a,
                                      const float *src_b, float *work_b, float *work_b2, int filter_b, int nx,
                                      int ny, int nz, double box_len, double box_len_z, float R, float R2,
                                      int phases, void *stream);
/* one grid, two radii, window a of the tables built for the two-grid sweep of those radii */
int c21hip_split_filter_xy_shared_pair(const float *src, float *work, float *work2,
                                       int filter_type, int nx, int ny, int nz, double box_len,
                                       double box_len_z, float R, float R2, int table_slot,
                                       int table_slot2, int phases, void *stream);
/* Node tables of W(x) for the radii of one excursion-set call: when *enabled comes back 1 the
 * passes X of these radii (c21hip_split_filter_xy2[_pair], _xy_shared[_pair]) evaluate their
 * windows in the kernel and c21hip_window_tables need not be called; c21hip_wev_release ends it */
int c21hip_wev_prepare(int filter_a, float R_param_a, int filter_b, float R_param_b, int n_grids,
                       const float *R, int n_R, int nx, int ny, int nz, double box_len,
                       double box_len_z, int pair, int *enabled, void *stream);
void c21hip_wev_release(void);
/* -1: no set is active; 1: the node tables cover every kR of the set; 0: direct evaluation beyond them */
int c21hip_wev_covers(void);
int c21hip_wev_applicable(int filter_a, int filter_b, int n_grids, int nx, int ny, int nz);
/* one grid, two radii per pass-X sweep, under window a or b of the prepared set (phases: 2 pass X,
 * 4 / 8 pass Y of the first / second radius) */
int c21hip_split_filter_xy_single_pair(const float *src, float *work, float *work2, int filter_type,
                                       float R_param, int nx, int ny, int nz, double box_len,
                                       double box_len_z, float R, float R2, int phases, void *stream);
/* Fused pass Z of delta_R and the filtered emissivity + sum(stars) + ionisation barrier for Lagrangian source
 * grids at radius index > 0 (IonisationBox.c:634-638,821-837,1054-1151): one entry, one descriptor.  NULL: absent. */
typedef struct c21hip_z_ionise_desc {
    size_t size;                  /* sizeof(c21hip_z_ionise_desc); any other value is refused (C21CM_VALUE_ERROR) */
    const float *delta_work;      /* density and emissivity spectra after passes X, Y */
    const float *stars_work;
    const float *xe_work;         /* filtered x_e spectrum of a spin-temperature run: barrier f zeta > 1 - x_e
                                   * (IonisationBox.c:1118); 256- / 512- / 1024-point z-lines */
    const float *nrec_work;       /* recomb, CELL_RECOMB = false: the previous snapshot's N_rec filtered at this
                                   * radius (with xe_work too: four spectra, 512-point z-lines) */
    const float *nrec;            /* recomb without nrec_work: the cell's own previous N_rec, dense ... */
    double rec0;                  /* ... or, nrec == NULL, the homogeneous model's one number */
    int recomb;                   /* recombination model: barrier (1 + N_rec / (1 + delta)); a first crossing
                                   * leaves delta_R in g12 for c21hip_split_z_sfr_gamma12; sum_out is not used */
    int cross_by_memory_line;     /* cross_plane is indexed by memory line of the (x-blocked) spectrum, to be resolved
                                   * by c21hip_resolve_crossings_lines; 0: by logical line x * ny + y
                                   * (c21hip_resolve_crossings).  Sits in what was padding: the size is unchanged */
    float *g12;                   /* recomb: dense Gamma_12 grid */
    unsigned char *first_cross;   /* uint8 [N] mask of first crossings, updated; or, instead of it, ... */
    unsigned *cross_plane;        /* ... this radius' plane of crossing bits (c21hip_z_cross_bits_supported) */
    double *partials;             /* c21hip_z_ionise_partials doubles: sum(stars) per workgroup */
    double *sum_out;              /* the sum on the device; NULL defers the reduction: the partials of every radius
                                   * stay at partials + R * stride and c21hip_batched_means reduces them at once */
    int nx, ny, nz, r_index;
    double rhocrit_omb, ion_eff;
    int mass_dep_zeta;
    double f_limit;
} c21hip_z_ionise_desc;
int c21hip_split_z_ionise(const c21hip_z_ionise_desc *desc, void *stream);
/* which boxes the entry serves with ... an x_e grid */
int c21hip_z_ionise_xe_supported(int nx, int ny, int nz);
/* ... a recombination model; with a third spectrum too (x_e or the filtered N_rec); with both */
int c21hip_z_ionise_recomb_supported(int nx, int ny, int nz);
int c21hip_z_ionise_recomb_xe_supported(int nx, int ny, int nz);
int c21hip_z_ionise_recomb_xe_nrec_supported(int nx, int ny, int nz);
int c21hip_z_ionise_partials(int nx, int ny, int nz);
/* a recombination radius is followed by the pass Z of the filtered whalo_sfr: first crossings of r_index
 * (g12 holds their delta_R) receive Gamma_12 = g12_scale / (1 + delta_R) max(sfr_R, 0) */
int c21hip_split_z_sfr_gamma12(const float *sfr_work, const unsigned char *first_cross, float *g12,
                               int nx, int ny, int nz, int r_index, double g12_scale, void *stream);
/* Eulerian source models with an x_e grid: pass Z of the filtered x_e spectrum with the barrier
 * f_coll zeta > 1 - x_e(R) fused in (nion_dense: the radius' dense f_coll, *mean_dev its mean);
 * first crossings go into the mask, x_e(R) is never stored (IonisationBox.c:1091-1118) */
int c21hip_z_xe_mask_supported(int nx, int ny, int nz);
int c21hip_split_z_xe_mask(const float *xe_work, const float *nion_dense, const double *mean_dev,
                           unsigned char *first_cross, int nx, int ny, int nz, int r_index,
                           double mean_f_coll, int fix_mean, int mass_dep_zeta, double f_limit,
                           double ion_eff, void *stream);
/* first-crossing mask + Gamma_12 grid of the fused recombination loop -> x_HI = 0, z_reion,
 * mean free path = R[index] (R_dev: float per radius index) */
int c21hip_apply_first_cross_recomb(const unsigned char *first_cross, const float *R_dev,
                                    const float *prev_z_reion, int first_snapshot, double redshift,
                                    float *xH, float *z_reion, float *mfp, size_t ntot, void *stream);
/* W(kR) tables of one radius for c21hip_split_filter_xy2, on any stream */
int c21hip_window_tables(int table_slot, int filter_a, float R_param_a, int filter_b,
                         float R_param_b, int nx, int ny, int nz, double box_len,
                         double box_len_z, float R, void *stream);
/* pass Z of the filtered density + its extrema on the device (minmax_out[2]);
 * partials: 2 * nx*ny/16 doubles (IonisationBox.c:668-699) */
int c21hip_split_z_c2r_minmax(const float *split_work, float *real_out, long out_zstride, int nx,
                              int ny, int nz, double *partials, double *minmax_out, void *stream);
/* Eulerian table loop without the delta_R round trip (round 6): the extrema alone (nothing stored), then the
 * table sweep + banded barrier as the epilogue of a SECOND pass Z of the same spectrum (nx*ny/16 partial sums of
 * f_coll left in `partials` for c21hip_eul_band) */
int c21hip_z_table_band_supported(int nx, int ny, int nz);
int c21hip_split_z_minmax_only(const float *split_work, int nx, int ny, int nz, double *partials,
                               double *minmax_out, void *stream);
int c21hip_split_z_fcoll_table_band(const float *split_work, float *f_pend, const double *band_dev,
                                    const double *thr_prev_dev, unsigned char *first_cross, int r_index,
                                    int r_prev, int nx, int ny, int nz, int mode, double tab_min, double tab_width,
                                    const float *table_dev, double *partials, void *stream);
/* pass Z fused with the CONST-ION-EFF closed-form f_coll(delta_R): dense f_coll grid + sum
 * (IonisationBox.c:785-961, hmf.c:1205-1241); partials: 2 * nx*ny/16 doubles */
int c21hip_split_z_fcoll_erfc(const float *split_work, float *nion_dense, int nx, int ny, int nz,
                              double growthf, double sigma_min, double sigma_max, double delta_c,
                              double *partials, double *sum_out, void *stream);
/* pass Z with out = max(v, min_value) * const_factor into dense rows and stats_out[3] =
 * {min, max, sum} of the stored values on the device (SpinTemperatureBox.c:606-629);
 * partials: 3 * nx*ny/16 + 2 * (nx*ny/16384 + 2) doubles */
int c21hip_split_z_c2r_stats(const float *split_work, float *real_out, long out_zstride, int nx,
                             int ny, int nz, double min_value, double const_factor,
                             double *partials, double *stats_out, void *stream);
/* stats_out == NULL above defers the reduction: window i keeps its partials (nb = nx*ny/16 minima,
 * maxima, sums) at partials + i * stride and one launch reduces `count` windows */
int c21hip_batched_stats(const double *partials, long stride, int nb, int count,
                         double *stats_out, void *stream);
/* the same store + statistics from real rows of in_zstride floats (generic sizes; out may be
 * NULL for the statistics alone); partials: 3 * C21HIP_PARTIALS doubles */
int c21hip_floor_scale_stats(const float *in, long in_zstride, float *out, int nx, int ny, int nz,
                             double min_value, double const_factor, double *partials,
                             double *stats_out, void *stream);
/* pass Z storing v / divisor (0: no division) */
int c21hip_split_z_c2r_div(const float *split_work, float *real_out, long out_zstride, int nx,
                           int ny, int nz, float divisor, void *stream);
/* pass Z storing v * scale / divisor (0: no division), floored at -1 + 1e-7 when floor_density */
int c21hip_split_z_c2r_out(const float *split_work, float *real_out, long out_zstride, int nx,
                           int ny, int nz, float scale, float divisor, int floor_density,
                           void *stream);
int c21hip_split_xblock_log2(int nx); /* 0: plain split layout */
/* split-layout InitialConditions pipeline (ics_kernels.hip, plain layout only) */
int c21hip_split_kop(const float *in_split, float *out_split, int nx, int ny, int nz,
                     double box_len, double box_len_z, int axis0, int axis1, void *stream);
/* passes X, Y of the inverse transform of op(P), P = spectrum / k^2 (c21hip_split_kop with
 * axis0 = -2): the gradient / second-derivative operator is applied inside pass X */
int c21hip_split_sepop_xy(const float *split_src, float *split_work, int nx, int ny, int nz,
                          double box_len, double box_len_z, int axis0, int axis1, void *stream);
int c21hip_split_fold(const float *hi_split, float *lo_split, int nx, int ny, int nz, int f,
                      double box_len, double box_len_z, int axis0, int axis1, void *stream);
/* ... up to four folded spectra of one hi spectrum in one read: ops[k] = -1 identity, 0 / 1 / 2 gradient axis;
 * tophat_R > 0: the top-hat of that radius applied to the stored elements on the way (the filtered spectrum is
 * never written) */
int c21hip_split_fold_multi(const float *hi_split, float *const lo_split[4], const int ops[4], int n_out, int nx,
                            int ny, int nz, int f, double box_len, double box_len_z, float tophat_R, void *stream);
int c21hip_lpt2_source(const float *const diag[3], const float *const off[3], float *out, size_t n,
                       float norm, void *stream);
int c21hip_copy_filter_split(const float *src_split, float *dst_split, int nx, int ny, int nz,
                             double box_len, double box_len_z, int filter_type, float R,
                             float R_param, int apply, void *stream);
int c21hip_split_z_c2r(const float *split_work, float *real_out, long out_zstride, int nx, int ny,
                       int nz, void *stream);
/* the deferred sums of the fused pass Z (c21hip_z_ionise_desc.sum_out == NULL): ONE launch turns the partials at
 * partials + R * stride into sums[R] / means[R] for R = first, first - step, ... (count radii) */
int c21hip_batched_means(const double *partials, long stride, int n_partials, int first, int step,
                         int count, double ntot, int mass_dep_zeta, double f_limit, double *sums,
                         double *means, void *stream);
/* Crossing bits: the two-grid fused pass Z on 512-point z-lines writes this radius' barrier outcome as
 * one bit per cell into its own plane (nx*ny*nz/8 bytes, write only) instead of updating the uint8
 * mask; c21hip_resolve_crossings turns the planes of the radii r_hi ... r_lo (the plane of radius r at
 * bits + (r - 1) * nlines * 16 words) into first_cross[nlines][512], every byte written.  The bit order
 * is private to the two kernels.  C21CM_CROSS_BITS=0: _supported returns 0 (the mask path). */
int c21hip_z_cross_bits_supported(int nx, int ny, int nz);
int c21hip_resolve_crossings(const unsigned *bits, int r_hi, int r_lo, unsigned char *first_cross,
                             size_t nlines, void *stream);
/* the same for planes indexed by memory line (c21hip_z_ionise_desc.cross_by_memory_line) of a spectrum with ny
 * lines per x and block shift lb (c21hip_split_xblock_log2(nx)): memory line m goes to mask row
 * c21_logical_line(m, ny, lb); the mask stays in logical order.  nlines must be a multiple of ny << lb. */
int c21hip_resolve_crossings_lines(const unsigned *bits, int r_hi, int r_lo, unsigned char *first_cross,
                                   size_t nlines, int ny, int lb, void *stream);
/* passes X, Y of one grid with window a of the two-grid tables in buffer table_slot */
int c21hip_split_filter_xy_shared(const float *src, float *work, int filter_type, int nx, int ny,
                                  int nz, double box_len, double box_len_z, float R, int apply,
                                  int table_slot, void *stream);
/* time `reps` launches of one pass with HIP events on `stream` (bench.py roofline leg);
 * kind: 0 pass X and 1 pass Y as the excursion-set loop launches them (two grids, windows
 * filter_a / filter_b streamed from the per-radius tables), 2 fused pass Z, 3 plain pass Z,
 * 4 the window-table kernel */
int c21hip_bench_pass(int kind, int n, int filter_a, int filter_b, float R, float R_param_b,
                      double box_len, int reps, void *stream, float *ms_out);
/* deterministic single-workgroup sum of n doubles (ionize_kernels.hip) */
int c21hip_reduce_sum(const double *partials, int n, double *out, void *stream);
/* op 1 = min, 2 = max of n doubles; stage: >= n/1024 + 1 doubles of scratch for long inputs */
int c21hip_reduce_op(const double *partials, int n, int op, double *stage, double *out,
                     void *stream);

/* ---- grid_kernels.hip : generic sweeps ---- */
/* padded[l][k] = clip(dense[l][k] * factor, lo, hi); pad columns zeroed.
 * reference: IonisationBox.c:333-350 */
int c21hip_pack_clip(const float *dense, float *padded, int nx, int ny, int nz, double factor,
                     double lo, double hi, void *stream);
/* dense[l][k] = padded[l][k] * scale (scale applied in float) */
int c21hip_unpack_scale(const float *padded, float *dense, int nx, int ny, int nz, float scale,
                        void *stream);
/* buf[i] /= divisor, float arithmetic (reference: IonisationBox.c:356-359) */
int c21hip_divide_inplace(float *buf, size_t n, float divisor, void *stream);
/* buf[i] = (float)(buf[i] / divisor), double arithmetic (reference: filtering.c:422-424) */
int c21hip_divide_inplace_f64(float *buf, size_t n, double divisor, void *stream);
int c21hip_fill(float *buf, size_t n, float value, void *stream);
int c21hip_add_scalar(float *buf, size_t n, float value, void *stream); /* buf[i] += value */
/* out[i] = (double)in[i] */
int c21hip_widen(const float *in, double *out, size_t n, void *stream);

/* dst = src * W(kR), the fused memcpy + filter_box of copy_filter_transform.
 * reference: IonisationBox.c:577-631 + filtering.c:308-394.  `apply` = 0 copies only. */
int c21hip_copy_filter(const float *src_c, float *dst_c, int nx, int ny, int nz, double box_len,
                       double box_len_z, int filter_type, float R, float R_param, int apply,
                       void *stream);
/* the same with filter_box's full argument list: R_star of the multiple-scattering window 5 */
int c21hip_copy_filter_star(const float *src_c, float *dst_c, int nx, int ny, int nz,
                            double box_len, double box_len_z, int filter_type, float R,
                            float R_param, float R_star, int apply, void *stream);

/* gsl_stream_kernels.hip: the same streams drawn on the device (layouts: gsl_stream.c).
 *   draw    one launch over n_streams descriptors; every stream resumes from its saved state and stops after at
 *           most max_pairs accepted pairs, at its count, or at the tile cap (tile_cap <= 0: derived from the pairs
 *           asked for), which sets its error word and *flag_dev
 *   accept  the compaction alone on words in device memory; result_dev[0] = pairs found, [1] = words used
 *   raw     the first n raw outputs of one generator state */
typedef struct c21_gsl_stream_desc {
    unsigned long long out_offset; /* first pair of the stream in the output, grid order */
    unsigned long long count;      /* pairs the stream owes: 2 rows ny nzc */
    unsigned int kind;             /* 0 mt19937, 1 gfsr4, 2 cmrg, 3 mrg, 4 taus2 */
    unsigned int state_offset;     /* of the stream's record in the state buffer, in 32-bit words */
} c21_gsl_stream_desc;
/* a stream's record: C21_GSL_HDR header words (0-1 accepted pairs, 2 carry present, 3 carry word, 4 error), then
 * the generator state as c21_gsl_export_state writes it */
#define C21_GSL_HDR 8
/* cmrg, mrg, taus2: every thread owns C21_GSL_RUN consecutive outputs of a tile; jump matrix j of C21_GSL_JUMPS
 * is A^(C21_GSL_RUN 2^j).  Tables back to back: cmrg (two 3x3), mrg (5x5), taus2 (three times 32 columns). */
#define C21_GSL_RUN 8
#define C21_GSL_JUMPS 9
#define C21_GSL_JUMP_CMRG 0
#define C21_GSL_JUMP_MRG (C21_GSL_JUMPS * 18)
#define C21_GSL_JUMP_TAUS2 (C21_GSL_JUMP_MRG + C21_GSL_JUMPS * 25)
#define C21_GSL_JUMP_WORDS (C21_GSL_JUMP_TAUS2 + C21_GSL_JUMPS * 96)
int c21hip_gsl_tile_words(int kind); /* words per tile of generator `kind`; -1: words in memory */
int c21hip_gsl_stream_draw(const void *desc_dev, int n_streams, unsigned int *state_dev, const unsigned int *jump_dev,
                           unsigned long long *pairs_dev, unsigned long long max_pairs, long tile_cap, int *flag_dev,
                           void *stream);
int c21hip_gsl_accept_pairs(int kind, const unsigned int *words_dev, size_t n_words, size_t want,
                            unsigned long long *pairs_dev, unsigned long long *result_dev, void *stream);
int c21hip_gsl_raw_words(int kind, const unsigned int *state_dev, const unsigned int *jump_dev, size_t n,
                         unsigned int *out_dev, void *stream);
/* ics_kernels.hip: the raw word pairs of the reference's IC random stream (gsl_stream.c: two accepted
 * 32-bit outputs per deviate, generator kind per x-row) -> gsl_ran_ugaussian deviates, in place */
int c21hip_gsl_words_to_deviates(void *buf, size_t n_deviates, const unsigned char *row_kind_dev,
                                 size_t deviates_per_row, void *stream);

/* ---- perturb_kernels.hip ---- */
/* move_grid_masses: map_mass.c:146-208.  `out` (double[out_dim]) must be zeroed by the caller.
 * fixed_out != NULL: the deposit may leave 64-bit FIXED-POINT integers (scale 2^44) in `out` instead of
 * doubles -- deterministic whatever the order of the atomics -- and says so in *fixed_out;
 * c21hip_widen_normalise(fixed = 1) reads them.  NULL: doubles. */
int c21hip_cic_scatter(const float *hires_density, const int dens_dim[3], const float *const vel[3],
                       const float *const vel2[3], const int vel_dim[3], double *out,
                       const int out_dim[3], double box_len, double box_len_z, double growth,
                       double init_growth, int lpt2, int *fixed_out, void *stream);
/* after a fixed-point deposit: *bad = 1 when a particle mass or position was non-finite or beyond what the
 * 63 bits (or an int index) hold (synchronises the stream) */
int c21hip_cic_fixed_status(int *bad, void *stream);
/* which deposit kernel the last c21hip_cic_scatter launched: 1 per velocity cell, 2 tiled, 3 direct
 * (0: none yet).  Read-only, for tests that must know which kernel they compared. */
int c21hip_cic_last_path(void);
/* double grid -> padded float [, *= mass_factor, -= 1]: PerturbedField.c:115-128,180-210 */
/* ComputeHaloBox deposit (map_mass.c:214-344): exp(lerp(ln-table, delta*D)) * prefactor for the
 * two tables in tables_dev[2][NDELTA], CIC-deposited at the displaced positions (double grids) */
int c21hip_halobox_scatter(const float *src_density, const int dens_dim[3],
                           const float *const vel[3], const float *const vel2[3],
                           const int vel_dim[3], double *out_nion, double *out_sfr,
                           double *out_xray /* NULL: two values */, const int out_dim[3],
                           double box_len, double box_len_z, double growth, double init_growth,
                           int lpt2, const float *tables_dev /* [2 or 3][NDELTA] */,
                           double tab_min, double tab_width, double pref_nion, double pref_sfr,
                           double pref_xray, void *stream);
/* ComputeHaloBox with USE_MINI_HALOS.  get_log10_turnovers (HaloBox.c:465-516): n_chunks = the
 * N_THREADS shares over which upstream's running maximum of the atomic turnover restarts;
 * sums_dev[2] (zeroed by the caller) receive the sums of the two log10 grids. */
int c21hip_halobox_turnovers(size_t ntot, int n_chunks, int below_z_heat_max, double redshift,
                             double mturn_a_nofb, double m_turn, double vcb_const, double A_LW,
                             double BETA_LW, double A_VCB, double BETA_VCB, double sigma_vcb,
                             const float *prev_G12, const float *prev_z_reion, const float *J_21_LW,
                             const float *vcb, float *out_a, float *out_m, double *sums_dev,
                             void *stream);
/* move_grid_galprops with mini-halos (map_mass.c:285-321): low-resolution sources; ranges =
 * {delta min, width, log10 M_turn,a min, width, log10 M_turn,m min, width, fixed turnover grid
 * min, width}; prefactors = {nion, nion_mini, sfr, sfr_mini, xray}; out_xray / tab_xray may be
 * NULL; double accumulation grids */
int c21hip_halobox_scatter_mini(const float *src_density, const int dim[3],
                                const float *const vel[3], const float *const vel2[3],
                                const float *mturn_a, const float *mturn_m, double *out_nion,
                                double *out_sfr, double *out_sfr_mini, double *out_xray,
                                double box_len, double box_len_z, double growth, double init_growth,
                                int lpt2, const float *tab_sfrd, const float *tab_nion_a,
                                const float *tab_nion_m, const float *tab_sfrd_m,
                                const float *tab_xray, const double *ranges,
                                const double *prefactors, void *stream);
/* move_halo_galprops (map_mass.c:346-476) for a catalogue in device arrays: fp64 accumulation
 * grids, values per unit output-cell volume; out_sfr_mini / out_xray / out_wsfr and (without
 * mini-halos) the turnover grids may be NULL.  scratch: c21hip_halo_deposit_scratch_ints() ints
 * for the binned, LDS-tiled path (NULL or C21CM_HALO_DEPOSIT=direct: global atomics only). */
struct c21cm_halo_consts;
size_t c21hip_halo_deposit_scratch_ints(unsigned long long n_halos, const int out_dim[3]);
/* test_halo_props (HaloBox.c:658-779): twelve floats per halo; lw = {A_LW, BETA_LW, A_VCB,
 * BETA_VCB, sigma_vcb, vcb_const, M_TURN}; the grids are read with mini-halos only */
int c21hip_halo_props(const struct c21cm_halo_consts *consts, unsigned long long n_halos,
                      const float *masses, const float *coords, const float *star_rng,
                      const float *sfr_rng, const float *xray_rng, const int dim[3],
                      double cell_length, double redshift, int below_z_heat_max, int vcb_flucts,
                      const double lw[7], const float *vcb, const float *J21, const float *z_re,
                      const float *G12, float *out, void *stream);
int c21hip_halo_deposit(const struct c21cm_halo_consts *consts, unsigned long long n_halos,
                        const float *masses, const float *coords, const float *star_rng,
                        const float *sfr_rng, const float *xray_rng, const float *const vel[3],
                        const float *const vel2[3], const int vel_dim[3], const int out_dim[3],
                        double box_len, double box_len_z, double growth, double init_growth, int lpt2,
                        const float *mturn_a, const float *mturn_m, double *out_nion, double *out_sfr,
                        double *out_sfr_mini, double *out_xray, double *out_wsfr, int *scratch,
                        void *stream);
/* ComputePerturbedHaloCatalog + convert_halo_props (PerturbedHaloCatalog.c:25-149, HaloBox.c:781-880)
 * for a catalogue in device arrays: one thread per halo, rows in input order.  vdf / vdf2: D - D_i and
 * its 2LPT analogue; lo_dim: the turnover grids' dimensions; box_to_lores = HII_DIM / DIM.
 * out = {coords [3 n], masses, M*, SFR, n_ion, L_X, f_esc-weighted SFR, M*_mini, SFR_mini}: the first
 * five are required, the rest are written where given (L_X with use_xray, the mini pair with
 * use_mini_halos only); halos of zero mass get coordinates and keep their property rows */
int c21hip_halo_catalog(const struct c21cm_halo_consts *consts, unsigned long long n_halos,
                        const float *masses, const float *coords, const float *star_rng,
                        const float *sfr_rng, const float *xray_rng, const float *const vel[3],
                        const float *const vel2[3], const int vel_dim[3], const int lo_dim[3],
                        double box_len, double box_len_z, double vdf, double vdf2, int lpt2,
                        double box_to_lores, const float *mturn_a, const float *mturn_m,
                        float *const out[9], void *stream);
int c21hip_narrow(const double *in, float *out, float *out_scaled, double scale, size_t n,
                  void *stream);
/* {min, max} of n floats into out2 (device); partials: 2 * 2048 doubles */
int c21hip_minmax_dense(const float *a, size_t n, double *partials, double *out2, void *stream);
int c21hip_widen_normalise(const double *in, float *padded, int nx, int ny, int nz, int normalise,
                           double mass_factor, int fixed, void *stream);
/* padded = (float)(factor * dense): PerturbedField.c:64-80 */
int c21hip_scale_pack(const float *dense, float *padded, int nx, int ny, int nz, double factor,
                      void *stream);
/* nearest-index gather from a padded real grid [, /divisor][, clip at -1+1e-7] into a dense
 * (or padded) low-res grid: PerturbedField.c:162-177,251-276,367-383,450-464 */
int c21hip_gather(const float *src_padded, const int src_dim[3], float *dst, const int lo_dim[3],
                  int dst_padded, float divisor, int clip, void *stream);
/* grid = saved * (dD/dt / D) i k_axis / k^2 / N: PerturbedField.c:320-350 */
int c21hip_velocity_kspace(const float *saved_c, float *grid_c, int nx, int ny, int nz,
                           double box_len, double box_len_z, int axis, double dDdt_over_D,
                           void *stream);

/* ---- ics_kernels.hip ---- */
/* delta_k = sqrt(V P/2)(a + ib) with Hermitian planes: InitialConditions.c:26-139 */
/* compute_relative_velocities (InitialConditions.c:141-238): k-space operator of one component,
 * and the subsampled sum of squares (sqrt / VOLUME on the last component) into lowres_vcb */
int c21hip_vcb_op(const float *in_c, float *out_c, int nx, int ny, int nz, double box_len,
                  double box_len_z, int axis, const double *h_by_m_dev, void *stream);
int c21hip_vcb_accumulate(const float *src_padded, const int hi_dim[3], float *dst,
                          const int lo_dim[3], int first, int last, float volume, void *stream);
int c21hip_sample_modes(float *cbox, int nx, int ny, int nz, const double *pk_by_m_dev,
                        float volume, unsigned long long seed, const double *deviates_dev,
                        void *stream);
/* ... straight into the split layout of the native transforms */
int c21hip_sample_modes_split(float *split, int nx, int ny, int nz, const double *pk_by_m_dev, float volume,
                              unsigned long long seed, const double *deviates_dev, void *stream);
/* axis1 < 0: out = in*i*k_axis0/k^2 (:240-267); else out = -k_axis0*k_axis1*in/k^2 (:269-297) */
int c21hip_kspace_op(const float *in_c, float *out_c, int nx, int ny, int nz, double box_len,
                     double box_len_z, int axis0, int axis1, void *stream);
/* padded = dense * VOLUME / N (:637-653) */
int c21hip_pack_density(const float *dense, float *padded, int nx, int ny, int nz, float volume,
                        void *stream);
/* box += phi_ii*phi_jj; box -= phi_ij^2 (:451-482) */
int c21hip_lpt2_accumulate(float *box, const float *phi_ij_padded, const float *diag_i,
                           const float *diag_j, int nx, int ny, int nz, void *stream);

/* ---- ionize_kernels.hip ---- */
typedef struct c21hip_ionize_args {
    int nx, ny, nz;
    int r_index;        /* 0 = last (cell-scale) radius: partial ionisation branch */
    int lagrangian;     /* stars grid divides by rhocrit_omb*(1+delta)             */
    int mass_dep_zeta;  /* floor f at f_limit                                      */
    int use_ts_fluct;
    int minimize_memory;
    int first_snapshot; /* previous z_reion treated as -1                          */
    int fix_mean;
    double mean_f_coll; /* fix_mean numerator                                      */
    double f_limit;
    double ion_eff_factor;
    double rhocrit_omb;
    double photoncons_factor;
    double redshift;
    double TK_nofluct, adia_TK_term, T_re;
} c21hip_ionize_args;

/* All reductions are two-stage and deterministic: `partials` is device scratch of
 * C21HIP_PARTIALS doubles, the result lands in a device double. */
#define C21HIP_PARTIALS 4096

/* min/max of the filtered delta (the clip of :689 is applied in registers by the
 * consumers).  reference: IonisationBox.c:668-699.  minmax_out = {min, max}. */
int c21hip_clip_minmax(float *delta_fil, int nx, int ny, int nz, double *partials,
                       double *minmax_out, void *stream);
/* Eulerian source models: f_coll(delta_R) -> unnormalised_nion (dense) and sum(f_coll).
 * mode: enum c21cm_fcoll_mode (ERFC / TABLE_LINEAR / TABLE_EXP).
 * reference: IonisationBox.c:773-962 */
int c21hip_fcoll_eulerian(const float *delta_fil, float *nion_dense, int nx, int ny, int nz,
                          int mode, double growthf, double sigma_min, double sigma_max,
                          double delta_c, double tab_min, double tab_width,
                          const float *table_dev, double *partials, double *sum_out,
                          void *stream);
/* the same on rows of `zstride` floats: 2 (nz / 2 + 1) (padded) or nz (dense: 16-byte pieces when nz % 4 == 0) */
int c21hip_fcoll_eulerian_zs(const float *delta_fil, long zstride, float *nion_dense, int nx, int ny, int nz,
                             int mode, double growthf, double sigma_min, double sigma_max, double delta_c,
                             double tab_min, double tab_width, const float *table_dev, double *partials,
                             double *sum_out, void *stream);
/* Lagrangian source grids: sum(stars) + barrier test + partial ionisation, one sweep.
 * first_cross != NULL switches to shard mode (records the radius index instead of
 * touching xH / z_reion).  reference: IonisationBox.c:821-837,1008-1201 */
int c21hip_ionise_stars(const c21hip_ionize_args *a, const float *delta_fil,
                        const float *stars_fil, const float *xe_fil, const float *density,
                        const float *prev_z_reion, const float *kinetic_temp_neutral, float *xH,
                        float *z_reion, float *kinetic_temperature, unsigned char *first_cross,
                        double *partials, double *sum_out, void *stream);
/* Eulerian barrier test; mean_dev holds the clamped grid mean (fix_mean denominator).
 * reference: IonisationBox.c:1008-1201 */
int c21hip_ionise_eulerian(const c21hip_ionize_args *a, const float *nion_dense,
                           const float *xe_fil, const float *density, const float *prev_z_reion,
                           const float *kinetic_temp_neutral, const double *mean_dev, float *xH,
                           float *z_reion, float *kinetic_temperature,
                           unsigned char *first_cross, void *stream);
/* mean = clamp(sum/N): reference IonisationBox.c:960,1566-1576 */
int c21hip_finish_mean(const double *sum_dev, double ntot, int mass_dep_zeta, double f_limit,
                       double *mean_dev, void *stream);
/* Ionised-cell temperatures + sum(xH) + NaN flag.  reference: IonisationBox.c:1203-1256,1597-1608 */
int c21hip_finalize(const c21hip_ionize_args *a, double stored_redshift, const float *density,
                    const float *kinetic_temp_neutral, const float *xH, const float *z_reion,
                    float *kinetic_temperature, size_t ntot, double *partials, double *sum_out,
                    int *flag_out, void *stream);
/* set_fully_neutral_box: IonisationBox.c:531-565 */
int c21hip_neutral_box(const float *density, const float *xe, const float *Tneutral, float *xH,
                       float *Tk, size_t ntot, int ts, double global_xH, double TK, double adia,
                       void *stream);
int c21hip_any_nonzero(const float *a, size_t n, int *flag_host, void *stream);
/* xH/z_reion from a max-reduced first_cross mask (multi-GPU tail). */
/* Eulerian barrier test on the dense f_coll grid, first crossing into a uint8 mask
 * (radius index > 0, no x_e grid; IonisationBox.c:1022-1027,1077,1118) */
/* find_ionised_regions with a recombination model (IonisationBox.c:1084-1140): rec in the barrier,
 * Gamma_12 / mean free path at the first crossing.  src_grid = filtered n_ion (padded real,
 * lagrangian) or the dense unnormalised_nion grid; nrec_fil padded (no CELL_RECOMB) or prev_nrec
 * dense (CELL_RECOMB; one value for the homogeneous model).  sum_out (Lagrangian f_coll sum) may
 * be NULL. */
int c21hip_ionise_recomb(const c21hip_ionize_args *a, int lagrangian, int inhomo, int cell_recomb,
                         double R, double gamma_prefactor, const float *delta_fil,
                         const float *src_grid, const float *sfr_fil, const float *xe_fil,
                         const float *nrec_fil, const float *prev_nrec, const float *density,
                         const float *prev_z_reion, const float *kinetic_temp_neutral,
                         const double *mean_dev, float *xH, float *z_reion,
                         float *kinetic_temperature, float *G12, float *mfp, double *partials,
                         double *sum_out, void *stream);
/* USE_MINI_HALOS (E-INTEGRAL).  calculate_mcrit_boxes (IonisationBox.c:403-457): dense [N]
 * device arrays, sums_out[2] = sum of the two log10 grids, *flag_dev set on a NaN/zero threshold.
 * partials: >= 2 * 2048 doubles. */
int c21hip_mturn_grids(size_t ntot, int first_snapshot, double redshift, double mturn_a_nofb,
                       double mturn_m_nofb, double vcb_const, double A_LW, double BETA_LW,
                       double A_VCB, double BETA_VCB, double sigma_vcb, const float *prev_G12,
                       const float *prev_z_reion, const float *J_21_LW, const float *vcb,
                       float *out_a, float *out_m, double *partials, double *sums_out,
                       int *flag_dev, void *stream);
/* calculate_fcoll_grid with both populations and the per-radius history (:838-936).  Filtered
 * grids padded, history / outputs dense; tables_dev = 4 tables of NDELTA x NMTURN floats (acg, mcg,
 * previous-redshift acg, mcg); ranges = {delta min, width, prev delta min, width, log10 M_turn,a
 * min, width, log10 M_turn,m min, width}; sums_out[2] = sum f_a, sum f_m. */
int c21hip_fcoll_mini(int nx, int ny, int nz, int need_prev, const double *ranges,
                      const float *delta_fil, const float *pdelta_fil, const float *mta_fil,
                      const float *mtm_fil, const float *tables_dev, const float *prev_nion,
                      const float *prev_mini, float *nion_out, float *mini_out, double *partials,
                      double *sums_out, void *stream);
/* find_ionised_regions with the two-population barrier (:1068-1200), recombinations optional.
 * lagrangian: nion_dense = stars_fil and mini_dense = sfr_fil (padded rows; sfr_fil only with a
 * recombination model), the second population contributes its floor f_limit_mcg only, and the sum
 * of the source grid goes to sum_out (partials: C21HIP_PARTIALS doubles). */
int c21hip_ionise_mini(const c21hip_ionize_args *a, int lagrangian, int recomb, int inhomo,
                       int cell_recomb,
                       double R, double gamma_prefactor, double gamma_prefactor_mini,
                       double ion_eff_mini, double f_limit_mcg, double mean_f_coll_mini,
                       const float *delta_fil, const float *nion_dense, const float *mini_dense,
                       const float *xe_fil, const float *nrec_fil, const float *prev_nrec,
                       const float *density, const float *prev_z_reion,
                       const float *kinetic_temp_neutral, const double *mean_a_dev,
                       const double *mean_m_dev, float *xH, float *z_reion,
                       float *kinetic_temperature, float *G12, float *mfp, double *partials,
                       double *sum_out, void *stream);
/* IONISE_ENTIRE_SPHERE (IonisationBox.c:1150-1158): every cell of the first-crossing mask flags
 * the cells closer than its radius; rsq_dev[r] = (R_r in cells)^2 as update_in_sphere forms it
 * (float), compared strictly with the integer distances (bubble_helper_progs.c:292-325) */
int c21hip_paint_spheres(const unsigned char *first_cross, const float *rsq_dev, float *xH, int nx,
                         int ny, int nz, void *stream);
/* set_recombination_rates, inhomogeneous model (IonisationBox.c:1277-1339); rate_scale =
 * fabs_dtdz * dz; rr tables on the device */
int c21hip_recomb_rates(const float *density, const float *G12, const float *xH,
                        const float *prev_nrec, float *nrec, size_t ntot, double stored_redshift,
                        double rate_scale, const double *rr_y_dev, const double *rr_c_dev,
                        int *flag_dev, void *stream);
/* sharded R loop with a recombination model: (mean free path, Gamma_12) of a rank's first
 * crossings packed into order-preserving 64-bit keys, and the reduced keys applied to the outputs */
int c21hip_pack_cross_keys(const float *mfp, const float *G12, unsigned long long *keys,
                           size_t ntot, void *stream);
int c21hip_apply_cross_keys(const unsigned long long *keys, const float *prev_z_reion,
                            int first_snapshot, double redshift, float *xH, float *z_reion,
                            float *G12, float *mfp, size_t ntot, void *stream);
/* one bit per cell of a first-crossing grid (non-zero -> 1), and the OR of `world` such packed
 * grids (stride_words apart) expanded back to 0 / 1 bytes: the exchange of a sharded run */
int c21hip_pack_mask_bits(const unsigned char *fc, unsigned *bits, size_t ntot, void *stream);
int c21hip_or_unpack_mask_bits(const unsigned *bits, size_t stride_words, int world,
                               unsigned char *fc, size_t ntot, void *stream);
/* in-loop kernel timing (bench.py): HIP events around every pass launch on its stream while enabled;
 * kinds as in c21hip_bench_pass (12: one-grid pass Z + closed-form f_coll of the Eulerian loop; 1 pass Y, 2 fused pass Z, 7 / 8 pass X / two-radius pass X with
 * evaluated windows, 0 / 6 with streamed tables, 9 forward line passes) */
/* closed-form Eulerian loop: pass Z + f_coll of a radius with the barrier of the PREVIOUS radius of the
 * loop (its dense grid, its mean, its index) applied in the same sweep */
int c21hip_z_fcoll_erfc_mask_supported(int nx, int ny, int nz);
int c21hip_split_z_fcoll_erfc_mask(const float *split_work, float *nion_dense, const float *nion_prev,
                                   const double *mean_prev_dev, unsigned char *first_cross, int r_index_prev,
                                   int fix_mean, double mean_f_coll, int mass_dep_zeta, double f_limit,
                                   double ion_eff, int nx, int ny, int nz, double growthf, double sigma_min,
                                   double sigma_max, double delta_c, double *partials, double *sum_out,
                                   void *stream);
/* closed-form Eulerian loop, banded barrier: the barrier of a radius decided inside its own pass Z
 * wherever it does not depend on the exact box mean.  The barrier test is monotone in the cell's f_coll,
 * i.e. a threshold; band_dev[0] / band_dev[1] = the thresholds at the two ends of the predicted band of
 * mean_f_coll / mean (at or above [0]: crosses for sure; below [1]: does not).  Cells in between carry
 * the marker 255 in first_cross and their f_coll in f_pend until the next radius' sweep (r_prev,
 * thr_prev_dev = its exact threshold) or c21hip_eul_resolve_pending settles them.  c21hip_eul_band =
 * [the sum of the pass-Z partials, c21hip_reduce_sum's arithmetic, when partials != NULL +] finish_mean of r_cur + its exact threshold (thr_dev[r_cur]) + the check of r_cur's band (*fail_dev =
 * the largest radius index whose band missed; c21hip_eul_rewind clears what that radius and the ones
 * after it wrote) + the band of r_next. */
int c21hip_split_z_fcoll_erfc_band(const float *split_work, float *f_pend, const double *band_dev,
                                   const double *thr_prev_dev, unsigned char *first_cross, int r_index,
                                   int r_prev, int nx, int ny, int nz, double growthf, double sigma_min,
                                   double sigma_max, double delta_c, double *partials, double *sum_out,
                                   void *stream);
int c21hip_eul_band(const double *partials, int n, double *sum_dev, double ntot, int mass_dep_zeta,
                    double f_limit, double *means_dev, int r_cur, int r_p1, int r_p2, double t_cur,
                    double t_next, int r_next, int cur_banded, int fix_mean, double mean_f_coll,
                    double ion_eff, double min_rel, double shift, double *band_dev, double *thr_dev,
                    int *fail_dev, unsigned *counter_dev, int mf_space, int quad, double *pred_dev,
                    void *stream);
/* the same for the table models WITH an x_e grid (mf_space = 1: the band and thr_dev hold the mean fix
 * itself -- the barrier f mf zeta > 1 - x_e has no single threshold): pass Z of the filtered x_e + the
 * table sweep of the dense filtered density + the barrier in one launch (512-point z-lines) */
int c21hip_z_xe_fcoll_band_supported(int nx, int ny, int nz);
int c21hip_split_z_xe_fcoll_band(const float *xe_work, const float *delta_fil, long delta_zstride, float *f_pend,
                                 float *xe_pend, const double *band_dev, const double *mf_prev_dev,
                                 unsigned char *first_cross, int r_index, int r_prev, int mode, double tab_min,
                                 double tab_width, const float *table_dev, int mass_dep_zeta, double f_limit,
                                 double ion_eff, int nx, int ny, int nz, double *partials, void *stream);
int c21hip_eul_resolve_pending_xe(int r_index, const float *f_pend, const float *xe_pend, const double *mf_dev,
                                  int mass_dep_zeta, double f_limit, double ion_eff, unsigned char *first_cross,
                                  size_t ntot, void *stream);
int c21hip_eul_rewind(unsigned char *first_cross, int r_fail, size_t ntot, void *stream);
/* the same for the table modes: c21hip_fcoll_eulerian with the barrier decided in the sweep; the dense
 * f_coll grid is not written, *n_partials_out partial sums stay in `partials` for c21hip_eul_band */
int c21hip_fcoll_eulerian_band(const float *delta_fil, long zstride, float *f_pend, unsigned char *first_cross,
                               int nx, int ny, int nz, int mode, double tab_min, double tab_width,
                               const float *table_dev, const double *band_dev, const double *thr_prev_dev,
                               int r_index, int r_prev, double *partials, int *n_partials_out, void *stream);
int c21hip_eul_resolve_pending(int r_index, const float *f_pend, const double *thr_dev,
                               unsigned char *first_cross, size_t ntot, void *stream);
void c21hip_ktime_enable(int on);
int c21hip_ktime_report(int kind, double *ms_total, int *count);
int c21hip_max_into(void *dst, const void *src, size_t count, int bytes_per_element, void *stream);
/* sharded fused recombination loop: own slab (mask, g12; in place) against n_peers received slabs
 * of `stride` cells each -- larger first-crossing index wins, with its Gamma_12 */
int c21hip_combine_cross_g12(unsigned char *mask, float *g12, const unsigned char *peer_mask,
                             const float *peer_g12, int n_peers, size_t stride, size_t n, void *stream);
int c21hip_sum_float(const float *v, size_t n, double *partials, double *sum_out, void *stream);
int c21hip_eulerian_mask(const c21hip_ionize_args *a, const float *nion_dense,
                         const float *xe_dense, const double *mean_dev,
                         unsigned char *first_cross, void *stream);
/* mask of radii > 0 + radius index 0 + post-loop sweep of the fused Lagrangian path in one pass
 * (IonisationBox.c:1031-1256,1597-1608); partials: 2 * 2048 doubles; writes every z_reion.
 * stars_direct = 1: stars_fil is the dense emissivity input (clipped on load) instead of its
 * padded, window-less transform round trip.  a->use_ts_fluct (stars_direct only): xe_dense and
 * kinetic_temp_neutral are the dense x_e / T_k inputs of the spin-temperature run. */
int c21hip_final_sweep(const c21hip_ionize_args *a, double stored_redshift,
                       const unsigned char *first_cross, const float *stars_fil,
                       const float *density, const float *prev_z_reion, float *xH, float *z_reion,
                       float *kinetic_temperature, double *partials, double *sum_stars_out,
                       double *sum_xh_out, int *flag_out, int stars_direct, const float *xe_dense,
                       const float *kinetic_temp_neutral, void *stream);
/* The final sweep walks the box in CHUNKS of contiguous cells, one workgroup each; the chunking depends on
 * the box alone.  _chunks: their number and size (dense: the sweep reads dense grids); _range: chunks
 * [chunk_begin, chunk_end) only (chunk_end < 0: all), partials left at partials[chunk] (stars) and
 * partials[2048 + chunk] (x_HI), no reduce; _reduce: the fixed-order reduce over ALL chunk partials.
 * A rank that sweeps a slab of whole chunks leaves the partials the single pass leaves there (sharded
 * finish phase, c21cm_ionize_shard_finish_slab). */
int c21hip_final_sweep_chunks(const c21hip_ionize_args *a, int dense, int *n_chunks, size_t *chunk_cells);
int c21hip_final_sweep_range(const c21hip_ionize_args *a, double stored_redshift,
                             const unsigned char *first_cross, const float *stars_fil,
                             const float *density, const float *prev_z_reion, float *xH, float *z_reion,
                             float *kinetic_temperature, double *partials, int *flag_out, int stars_direct,
                             const float *xe_dense, const float *kinetic_temp_neutral, int chunk_begin,
                             int chunk_end, void *stream);
int c21hip_final_sweep_reduce(const c21hip_ionize_args *a, int dense, double *partials,
                              double *sum_stars_out, double *sum_xh_out, void *stream);
int c21hip_final_sweep_eulerian_range(const c21hip_ionize_args *a, double stored_redshift,
                                      const unsigned char *first_cross, const float *nion_dense,
                                      const double *mean_dev, const float *density, const float *prev_z_reion,
                                      float *xH, float *z_reion, float *kinetic_temperature, double *partials,
                                      int *flag_out, const float *xe_dense, const float *kinetic_temp_neutral,
                                      int chunk_begin, int chunk_end, void *stream);
/* the same sweep for the Eulerian source models: the dense f_coll grid of radius index 0 and its box mean
 * in place of the emissivity grid (apply_first_cross + ionise_eulerian<LAST> + finalize in one pass) */
int c21hip_final_sweep_eulerian(const c21hip_ionize_args *a, double stored_redshift,
                                const unsigned char *first_cross, const float *nion_dense,
                                const double *mean_dev, const float *density, const float *prev_z_reion,
                                float *xH, float *z_reion, float *kinetic_temperature, double *partials,
                                double *sum_xh_out, int *flag_out, const float *xe_dense,
                                const float *kinetic_temp_neutral, void *stream);
/* delta_T (and tau_21) per cell + their sum (BrightnessTemperatureBox.c:58-87); partials: 2048 */
int c21hip_brightness_temp(const float *density, const float *xH, const float *Ts, float *bt,
                           float *tau, size_t n, float const_factor, float T_rad, double redshift,
                           int use_ts, double *partials, double *sum_out, void *stream);
int c21hip_apply_first_cross(const unsigned char *first_cross, const float *prev_z_reion,
                             int first_snapshot, double redshift, float *xH, float *z_reion,
                             size_t ntot, void *stream);

/* ---- lightcone_kernels.hip : rectilinear lightcone slabs and the dv/dr correction (lightconers.py,
 * rsds.py) ---- */
#define C21HIP_LC_MAX_FIELDS 16
typedef struct c21hip_lc_slice { /* one slice of a node pair's run, built by the host */
    int plane;                   /* node-box plane along the line of sight, in [0, d_para) */
    int pad_;
    double w_lo, w_hi;           /* weights of the low- and high-redshift box */
} c21hip_lc_slice;
/* slices j in [0, run) of every column: dst[q][col*dst_stride + dst_off + j] from plane tab[j].plane
 * of lo[q] / hi[q] (boxes of n_cols columns of d_para planes); bit q of mean_max: z_reion's rule */
int c21hip_lightcone_slab(const float *const *lo, const float *const *hi, float *const *dst,
                          int n_fields, unsigned mean_max, size_t n_cols, int run, int d_para,
                          long dst_stride, long dst_off, const c21hip_lc_slice *tab, double w_norm,
                          void *stream);
/* brightness_temp corrected in place by the line-of-sight gradient of vel (n_slices >= 3);
 * hubble: H(z) [1/s] per slice, device; tau: USE_TS_FLUCT only */
int c21hip_lightcone_dvdr(float *bt, const float *vel, const float *tau, const double *hubble,
                          size_t n_cols, int n_slices, double dx, double max_dvdr, int use_ts,
                          void *stream);
int c21hip_d2h_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                  size_t height, void *stream);

/* ---- dvdr_periodic_kernels.hip : the dv/dr correction of a coeval box, periodic line of sight
 * (rsds.py:16-103 with periodic = True) ----
 * bt_out = bt_in corrected by g = irfft(i k rfft(vel)) along every line of n cells (float[n_cols][n], the
 * line of sight fastest), k = 2 pi rfftfreq(n, dx); then the per-cell arithmetic of c21hip_lightcone_dvdr.
 * bt_out may be bt_in.  hubble: H(z) [1/s] per slice, device; tau: USE_TS_FLUCT only.  method 0: automatic,
 * 1: transform (n = 2^k, 8 <= n <= 1024), 2: direct circulant sum (2 <= n <= 1536).  Device pointers only;
 * one launch.  An unsupported n, a method that does not fit n or a NULL array is C21CM_VALUE_ERROR, and
 * nothing is launched. */
int c21hip_dvdr_periodic(float *bt_out, const float *bt_in, const float *vel, const float *tau,
                         const double *hubble, size_t n_cols, int n, double dx, double max_dvdr, int use_ts,
                         int method, void *stream);

/* ---- angular_lightcone_kernels.hip : angular lightcone sampling and the periodic B-spline prefilter
 * (lightconers.py AngularLightconer) ---- */
#define C21HIP_ANG_MAX_BOXES (3 * C21HIP_LC_MAX_FIELDS) /* a vector field takes three boxes */
typedef struct c21hip_ang_slice { /* one slice of a node pair's run, built by the host */
    double d;                     /* comoving distance [cells] */
    double w_lo, w_hi;            /* weights of the low- and high-redshift box */
} c21hip_ang_slice;
/* slices j in [0, run) of every pixel: dst[q][pix*dst_stride[q] + dst_off[q] + j] sampled at
 * d_j nhat[:, pix] + origin from the boxes lo / hi (n0 x n1 x n2, periodic); field q takes one box, or
 * three (bit q of vec: the projection on nhat); nhat: device, [3][n_pix]; *bad |= 1 where a sum is not
 * finite.  Device pointers only. */
int c21hip_angular_sample(const float *const *lo, const float *const *hi, float *const *dst,
                          const long *dst_stride, const long *dst_off, int n_fields, unsigned mean_max,
                          unsigned vec, int order, size_t n_pix, int run, int n0, int n1, int n2,
                          const double *nhat, const double *origin, const c21hip_ang_slice *tab,
                          double w_norm, int *bad, void *stream);
/* B-spline coefficients (order 3 or 5) of a periodic n0 x n1 x n2 box, src -> dst (may alias);
 * *bad |= 1 where a src value is not finite.  Device pointers only. */
int c21hip_spline_prefilter(const float *src, float *dst, int n0, int n1, int n2, int order, int *bad,
                            void *stream);

/* ---- rsd_kernels.hip : redshift-space distortions along the line of sight (rsds.py:184-255) ---- */
#define C21HIP_RSD_MAX_FIELDS 16
#define C21HIP_RSD_MAX_LDS (159 * 1024) /* dynamic LDS of one workgroup: 160 KiB less the static part */
/* LDS bytes of one launch for nf fields of n-slice columns; *cpb: columns per workgroup */
size_t c21hip_rsd_lds_bytes(int n, int nf, int *cpb);
/* out[q] = the shift of in[q] (columns of n slices, the line of sight fastest) by vel * disp_scale[j]
 * pixels on a grid of m sub-cells; out[q] may alias in[q].  Device pointers only; *bad |= 1 where a
 * field or velocity value is not finite (the caller clears and reads it) */
int c21hip_rsd_shift(const float *const *in, float *const *out, int nf, const float *vel,
                     const double *disp_scale, size_t n_cols, int n, int m, int periodic, int *bad,
                     void *stream);

/* ---- power_kernels.hip : power spectra of boxes and lightcone chunks, binned on the device ---- */
#define C21HIP_POWER_MAX_LDS (144 * 1024) /* dynamic LDS of one bin workgroup */
typedef struct c21hip_power_tabs { /* device pointers the driver fills (power_driver.c) */
    const double *kx, *ky, *kz; /* wavenumbers per axis: nx, ny, nz/2 + 1 (numpy's fftfreq(n, L/n) 2 pi) */
    const double *edges;        /* n_local + 1: |k|^2 thresholds of the |k| edges, or k_par edges (cylindrical) */
    const int *rows;            /* row ids i ny + j, grouped (cylindrical: by k_perp bin) */
    const int *wg_rows;         /* n_wg + 1: workgroup w bins rows[wg_rows[w] .. wg_rows[w + 1]) */
    const int *group_wg;        /* n_groups + 1: the workgroups of group g (its bins g n_local ..) */
    int n_wg, n_groups, n_local;
    int ignore_zero_mode, ignore_kpar_zero;
    /* cuts of the spherical average (read by the instantiations with cuts only): mu_min^2, mu_max^2, the wedge's
     * slope^2 and its buffer */
    int use_mu, use_wedge;
    double mu_min_sq, mu_max_sq, wedge_slope_sq, wedge_buffer;
} c21hip_power_tabs;
/* accumulators per bin: sum w P, sum w k, [sum w k_par (cylindrical)], [sum w P^2 (variance)], sum w */
#define C21HIP_POWER_NV(cylindrical, variance) (3 + ((cylindrical) ? 1 : 0) + ((variance) ? 1 : 0))
size_t c21hip_power_lds_bytes(int n_local, int cylindrical, int variance);
/* (in[offsets[b] + (i ny + j) row_pitch + l] - mean[b]) [* wrow[i ny + j] * wz[l]] -> padded[b][i][j][l] for
 * l < nz; *bad |= 1 on a non-finite value.  mean[n_batch] is written here and goes on to c21hip_power_bin: without
 * a window each box's mean rounded to fp32 (a plain fp32 subtraction); with one (wrow and wz not NULL, device,
 * nx ny and nz floats) the fp64 mean, subtracted in fp64.  rowsum: n_batch nx ny doubles of scratch */
int c21hip_power_pack(const float *in, float *padded, int nx, int ny, int nz, long long row_pitch,
                      const long long *offsets, int n_batch, double *rowsum, double *mean, const float *wrow,
                      const float *wz, int *bad, void *stream);
/* one pass over the half spectra complex[n_batch][nx][ny][nz/2+1] (spec2: cross power, or NULL) into
 * partials[n_batch][n_wg][n_local][NV]; mean1 / mean2: what goes back onto the k = 0 mode (the means the pack took
 * out of each box; zeros with a window) */
int c21hip_power_bin(const float *spec1, const float *spec2, int nx, int ny, int nz, int n_batch,
                     int cylindrical, int variance, const c21hip_power_tabs *t, const double *mean1,
                     const double *mean2, double *partials, int *bad, void *stream);
/* partials -> totals[n_batch][n_groups n_local][NV] -> means (device outputs); var (variance only): the population
 * variance of the per-mode power, scale^2 (sum w P^2 / sum w - (sum w P / sum w)^2) */
int c21hip_power_finish(const double *partials, double *totals, int n_batch, int cylindrical, int variance,
                        const c21hip_power_tabs *t, double scale, double *power, double *kmean, double *var,
                        long long *counts, void *stream);

/* ---- moments_kernels.hip : one-point statistics of boxes and lightcone chunks ---- */
#define C21HIP_MOMENTS_MAX_BINS 4096 /* edges (fp64) and counts (32 bits) of one workgroup: 48 KiB of LDS and 8 bytes */
/* pass 1: mean[b] = the fp64 mean of box b (row sums with lanes strided, then a fixed tree); *bad |= 1 on a
 * non-finite value.  rowsum: n_batch nx ny doubles of scratch; part: c21hip_moments_part_doubles of scratch (the
 * first level of a box's sum over its rows) */
size_t c21hip_moments_part_doubles(int nx, int ny, int n_batch);
int c21hip_moments_mean(const float *in, int nx, int ny, int nz, long long row_pitch, const long long *offsets,
                        int n_batch, double *rowsum, double *part, double *mean, int *bad, void *stream);
/* pass 2: moments[b] = {mean, sum d^2 / N, sum d^3 / N, sum d^4 / N}, d = (double)v - mean[b], in a fixed order;
 * hist[b][n_bins] (zeroed here; skipped when n_bins = 0) counts np.digitize((double)v, edges) - 1 where it lies in
 * [0, n_bins).  edges: device, n_bins + 1; rowsum: 3 n_batch nx ny doubles of scratch */
int c21hip_moments_central(const float *in, int nx, int ny, int nz, long long row_pitch, const long long *offsets,
                           int n_batch, const double *mean, int n_bins, const double *edges, double *rowsum,
                           double *part, double *moments, unsigned long long *hist, void *stream);

/* ---- bispectrum_kernels.hip : bispectra of boxes and lightcone chunks (bispectrum_driver.c) ---- */
#define C21HIP_BISPEC_MAX_BINS 32
#define C21HIP_BISPEC_GROUP 8 /* third shells one products workgroup accumulates */
/* ints per products group: b1, b2, the number of third shells (1 .. GROUP), then GROUP third shells (unused
 * places repeat b2 and are not read) */
#define C21HIP_BISPEC_GROUP_INTS (3 + C21HIP_BISPEC_GROUP)
typedef struct c21hip_bispec_tabs { /* device pointers the driver fills */
    const double *kx, *ky, *kz; /* wavenumbers per axis: nx, ny, nz/2 + 1 */
    const double *thr;          /* n_bins + 1: the |k|^2 thresholds of the shell edges (as the power bins') */
    int n_bins;
} c21hip_bispec_tabs;
/* one pass over the half spectrum complex[nx][ny][nz/2+1]: stack[s][mode] = the mode where its shell is s, else 0,
 * for every s < n_bins and every mode (each element written once).  as_double = 0: float2 stack, the modes of spec;
 * 1: double2 stack, 1 + 0i in place of the mode (the shell indicators; spec is not read) */
int c21hip_bispec_fill(const float *spec, void *stack, int as_double, int nx, int ny, int nz,
                       const c21hip_bispec_tabs *t, void *stream);
/* slabs of whole rows the products kernel cuts a box into, and rows per slab: a function of the shape alone */
int c21hip_bispec_slabs(int nx, int ny, int nz, int *rows_per_slab);
/* stack: n_bins padded real boxes [nx ny][2(nz/2+1)] (float, or double when as_double).  Group g (groups, device:
 * n_groups x C21HIP_BISPEC_GROUP_INTS) and slab s give partials[s][g GROUP + j] = the fp64 sum over the slab's
 * cells, in a fixed order, of box(b1) box(b2) box(b3_j) */
int c21hip_bispec_products(const void *stack, int as_double, int nx, int ny, int nz, const int *groups,
                           int n_groups, double *partials, void *stream);
/* S[b][t] = the sum over the slabs, in a fixed order, of partials[b][slab][slot[t]].  counts_in given: out_b[b][t] =
 * scale S / (n_cells counts_in[t]), NaN where the count is 0.  Otherwise (n_batch = 1) counts_out[t] = the nearest
 * integer to S / n_cells */
int c21hip_bispec_finish(const double *partials, int n_batch, int n_slabs, int n_slots, const int *slot, int n_tri,
                         double scale, double n_cells, const long long *counts_in, double *out_b,
                         long long *counts_out, void *stream);

/* ---- bubble_kernels.hip : mean-free-path bubble sizes of boxes and lightcone chunks (bubble_driver.c) ---- */
#define C21HIP_BUBBLE_MAX_BINS 4096 /* edges (fp64) and counters (32 bits) of one workgroup: 48 KiB of LDS */
#define C21HIP_BUBBLE_CHUNK 64      /* mask words per chunk: one pack workgroup, one lane each in the prefix pass */
/* The mask of box b: nx ny rows of W = (nz + 63) / 64 words, bit l & 63 of word l >> 6 of a row set where the cell
 * is selected ((double)v < threshold, or >= with select_below = 0), the padding bits zero.  chunk_sum[b][c] = the
 * set bits of words [64 c, 64 c + 64) of the box; *bad |= 1 on a non-finite value */
int c21hip_bubble_pack(const float *in, int nx, int ny, int nz, long long row_pitch, const long long *offsets,
                       int n_batch, double threshold, int select_below, unsigned long long *mask, int *chunk_sum,
                       int *bad, void *stream);
/* prefix[b][w] = the set bits of the box's words before w (chunk_off: n_batch x chunks of scratch, the exclusive scan
 * of chunk_sum), stats[b][0] = the set bits of box b */
int c21hip_bubble_rank(const unsigned long long *mask, const int *chunk_sum, int nx, int ny, int nz, int n_batch,
                       long long *chunk_off, long long *prefix, long long *stats, void *stream);
typedef struct c21hip_bubble_walk_args {
    const unsigned long long *mask; /* device, as c21hip_bubble_pack wrote it */
    const long long *prefix;
    int nx, ny, nz, n_batch;
    double cell[3], max_length;
    int periodic[3], los;
    long long n_rays, max_steps;
    unsigned long long seed;
    int n_bins;
    const double *edges;         /* device, n_bins + 1 */
    unsigned long long *hist;    /* [n_batch][n_bins], zeroed by the caller */
    long long *stats;            /* [n_batch][4]: n_sel as c21hip_bubble_rank left it, the other three zeroed */
    double *lengths;             /* [n_batch][n_rays] or NULL */
    unsigned char *flags;        /* [n_batch][n_rays] or NULL */
    long long *starts;           /* [n_batch][n_rays] or NULL */
} c21hip_bubble_walk_args;
/* the rays of every box: the estimator of c21cm_bubble_sizes_grids (include/c21cm_grid.h) */
int c21hip_bubble_walk(const c21hip_bubble_walk_args *a, void *stream);

/* ---- cluster_kernels.hip : friends-of-friends clusters of boxes and lightcone chunks (cluster_driver.c) ---- */
/* From the mask of c21hip_bubble_pack: label[b][c] = the smallest flat index of the cluster of cell c (adjacency as
 * c21cm_bubble_clusters_grids writes it down), -1 where c is not selected; size[b][r] = the cells of the cluster with
 * root r, 0 at every other cell.  nx ny nz < 2^31.  Three launches: init, merge, count (which flattens) */
int c21hip_cluster_label(const unsigned long long *mask, int nx, int ny, int nz, int n_batch, int connectivity,
                         int periodic_mask, int *label, int *size, void *stream);
/* root_mask: the layout of the pack's mask, a bit set where label[b][c] == c; chunk_sum as the pack leaves it, so
 * that c21hip_bubble_rank counts and ranks the roots */
int c21hip_cluster_roots(const int *label, int nx, int ny, int nz, int n_batch, unsigned long long *root_mask,
                         int *chunk_sum, void *stream);
typedef struct c21hip_cluster_emit_args {
    const unsigned long long *root_mask;
    const long long *prefix;     /* of root_mask, by c21hip_bubble_rank */
    const long long *n_clusters; /* [n_batch][4], entry 0 as c21hip_bubble_rank left it for root_mask */
    const int *size;
    int nx, ny, nz, n_batch;
    int n_bins;
    const long long *edges;         /* device, n_bins + 1 */
    unsigned long long *hist_n;     /* [n_batch][n_bins], zeroed by the caller */
    unsigned long long *hist_cells; /* [n_batch][n_bins], zeroed by the caller */
    unsigned long long *best;       /* [n_batch], zeroed by the caller */
    long long *stats;               /* [n_batch][4]: n_sel as c21hip_bubble_rank left it; the other three are written */
    long long max_clusters;
    long long *roots, *sizes; /* [n_batch][max_clusters], filled with -1 / 0 by the caller; or both NULL */
} c21hip_cluster_emit_args;
/* (root, size) of the clusters in ascending root, the two histograms, the four stats */
int c21hip_cluster_emit(const c21hip_cluster_emit_args *a, void *stream);

/* ---- granulometry_kernels.hip : distance transforms and granulometry of boxes and lightcone chunks
 * (granulometry_driver.c) ---- */
#define C21HIP_EDT_NONE (1 << 30)     /* D2 of a box without an unselected cell (C21CM_EDT_NONE) */
#define C21HIP_GRAN_MAX_RADII 255     /* radii and erosion counters of one workgroup: 3 KiB of LDS */
/* From the mask of c21hip_bubble_pack: dist2[b][c] = D2 of c21cm_granulometry_grids (include/c21cm_grid.h); where not
 * NULL level[b][c] = -1 at unselected cells and 0 elsewhere; eroded[b][k] = the cells with D2 > radii2[k] (radii2:
 * device, increasing); stats[b][1..3] = {max D2, its smallest flat index, n_unselected} beside stats[b][0] as
 * c21hip_bubble_rank left it.  hist [n_batch][256] and key [n_batch] are zeroed by the caller; work_a and work_b are
 * n_batch boxes of int32 each.  nx^2 + ny^2 + nz^2 < 2^30.  Four launches: z, y, x, finish */
int c21hip_gran_edt(const unsigned long long *mask, int nx, int ny, int nz, int n_batch, int periodic_mask,
                    int n_radii, const long long *radii2, int *work_a, int *work_b, int *dist2, int *level,
                    unsigned long long *hist, unsigned long long *key, long long *eroded, long long *stats,
                    void *stream);
/* covered[b][k] += the cells of box b inside an inscribed ball with D2 > radius2 (zeroed by the caller), and level
 * += 1 at those cells where not NULL; stats as c21hip_gran_edt left it.  Three launches: z, y, x */
int c21hip_gran_cover(const int *dist2, int nx, int ny, int nz, int n_batch, int periodic_mask, int radius2, int k,
                      int n_radii, const long long *stats, int *work_a, int *work_b, unsigned long long *covered,
                      int *level, void *stream);

/* ---- observe_kernels.hip : telescope-resolution smoothing of boxes and lightcones (observe_driver.c) ----
 * Fields are dense (nx, ny, ns) float32 with s fastest; every pointer is a device pointer and in != out. */
#define C21HIP_OBSERVE_MAX_LW 512   /* the widest half kernel: sigma <= 128 cells */
#define C21HIP_OBSERVE_TILE_ROWS 248 /* cells of a transverse line, halo included, a beam workgroup holds in LDS */
#define C21HIP_OBSERVE_LDS_LW 64     /* the widest half kernel of the LDS beam kernel; wider ones read global memory */
/* the two constants above as the library was built with them (for the tests) */
void c21hip_observe_geometry(int *tile_rows, int *lds_lw);
/* the parts the rows of a slice are dealt into for the means: a function of nx ny alone */
int c21hip_observe_mean_parts(long long rows);
/* means[s] = the fp64 mean of field[:, :, s], fixed order; partial: 4 c21hip_observe_mean_parts(nx ny) ns doubles;
 * *bad |= 1 on a non-finite value.  Two launches */
int c21hip_observe_means(const float *field, int nx, int ny, int ns, double *partial, double *means, int *bad,
                         void *stream);
/* One transverse pass of the beam of c21cm_observe_smooth_grids (include/c21cm_grid.h) along x (axis 0) or y (1),
 * wrapping.  tab[lw_max + 1][ns]: the weight w[d] of every slice, zero beyond its lw; lw[ns]; lw_block[ceil(ns /
 * 64)]: the largest lw of each 64 slices; 1 <= lw_max <= C21HIP_OBSERVE_MAX_LW the largest of all.  means != NULL:
 * (float)((double)in - means[s]) is convolved instead of in.  A slice with lw = 0 is copied */
int c21hip_observe_beam(const float *in, float *out, int nx, int ny, int ns, int axis, const float *tab,
                        const int *lw, const int *lw_block, int lw_max, const double *means, void *stream);
/* out[i][j][s] = the mean of in[i][j][s - below[s] .. s + above[s]], ascending, the range clipped to the line or,
 * with periodic, wrapped (below + above + 1 <= ns); means as above */
int c21hip_observe_channel(const float *in, float *out, int nx, int ny, int ns, const int *below, const int *above,
                           int periodic, const double *means, void *stream);

/* ---- minkowski_kernels.hip : Minkowski functionals of boxes and lightcone chunks (minkowski_driver.c) ---- */
#define C21HIP_MINKOWSKI_MAX_THRESHOLDS 255 /* a level fits a byte; thresholds and counters of one workgroup: 10 KiB */
/* The element counts of c21cm_minkowski_grids (include/c21cm_grid.h) for every threshold from one read of the boxes.
 * thresholds: device, n_thresholds increasing values; offsets: device.  hist[n_batch][8][n_thresholds + 1] is zeroed
 * by the caller and receives, per element kind, the elements by the largest level of their cells (the level of a
 * cell: the thresholds <= v, or with select_below n_thresholds less that; bin 0 is not filled);
 * counts[n_batch][n_thresholds][8] are its suffix sums.  *bad |= 1 on a non-finite value */
int c21hip_minkowski(const float *in, int nx, int ny, int nz, long long row_pitch, const long long *offsets,
                     int n_batch, int n_thresholds, const double *thresholds, int select_below, int periodic_mask,
                     unsigned long long *hist, long long *counts, int *bad, void *stream);

/* ---- ts_kernels.hip : per-cell part of ComputeTsBox (SpinTemperatureBox.c:892-927,1010-1086,
 * 1210-1383,1499-1848) ---- */
typedef struct c21hip_ts_args { /* the scalars of c21cm_ts_spec, passed by value */
    int n_step, lagrangian, use_xray_heating, use_cmb_heating, use_lya_heating, no_light;
    int table_exp; /* Eulerian: the per-shell table holds ln SFRD (1) or dfcoll/dz itself (0) */
    double redshift, dzp, growth_ratio;
    double No, N_b0, h_frac, he_frac, k_B, h_p, m_p, c_cms, A10, T_21, lambda_21, nu_Ly_alpha;
    double clumping_factor;
    double xray_prefactor, Trad, Ts_prefactor, xa_tilde_prefactor, xc_inverse, dcomp_dzp_prefactor;
    double Nb_zp, N_zp, lya_star_prefactor, volunit_inv, hubble_zp, growth_zp, dgrowth_dzp, dt_dzp;
    double sfr_scale, xray_scale;
    int sums_ready; /* the shell loop already ran (USE_MINI_HALOS: c21hip_ts_accumulate_mini) */
} c21hip_ts_args;
/* USE_MINI_HALOS (E-INTEGRAL).  Mini shell buffer: 6 per-shell rows (starlya, lya_cont, lya_inj of
 * the molecularly cooled population, the Lyman-Werner prefactors of both populations,
 * avg_fix_term_MINI written by c21hip_ts_sfrd_means_mini). */
#define C21HIP_TS_MINI_ROWS 6
int c21hip_ts_mcrit_grid(const float *J_21_LW, const float *vcb, double vcb_const, double redshift,
                         double A_LW, double BETA_LW, double A_VCB, double BETA_VCB,
                         double sigma_vcb, double m_turn, float *out, size_t ntot, void *stream);
int c21hip_ts_sfrd_means_mini(const float *filtered_density, const float *filtered_mcrit,
                              const float *tables2_dev, const double *dev_tab,
                              double *mini_shell_dev, const double *mean_sfr_mini_dev, int n_step,
                              size_t ntot, double mt_min, double mt_width, double *partials,
                              double *ave_out_dev, void *stream);
/* Lagrangian source grids with mini-halos: sfr_lw / sfr_mini_lw NULL unless the straight-line
 * copies exist (LYA_MULTIPLE_SCATTERING); same outputs and follow-up as the next function */
int c21hip_ts_accumulate_grids_mini(const c21hip_ts_args *a, const float *prev_xe, const float *sfr,
                                    const float *xray, const float *sfr_mini, const float *sfr_lw,
                                    const float *sfr_mini_lw, const double *dev_tab,
                                    const double *mini_shell_dev, double *sums_ws, float *J_21_LW,
                                    size_t ntot, void *stream);
/* the shell loop with both populations: sums_ws (6 * ntot doubles) and J_21_LW; follow with
 * c21hip_ts_cells(a with sums_ready = 1, ...) */
int c21hip_ts_accumulate_mini(const c21hip_ts_args *a, double sfr_scale_mini,
                              double xray_scale_mini, double mt_min, double mt_width,
                              const float *prev_xe, const float *delNL0, const float *mcrit,
                              const float *tables_dev, const float *tables2_dev,
                              const double *dev_tab, const double *mini_shell_dev, double *sums_ws,
                              float *J_21_LW, size_t ntot, void *stream);
/* device table buffer: 10 per-shell rows (z_edge_factor, xray_R_factor, starlya, lya_cont, lya_inj,
 * zpp_growth, tab_min, tab_width, avg_fix_term, 1 / tab_width) then the three [14][n_step]
 * frequency tables */
#define C21HIP_TS_SHELL_ROWS 10
size_t c21hip_ts_table_doubles(int n_step);
/* SFRD_TABLE: box mean of exp(table) per shell -> avg_fix_term row of dev_tab, means to ave_out;
 * partials: 512 * n_step doubles */
int c21hip_ts_sfrd_means(const float *filtered_density, const float *tables_dev, int table_exp,
                         double *dev_tab, const double *mean_sfr_zpp_dev, int n_step, size_t ntot,
                         double *partials, double *ave_out_dev, void *stream);
/* the two cell sweeps (R loop into sums_ws = 6 * ntot doubles, then the temperature update);
 * grid_a/grid_b = filtered_sfr/filtered_xray (lagrangian) or delNL0/NULL; partials: 6 * 2048
 * doubles; sums_out_dev: 6 doubles (Ts, Tk, x_e, J_alpha, xheat, xion) */
int c21hip_ts_cells(const c21hip_ts_args *a, const float *density, const float *prev_Ts,
                    const float *prev_Tk, const float *prev_xe, const float *grid_a,
                    const float *grid_b, const float *tables_dev, const double *dev_tab,
                    const double *lya_dEC_dev, const double *lya_dEI_dev, float *Ts_out,
                    float *Tk_out, float *xe_out, size_t ntot, double *sums_ws, double *partials,
                    double *sums_out_dev, int *flag_dev, void *stream);
/* the shell loop alone (sums_ws: [6][ntot] doubles) */
int c21hip_ts_shell_loop(const c21hip_ts_args *a, const float *prev_xe, const float *grid_a,
                         const float *grid_b, const float *tables_dev, const double *dev_tab,
                         double *sums_ws, size_t ntot, void *stream);
/* sharded ComputeTsBox: cell slabs of the ranks (rank r owns [begin(r), begin(r + 1))), the partial
 * sums of every peer's slab packed per peer ([world - 1] slots of c21hip_ts_slot_elems elements, each
 * [rows][maxlen] doubles -- or floats scaled by a per-row power of two, whose exponents close the slot), and the
 * complete sums of this rank's slab from its own partial and the received ones.  rowmax: 64 bytes of device
 * scratch, written by the pack and read by the combine of the same call. */
size_t c21hip_ts_slab_begin(size_t ntot, int world, int r);
size_t c21hip_ts_slot_elems(int rows, size_t maxlen, int as_float);
int c21hip_ts_pack_slabs(const double *sums, size_t ntot, int world, int rank, int rows,
                         size_t maxlen, int as_float, void *rowmax, void *out, void *stream);
int c21hip_ts_combine_slab(const double *sums, size_t ntot, int world, int rank, int rows,
                           size_t maxlen, int as_float, const void *rowmax, const void *recv, double *out,
                           void *stream);
/* What the last c21hip_ts_shell_loop / c21hip_ts_sfrd_means launched (0 before the first call); read-only,
 * for the tests: shell-loop version (1, 2, 3), cells per thread (1, 2), source mode (0 Lagrangian grids,
 * 1 ln SFRD tables, 2 dfcoll/dz tables) and the box-sum kernel of the table modes (0 with Lagrangian grids).
 * Two process-wide ints without synchronisation: meaningful only when one host thread drives ComputeTsBox. */
#define C21HIP_TS_ROUTE_LOOP_MASK 0x3
#define C21HIP_TS_ROUTE_CELLS_SHIFT 2
#define C21HIP_TS_ROUTE_MODE_SHIFT 4
#define C21HIP_TS_ROUTE_SUM_SHIFT 6
#define C21HIP_TS_SUM_SCALAR 1 /* sfrd_sum_kernel, one cell per load */
#define C21HIP_TS_SUM_VEC4 2   /* sfrd_sum_kernel, 16-byte loads */
#define C21HIP_TS_SUM_V2 3     /* sfrd_sum2_kernel */
int c21hip_ts_last_route(void);
struct c21cm_ts_first_spec;
int c21hip_ts_first(const struct c21cm_ts_first_spec *s, const float *density, float *Ts_out,
                    float *Tk_out, float *xe_out, size_t ntot, void *stream);
/* spin-exchange rate coefficients kappa_10 (H-H, e-H, p-H) at temperature T [K] */
void c21hip_kappa_rates(double T, double *k_HH, double *k_eH, double *k_pH);

/* ---- halo_sampler_kernels.hip: c21cm_sample_halos_grids (include/c21cm_grid.h) on device arrays ----
 * pass A: one condition per thread (block 256) or per wave64 (wave_threshold: expected halos from which a
 * wave takes the condition; both give the same words); words[4 n], FOUR per condition: halos kept, draws made, draws removed |
 * C21HIP_HS_DROP_LAST, the row of its first halo inside its block of 256 conditions; block_sums[ceil(n / 256)]: kept halos per 256 conditions; *bad (preset to ~0):
 * min over failing conditions of (index << 3 | code), codes C21HIP_HS_BAD_*.  scan: exclusive, in place,
 * the total to *total.  pass B writes the halos of condition i from row first_row + its offset. */
struct c21cm_sample_halos_spec;
#define C21HIP_HS_BLOCK 256
#define C21HIP_HS_DROP_LAST 0x80000000u
enum { C21HIP_HS_BAD_DRAWS = 1, C21HIP_HS_BAD_MASS = 2, C21HIP_HS_BAD_WALK = 3 };
typedef struct c21hip_hs_arrays {
    const double *tables;      /* device copy of spec->tables */
    const float *cond_masses;  /* descendants: masses, coordinates [3 n], the three deviates */
    const float *cond_coords, *cond_star, *cond_sfr, *cond_xray;
    const float *density, *overlap; /* cells; overlap may be NULL */
    unsigned long long n_cond;
    double wave_threshold;
    /* single_test_sample's cells: `density` holds overdensities at the redshift itself and cond_coords a
     * position inside the cell each one stands for (Stochasticity.c:1216-1222) */
    int cells_listed;
} c21hip_hs_arrays;
/* ---- dexm_kernels.hip: the DexM halo finder ---- */
struct c21cm_find_halos_spec;
typedef struct c21hip_dexm_arrays {
    unsigned char *in_halo, *forbidden, *state; /* [N] bytes; forbidden only with DEXM_OPTIMIZE */
    unsigned short *rung_grid;                  /* [N]: rung + 1 of the halo centred on the cell, else 0 */
    unsigned int *list, *found;                 /* [N]: the rung's candidates in raster order; halo cells as found */
    unsigned int *counters;                     /* decided, accepted (this rung), found (all rungs), last round */
} c21hip_dexm_arrays;
unsigned long long c21hip_dexm_blocks(size_t n); /* workgroups (= partial counts) of the compaction kernels */
int c21hip_dexm_count(int halos, const float *delta, float crit, const unsigned char *mask,
                      const unsigned short *rung_grid, size_t n, unsigned long long *counts, void *stream);
int c21hip_dexm_list(const float *delta, float crit, const unsigned char *mask, size_t n,
                     const unsigned long long *offsets, unsigned int *list, unsigned char *state, void *stream);
/* one round: decide marks the undecided candidates of rung r (rejected / accepted in this round), paint adds the
 * accepted spheres and settles the marks */
int c21hip_dexm_decide(const struct c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                       void *stream);
int c21hip_dexm_paint(const struct c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                      unsigned int round, void *stream);
int c21hip_dexm_serial(const struct c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_cand,
                       void *stream);
int c21hip_dexm_forbid(const struct c21cm_find_halos_spec *s, int r, const c21hip_dexm_arrays *a, unsigned int n_found,
                       const float *r_of_rung, void *stream);
int c21hip_dexm_extract(const struct c21cm_find_halos_spec *s, const c21hip_dexm_arrays *a, size_t n,
                        const unsigned long long *offsets, const float *mass_of_rung, float *masses, float *coords,
                        float *star, float *sfr, float *xray, void *stream);
int c21hip_dexm_mask_float(const unsigned char *mask, float *out, size_t n, void *stream);
int c21hip_dexm_downsample(const float *smooth, int dim, int dim_z, int hii_dim, int hii_dim_z, float *out, void *stream);

int c21hip_hs_pass_a(const struct c21cm_sample_halos_spec *s, const c21hip_hs_arrays *a, unsigned int *words,
                     unsigned long long *block_sums, unsigned long long *bad, void *stream);
int c21hip_hs_scan(unsigned long long *block_sums, unsigned long long n_blocks, unsigned long long *total,
                   void *stream);
int c21hip_hs_pass_b(const struct c21cm_sample_halos_spec *s, const c21hip_hs_arrays *a, const unsigned int *words,
                     const unsigned long long *block_bases, unsigned long long first_row, float *masses,
                     float *coords, float *star, float *sfr, float *xray, void *stream);

#ifdef __cplusplus
}
#endif
#endif
