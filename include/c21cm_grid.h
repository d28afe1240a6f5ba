/*
 * c21cm_grid.h -- explicit-scalar ("grid level") entry points of lib21cmfast_hip.so.
 *
 * The drop-in entry points of c21cm_abi.h read their physics scalars from the
 * process-global parameter structs and from host-side cosmology / HMF
 * integrals.  Everything they do on the GRIDS is delegated to the functions
 * declared here, which take every scalar explicitly.  These are what
 * bench.py and the parity tests call: the grid work can then be compared with
 * the CPU oracle on identical numbers, independent of host-integral numerics
 * ("mean_f_coll, f_limit supplied as fixed scalars").
 *
 * Pointer arguments may address host memory or MI355X HBM; the library detects
 * which (hipPointerGetAttributes) and stages host arrays through device
 * scratch.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Every function returns a c21cm_status code.
 */
#ifndef C21CM_GRID_H
#define C21CM_GRID_H

#include <stddef.h>

#include "c21cm_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define C21CM_MAX_RADII 256
#define C21CM_NDELTA_TABLE 400 /* reference: src/py21cmfast/src/interp_tables.c:27,34 */

/* How the per-cell collapsed fraction is obtained inside the R loop
 * (reference: src/py21cmfast/src/IonisationBox.c:821-881). */
enum c21cm_fcoll_mode {
    C21CM_FCOLL_STARS_GRID = 0,   /* Lagrangian source grids: f = filtered HaloBox.n_ion    */
    C21CM_FCOLL_ERFC = 1,         /* CONST-ION-EFF, no tables: FgtrM_bias_fast closed form  */
    C21CM_FCOLL_TABLE_LINEAR = 2, /* CONST-ION-EFF with tables: lerp(table, delta)          */
    C21CM_FCOLL_TABLE_EXP = 3,    /* E-INTEGRAL: exp(lerp(table, delta))                    */
    C21CM_FCOLL_NODES = 4         /* E-INTEGRAL WITHOUT interpolation tables: the conditional integral
                                   * Nion_ConditionalM per cell (IonisationBox.c:889-893, hmf.c:1106-1140)
                                   * on the Gauss-Legendre nodes of the radius, see below          */
};

/* Host callback used by the two TABLE modes: fill `table[C21CM_NDELTA_TABLE]`
 * (float, like the reference's RGTable1D_f) for filter radius index `r_index`
 * on the regular delta grid x_i = dens_min + i*(dens_max-dens_min)/(NDELTA-1).
 * reference: src/py21cmfast/src/IonisationBox.c:702-768. */
/* Mode C21CM_FCOLL_NODES: table_fn is called as table_fn(r_index, 0, 0, (float *)nodes, user) and fills
 * C21CM_NODE_DOUBLES DOUBLES instead of a float table -- everything of the integrand that does not
 * depend on the cell's overdensity:
 *   nodes[0] number of Gauss-Legendre nodes n (<= 100)   nodes[1] 0: extended Press-Schechter, 1: Sheth-Tormen
 *   nodes[2] growth factor                                nodes[3] delta above which the cell has collapsed
 *   nodes[4] the value returned for such a cell           nodes[5] != 0: the integral is empty (M_min >= M_cond)
 *   nodes[8 + 4 i ..]  (w_i x prefactor_i, barrier-expansion factor_i, barrier_i, 1 / (sigma_i^2 - sigma_c^2))
 * and the device sums  - w_i pref_i (factor_i - d0) exp(-(barrier_i - d0)^2 sdi_i / 2),  d0 = delta / D
 * (ST), or the same with (delta_c - delta) / D for both factors (PS), over the nodes. */
#define C21CM_NODE_DOUBLES 408
typedef int (*c21cm_table_fn)(int r_index, double dens_min, double dens_max, float *table,
                              void *user);

/* USE_MINI_HALOS: the two conditional N_ion tables of one radius are 2-D, overdensity x log10 of
 * the turnover mass (interp_tables.c:291-405): table[i * C21CM_NMTURN_TABLE + j] = ln N_ion at
 * delta_i = dens_min + i (dens_max - dens_min)/(NDELTA-1) and turnover 10^(l10mt_min +
 * j (l10mt_max - l10mt_min)/(NMTURN-1)); `table_acg` for the atomically cooled galaxies (turnover
 * range l10mt_*), `table_mcg` for the molecularly cooled ones (range l10mt_*_mini).  prev != 0:
 * the tables at the previous snapshot's redshift (trapezoidal history, IonisationBox.c:752-760). */
#define C21CM_NMTURN_TABLE 50 /* interp_tables.c:28 */
typedef int (*c21cm_table2d_fn)(int r_index, int prev, double dens_min, double dens_max,
                                double l10mt_min, double l10mt_max, double l10mt_min_mini,
                                double l10mt_max_mini, float *table_acg, float *table_mcg,
                                void *user);

/* All scalars of one ComputeIonizedBox call.
 * reference: struct IonBoxConstants / RadiusSpec, src/py21cmfast/src/IonisationBox.c:38-102. */
typedef struct c21cm_ionize_spec {
    /* geometry */
    int hii_dim;      /* cells along x and y                          */
    int hii_dim_z;    /* cells along z (= NON_CUBIC_FACTOR * HII_DIM) */
    double box_len;   /* Mpc, x and y                                 */
    double box_len_z; /* Mpc, z                                       */

    /* filter radii, ascending; index 0 is the cell-scale radius (setup_radii :964-1006) */
    int n_radii;
    int r_lowest; /* lowest radius index that is processed (0 unless M_min > RtoM(R) breaks :1537) */
    double R[C21CM_MAX_RADII];
    double sigma_maxmass[C21CM_MAX_RADII]; /* sigma_z0(RtoM(R)); ERFC / TABLE_LINEAR modes */

    /* filters (copy_filter_transform :572-664) */
    int hii_filter;      /* delta, x_e, N_rec grids                 */
    int stars_filter;    /* n_ion, whalo_sfr grids (3 = exp-MFP)    */
    double mfp_meandens; /* R_param of filter 3                     */

    /* source model */
    int fcoll_mode;   /* enum c21cm_fcoll_mode                                         */
    int fix_mean;     /* rescale grid f_coll to mean_f_coll (Eulerian models)          */
    int mass_dep_zeta; /* floor f at f_limit_acg (:1077-1082) and mean clamp (:1566)  */
    c21cm_table_fn table_fn;
    void *table_user;

    /* option flags */
    int use_ts_fluct;          /* filter TsBox.xray_ionised_fraction, partial T from Ts    */
    int recomb_model;          /* enum C21CM_RECOMB_*                                      */
    int cell_recomb;           /* AstroOptions.CELL_RECOMB                                 */
    int minimize_memory;       /* skip kinetic_temperature / mean_free_path                */
    int first_snapshot;        /* prev_redshift < 1: previous z_reion := -1 (:365-401)     */

    /* redshift / astro scalars (set_ionbox_constants :125-227) */
    double redshift;        /* written into z_reion on first crossing  */
    double stored_redshift; /* used by the ionised-temperature formula */
    double photoncons_adjustment_factor;
    double ion_eff_factor;  /* zeta applied to the per-cell f_coll     */
    double mean_f_coll;     /* global expectation (fix_mean numerator) */
    double f_limit_acg;
    double gamma_prefactor;
    double rhocrit_omb; /* RHOcrit * OMb, Lagrangian absorber normalisation (:1066) */
    double growth_factor;
    double sigma_minmass;
    double delta_c; /* physconst.delta_c_sph = 1.686 */
    double TK_nofluct;
    double adia_TK_term;
    double T_re;
    double fabs_dtdz;
    double dz;

    /* recombinations (recomb_model != none): the table behind splined_recombination_rate
     * (recombinations.c:64-122): rr_y[z_ct * C21CM_RR_NGAMMA + g] = recombination_rate(z_ct * 0.2f,
     * exp(ln Gamma_g), T4 = 1, case B) with ln Gamma_g = -10 + 0.1f g, and rr_c = the natural cubic
     * spline's c coefficients (half the second derivatives) of each row in ln Gamma, as
     * gsl_interp_cspline holds them.  Host arrays; c21_rr_tables() builds them (init_MHR). */
    const double *rr_y, *rr_c;

    /* mini-halos: E-INTEGRAL with USE_MINI_HALOS (need_minihalo_nion, IonisationBox.c:30-31).
     * Four filtered grids per radius (delta, the previous snapshot's delta and the two log10
     * turnover-mass grids of c21cm_mturn_grids), f_coll of both populations from the 2-D tables,
     * accumulated over snapshots per radius (box->unnormalised_nion[_mini][n_radii][N], :908-936):
     *   f(R) = f_prev_box(R) + f(z, M_turn) - f(z_prev, M_turn)
     * and the barrier f zeta + f_m zeta_m > (1 - x_e)(1 + rec) (:1118-1120). */
    int use_mini_halos;
    int need_prev_ion; /* previous box: mean_f_coll zeta + mean_f_coll_MINI zeta_m > 1e-4 (:1546) */
    double ion_eff_factor_mini;
    double mean_f_coll_mini;
    double f_limit_mcg;
    double gamma_prefactor_mini;
    const float *prev_density;    /* previous PerturbedField.density [N]          */
    const float *log10_mturn_acg; /* [N], calculate_mcrit_boxes (:403-457)        */
    const float *log10_mturn_mcg;
    c21cm_table2d_fn table2d_fn;
    void *table2d_user;

    /* AstroOptions.IONISE_ENTIRE_SPHERE (IonisationBox.c:1150-1158): a crossing cell flags all
     * cells within R as ionised (x_HI only; z_reion stays with the centres).  Without a
     * recombination model and without mini-halos (upstream's result then depends on the order in
     * which its threads paint), and with a cell-scale radius below one cell. */
    int ionise_entire_sphere;
} c21cm_ionize_spec;

#define C21CM_RR_NZ 300       /* recombinations.c:35 RR_Z_NPTS        */
#define C21CM_RR_NGAMMA 250   /* :39 RR_lnGamma_NPTS                  */
#define C21CM_RR_DZ 0.2f      /* :38 RR_DEL_Z      (a float upstream) */
#define C21CM_RR_LNGAMMA_MIN (-10.0) /* :40                            */
#define C21CM_RR_DLNGAMMA 0.1f       /* :41 RR_DEL_lnGamma (float)     */

/* Per-call diagnostics returned by the grid-level ionisation driver. */
typedef struct c21cm_ionize_report {
    double f_coll_grid_mean[C21CM_MAX_RADII]; /* after the clamp of :1566-1576 */
    double global_xH;
    double mean_f_coll_out; /* what ComputeIonizedBox leaves in box->mean_f_coll */
    double ms_preloop, ms_rloop, ms_postloop; /* device timings (hip events)     */
    double f_coll_grid_mean_mini[C21CM_MAX_RADII]; /* USE_MINI_HALOS */
    double mean_f_coll_mini_out;
} c21cm_ionize_report;

/* calculate_mcrit_boxes (IonisationBox.c:403-457): per cell log10 of the turnover masses
 *   M_turn,a = max(M_reion-feedback, mturn_a_nofb),  M_turn,m = max(M_rf, M_LW(J_21_LW, v_cb), mturn_m_nofb)
 * from the previous box's Gamma_12 / z_reion and the TsBox's J_21_LW (vcb == NULL: vcb_const).
 * Arrays on the host or the device ([N], dense); averages of the two log10 grids returned. */
typedef struct c21cm_mturn_spec {
    int hii_dim, hii_dim_z;
    int first_snapshot; /* previous z_reion is -1 everywhere (no feedback)           */
    double redshift;
    double mturn_a_nofb, mturn_m_nofb, vcb_const;
    double A_LW, BETA_LW, A_VCB, BETA_VCB, sigma_vcb; /* sigma_vcb = V_CB_AVG sqrt(3 pi / 8) */
} c21cm_mturn_spec;
int c21cm_mturn_grids(const c21cm_mturn_spec *spec, const float *prev_G12,
                      const float *prev_z_reion, const float *J_21_LW, const float *vcb,
                      float *log10_mturn_acg, float *log10_mturn_mcg, double *ave_acg,
                      double *ave_mcg, void *stream);

/* The whole ComputeIonizedBox grid algorithm (pre-loop r2c, R loop, post-loop).
 * reference: src/py21cmfast/src/IonisationBox.c:1477-1628. */
int c21cm_ionize_grids(const c21cm_ionize_spec *spec, const PerturbedField *perturbed_field,
                       const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                       const HaloBox *halos, IonizedBox *box, c21cm_ionize_report *report,
                       void *stream);

/* Early exit of ComputeIonizedBox (expected HII fraction < 1e-5): uniform neutral box.
 * reference: src/py21cmfast/src/IonisationBox.c:531-565 */
int c21cm_neutral_box(const c21cm_ionize_spec *spec, const PerturbedField *perturbed_field,
                      const TsBox *spin_temp, IonizedBox *box, size_t ntot);

/* R-loop sharding over GPUs.  Each rank runs the radii
 * r = n_radii-1-rank, n_radii-1-rank-world, ... > 0 and records in
 * `first_cross[N]` (uint8, device) the largest 1-based radius index whose
 * barrier the cell crossed (0 = none).  The caller max-reduces first_cross over
 * ranks (RCCL), then the rank that owns the outputs calls the finish step, which
 * applies the mask, runs radius index 0 (partial ionisation) and the post-loop. */
int c21cm_ionize_shard_radii(const c21cm_ionize_spec *spec, int rank, int world,
                             const PerturbedField *perturbed_field,
                             const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                             const HaloBox *halos, unsigned char *first_cross,
                             c21cm_ionize_report *report, void *stream);
/* Per-radius f_coll grid means for the finish step: the element-wise SUM over ranks of the shard
 * phases' report->f_coll_grid_mean (each radius > 0 belongs to one rank).  Optional; consumed by
 * the next c21cm_ionize_shard_finish of this process.  Needed for box->mean_f_coll of Lagrangian
 * models when r_lowest > 0 (IonisationBox.c:1623-1628) and for a complete report. */
int c21cm_ionize_shard_set_means(const double *means, int n_radii);
int c21cm_ionize_shard_finish(const c21cm_ionize_spec *spec, const unsigned char *first_cross,
                              const PerturbedField *perturbed_field,
                              const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                              const HaloBox *halos, IonizedBox *box, c21cm_ionize_report *report,
                              void *stream);

/* The finish phase split by cell slabs (round 5).  The cell-scale radius and the post-loop are per cell
 * (IonisationBox.c:1031-1256,1597-1608) and every rank holds the replicated inputs, so rank r finishes
 * the cells of ITS slab only -- whole chunks of the final sweep, c21cm_ionize_shard_slab -- from the
 * combined first crossings of that slab (first_cross is read on [cell_begin, cell_end) only: the
 * exchange before it moves 1 / world of each rank's packed grid per link instead of whole grids onto one
 * rank).  The sweep leaves the chunks' partial sums where the single pass leaves them; `exchange` then
 * all-gathers them (and, if the caller wants full boxes on every rank, the output slabs), after which
 * every rank reduces ALL chunks in the single pass' fixed order: global_xH and mean_f_coll are the
 * single pass' to the last bit on every rank, without a scalar broadcast.
 *   exchange(user, state, local_status, stream) is entered exactly once per call whatever happened
 *   locally (local_status != 0: this rank failed before its sweep; `state` may then be incomplete) and
 *   returns the status the ranks agreed on; NULL on a one-rank run.
 *   outputs_gathered != 0: the callback gathered the output slabs, host arrays receive whole grids;
 *   0: the outputs are slab-resident (host arrays receive this rank's slab only). */
typedef struct c21cm_shard_slab_state {
    int rank, world;
    int n_chunks, chunk_begin, chunk_end; /* this rank's chunks of the final sweep */
    size_t chunk_cells, cell_begin, cell_end, ntot;
    double *partials_stars, *partials_xh; /* device, n_chunks each; [chunk_begin, chunk_end) filled */
    int *flag;                            /* device: non-finite flag of this rank's slab (combine: max) */
    float *out[3]; /* device addresses of neutral_fraction, z_reion, kinetic_temperature (NULL: absent) */
} c21cm_shard_slab_state;
typedef int (*c21cm_shard_slab_exchange_fn)(void *user, const c21cm_shard_slab_state *state,
                                            int local_status, void *stream);
int c21cm_ionize_shard_slab_supported(const c21cm_ionize_spec *spec);
int c21cm_ionize_shard_slab(const c21cm_ionize_spec *spec, int rank, int world, int *chunk_begin,
                            int *chunk_end, size_t *cell_begin, size_t *cell_end, int *n_chunks,
                            size_t *chunk_cells);
int c21cm_ionize_shard_finish_slab(const c21cm_ionize_spec *spec, const unsigned char *first_cross,
                                   int rank, int world, const PerturbedField *perturbed_field,
                                   const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                                   const HaloBox *halos, IonizedBox *box, c21cm_ionize_report *report,
                                   c21cm_shard_slab_exchange_fn exchange, void *exchange_user,
                                   int outputs_gathered, void *stream);
/* device helpers of the slab exchange of the packed first crossings (one bit per cell):
 * pack the uint8 grid (n cells, n and the grid's start multiples of 32 cells or the box end);
 * OR `world` packed pieces (`stride_words` apart) into n bytes at `first_cross` */
int c21cm_shard_pack_mask_bits(const unsigned char *first_cross, unsigned *bits, size_t n, void *stream);
int c21cm_shard_or_unpack_mask_bits(const unsigned *bits, size_t stride_words, int world,
                                    unsigned char *first_cross, size_t n, void *stream);

/* The same two phases for a recombination model (spec->recomb_model != none): a first crossing
 * carries the radius (= mean free path) and Gamma_12, so the shard phase leaves 64-bit keys
 * bits(mfp) << 32 | bits(G12) in `cross_keys[N]` (device) -- non-negative floats order like their
 * bit patterns -- the caller max-reduces them as unsigned 64-bit integers, and the finish phase
 * unpacks the winner of every cell (reference: IonisationBox.c:1124-1140). */
int c21cm_ionize_shard_radii_keys(const c21cm_ionize_spec *spec, int rank, int world,
                                  const PerturbedField *perturbed_field,
                                  const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                                  const HaloBox *halos, unsigned long long *cross_keys,
                                  c21cm_ionize_report *report, void *stream);
int c21cm_ionize_shard_finish_keys(const c21cm_ionize_spec *spec,
                                   const unsigned long long *cross_keys,
                                   const PerturbedField *perturbed_field,
                                   const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                                   const HaloBox *halos, IonizedBox *box,
                                   c21cm_ionize_report *report, void *stream);

/* The fused recombination loop sharded (CELL_RECOMB, no x_e grid, native line lengths with the
 * windows evaluated in pass X: c21cm_ionize_shard_rc_supported != 0): a rank's radii leave the
 * uint8 first-crossing index and Gamma_12 at the crossing -- 5 bytes per cell instead of the
 * 8-byte key; the mean free path is the radius of the index.  Between the phases the caller keeps,
 * per cell, the entry of the rank with the LARGER index (an index > 0 is owned by one rank):
 * c21cm_ionize_sharded does it with a reduce-scatter by cell slabs + a gather (5 N / world bytes
 * per link and hop).  reference: IonisationBox.c:1084-1140,1531-1588 */
int c21cm_ionize_shard_rc_supported(const c21cm_ionize_spec *spec);
int c21cm_ionize_shard_radii_rc(const c21cm_ionize_spec *spec, int rank, int world,
                                const PerturbedField *perturbed_field,
                                const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                                const HaloBox *halos, unsigned char *first_cross, float *cross_g12,
                                c21cm_ionize_report *report, void *stream);
int c21cm_ionize_shard_finish_rc(const c21cm_ionize_spec *spec, const unsigned char *first_cross,
                                 const float *cross_g12, const PerturbedField *perturbed_field,
                                 const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                                 const HaloBox *halos, IonizedBox *box,
                                 c21cm_ionize_report *report, void *stream);
/* device helper of that exchange (own slab in place against n_peers received slabs of `stride`
 * cells; all starts at multiples of 4 cells) */
int c21cm_shard_combine_cross_g12(unsigned char *mask, float *g12, const unsigned char *peer_mask,
                                  const float *peer_g12, int n_peers, size_t stride, size_t n,
                                  void *stream);

/* ---- the sharded R loop behind the C ABI ---------------------------------------------------
 * One process per GPU; every rank calls c21cm_ionize_sharded with the same (replicated) inputs.
 * Collectives go through RCCL (librccl resolved at run time with dlopen: inside a PyTorch
 * process that is torch's own copy, so there is one RCCL per process).  Bootstrap: rank 0
 * obtains 128 bytes from c21cm_shard_unique_id, the launcher distributes them by any means
 * (torch.distributed, MPI, a file), every rank calls c21cm_shard_init.  Once initialised,
 * ComputeIonizedBox itself shards (C21CM_SHARD=0 keeps it single-GPU).
 * The rank that would own radius index 0 finishes and holds the outputs; with broadcast != 0
 * they are broadcast so that every rank returns the full box, as a drop-in caller expects. */
#define C21CM_SHARD_ID_BYTES 128
int c21cm_shard_unique_id(void *id128);
int c21cm_shard_init(int rank, int world, const void *id128);
int c21cm_shard_finalize(void);
int c21cm_shard_info(int *rank, int *world); /* returns 0 and fills them when initialised */
/* device time (ms) of this rank's last c21cm_ionize_sharded call: shard phase, exchange (includes
 * the wait for the slowest peer), finish; and the rank count RCCL itself reports (ncclCommCount) */
int c21cm_shard_last_phases(double ms[3]);
int c21cm_shard_comm_count(void);
/* 1: the communicator is RCCL's (not the in-process emulation the tests use) */
int c21cm_shard_is_rccl(void);
/* collective: 1 when EVERY rank passed a non-zero `local_yes` (ranks agree on a path before they
 * take it: ComputeTsBox shards only if all of them hold device arrays) */
int c21cm_shard_all_agree(int local_yes);
/* 1: shard_rccl.c was compiled against <rccl/rccl.h> and its hand-declared ncclUniqueId /
 * ncclDataType_t / ncclRedOp_t values and the prototypes it calls were checked against it */
int c21cm_shard_rccl_header_checked(void);

/* ---- ComputeTsBox sharded over the same communicator (the N_STEP_TS shells dealt round-robin;
 * reference: SpinTemperatureBox.c:1541-1784 is linear in the shells).  With a communicator in place
 * ComputeTsBox shards by itself for the Eulerian table models on device arrays (C21CM_SHARD_TS=0
 * opts out); the two compute phases are exported for tests and other transports:
 *   c21cm_ts_box_shard_sums    rank's shells: density filter loop, tables, box means, shell loop ->
 *                              partial sums [6][N] doubles (device), *n_rows of them in use
 *   (exchange)                 sum the partials over the ranks; rank r needs cells
 *                              [c21cm_ts_slab_begin(N, world, r), c21cm_ts_slab_begin(N, world, r + 1))
 *   c21cm_ts_box_shard_finish  temperature update of a cell range from its complete sums
 *                              ([n_rows][ncell] doubles, device) into the output boxes
 * Parameters come from the broadcast globals like ComputeTsBox's. */
int c21cm_ts_shardable(float redshift, const PerturbedField *pf, const TsBox *prev, const TsBox *out);
int c21cm_ts_shard_shells(int n_step, int rank, int world, int *idx);
size_t c21cm_ts_slab_begin(size_t ntot, int world, int r);
int c21cm_ts_box_shard_sums(float redshift, float prev_redshift, float perturbed_field_redshift,
                            PerturbedField *perturbed_field, TsBox *previous_spin_temp, int rank,
                            int world, double *sums_dev, int *n_rows);
int c21cm_ts_box_shard_finish(float redshift, float prev_redshift, float perturbed_field_redshift,
                              PerturbedField *perturbed_field, TsBox *previous_spin_temp,
                              const double *slab_sums, size_t cell0, size_t ncell,
                              TsBox *this_spin_temp);
int c21cm_ts_box_sharded(float redshift, float prev_redshift, float perturbed_field_redshift,
                         PerturbedField *perturbed_field, TsBox *previous_spin_temp,
                         TsBox *this_spin_temp);
int c21cm_ts_box_sharded_calls(void); /* calls of c21cm_ts_box_sharded in this process (tests) */
int c21cm_shard_owner(int n_radii, int world);
/* Test hook: replace the transport by an in-process device mailbox so that the ranks of a
 * world > 1 run can be executed one after the other in ONE process (non-owners first, the owner
 * last; mailbox zeroed before each round, >= world * N/8 + 8 N bytes).  See shard_rccl.c. */
int c21cm_shard_emulate(int rank, int world, void *mailbox, size_t mailbox_bytes);
/* Diagnostic: where the time of this process' last ComputeIonizedBox went -- out[0] host ms before the
 * device driver (scalars, tables, spec), [1] device pre-loop, [2] R loop, [3] post-loop, [4] wall ms of
 * the call, [5] number of filter radii. */
int c21cm_last_ionize_timing(double out[6]);
/* diagnostic: which R loop the last ionisation call set up -- 1 fused loop, 2 fused recombination loop,
 * 4 a third spectrum in the barrier kernel, 8 ... which is the filtered N_rec, 16 a fourth spectrum
 * (x_e AND filtered N_rec), 32 two radii per pass-X sweep, 64 the Eulerian loops' cell-scale radius and
 * post-loop ran as one sweep (set when that call finishes) */
int c21cm_ionize_last_loop_flags(void);

/* What a sharded call leaves in the output arrays -- `broadcast` of c21cm_ionize_sharded, and what the
 * drop-in ComputeIonizedBox passes (c21cm_shard_output_mode: c21cm_shard_set_output, else the environment
 * C21CM_SHARD_OUTPUT = all | none | auto, default auto):
 *    1  whole boxes on every rank (all-gather of the output slabs, or a broadcast of the owner's box)
 *    2  (slab finish) the whole neutral-fraction box on every rank, z_reion and T_k slab-resident:
 *       4 of the 12 bytes per cell of mode 1 (C21CM_SHARD_OUTPUT=xH); device arrays only
 *    0  what the finish leaves: every rank its slab (c21cm_ionize_shard_slab) where the finish phase runs
 *       by cell slabs, the owner's box otherwise; scalars (global_xH, mean_f_coll) complete on every rank
 *       of a slab finish
 *   -1  auto: slab-resident where the finish runs by slabs, the owner's box broadcast otherwise
 * c21cm_shard_last_finish_was_slab(): 1 if this process' last c21cm_ionize_sharded finished by slabs. */
int c21cm_shard_set_output(int mode);
int c21cm_shard_output_mode(void);
int c21cm_shard_last_finish_was_slab(void);
int c21cm_ionize_sharded(const c21cm_ionize_spec *spec, const PerturbedField *perturbed_field,
                         const IonizedBox *previous_ionize_box, const TsBox *spin_temp,
                         const HaloBox *halos, IonizedBox *box, c21cm_ionize_report *report,
                         int broadcast, void *stream);

/* filter_box on an explicit geometry: r2c, /N, W(kR) multiply, c2r.
 * reference: src/py21cmfast/src/filtering.c:308-445 (filter_box / test_filter). */
int c21cm_filter_grid(const float *input, float *output, int nx, int ny, int nz, double box_len,
                      double box_len_z, int filter_type, double R, double R_param, void *stream);

/* In-place padded real FFTs (reference: src/py21cmfast/src/dft.c:18-72).
 * `box` is float[nx][ny][2*(nz/2+1)] on the device. */
int c21cm_fft_r2c(float *box, int nx, int ny, int nz, void *stream);
int c21cm_fft_c2r(float *box, int nx, int ny, int nz, void *stream);

/* Scalars of one ComputePerturbedField call
 * (reference: src/py21cmfast/src/PerturbedField.c:24-135,389-496, map_mass.c:146-208). */
typedef struct c21cm_perturb_spec {
    int dim, dim_z;         /* hi-res particle grid (DIM, D_PARA)                         */
    int hii_dim, hii_dim_z; /* low-res output grid (HII_DIM, HII_D_PARA)                  */
    double box_len, box_len_z;
    int perturb_algorithm;  /* enum C21CM_PERTURB_*                                       */
    int perturb_on_high_res;
    int keep_3d_velocities;
    int smooth_evolved_density;
    double density_smooth_radius_mpc; /* Gaussian R handed to filter_box (PerturbedField.c:222-225) */
    double growth_factor;      /* dicke(z)                                                */
    double init_growth_factor; /* dicke(INITIAL_REDSHIFT)                                 */
    double dDdt_over_D;        /* ddickedt(z)/dicke(z)                                    */
} c21cm_perturb_spec;

int c21cm_perturb_grids(const c21cm_perturb_spec *spec, const InitialConditions *ics,
                        PerturbedField *pf, void *stream);

/* Scalars of one ComputeInitialConditions call
 * (reference: src/py21cmfast/src/InitialConditions.c:547-772). */
typedef struct c21cm_ics_spec {
    int dim, dim_z;         /* DIM, D_PARA                                                   */
    int hii_dim, hii_dim_z; /* HII_DIM, HII_D_PARA                                           */
    double box_len, box_len_z;
    float volume;           /* VOLUME macro: float product BOX_LEN^3 * NON_CUBIC_FACTOR      */
    int perturb_algorithm;  /* 2LPT fields only when == C21CM_PERTURB_2LPT                   */
    int perturb_on_high_res;
    int density_is_input;   /* regenerate everything from boxes->hires_density (:620-663)    */
    /* mode sampling (density_is_input == 0), cubic grids only: P(k) tabulated at
     * k = (2 pi / L) sqrt(m), m = 0 .. 3 (DIM/2)^2, in Mpc^3 (power_in_k, cosmology.c:278) */
    int n_m;
    const double *pk_by_m; /* host array */
    unsigned long long seed;
    /* which random stream turns `seed` into delta_k:
     *   C21CM_RNG_PHILOX (0)  counter-based Philox-4x32-10 + Box-Muller on the device (counter =
     *                         mode index: independent of launch geometry and of N_THREADS)
     *   C21CM_RNG_GSL    (1)  the reference's streams -- seed_rng_threads (rng.c:31-90) and two
     *                         gsl_ran_ugaussian per mode from the generator of the OpenMP thread
     *                         that owns the mode's n_x (InitialConditions.c:103-139) -- for
     *                         N_THREADS = rng_threads (1 or 2): same seed, same universe as upstream.
     *                         The acceptance loop runs on the host, ln and sqrt on the device.
     *   C21CM_RNG_GSL_DEVICE (2)  the same streams drawn on the device, one workgroup per stream
     *                         (gsl_stream_kernels.hip): the same accepted pairs, so the same fields bit
     *                         for bit as C21CM_RNG_GSL. */
    int rng_stream;
    int rng_threads;
    /* V_CB_MODEL = FLUCTS (compute_relative_velocities, InitialConditions.c:141-238), cubic grids:
     * sqrt(P_vcb(k) / P(k)) c_kms / k at k = (2 pi / L) sqrt(m), m = 0 .. 3 (DIM/2)^2 (entry 0
     * unused); NULL = no relative velocities.  Output: InitialConditions.lowres_vcb. */
    const double *vcb_by_m;
} c21cm_ics_spec;
enum { C21CM_RNG_PHILOX = 0, C21CM_RNG_GSL = 1, C21CM_RNG_GSL_DEVICE = 2 };

int c21cm_ics_grids(const c21cm_ics_spec *spec, InitialConditions *ics, void *stream);

/* ---- the reference's IC random streams, piece by piece (gsl_stream.c, gsl_stream_kernels.hip) ----
 * kind: 0 mt19937, 1 gfsr4, 2 cmrg, 3 mrg, 4 taus2.  on_device = 0 computes on the host, 1 on the device; the
 * two give the same bits.  Output (and `words`) may be host or device arrays.
 *   raw_words     the first n raw outputs after gsl_rng_set(seed), before zero rejection
 *   accept_pairs  the polar method's compaction alone on caller-supplied words: zero words dropped, survivors
 *                 paired, a pair (a, c) kept iff 0 < x^2 + y^2 <= 1 and stored as a | c << 32; stops after `want`
 *                 pairs.  pairs_out holds min(want, n_words / 2) entries.  *n_words_used: words consumed up to the
 *                 last pair when `want` was reached, else n_words.
 *   stream_pairs  the whole draw of seed_rng_threads(seed) with n_threads streams for nx x ny x nzc modes: two
 *                 pairs per mode in grid order, 2 nx ny nzc entries.  max_pairs_per_launch bounds what one launch
 *                 of the device draw accepts per stream (<= 0: the default); the result does not depend on it.
 *                 tile_cap: the most tiles one launch of the device draw may work through per stream (<= 0:
 *                 derived from the pairs the launch is asked for, several times what they need on average); a
 *                 launch that gets there without its pairs makes the call fail with C21CM_VALUE_ERROR. */
int c21cm_gsl_raw_words(int kind, unsigned long long seed, size_t n, int on_device, unsigned int *out_u32);
int c21cm_gsl_accept_pairs(int kind, const unsigned int *words, size_t n_words, size_t want, int on_device,
                           unsigned long long *pairs_out, size_t *n_pairs, size_t *n_words_used);
int c21cm_gsl_stream_pairs(unsigned long long seed, int n_threads, int nx, int ny, int nzc, int on_device,
                           long long max_pairs_per_launch, long tile_cap, unsigned long long *pairs_out,
                           void *stream);
long long c21cm_gsl_default_pairs_per_launch(void);
/* words per tile of the device draw of generator `kind`; kind -1: of c21cm_gsl_accept_pairs */
int c21cm_gsl_tile_words(int kind);
/* host helpers.  export_state: the state after gsl_rng_set(seed) as 32-bit words, the form the device loads --
 * kinds 2, 3, 4: 6, 5, 3 words (x1..x3 y1..y3 / x1..x5 / s1..s3); kinds 0, 1: a position word, then the 624 state /
 * 16384 ring words.  step (kinds 2, 3, 4): one step, returning the output; jump (kinds 2, 3, 4): n steps at once
 * by matrix powers */
int c21_gsl_export_state(int kind, unsigned long seed, unsigned int *state);
unsigned int c21_gsl_step(int kind, unsigned int *state);
int c21_gsl_jump(int kind, unsigned int *state, unsigned long long n);

/* ---- ComputeBrightnessTemp grid algorithm (BrightnessTemperatureBox.c:22-105) -----------
 * delta_T = const_factor * x_HI * (1 + delta) [mK]; with spin temperatures additionally the
 * optical depth tau_21 and (1 - exp(-tau)) (T_S - T_rad)/(1+z).  Arrays may be host or device.
 * mean_out (optional): the box average the reference logs and checks for finiteness. */
typedef struct c21cm_brightness_spec {
    size_t n_cells;
    double redshift;
    float const_factor; /* 27 (Ob h^2/0.023) sqrt(0.15/(Om h^2) (1+z)/10), float as in :44-49 */
    float T_rad;        /* T_cmb (1+z), float */
    int use_ts_fluct;
} c21cm_brightness_spec;

int c21cm_brightness_grids(const c21cm_brightness_spec *spec, const float *density,
                           const float *neutral_fraction, const float *spin_temperature,
                           float *brightness_temp, float *tau_21, double *mean_out, void *stream);

/* ---- ComputeHaloBox, integrated ("fixed grid") branch: HaloBox.c:302-436 + map_mass.c:214-344 --
 * Each cell of the Lagrangian grid (`hires_density` with PERTURB_ON_HIGH_RES, else
 * `lowres_density`, times the growth factor) gets its expected emissivity and star-formation
 * rate from two 400-bin conditional-mass-function tables (ln N_ion(delta), ln SFRD(delta));
 * the values are moved with the 1LPT/2LPT displacement and CIC-deposited on the HII_DIM grid. */
typedef struct c21cm_halobox_spec {
    int dim, dim_z;         /* grid of the source cells (DIM or HII_DIM) */
    int hii_dim, hii_dim_z; /* output grid */
    double box_len, box_len_z;
    int perturb_on_high_res; /* sources = hires_density + hires_v*, else lowres_density + lowres_v* */
    int lpt2;                /* PERTURB_ALGORITHM == 2LPT */
    double growth_factor, init_growth_factor;
    /* tables over delta = density * growth_factor in [tab_min, tab_min + 399 tab_width]
     * (interp_tables.c:291-405,415-494), evaluated as exp(lerp) */
    double tab_min, tab_width;
    const float *ln_nion_table; /* host, C21CM_NDELTA_TABLE floats */
    const float *ln_sfrd_table; /* host, C21CM_NDELTA_TABLE floats */
    double prefactor_nion, prefactor_sfr; /* map_mass.c:228-239 */
    double prefactor_wsfr;                /* 1 / t_h / t_star, used when whalo_sfr != NULL (:340-346) */
    /* X-ray emissivity grid (USE_TS_FLUCT; HaloBox.c:279-283, map_mass.c:231,316-319): filled
     * when both the table and HaloBox.halo_xray are given */
    const float *ln_xray_table; /* host, C21CM_NDELTA_TABLE floats, or NULL */
    double prefactor_xray;      /* rho_crit Omega_m x volume ratio */
    /* USE_MINI_HALOS (HaloBox.c:245-283, map_mass.c:285-321): per source cell the turnover masses
     * of the cell (grids at the OUTPUT resolution, indexed with the source-cell index as upstream
     * does, map_mass.c:291-292: low-resolution sources only), N_ion of both populations from 2-D
     * tables over (delta, log10 M_turn) on the grids' own ranges, the molecularly cooled SFRD and
     * the X-ray luminosity from 2-D tables on the fixed turnover grid; halo_sfr_mini is filled and
     * n_ion sums both populations.  Tables: host, [NDELTA][NMTURN] floats (ln values). */
    int use_mini_halos;
    const float *log10_mturn_acg, *log10_mturn_mcg; /* [N out], host or device */
    const float *ln_nion_table2d, *ln_nion_mini_table2d;
    double mta_min, mta_width, mtm_min, mtm_width;
    const float *ln_sfrd_mini_table2d, *ln_xray_table2d; /* the second one NULL without halo_xray */
    double mt_fixed_min, mt_fixed_width;
    double prefactor_nion_mini, prefactor_sfr_mini;
    /* Halo-catalogue branch (sum_halos_onto_grid, HaloBox.c:518-560; move_halo_galprops,
     * map_mass.c:346-476): every halo of non-zero mass is displaced with the velocities of its
     * Lagrangian cell, gets its properties (set_halo_properties, HaloBox.c:62-102; with mini-halos
     * the turnover masses CIC-read at its position) and is CIC-deposited per unit cell volume; the
     * integrated branch above then adds the sources below the catalogue's mass limit unless
     * `skip_integral` (HaloBox.c:635: M_min >= the limit; the tables are not read then and, with a
     * recombination model, whalo_sfr comes from the halos instead of n_ion). */
    const HaloCatalog *halos; /* NULL: integrated branch only; arrays host or device */
    const struct c21cm_halo_consts *halo_consts;
    int skip_integral;
} c21cm_halobox_spec;

/* the ScalingConstants read by set_halo_properties (scaling_relations.c:29-118,331-500) */
typedef struct c21cm_halo_consts {
    double redshift;
    double fstar_10, alpha_star, sigma_star;
    double alpha_upper, pivot_upper, upper_pivot_ratio;
    double fstar_7, alpha_star_mini, acg_thresh;
    double baryon_ratio; /* OMb / OMm */
    double t_h, t_star, sigma_sfr_lim, sigma_sfr_idx;
    double l_x, l_x_mini, sigma_xray; /* L_X in 1e38 erg/s */
    double fesc_10, fesc_7, alpha_esc, pop2_ion, pop3_ion;
    double mturn_a_nofb, mturn_m_nofb; /* the turnovers without mini-halos */
    int scaling_median;                /* HALO_SCALING_RELATIONS_MEDIAN */
    int upper_stellar_turnover;        /* USE_UPPER_STELLAR_TURNOVER */
    int use_mini_halos, use_xray;      /* USE_MINI_HALOS, USE_TS_FLUCT */
} c21cm_halo_consts;

int c21cm_halobox_grids(const c21cm_halobox_spec *spec, const InitialConditions *ics,
                        HaloBox *grids, void *stream);

/* get_log10_turnovers (HaloBox.c:465-516): the two log10 turnover grids of a USE_MINI_HALOS HaloBox
 * and their averages.  Atomic: max(M_acg, M_TURN, reionisation feedback) -- upstream keeps this one
 * as a RUNNING maximum within each OpenMP thread's share of the cells (:481,497), which `n_threads`
 * reproduces for libgomp's static schedule; molecular: max(M_LW, M_TURN, feedback) per cell.
 * The spec's mturn_m_nofb and first_snapshot are not read; below_z_heat_max: :488-492. */
int c21cm_halobox_turnovers(const c21cm_mturn_spec *spec, double m_turn, int below_z_heat_max,
                            int n_threads, const float *prev_G12, const float *prev_z_reion,
                            const float *J_21_LW, const float *vcb, float *log10_mturn_acg,
                            float *log10_mturn_mcg, double averages[2], void *stream);

/* ---- ComputePerturbedHaloCatalog: PerturbedHaloCatalog.c:25-149 + convert_halo_props
 * (HaloBox.c:781-880) with explicit scalars.  Every halo of `halos` is displaced by
 * v[cell] * velocity_displacement_factor (2LPT: minus v2[cell] * velocity_displacement_factor_2lpt),
 * `cell` the nearest cell of the velocity grid (hires_v* on dim x dim x dim_z with
 * perturb_on_high_res, else lowres_v* on hii_dim x hii_dim x hii_dim_z), wrapped into
 * {box_len, box_len, box_len_z} in fp64 and stored as float: out->halo_coords, for every halo.
 * Halos of non-zero mass then get set_halo_properties: with consts->use_mini_halos the turnover
 * masses are 10^CIC-read of the two log10 grids [hii_dim, hii_dim, hii_dim_z] at the stored
 * coordinate times hii_dim / dim (upstream's scale, HaloBox.c:825-827), else the constants.
 * Required outputs: halo_coords, halo_masses, stellar_masses, sfr, ion_emissivity.  Written where
 * non-NULL: fesc_sfr; xray_emissivity (consts->use_xray only); stellar_mini, sfr_mini
 * (consts->use_mini_halos only).  Rows of zero-mass halos keep their property values.  Sets
 * out->n_halos; n_halos == 0 launches nothing.  Catalogue arrays and grids: host or device. */
typedef struct c21cm_perturb_halos_spec {
    int dim, dim_z;         /* high-resolution grid */
    int hii_dim, hii_dim_z; /* low-resolution grid (the turnover grids) */
    double box_len, box_len_z;
    int perturb_on_high_res; /* velocities: hires_v*, else lowres_v* */
    int lpt2;                /* PERTURB_ALGORITHM == 2LPT */
    double velocity_displacement_factor;      /* D(z) - D(z_init) */
    double velocity_displacement_factor_2lpt; /* D2(z) - D2(z_init), D2 = -3/7 D^2 */
} c21cm_perturb_halos_spec;

int c21cm_perturb_halos_grids(const c21cm_perturb_halos_spec *spec, const c21cm_halo_consts *consts,
                              const InitialConditions *ics, const float *log10_mturn_acg,
                              const float *log10_mturn_mcg, const HaloCatalog *halos,
                              PerturbedHaloCatalog *out, void *stream);

/* ---- the halo sampler (SOURCE_MODEL = CHMF-SAMPLER): Stochasticity.c:663-1113 with explicit scalars.
 * Every condition -- a descendant halo (from_catalog) or a cell of the low-resolution density field --
 * samples the conditional mass function of its tables and appends its halos to `out` in condition order,
 * then draw order (the reference's order at N_THREADS = 1; grid mode copies `large` to the front first).
 *
 * Random numbers.  NOT the reference's GSL streams: every uniform and Gaussian deviate is word(s) of one
 * Philox-4x32-10 block with key = seed + (uint64)(redshift * 1000) and counter = {draw index, purpose,
 * condition index low, high}; the purposes are the C21CM_HS_DRAW_* below.  A catalogue therefore depends
 * on nothing but the inputs: not on launch geometry, and not on which condition ran first.  It is another,
 * equally valid realisation than the reference's.
 *
 * Two passes: pass A samples every condition and keeps four words of it (halos kept, draws made, its row in its block, draws
 * removed + flags); an exclusive scan gives the offsets and the total; pass B repeats the same draws and
 * writes.  total > out->buffer_size: ValueError, nothing written.  A condition that needs more than
 * max_halo_cell draws (or a descendant mass outside [m_min, m_max_tables]): ValueError naming the
 * condition.  On success out->n_halos is set and the five arrays are zero from n_halos to buffer_size.
 *
 * tables (doubles, host or device): [nhalo n_cond][mcoll n_cond][sigma n_cond][inverse n_cond * n_prob]:
 * expected N / M_cond and M / M_cond per unit condition mass on the nodes x_min + i x_width (delta for
 * cells, ln M for descendants), sigma(M) on the same nodes (descendants only, else zeros), and the inverse
 * CDF M / M_cond on those rows times the columns ln p = p_min + k p_width.  c21cm_sampler_setup builds
 * them from the broadcast globals.  Sums that decide control flow (the mass-limited loop and its
 * removals) are kept as 64-bit integers of the float-rounded masses in units of 1 Msun: a float >= 2^24
 * is an integer, so the sums are exact and do not depend on the order of the additions. */
enum { C21CM_HS_DRAW_MASS = 0, C21CM_HS_DRAW_SELECT = 1, C21CM_HS_DRAW_PERMUTE = 2, C21CM_HS_DRAW_POISSON = 3,
       C21CM_HS_DRAW_POSITION = 4, C21CM_HS_DRAW_POSITION2 = 5, C21CM_HS_DRAW_PROPS = 6, C21CM_HS_DRAW_PROPS2 = 7,
       C21CM_HS_DRAW_DEXM = 8 /* the deviates of a DexM halo: counter {0, 8, hi-res cell index low, high} */ };
#define C21CM_MAX_HALO_CELL 100000 /* Stochasticity.h MAX_HALO_CELL */
typedef struct c21cm_sample_halos_spec {
    int from_catalog;  /* 1: conditions are the halos of `desc`; 0: the cells of `density` */
    int sample_method; /* 0 MASS-LIMITED, 1 NUMBER-LIMITED; cells are always number-limited */
    int hmf;           /* C21CM_HMF_PS or C21CM_HMF_ST */
    int hii_dim, hii_dim_z;
    int n_cond, n_prob;
    int max_halo_cell; /* draws per condition before ValueError; <= 0: C21CM_MAX_HALO_CELL */
    int path;          /* 0: a wave takes the conditions that expect >= 64 halos (not tuned); 1 / 2: every
                        * condition on the thread / the wave path.  The catalogue does not depend on it. */
    unsigned long long seed;
    double redshift, redshift_desc;
    double box_len, box_len_z;
    double growth_out, growth_in;
    double m_min, m_max_tables;          /* SAMPLER_MIN_MASS / SAMPLER_BUFFER_FACTOR, M_MAX_INTEGRAL */
    double sampler_min_mass;             /* halos below it are drawn but not stored (compared as floats) */
    double halomass_correction;
    double corr_star, corr_sfr, corr_xray; /* exp(-dz / CORR_*), 0 where CORR_* <= 0 */
    double m_cell, sigma_cell;           /* cells: the condition mass and sigma(m_cell) */
    double rtom_unit;                    /* mass of a sphere of radius 1 Mpc: R(M) = cbrt(M / rtom_unit) */
    double x_min, x_width, p_min, p_width;
    const double *tables;
} c21cm_sample_halos_spec;

/* stoc_set_consts_z (Stochasticity.c:77-155) from the broadcast globals: every scalar of the spec, and
 * `tables` pointing at library-owned host tables that stay valid until the next call.  redshift_desc > 0:
 * descendants.  The tables of one snapshot are cached under the exact values of the two redshifts: a caller
 * that names one snapshot once as a float widened to double (ComputeHaloCatalog does) and once as a double
 * builds them twice, so use one spelling per snapshot.  c21cm_sample_halos_last_counts below reads state of
 * the last call and is not for concurrent callers.  ValueError for redshift < redshift_desc and for options outside HMF = PS / ST,
 * SAMPLE_METHOD = MASS-LIMITED / NUMBER-LIMITED, USE_INTERPOLATION_TABLES = hmf-interpolation. */
int c21cm_sampler_setup(double redshift, double redshift_desc, unsigned long long seed,
                        c21cm_sample_halos_spec *spec);
/* density: float[hii_dim^2 hii_dim_z], the z = 0 field (multiplied by growth_out); overlap (may be NULL):
 * the fraction of each cell inside `large` halos; large (may be NULL); desc: read with from_catalog only.
 * Arrays host or device. */
int c21cm_sample_halos_grids(const c21cm_sample_halos_spec *spec, const float *density, const float *overlap,
                             const HaloCatalog *large, const HaloCatalog *desc, HaloCatalog *out,
                             void *stream);
/* halos kept per condition by the last c21cm_sample_halos_grids call, into a host array.  ValueError unless
 * that call succeeded, sampled exactly n conditions and the workspace has not been released since. */
int c21cm_sample_halos_last_counts(unsigned long long n, int *counts);
/* the reference's DexM radius ladder (HaloCatalog.c:156-200) without a field: 1 when every scale is
 * skipped as rarer than 7 sigma, i.e. DexM would find nothing at this redshift in this box */
int c21cm_dexm_is_empty(double redshift);

/* ---- the DexM halo finder (HaloCatalog.c:38-456, check_halo, pixel_in_halo) with explicit scalars.
 * The hi-res density is filtered on a descending ladder of radii; on each rung the reference walks the box
 * serially in raster order and a cell with delta_m > delta_crit becomes a halo unless its own cell is in
 * a halo already or a cell in a halo lies within r_overlap * R of it; an accepted halo paints its sphere.
 * The result depends on the scan order.  Here the rung's candidates are compacted in raster order and
 * decided in rounds that give the serial result exactly: a candidate that fails the mask
 * test is rejected for good; one that passes and has no undecided earlier candidate within the range in
 * which a halo of this rung can change its test is accepted; the accepted spheres are painted; repeat.
 * A rung that is not finished after C21CM_DEXM_ROUND_CAP rounds is finished by one workgroup that walks
 * the undecided candidates serially.
 *
 * Rows of `out` are in raster order of the hi-res cell: mass = the rung's M, coordinates = index *
 * (BOX_LEN / DIM), the three deviates standard normals from one Philox block per halo (key as the sampler's,
 * purpose C21CM_HS_DRAW_DEXM, counter the cell index).  total > out->buffer_size: ValueError, nothing written.
 * On success the five arrays are zero from n_halos to buffer_size. */
#define C21CM_MAX_DEXM_RADII 256
#define C21CM_DEXM_ROUND_CAP 64  /* rounds per rung before the serial tail takes the rest (not tuned) */
#define C21CM_DEXM_ROUND_BATCH 8 /* rounds between two readbacks of the undecided count */
typedef struct c21cm_find_halos_spec {
    int dim, dim_z;         /* the hi-res grid [dim][dim][dim_z] */
    int hii_dim, hii_dim_z; /* the overlap box; 0: none */
    int halo_filter;        /* 0 real-space top-hat, 1 sharp-k, 2 Gaussian */
    int n_R;
    int optimize;      /* DEXM_OPTIMIZE */
    int filtered_mode; /* 0: `filtered` unused; 1: read (no transform runs); 2: written */
    int path;          /* 0: rounds, then the serial tail; 1: serial only; 2: rounds only */
    unsigned long long seed;
    double redshift;
    double box_len, box_len_z;
    double growth;           /* dicke(z) as the reference's float */
    double r_overlap;        /* DEXM_R_OVERLAP */
    double optimize_minmass; /* DEXM_OPTIMIZE_MINMASS */
    double rtom_unit;        /* mass of a sphere of radius 1 Mpc: MtoR(M) = cbrt(M / rtom_unit) */
    float R[C21CM_MAX_DEXM_RADII], mass[C21CM_MAX_DEXM_RADII], delta_crit[C21CM_MAX_DEXM_RADII];
} c21cm_find_halos_spec;

typedef struct c21cm_find_halos_report {
    int n_R;
    unsigned long long n_halos;
    /* per rung: candidates (cells over the threshold whose own cell is free), accepted halos, rounds run,
     * 1 where the serial workgroup ran (path 1, or the tail after the round cap) */
    unsigned int candidates[C21CM_MAX_DEXM_RADII], accepted[C21CM_MAX_DEXM_RADII];
    int rounds[C21CM_MAX_DEXM_RADII], tail[C21CM_MAX_DEXM_RADII];
    /* wall-clock milliseconds per phase, filled only when C21CM_DEXM_TIMING=1 drains the stream around each */
    double ms[5];
} c21cm_find_halos_report;
enum { C21CM_DEXM_MS_TRANSFORMS = 0, C21CM_DEXM_MS_COMPACTION = 1, C21CM_DEXM_MS_DECIDE = 2, C21CM_DEXM_MS_PAINT = 3,
       C21CM_DEXM_MS_SERIAL = 4 };

/* HaloCatalog.c:81-200 from the broadcast globals: the kept rungs (R, M, delta_crit; those rarer than
 * 7 sigma skipped), the growth factor and the options.  n_R == 0 exactly where c21cm_dexm_is_empty.
 * Parameters that describe no box: ValueError at once; more than C21CM_MAX_DEXM_RADII rungs: ValueError. */
int c21cm_dexm_ladder(double redshift, c21cm_find_halos_spec *spec);
/* hires_density [dim^2 dim_z] (the z = 0 field; unused with filtered_mode 1); filtered [n_R][N] (test hook,
 * see filtered_mode: the values are delta_m, already times growth); in_halo (may be NULL) [N] bytes, 1 inside
 * a halo; overlap (NULL unless hii_dim > 0) [hii_dim^2 hii_dim_z]: the fraction of each low-res cell inside
 * halos (HaloCatalog.c:361-420).  Arrays host or device. */
int c21cm_find_halos_grids(const c21cm_find_halos_spec *spec, const float *hires_density, float *filtered,
                           HaloCatalog *out, unsigned char *in_halo, float *overlap, void *stream);
/* the report of the last c21cm_find_halos_grids call (also of one that stopped at the buffer check) */
void c21cm_find_halos_last_report(c21cm_find_halos_report *report);

/* min and max of n floats (host or device array), e.g. the table range of the above */
int c21cm_grid_minmax(const float *values, size_t n, double out_minmax[2], void *stream);

/* ---- spin-temperature filtering stage --------------------------------------
 * The two filter loops of the spin-temperature calculation, on the same transform passes as
 * the excursion-set loop.
 *
 * c21cm_fill_Rbox_grids: prepare_filter_boxes + fill_Rbox_table (SpinTemperatureBox.c:502-520,
 * 560-636).  `input` [N] is transformed once (r2c, / N); for every radius the spectrum is
 * multiplied by window `filter_type` (HEAT_FILTER) at R -- radii not above `cell_radius`
 * (L_FACTOR BOX_LEN / HII_DIM) are left unfiltered (:585-588) -- transformed back, floored at
 * `min_value` (before the constant factor, :617-620), multiplied by `const_factor` and stored
 * to result[r * N ...]; min_arr / average_arr / max_arr [n_R] get the statistics of the stored
 * values.  Arrays may be host or device. */
#define C21CM_MAX_TS_RADII 128
typedef struct c21cm_rbox_spec {
    int hii_dim, hii_dim_z;
    double box_len, box_len_z;
    int filter_type;
    int n_R;
    double R[C21CM_MAX_TS_RADII];
    double cell_radius;
    double min_value, const_factor;
} c21cm_rbox_spec;

int c21cm_fill_Rbox_grids(const c21cm_rbox_spec *spec, const float *input, float *result,
                          double *min_arr, double *average_arr, double *max_arr, void *stream);

/* c21cm_annular_filter_grids: one_annular_filter (SpinTemperatureBox.c:642-742) for n_grids
 * grids of one shell: r2c, / N, window filter_type[g] (4 = spherical shell, 5 = multiple
 * scattering) between R_inner and R_outer unless R_inner <= 0, c2r, negative values (aliasing)
 * set to zero.  u_avg / f_avg [n_grids]: box averages of the input and of the output. */
#define C21CM_MAX_ANNULAR_GRIDS 5
typedef struct c21cm_annular_spec {
    int hii_dim, hii_dim_z;
    double box_len, box_len_z;
    double R_inner, R_outer, R_star;
    int n_grids;
    int filter_type[C21CM_MAX_ANNULAR_GRIDS];
} c21cm_annular_spec;

int c21cm_annular_filter_grids(const c21cm_annular_spec *spec, const float *const *inputs,
                               float *const *outputs, double *u_avg, double *f_avg,
                               void *stream);

/* ---- spin temperature: the per-cell part of ComputeTsBox ---------------------------------------
 * reference: src/py21cmfast/src/SpinTemperatureBox.c
 *   :892-927    init_first_Ts   (redshift >= Z_HEAT_MAX)      -> c21cm_ts_first_grids
 *   :1010-1086  calculate_sfrd_from_grid                      -> source_mode SFRD_TABLE
 *   :1210-1383  get_Ts_fast     (x_e, T_k update and T_s)     -> the cell epilogue
 *   :1499-1522  x_e interpolation index per cell
 *   :1541-1784  the R loop: SFR of every shell -> dxheat / dxion / dxlya / dstarlya sums
 *   :1794-1848  prefactors of the sums, get_Ts_fast, outputs
 * Everything that depends on the cosmology, on the spectra or on the frequency integrals is a
 * scalar or a small table of this struct (the host builds them: heating.c); the library kernel
 * and the oracle evaluate the same formulae on the same numbers.
 *
 * source_mode C21CM_TS_SRC_GRIDS: the shells' star-formation and X-ray grids are given
 *   (XraySourceBox.filtered_sfr / filtered_xray [n_step][N], Lagrangian source models);
 * source_mode C21CM_TS_SRC_SFRD_TABLE: `filtered_density` [n_step][N] (fill_Rbox_table's
 *   delNL0, i.e. linearly extrapolated to z = 0) is turned into an SFRD per shell through
 *   exp(lerp(ln_sfrd_tables[R], delta zpp_growth[R])) (1 + delta zpp_growth[R]), normalised to
 *   mean_sfr_zpp[R] over the box mean of the table values (avg_fix_term, :1624);
 * source_mode C21CM_TS_SRC_FCOLL_TABLES (CONST-ION-EFF): two linear tables per shell, the
 *   conditional collapsed fraction (`fcoll_tables`, its box mean normalises) and its redshift
 *   derivative (`dfcoll_tables`, the source: (1 + delta) dfcoll/dz, :1067-1072). */
#define C21CM_X_INT_NXHII 14 /* elec_interp.h:5 */
#define C21CM_X_INT_XHII                                                                        \
    { 1.0e-4f, 2.318e-4f, 4.677e-4f, 1.0e-3f, 2.318e-3f, 4.677e-3f, 1.0e-2f, 2.318e-2f, 4.677e-2f, \
      1.0e-1f, 0.5f, 0.9f, 0.99f, 0.999f } /* elec_interp.c:57-70 */
#define C21CM_LYA_NT 101  /* heating_helper_progs.c:50-55: log10 T_k, log10 T_s in [-1, 3] */
#define C21CM_LYA_NGP 51  /* log10 tau_GP in [1, 7] */
#define C21CM_TS_MAX_TK 5e4 /* SpinTemperatureBox.c:30 */
enum { C21CM_TS_SRC_GRIDS = 0, C21CM_TS_SRC_SFRD_TABLE = 1, C21CM_TS_SRC_FCOLL_TABLES = 2 };

typedef struct c21cm_ts_spec {
    int hii_dim, hii_dim_z;
    int n_step;      /* N_STEP_TS, <= C21CM_MAX_TS_RADII */
    int source_mode; /* C21CM_TS_SRC_* */
    int use_xray_heating, use_cmb_heating, use_lya_heating;
    int no_light;    /* global_reion_properties: nothing has formed yet, the sums stay zero */
    double redshift; /* z' */
    double dzp;      /* z' - previous z' (negative) */
    double growth_ratio; /* dicke(z') / dicke(perturbed_field_redshift) */
    /* constants (Constants.c / Constants.h:98-112 with the run's cosmology) */
    double No, N_b0, h_frac, he_frac;
    double k_B, h_p, m_p, c_cms, A10, T_21, lambda_21, nu_Ly_alpha;
    double clumping_factor;
    /* set_zp_consts (:1098-1184) */
    double xray_prefactor, Trad, Ts_prefactor, xa_tilde_prefactor, xc_inverse, dcomp_dzp_prefactor;
    double Nb_zp, N_zp, lya_star_prefactor, volunit_inv, hubble_zp, growth_zp, dgrowth_dzp, dt_dzp;
    /* per shell */
    double z_edge_factor[C21CM_MAX_TS_RADII]; /* :1546-1553 */
    double xray_R_factor[C21CM_MAX_TS_RADII]; /* (1 + z'')^-X_RAY_SPEC_INDEX */
    double starlya_prefactor[C21CM_MAX_TS_RADII];  /* dstarlya_dt_prefactor */
    double lya_cont_prefactor[C21CM_MAX_TS_RADII]; /* dstarlya_cont_dt_prefactor */
    double lya_inj_prefactor[C21CM_MAX_TS_RADII];  /* dstarlya_inj_dt_prefactor */
    /* C21CM_TS_SRC_SFRD_TABLE */
    double zpp_growth[C21CM_MAX_TS_RADII];
    double mean_sfr_zpp[C21CM_MAX_TS_RADII];
    double tab_min[C21CM_MAX_TS_RADII], tab_width[C21CM_MAX_TS_RADII];
    const float *ln_sfrd_tables; /* host, [n_step][C21CM_NDELTA_TABLE] */
    const float *fcoll_tables, *dfcoll_tables; /* C21CM_TS_SRC_FCOLL_TABLES, same shape */
    double sfr_scale;            /* F_STAR10 */
    double xray_scale;           /* L_X s_per_yr */
    /* fill_freqint_tables (:810-889): host, [C21CM_X_INT_NXHII][n_step] each */
    const double *freq_int_heat, *freq_int_ion, *freq_int_lya;
    /* Energy_Lya_heating's two tables, host, [NT][NT][NGP]; needed with use_lya_heating */
    const double *lya_dEC, *lya_dEI;
    /* USE_MINI_HALOS with C21CM_TS_SRC_SFRD_TABLE (SpinTemperatureBox.c:1011-1075,1642-1716): the
     * molecularly cooled population adds, per shell, a star-formation term from a 2-D table
     * (overdensity x log10 of the shell-filtered Lyman-Werner turnover mass), its own Lyman-alpha
     * prefactors and X-ray luminosity, and both populations feed the Lyman-Werner background
     * written to TsBox.J_21_LW (:1843-1845). */
    int use_mini_halos;
    double starlya_prefactor_mini[C21CM_MAX_TS_RADII];
    double lya_cont_prefactor_mini[C21CM_MAX_TS_RADII], lya_inj_prefactor_mini[C21CM_MAX_TS_RADII];
    double lw_prefactor[C21CM_MAX_TS_RADII], lw_prefactor_mini[C21CM_MAX_TS_RADII];
    double mean_sfr_zpp_mini[C21CM_MAX_TS_RADII];
    const float *ln_sfrd_tables_mini; /* host, [n_step][C21CM_NDELTA_TABLE][C21CM_NMTURN_TABLE] */
    double mturn_tab_min, mturn_tab_width; /* LOG10_MTURN_MIN and the bin width (interp_tables.c:29-30) */
    double sfr_scale_mini;  /* F_STAR7_MINI   */
    double xray_scale_mini; /* L_X_MINI s_per_yr */
    const float *filtered_log10_mcrit; /* [n_step][N]: fill_Rbox_table of log10 M_crit,LW (:1459-1466) */
} c21cm_ts_spec;

typedef struct c21cm_ts_report { /* box means, as the reference logs them at DEBUG level */
    double Ts_ave, Tk_ave, x_e_ave, J_alpha_ave, xheat_ave, xion_ave;
    double ave_sfrd[C21CM_MAX_TS_RADII]; /* SFRD_TABLE: mean table value per shell */
    double ave_sfrd_mini[C21CM_MAX_TS_RADII]; /* USE_MINI_HALOS */
} c21cm_ts_report;

/* prepare_filter_boxes with USE_MINI_HALOS (SpinTemperatureBox.c:535-565): per cell
 * log10(max(M_LW(z, J_21_LW, v_cb), M_TURN)) from the previous TsBox's J_21_LW (vcb NULL:
 * vcb_const); the spec's reionisation / no-feedback fields are not read. */
int c21cm_ts_mcrit_grid(const c21cm_mturn_spec *spec, double m_turn, const float *J_21_LW,
                        const float *vcb, float *log10_mcrit, void *stream);

/* `density` [N]: PerturbedField.density; `previous` holds the three boxes of the previous
 * snapshot; `source_box` (GRIDS) or `filtered_density` (SFRD_TABLE) as described above; `out`
 * receives spin_temperature, kinetic_temp_neutral, xray_ionised_fraction.  Arrays may be host
 * or device.  A non-finite spin temperature gives C21CM_INFINITY_OR_NAN_ERROR (:1884-1904). */
int c21cm_ts_grids(const c21cm_ts_spec *spec, const float *density, const TsBox *previous,
                   const XraySourceBox *source_box, const float *filtered_density, TsBox *out,
                   c21cm_ts_report *report, void *stream);
/* the cell part alone (ts_driver.c): the shell loop of a spec's shells into sums_dev ([6][N]), and
 * the temperature update of cells [cell0, cell0 + ncell) from sums ([6][ncell]) */
int c21cm_ts_shell_sums(const c21cm_ts_spec *spec, const float *density, const TsBox *previous,
                        const XraySourceBox *source_box, const float *filtered_density,
                        double *sums_dev, void *stream);
int c21cm_ts_cells_from_sums(const c21cm_ts_spec *spec, const float *density, const TsBox *previous,
                             const double *sums_dev, size_t cell0, size_t ncell, TsBox *out,
                             void *stream);

/* init_first_Ts: T_k = TK (1 + cT_ad delta), x_e = xe, T_s from collisions only. */
typedef struct c21cm_ts_first_spec {
    int hii_dim, hii_dim_z;
    double redshift;          /* z' of the requested box */
    double perturbed_redshift; /* get_Ts is called with this one (:923) */
    float inverse_growth_factor_z, growth_factor_zp; /* floats upstream (:896-897) */
    double xe, TK, cT_ad;
    double No, N_b0, A10, T_21, T_cmb;
} c21cm_ts_first_spec;
int c21cm_ts_first_grids(const c21cm_ts_first_spec *spec, const float *density, TsBox *out,
                         void *stream);

/* ---- Rectilinear lightcone (lightconers.py:162-319,483-529; drivers/lightcone.py:544-575) ----
 * One call fills slices [i0, i1) of up to C21CM_LC_MAX_FIELDS lightcones from the two node boxes
 * that bracket them: value = (w_lo[j] box_lo + w_hi[j] box_hi) / w_norm at plane plane[j] of the
 * boxes (fp64, stored as fp32); bit f of mean_max selects z_reion's rule (where box_lo * box_hi < 0
 * the larger of the two).  The host derives the per-slice tables (coeval_subselect,
 * redshift_interpolation); the kernel never does.  Node boxes are float[hii_dim][hii_dim][hii_d_para],
 * lightcones float[hii_dim][hii_dim][n_slices]; each pointer may be host or device memory (a host
 * lightcone receives the run of slices as a 2-D copy). */
#define C21CM_LC_MAX_FIELDS 16
typedef struct c21cm_lightcone_spec {
    int hii_dim;        /* columns per side */
    int hii_d_para;     /* planes of a node box along the line of sight */
    int n_slices;       /* length of the lightcone */
    int i0, i1;         /* slices filled by this call, 0 <= i0 < i1 <= n_slices */
    int n_fields;       /* 1 .. C21CM_LC_MAX_FIELDS */
    unsigned mean_max;  /* bit f: field f interpolates with mean_max */
    const int *plane;   /* host, i1 - i0 entries, each in [0, hii_d_para) */
    const double *w_lo; /* host, i1 - i0: |dc_hi - d| (pixels) */
    const double *w_hi; /* host, i1 - i0: |dc_lo - d| */
    double w_norm;      /* |dc_lo - dc_hi| > 0 */
} c21cm_lightcone_spec;

int c21cm_lightcone_slab_grids(const c21cm_lightcone_spec *spec, const float *const *box_lo,
                               const float *const *box_hi, float *const *lightcone, void *stream);

/* brightness_temp lightcone corrected in place by the line-of-sight velocity gradient
 * (rsds.py:16-103, periodic = False): np.gradient(los_velocity, dx, edge_order = 2) along the last
 * axis, then 1/|1 + clip(dv/dx, +-max_dvdr H)/H| or, with use_ts_fluct, the fp64 tau_21 form
 * (1 - e^(-tau/g)) / (1 - e^(-tau)), 1 where tau < 1e-10.  n_slices >= 3. */
typedef struct c21cm_dvdr_spec {
    int hii_dim;
    int n_slices;
    double dx;             /* BOX_LEN / HII_DIM [Mpc] */
    double max_dvdr;       /* AstroParams.MAX_DVDR */
    int use_ts_fluct;      /* tau_21 required */
    const double *hubble;  /* host, n_slices: H(z) of every slice [1/s] */
} c21cm_dvdr_spec;

int c21cm_lightcone_dvdr_grids(const c21cm_dvdr_spec *spec, float *brightness_temp,
                               const float *los_velocity, const float *tau_21, void *stream);

/* ---- Redshift-space distortions (rsds.py:106-255 apply_rsds / rsds_shift) ----
 * Every column of n_slices cells (the line of sight is the fastest axis; columns float[n_cols][n_slices])
 * of each field is moved by los_velocity * disp_scale[j] pixels: the displacement is interpolated
 * linearly onto n_sub sub-cells per slice, each sub-cell is deposited by linear cloud-in-cell and the
 * sub-cells are summed back (periodic: modulo the column; else what leaves [0, n_slices) is lost).
 * Deterministic: 64-bit fixed-point sums.  Pointers may be host or device memory, mixed; out[q] may
 * alias fields[q].  A non-finite field or velocity value is C21CM_INFINITY_OR_NAN_ERROR. */
typedef struct c21cm_rsd_spec {
    long long n_cols;          /* columns (HII_DIM^2 for a box or a rectilinear lightcone) */
    int n_slices;              /* >= 2 */
    int n_fields;              /* >= 1; launches take up to 16 at a time */
    int n_sub;                 /* n_rsd_subcells >= 1 */
    int periodic;              /* 1: coeval boxes, 0: lightcones */
    const double *disp_scale;  /* host, n_slices: pixels per unit of los_velocity, 1 / (H(z_j) cell) */
} c21cm_rsd_spec;

int c21cm_rsd_shift_grids(const c21cm_rsd_spec *spec, const float *const *fields, float *const *out,
                          const float *los_velocity, void *stream);

/* ---- Power spectra of boxes and lightcone chunks ----
 * n_batch boxes of nx x ny x nz cells, box b at field[batch_offsets[b] + (i ny + j) row_pitch + l]
 * (row_pitch = nz for a dense box; chunks of a lightcone of n_slices: row_pitch = n_slices, offset = the
 * chunk's first slice), each of lengths Lx, Ly, Lz.  F = (V/N) DFT(f) (fp32 transform), P = |F|^2 / V, or
 * Re(F F2*) / V when field2 is given (same layout).  Every mode of the full grid with its wavenumber
 * k = numpy's fftfreq(n, L/n) 2 pi per axis is binned with np.digitize on the given edges: |k| =
 * sqrt((kx^2 + ky^2) + kz^2) (fp64), or k_perp = sqrt(kx^2 + ky^2) and k_par = |kz| (cylindrical); each bin
 * is the plain mean.  Outputs (host or device): power[n_batch][n_bins (* n_bins_par)], kmean[n_batch][...]
 * (mean |k| per bin; cylindrical: mean k_perp per k_perp bin, then mean k_par per k_par bin), counts (modes
 * per bin); empty bins are NaN.  Deterministic: two calls give the same bits.  Pointers may be host or device
 * memory.  A non-finite field value (or transform output) is C21CM_INFINITY_OR_NAN_ERROR; nothing is written. */
typedef struct c21cm_power_bins {
    int cylindrical;           /* 0: |k| bins; 1: (k_perp, k_par) bins */
    int n_bins;                /* |k| (or k_perp) bins >= 1 */
    int n_bins_par;            /* k_par bins >= 1 (cylindrical) */
    const double *edges;       /* host, n_bins + 1, increasing */
    const double *edges_par;   /* host, n_bins_par + 1, increasing (cylindrical) */
    int ignore_zero_mode;      /* drop k = 0 */
    int ignore_kperp_zero;     /* drop kx = ky = 0 */
    int ignore_kpar_zero;      /* drop kz = 0 */
} c21cm_power_bins;

int c21cm_power_spectrum_grids(const float *field, const float *field2, int nx, int ny, int nz, int n_batch,
                               long long row_pitch, const long long *batch_offsets, double Lx, double Ly,
                               double Lz, const c21cm_power_bins *bins, double *power, double *kmean,
                               long long *counts, void *stream);

/* The options of c21cm_power_spectrum_ex_grids; NULL, or all of them off, is c21cm_power_spectrum_grids.
 * Taper: with any window_* given the packed field is f' = (f - m) wx[i] wy[j] wz[l] (m the box mean, a NULL
 * window is 1), the mean is NOT put back onto k = 0 and the power is multiplied by inv_mean_w2 = 1 / (mean(wx^2)
 * mean(wy^2) mean(wz^2)).  The device multiplies by the fp32 roundings of wz[l] and of wx[i] wy[j] (formed in
 * fp64).  Cuts (spherical bins only; fp64 + - x in this order, so numpy makes the same decisions): with x = (kx kx
 * + ky ky) + kz kz a mode is used iff kz kz >= mu_min_sq x and kz kz <= mu_max_sq x (use_mu), and, with a = |kz|
 * - wedge_buffer, iff a >= 0 and a a >= wedge_slope_sq (kx kx + ky ky) (use_wedge).  A cut mode counts nowhere;
 * cuts combine with the ignore flags and never move edges.  want_variance: variance[n_batch][bins] = the
 * population variance of the per-mode power over the modes of the full grid in the bin, sum(w P^2) / sum(w) -
 * (sum(w P) / sum(w))^2 in fp64 (cross spectra: P = Re(F F2*) / V), NaN in empty bins; it costs LDS, so at most
 * 1084 |k| bins or 877 k_par bins (1417 / 1084 without).  Errors are C21CM_VALUE_ERROR with a message. */
typedef struct c21cm_power_opts {
    const double *window_x;    /* host, nx weights, or NULL */
    const double *window_y;    /* host, ny weights, or NULL */
    const double *window_z;    /* host, nz weights, or NULL */
    double inv_mean_w2;        /* 1 / <W^2> (used with a window) */
    double mu_min_sq;          /* mu_min^2, 0 <= . <= mu_max_sq <= 1 */
    double mu_max_sq;
    int use_mu;
    double wedge_slope_sq;     /* slope^2 >= 0 */
    double wedge_buffer;       /* >= 0, in the units of k */
    int use_wedge;
    int want_variance;
} c21cm_power_opts;

/* variance: [n_batch][bins] as power; required iff opts->want_variance, otherwise ignored */
int c21cm_power_spectrum_ex_grids(const float *field, const float *field2, int nx, int ny, int nz, int n_batch,
                                  long long row_pitch, const long long *batch_offsets, double Lx, double Ly,
                                  double Lz, const c21cm_power_bins *bins, const c21cm_power_opts *opts,
                                  double *power, double *kmean, double *variance, long long *counts,
                                  void *stream);

/* ---- One-point statistics of boxes and lightcone chunks ----
 * The layout of c21cm_power_spectrum_grids.  moments[b] = {mean, m2, m3, m4} with m_p = sum d^p / N, d = (double)v
 * - mean, everything in fp64 and in a fixed order (two calls give the same bits).  With n_bins > 0 (edges: host,
 * n_bins + 1, increasing): hist[b][i] = the cells with np.digitize((double)v, edges) - 1 == i, half-open bins (a
 * value on the last edge is dropped); at most 4096 bins (the LDS of one workgroup), beyond that
 * C21CM_VALUE_ERROR.  n_bins = 0: edges and hist are ignored.  field, moments and hist may be host or device
 * memory.  A non-finite value is C21CM_INFINITY_OR_NAN_ERROR; nothing is written. */
int c21cm_field_moments_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                              const long long *batch_offsets, int n_bins, const double *edges, double *moments,
                              long long *hist, void *stream);

/* ---- Bispectra of boxes and lightcone chunks (the spec is tests/bispectrum_reference.py) ----
 * The layout, the wavenumbers and the half-open shells e[b] <= |k| < e[b+1] of c21cm_power_spectrum_grids (a shell
 * is exactly one of its bins).  With D the unnormalised DFT of a box (fp32 transforms), delta_b(x) = sum_{k in b}
 * D(k) exp(+i k x) and I_b(x) the same sum of ones, a triangle of shells b1 <= b2 <= b3 has S = sum_x delta_b1
 * delta_b2 delta_b3 (fp64 sums in a fixed order), n_tri = (1/N) sum_x I_b1 I_b2 I_b3 -- the number of mode triplets
 * with k1 + k2 + k3 = 0, an integer, from fp64 transforms and kept for the next call with the same shape, lengths
 * and edges -- and B = (V^2 / N^3) S / (N n_tri), V = Lx Ly Lz, N = nx ny nz; NaN where n_tri = 0.  1 <= n_bins <=
 * 32; 0 < edges[0]; edges[n_bins] <= (2/3) min(pi nx / Lx, pi ny / Ly, pi nz / Lz), below which no triplet closes
 * modulo the grid and no Nyquist mode is in a shell.  Outputs (host or device): bispectrum[n_batch][n_triangles],
 * n_triangles[n_triangles] (the same for every box).  Deterministic: two calls give the same bits, and a triangle's
 * value does not depend on which other triangles are asked for.  Device memory: n_bins padded boxes (twice that
 * while the counts of a new geometry are made) beside the packed boxes.  Errors are C21CM_VALUE_ERROR with a
 * message; a non-finite field value is C21CM_INFINITY_OR_NAN_ERROR, nothing is written. */
typedef struct c21cm_bispec_bins {
    int n_bins;            /* shells, 1 .. 32 */
    const double *edges;   /* host, n_bins + 1, increasing, edges[0] > 0 */
    int n_triangles;       /* >= 1 */
    const int *triangles;  /* host, n_triangles x {b1, b2, b3}, 0 <= b1 <= b2 <= b3 < n_bins */
} c21cm_bispec_bins;

int c21cm_bispectrum_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                           const long long *batch_offsets, double Lx, double Ly, double Lz,
                           const c21cm_bispec_bins *bins, double *bispectrum, long long *n_triangles, void *stream);

/* ---- Mean-free-path bubble size distributions of boxes and lightcone chunks (Mesinger & Furlanetto 2007; DESIGN
 * 4.11; the spec is tests/bubble_reference.py) ----
 * The layout of c21cm_power_spectrum_grids; the cells measure cell_a = L_a / n_a.  All arithmetic below is fp64 + - *
 * /, sqrt and one sincos per ray, without contraction.
 * Selection: a cell is selected iff (double)v < threshold (select_below = 1) or >= threshold (0).
 * Draws: ray r of box b takes the Philox-4x32-10 blocks with counter (r, p, b, 0) and key `seed`, p = 0, 1, 2, each
 *   turned into two uniforms on (0, 1) with 53 bits (philox_uniform_pair): p = 0 (u_cell, u_x), p = 1 (u_y, u_z),
 *   p = 2 (u_mu, u_phi).  A ray is a function of (seed, b, r) and the box alone.
 * Start: with n_sel selected cells in the box, the k-th of them in C order, k = min((long long)(u_cell (double)n_sel),
 *   n_sel - 1), cell (idx_x, idx_y, idx_z); the point p0_a = ((double)idx_a + u_a) cell_a.
 * Direction: isotropic (directions = 0): c = 2 u_mu - 1, s = sqrt(1 - c c), d = (s cos(2 pi u_phi), s sin(2 pi
 *   u_phi), c); along the line of sight (directions = 1): d = (0, 0, +1) if u_mu >= 0.5, else (0, 0, -1).
 * Walk (Amanatides & Woo, started in idx): tmax_a = (((double)(idx_a + (d_a > 0))) cell_a - p0_a) / d_a, tdel_a =
 *   cell_a / |d_a|, both +inf where d_a == 0.  Repeat: a = 0; if (tmax[1] < tmax[a]) a = 1; if (tmax[2] < tmax[a])
 *   a = 2; t = tmax[a]; if !(t < max_length) the ray is capped; the index steps along a; outside the box it wraps
 *   where bit a of periodic_mask is set, otherwise the ray has escaped at t; if the entered cell is not selected the
 *   ray has ended with length t; otherwise tmax[a] += tdel[a].  At most ceil(max_length / cell_x) + ceil(max_length
 *   / cell_y) + ceil(max_length / cell_z) + 3 steps (which must stay below 2^31), after which a ray counts as capped.
 * Outputs (host or device): hist[n_batch][n_bins] = the ended rays with np.digitize(t, edges) - 1 == i (half-open
 *   bins, other lengths dropped; at most 4096 bins); stats[n_batch][4] = {n_sel, n_ended, n_capped, n_escaped}; and
 *   where not NULL lengths[n_batch][n_rays] (t; max_length for a capped ray), flags[n_batch][n_rays] (0 ended, 1
 *   capped, 2 escaped), starts[n_batch][n_rays] (the flat index of the start cell in its box).  A box without a
 *   selected cell is no error: zeros, and NaN / 255 / -1 per ray.  Counts are integers summed with integer atomics:
 *   two calls give the same bytes, and a ray's result does not depend on n_rays.
 * Errors: C21CM_VALUE_ERROR with a message (n_rays outside [1, 2^31 - 1]; edges not finite and increasing, or
 *   edges[0] < 0; max_length not positive and finite; a threshold that is not finite; a NULL required array; a bad
 *   shape); a non-finite field value is C21CM_INFINITY_OR_NAN_ERROR.  Nothing is written on an error. */
int c21cm_bubble_sizes_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                             const long long *batch_offsets, double Lx, double Ly, double Lz, double threshold,
                             int select_below, long long n_rays, unsigned long long seed, int directions,
                             int periodic_mask, double max_length, int n_bins, const double *edges, long long *hist,
                             long long *stats, double *lengths, unsigned char *flags, long long *starts,
                             void *stream);

/* ---- Friends-of-friends clusters of boxes and lightcone chunks (Friedrich et al. 2011; the spec is
 * tests/cluster_reference.py) ----
 * The layout of c21cm_bubble_sizes_grids: n_batch boxes of nx x ny x nz float32 cells read at batch_offsets[b] with
 * row_pitch, z fastest.  Everything below is an integer and a function of the mask alone.
 * Selection: a cell is selected iff (double)v < threshold (select_below = 1) or >= threshold (0).
 * Adjacency: cells p and q of one box are adjacent iff q = p + o for an offset o in {-1, 0, 1}^3, o != 0, with at
 *   most `connectivity` non-zero components: connectivity 1, 2, 3 gives 6, 18, 26 neighbours.  On an axis a whose bit
 *   is set in periodic_mask (bit 0 x, 1 y, 2 z) the sum wraps modulo n_a; through an open face there is no neighbour.
 *   On a periodic axis with n_a = 1 the neighbour is the cell itself, with n_a = 2 both sides are the same cell.
 * Clusters: a cluster is a class of the transitive closure of adjacency over the selected cells of a box.  Its root
 *   is the smallest flat index (ix ny + iy) nz + iz among its cells, its size its number of cells; the clusters of a
 *   box are numbered in ascending root.
 * Outputs (host or device): stats[n_batch][4] = {n_selected, n_clusters, the size of the largest cluster, its root}
 *   (ties take the smallest root; without a selected cell 0, 0, 0, -1); hist_n[n_batch][n_bins] = the clusters with
 *   edges[i] <= size < edges[i + 1] and hist_cells[n_batch][n_bins] = the cells of those clusters (edges: host,
 *   n_bins + 1 values, increasing, edges[0] >= 1; 1 to 4096 bins); where not NULL labels[n_batch][nx ny nz] (int32,
 *   dense, C order) = the root of the cell's cluster, -1 where the cell is not selected; and, given as both or
 *   neither, cluster_roots / cluster_sizes [n_batch][max_clusters]: the first min(n_clusters, max_clusters) clusters
 *   in ascending root, the remaining entries -1 / 0.  n_clusters in stats is always the true count, so a caller sees
 *   that its capacity was too small.  Sums are integer atomics: two calls give the same bytes.
 * Errors: C21CM_VALUE_ERROR with a message (a NULL required pointer; a bad shape; nx ny nz >= 2^31; n_batch outside
 *   [1, 65535]; row_pitch < nz; a negative offset; a threshold that is not finite; connectivity outside 1..3;
 *   periodic_mask outside 0..7; n_bins outside [1, 4096]; edges not increasing or edges[0] < 1; only one of the
 *   cluster arrays; max_clusters < 1 with them), all before any array but edges and batch_offsets is touched; a
 *   non-finite field value is C21CM_INFINITY_OR_NAN_ERROR.  Nothing is written on an error. */
int c21cm_bubble_clusters_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                                const long long *batch_offsets, double threshold, int select_below,
                                int connectivity, int periodic_mask, int n_bins, const long long *edges,
                                long long *hist_n, long long *hist_cells, long long *stats, int *labels,
                                long long max_clusters, long long *cluster_roots, long long *cluster_sizes,
                                void *stream);

/* ---- Minkowski functionals of boxes and lightcone chunks (Schmalzing & Buchert 1997; Gleser et al. 2006;
 * Friedrich et al. 2011; the spec is tests/minkowski_reference.py) ----
 * Layout: as for c21cm_bubble_clusters_grids: n_batch boxes of nx x ny x nz float32 cells at batch_offsets[b], rows of
 *   row_pitch, z fastest, host or device pointers.
 * Thresholds: thresholds[n_thresholds] on the host, finite, strictly increasing, 1 <= n_thresholds <= 255.
 * Selection: as everywhere in this module: at threshold t a cell is selected iff (double)v < t (select_below = 1) or
 *   (double)v >= t (select_below = 0).
 * The complex: a box is the cubical complex of its cells.  Each cell is a closed cube with 6 faces, 12 edges and 8
 *   vertices, and neighbouring cells share elements.  On an axis whose bit is set in periodic_mask (bit 0 x, 1 y, 2 z)
 *   the complex wraps: with n_a = 1 a cell's two faces across a are the same face, with n_a = 2 they are two faces.
 *   Through an open face there is no cell; the elements on that face belong to the one cell inside.
 * Counting: an element is in the set at t iff at least one cell that contains it is selected at t.  That cell can be
 *   one of 1 cell for a cube, up to 2 for a face, 4 for an edge, 8 for a vertex.
 * Outputs (host or device): counts[n_batch][n_thresholds][8], int64, = {n3, n2x, n2y, n2z, n1x, n1y, n1z, n0}: n3
 *   selected cells; n2a faces perpendicular to axis a; n1a edges parallel to a; n0 vertices.  Everything is an
 *   integer, summed with integer atomics or a fixed-order reduction: two calls give the same bytes, and a row does
 *   not depend on which other thresholds were asked for.
 * Errors, checked before any output is touched: C21CM_VALUE_ERROR with a message for a NULL required pointer, a bad
 *   shape, nx ny nz >= 2^31, n_batch outside [1, 65535], row_pitch < nz, a negative offset, n_thresholds outside
 *   [1, 255], thresholds not finite or not increasing, or periodic_mask outside 0..7; C21CM_INFINITY_OR_NAN_ERROR for
 *   a non-finite field value.  Nothing is written. */
int c21cm_minkowski_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                          const long long *batch_offsets, int n_thresholds, const double *thresholds,
                          int select_below, int periodic_mask, long long *counts, void *stream);

/* ---- Squared distance transforms and granulometry bubble sizes of boxes and lightcone chunks (Kakiichi et al. 2017;
 * Lin et al. 2016; Giri et al. 2018; the spec is tests/granulometry_reference.py) ----
 * Layout and selection: as for c21cm_bubble_clusters_grids: n_batch boxes of nx x ny x nz float32 cells at
 *   batch_offsets[b], rows of row_pitch, z fastest, host or device pointers; a cell is selected iff (double)v <
 *   threshold (select_below = 1) or >= threshold (0).  Everything below is an integer and a function of the mask
 *   alone; distances are in cells.
 * Axis distance: d_a(i, j) = |i - j| on an open axis; where bit a of periodic_mask (bit 0 x, 1 y, 2 z) is set, d_a(i,
 *   j) = min(|i - j|, n_a - |i - j|).  Nothing lies beyond an open face: the outside is neither selected nor
 *   unselected (the convention of scipy.ndimage.distance_transform_edt).
 * Squared distance transform: D2[c] = the minimum of d_x^2 + d_y^2 + d_z^2 over the unselected cells q of the same
 *   box, centre to centre: 0 at unselected cells, and C21CM_EDT_NONE = 2^30 everywhere in a box without an unselected
 *   cell.  nx^2 + ny^2 + nz^2 < 2^30 is required, so that every real distance is below the sentinel and sentinel -
 *   d^2 stays positive in int32.
 * Radii: radii2[n_radii], int64 on the host, 0 <= s_0 < s_1 < ...; 0 <= n_radii <= 255.
 * Erosion curve: eroded[k] = the cells with D2[c] > s_k: the cells whose closed digital ball {o : |o|^2 <= s_k} holds
 *   only selected cells.
 * Granulometry: cell x is covered at s iff some centre c has D2[c] > s and |x - c|^2 < D2[c] (the same axis
 *   distances); covered[k] = the number of such cells.  Equivalently Q_s[x] = max_c (G_s[c] - |x - c|^2) > 0 with G_s
 *   = D2 where D2 > s and minus infinity elsewhere: the union of the inscribed balls of squared radius > s, which in
 *   the continuum is the opening by a ball of radius sqrt(s).  Unlike the two-step digital opening it is monotone in
 *   s, its rows do not depend on which other radii were asked for, and covered = n_selected at s = 0.
 * Outputs (host or device): covered[n_batch][n_radii] and eroded[n_batch][n_radii], int64; stats[n_batch][4] =
 *   {n_selected, max D2 over the selected cells (0 without one), the smallest flat index (ix ny + iy) nz + iz
 *   attaining it (-1 without one), n_unselected}; where not NULL dist2[n_batch][nx ny nz] (int32, dense, C order) = D2
 *   and level[n_batch][nx ny nz] (int32) = the number of asked radii at which the cell is covered, -1 at unselected
 *   cells; the coverage being monotone, level - 1 indexes the largest such radius.  Sums are integer atomics or
 *   fixed-order reductions: two calls give the same bytes.
 * Errors, checked before any output is touched: C21CM_VALUE_ERROR with a message for a NULL required pointer (field,
 *   batch_offsets, stats; with n_radii >= 1 also radii2, covered, eroded), a bad shape or nx^2 + ny^2 + nz^2 >= 2^30,
 *   nx ny nz >= 2^31, n_batch outside [1, 65535], row_pitch < nz, a negative offset, a threshold that is not finite,
 *   periodic_mask outside 0..7, n_radii outside [0, 255], radii negative or not strictly increasing;
 *   C21CM_INFINITY_OR_NAN_ERROR for a non-finite field value.  Nothing is written on an error. */
#define C21CM_EDT_NONE (1 << 30)
int c21cm_granulometry_grids(const float *field, int nx, int ny, int nz, int n_batch, long long row_pitch,
                             const long long *batch_offsets, double threshold, int select_below, int periodic_mask,
                             int n_radii, const long long *radii2, long long *covered, long long *eroded,
                             long long *stats, int *dist2, int *level, void *stream);

/* ---- Telescope-resolution smoothing of boxes and lightcones (the smooth_coeval / smooth_lightcone convention of
 * tools21cm; Giri et al. 2018; Kakiichi et al. 2017; the spec is tests/observe_reference.py) ----
 * Input: field[i][j][s], nx x ny x ns float32 cells, dense, the line of sight s fastest; host or device pointer.  Per
 *   slice a beam width sigma_cells[s] >= 0 in cells (fp64) and two counts los_below[s], los_above[s] >= 0; all three
 *   arrays on the host.
 * Step 1, mean: m[s] = the mean of field[:][:][s], accumulated in fp64 in a fixed order (the order depends on nx ny
 *   alone).  With subtract_mean g = (float)((double)f - m[s]), else g = f: a slice of equal values gives exactly 0.
 * Step 2, beam: with lw = (int)(4 sigma + 0.5) >= 1 the half kernel is w[d] = exp(-d^2 / (2 sigma^2)), d = 0 .. lw,
 *   divided in fp64 by w[0] + 2 sum_{d >= 1} w[d] and then rounded to fp32.  The slice is convolved along x and then
 *   along y, h[i] = sum_{d = -lw .. lw} w[|d|] g[(i + d) mod n]: both axes wrap, as often as lw asks for (lw > n is
 *   legal).  In exact arithmetic this is scipy.ndimage.gaussian_filter(slice, sigma, mode="wrap", truncate=4.0).  In
 *   fp32 it is acc = w[0] g[i]; acc = fma(w[d], g[i - d] + g[i + d], acc) for d = 1 .. lw: a slice's result does not
 *   depend on the widths of the other slices.  lw = 0 (sigma < 0.125) leaves the slice as it is, bit for bit.
 * Step 3, channel: out[i][j][s] = the mean of step 2 over the slices s - los_below[s] .. s + los_above[s], added in
 *   ascending order in fp32 and divided by their number.  On an open line of sight (periodic_los = 0: lightcones)
 *   the range is clipped to [0, ns - 1]; with periodic_los (coeval boxes) it wraps, and below + above + 1 <= ns is
 *   required.  below = above = 0 copies step 2.
 * Outputs (host or device): out[nx][ny][ns] float32, which must not overlap field; where not NULL slice_means[ns],
 *   fp64 = m, whether or not it was subtracted.  No floating-point atomics: two calls give the same bytes.
 * Axes of any length are convolved: a transverse line longer than a workgroup holds runs in tiles.
 * Errors, checked before any output is touched: C21CM_VALUE_ERROR with a message for a NULL required pointer (all but
 *   slice_means), an axis < 1, nx ny ns >= 2^31, a sigma that is negative, not finite or above 128 cells (lw > 512), a
 *   negative count, a periodic channel longer than ns, out overlapping field; C21CM_INFINITY_OR_NAN_ERROR for a
 *   non-finite field value. */
int c21cm_observe_smooth_grids(const float *field, int nx, int ny, int ns, const double *sigma_cells,
                               const int *los_below, const int *los_above, int periodic_los, int subtract_mean,
                               float *out, double *slice_means, void *stream);

/* ---- Angular lightcone (lightconers.py:541-701 AngularLightconer) ----
 * One call fills slices [i0, i1) of up to C21CM_LC_MAX_FIELDS angular lightcones from the two node
 * boxes that bracket them.  Pixel p of slice j sits at x = distance[j] nhat[:, p] + origin (cells);
 * each box (hii_dim x hii_dim x hii_d_para) is periodic along every axis.  The value is the B-spline
 * interpolation of the given order at x (scipy.ndimage.map_coordinates, mode "grid-wrap") in which
 * every tap is first redshift-interpolated, (w_lo[j] box_lo + w_hi[j] box_hi) / w_norm in fp64 (bit f
 * of mean_max: where box_lo * box_hi < 0 the larger of the two); the sum is fp64, stored as fp32.
 * Orders 3 and 5 read B-spline coefficients (c21cm_spline_prefilter_grids of each node box); the
 * prefilter is linear, so this is exact for "mean" fields; mean_max fields need order 0 or 1.
 * Bit f of vector: field f takes three consecutive boxes (x, y, z components) and stores their
 * projection sum_k v_k nhat_k (los_velocity).  box_lo / box_hi list n_fields + 2 popcount(vector)
 * boxes in field order, lightcone lists n_fields outputs float[n_pix][n_slices] (slices fastest).
 * Boxes, lightcones and nhat may be host or device memory, mixed; a host nhat is copied every call,
 * so a run keeps it on the device.  A non-finite sum (a non-finite tap) is C21CM_INFINITY_OR_NAN_ERROR. */
typedef struct c21cm_angular_spec {
    int hii_dim;              /* node boxes: hii_dim x hii_dim x hii_d_para */
    int hii_d_para;
    long long n_pix;          /* pixels (columns of the lightcone) */
    int n_slices;             /* length of the lightcone */
    int i0, i1;               /* slices filled by this call, 0 <= i0 < i1 <= n_slices */
    int n_fields;             /* outputs, 1 .. C21CM_LC_MAX_FIELDS */
    unsigned mean_max;        /* bit f: field f interpolates with mean_max */
    unsigned vector;          /* bit f: field f is the projection of a vector field (three boxes) */
    int order;                /* 0, 1, 3 or 5 */
    const double *nhat;       /* [3][n_pix] rotated unit directions */
    double origin[3];         /* cells */
    const double *distance;   /* host, i1 - i0: comoving distance of the slice [cells] */
    const double *w_lo;       /* host, i1 - i0: |dc_hi - d| (cells) */
    const double *w_hi;       /* host, i1 - i0: |dc_lo - d| */
    double w_norm;            /* |dc_lo - dc_hi| > 0 */
} c21cm_angular_spec;

int c21cm_lightcone_angular_grids(const c21cm_angular_spec *spec, const float *const *box_lo,
                                  const float *const *box_hi, float *const *lightcone, void *stream);

/* B-spline coefficients of order 3 or 5 of n_fields periodic boxes (n0 x n1 x n2, the last axis
 * fastest): what scipy.ndimage.spline_filter(box, order, mode = "grid-wrap") computes, stored as
 * fp32.  coefs[f] may alias boxes[f]; pointers may be host or device memory.  A non-finite box value
 * is C21CM_INFINITY_OR_NAN_ERROR. */
int c21cm_spline_prefilter_grids(int n0, int n1, int n2, int order, int n_fields, const float *const *boxes,
                                 float *const *coefs, void *stream);

/* c21cm_lightcone_dvdr_grids on n_cols columns of spec->n_slices slices (any lightcone whose line of sight
 * is its fastest axis: an angular one has n_pix columns); spec->hii_dim is not read. */
int c21cm_lightcone_dvdr_columns_grids(const c21cm_dvdr_spec *spec, long long n_cols, float *brightness_temp,
                                       const float *los_velocity, const float *tau_21, void *stream);

/* ---- The dv/dr correction of a coeval box: periodic line of sight (rsds.py:16-103, periodic = True;
 * drivers/coeval.py:242-278) ----
 * out = brightness_temp corrected by the line-of-sight velocity gradient g = irfft(i k rfft(los_velocity))
 * along every column of n_slices cells (the line of sight is the fastest axis: float[n_cols][n_slices]),
 * k = 2 pi rfftfreq(n_slices, dx) -- what irfftn(1j k_z rfftn(v)) gives, the transforms across the line of
 * sight cancelling -- then 1/|1 + clip(g, +-max_dvdr H)/H| or, with use_ts_fluct, the fp64 tau_21 form of
 * c21cm_dvdr_spec.  method 0 picks the path: an fp32 line transform in LDS for n_slices = 2^k, 8 .. 1024;
 * the exact circulant sum in fp64 for every other n_slices from 2 to 1536 (1: the transform, 2: the sum,
 * or C21CM_VALUE_ERROR where n_slices does not fit).  Each array may be host or device memory; out may be
 * brightness_temp, and no other input is ever written. */
typedef struct c21cm_dvdr_periodic_spec {
    long long n_cols;      /* columns (HII_DIM^2 for a box) */
    int n_slices;          /* cells per column = the period, >= 2 */
    double dx;             /* BOX_LEN / HII_DIM [Mpc] */
    double max_dvdr;       /* AstroParams.MAX_DVDR */
    int use_ts_fluct;      /* tau_21 required */
    int method;            /* 0: automatic, 1: transform, 2: direct */
    const double *hubble;  /* host, n_slices: H(z) of every slice [1/s] */
} c21cm_dvdr_periodic_spec;

int c21cm_dvdr_periodic_grids(const c21cm_dvdr_periodic_spec *spec, const float *brightness_temp,
                              const float *los_velocity, const float *tau_21, float *out, void *stream);

/* Library management */
const char *c21cm_version(void);
int c21cm_device_synchronize(void);
void c21cm_release_device_cache(void); /* drop cached rocFFT plans and scratch */
const char *c21cm_last_error(void);

/* Placement of the second work spectrum of a two-grid sweep (csrc/host/placement.c): what the last decision was.
 * out = {outcome (0 placed by timed launches, 1 off / not applicable, 2 other tenants on the device, 3 another
 * process walking, 4 nothing faster within the budget, 5 remembered failure, 6 tenancy unknown + busy device, 7 time budget exhausted),
 * GB held at the peak of the walk, timed probes, ms of the chosen pair, ms of the first candidate, wall ms of the
 * decision, tenants seen (-1 unknown), walks of this process so far}.  C21CM_VALUE_ERROR before any decision. */
int c21cm_placement_report(double out[8]);
/* The walk is opt-in: 1 on, 2 on even with other tenants on the device, 0 off, -1 the environment's C21CM_WS_PLACE
 * (unset: off).  Changing the setting re-opens the decisions taken under the old one. */
int c21cm_placement_set(int mode);

#ifdef __cplusplus
}
#endif
#endif /* C21CM_GRID_H */
