/*
 * ws_slots.h -- every slot of the device workspace (c21hip_ws, runtime.hip), in one enum.
 *
 * Rules:
 *   - no numeric initialisers: a slot's id follows from its position, so two names share an id only
 *     where a line says so;
 *   - add a slot by adding a line to its owner's group;
 *   - a range that code indexes as FIRST + k has a first and a last member, and the code that indexes
 *     it asserts the length it assumes;
 *   - sharing is written `WS_B = WS_A` here and nowhere else.  The alias line follows its target
 *     directly (after the last member of a range), so that the next plain enumerator continues where
 *     the target left off, and it carries the reason.  "Separate entries" below means: the two holders
 *     run in different library calls, every call refills what it reads from the slot, and neither keeps
 *     a pointer into the slot or a cache keyed on its contents from one call to the next -- so all one
 *     holder can do to the other is grow the buffer.
 * The ids appear in c21hip_ws's out-of-memory text and in the C21CM_WS_TRACE lines and nowhere else.
 */
#ifndef C21_WS_SLOTS_H
#define C21_WS_SLOTS_H

enum c21_ws_slot {
    /* ---- ionize_driver.c: spectra, dense inputs / outputs, reductions ---- */
    WS_DELTA_UNF,
    WS_DELTA_FIL,
    WS_STARS_UNF,
    WS_STARS_FIL,
    WS_XE_UNF,
    WS_XE_FIL,
    WS_DENSITY,
    WS_NION,
    WS_XE_DENSE,
    WS_TNEUTRAL,
    WS_PREV_ZRE,
    WS_XH,
    WS_ZRE,
    WS_TK,
    WS_NION_DENSE,
    WS_SCALARS,
    WS_TABLE,
    WS_FIRST_CROSS,
    WS_CROSS_BITS, /* two-grid fused loop on 512-point lines: one plane of crossing bits per radius > 0 */
    WS_DELTA_WORK,
    WS_STARS_WORK,
    WS_XE_WORK,
    /* separate entries: a filtered work spectrum, rewritten by every radius (the placement record of the slot
     * compares pointers and decides again after a reallocation) */
    WS_PT_LOW = WS_XE_WORK,
    WS_PARTIALS,
    /* separate entries: reduction partials live within one ionize entry, the sharded finish phases included */
    WS_PT_HIGH = WS_PARTIALS,

    /* ---- perturb_driver.c ---- */
    WS_PT_SAVED,
    WS_PT_RESAMPLED,
    /* halobox_driver.c shares PerturbedField's staging slots (the two never run at the same time).
     * separate entries: double accumulation grid, zeroed by every call */
    WS_HB_ACC0 = WS_PT_RESAMPLED,
    WS_PT_IN0, /* staged IC arrays: density, three velocities, three 2LPT velocities */
    WS_PT_IN_LAST = WS_PT_IN0 + 6,
    /* separate entries: the same IC arrays, uploaded by every call */
    WS_HB_IN0 = WS_PT_IN0,
    WS_HB_IN_LAST = WS_PT_IN_LAST,
    WS_PT_OUT0, /* staged outputs */
    WS_PT_OUT_LAST = WS_PT_OUT0 + 3,
    /* separate entries: outputs written and copied back within the call */
    WS_HB_OUT0 = WS_PT_OUT0,
    WS_HB_OUT_LAST = WS_PT_OUT0 + 2,
    /* separate entries: double accumulation grid, zeroed by every call, under perturb's fourth staged output */
    WS_HB_ACC1 = WS_PT_OUT_LAST,

    /* ---- brightness_driver.c, api_misc.c ---- */
    WS_BT_DENS,
    WS_BT_XH,
    WS_BT_TS,
    /* separate entries: staged spin temperature / the ln-tables of the spec, uploaded by every call */
    WS_HB_TABLES = WS_BT_TS,
    WS_BT_OUT,
    /* separate entries: staged output / min-max partials, written and read back within the call */
    WS_HB_PART = WS_BT_OUT,
    WS_MISC_A,
    WS_MISC_B,
    WS_MISC_C,
    WS_MISC_D,
    WS_BT_TAU,
    WS_BT_PART,

    /* ---- ionize_kernels.hip / fft_native.hip: small library-owned buffers ---- */
    WS_ANY_NONZERO_FLAG, /* c21hip_any_nonzero */
    WS_NATIVE_C2R_SPLIT, /* c21hip_native_fft_c2r: the split copy of a padded grid */
    WS_WIN_TAB0,         /* W(kR) tables of win_tables, one buffer per table slot */
    WS_WIN_TAB_LAST = WS_WIN_TAB0 + 3,

    /* ---- ics_driver.c, padded pipeline ---- */
    WS_IC_BOX,
    WS_IC_SAVED,
    WS_IC_PHI,
    WS_IC_DIAG0, /* the three diagonal second derivatives of the 2LPT source */
    WS_IC_DIAG_LAST = WS_IC_DIAG0 + 2,
    /* same entry: P(k) by mode is consumed by the mode sampling at the start of the call, the diagonals are
     * written on the same stream afterwards (growing the slot frees the buffer, which waits for the device) */
    WS_IC_PK = WS_IC_DIAG_LAST,
    WS_IC_IN,
    WS_IC_OUT0, /* staged outputs, reused one at a time */
    WS_IC_DEVIATES,
    /* separate entries: c21hip_bench_pass fills its spectra itself before it times a pass */
    WS_BENCH_A = WS_IC_DEVIATES,
    WS_IC_VCBTAB,
    WS_BENCH_B = WS_IC_VCBTAB, /* as WS_BENCH_A */

    /* ---- fft_native.hip: c21hip_bench_pass ---- */
    WS_BENCH_REAL,
    WS_BENCH_MASK,
    WS_BENCH_PARTIALS,
    WS_BENCH_REAL2,

    /* ---- tsfilter_driver.c ---- */
    WS_TF_IN,
    WS_TF_UNF,
    WS_TF_WORK,
    WS_TF_OUT,
    WS_TF_PART,
    WS_TF_UNF2,
    WS_TF_WORK2,
    WS_TF_IN2,
    WS_TF_OUT2,
    WS_TF_RPART,

    WS_DEF_PARTIALS, /* ionize_driver.c */
    WS_HB_ACC2,      /* halobox_driver.c */
    WS_HB_OUT3,
    WS_PT_SPLIT, /* perturb_driver.c: split-layout spectra */
    WS_PT_SPLIT_LAST = WS_PT_SPLIT + 2,

    /* ---- ionize_driver.c ---- */
    WS_DELTA_WORK2, /* second radius of a two-radius sweep */
    /* separate entries: the bench's second pair of work spectra, written by its own pass X */
    WS_BENCH_A2 = WS_DELTA_WORK2,
    WS_STARS_WORK2,
    WS_BENCH_B2 = WS_STARS_WORK2, /* as WS_BENCH_A2 */
    WS_XE_WORK2,
    WS_EUL_DFIL2, /* Eulerian table loop: second delta_R buffer, two dense x_e(R) buffers */
    WS_EUL_XE0,
    WS_EUL_XE1,

    /* ---- ics_driver.c, split-layout pipeline ---- */
    WS_IS_SAVED,
    WS_IS_FILT,
    WS_IS_WORK,
    WS_IS_LO,
    WS_IS_LOWORK,
    WS_IS_BOX,
    WS_IS_D0,
    WS_IS_D_LAST = WS_IS_D0 + 2,
    WS_IS_O0,
    WS_IS_O_LAST = WS_IS_O0 + 2,
    WS_IS_OUT,
    WS_IS_IN,
    WS_IS_PK2,
    WS_IS_LO1, /* the folded spectra of one fused fold (lo_fields) */
    WS_IS_LO1_LAST = WS_IS_LO1 + 2,

    /* ---- ionize_driver.c ---- */
    /* recombination models: filtered whalo_sfr and N_rec grids, staged arrays, rate tables */
    WS_SFR_UNF,
    WS_SFR_FIL,
    WS_SFR_WORK,
    WS_NREC_UNF,
    WS_NREC_FIL,
    WS_NREC_WORK,
    WS_WSFR,
    WS_PREV_NREC,
    WS_G12,
    WS_MFP,
    WS_NREC_OUT,
    WS_RR_TABLES,
    /* rank-local state of a sharded run with a recombination model */
    WS_SH_XH,
    WS_SH_ZRE,
    WS_SH_G12,
    WS_SH_MFP,

    /* ---- shard_rccl.c ---- */
    WS_SHARD_GRID,
    WS_SHARD_STAGE,
    WS_SHARD_SCALARS,
    WS_SHARD_BITS,

    /* ---- ts_driver.c ---- */
    WS_TS_DENS,
    WS_TS_PTS,
    WS_TS_PTK,
    WS_TS_PXE,
    WS_TS_GRID_A,
    WS_TS_GRID_B,
    WS_TS_TAB,
    WS_TS_SFRDTAB,
    WS_TS_LYA_C,
    WS_TS_LYA_I,
    WS_TS_OTS,
    WS_TS_OTK,
    WS_TS_OXE,
    WS_TS_PART,
    WS_TS_SMALL,
    WS_TS_MEANSFR,
    WS_TS_SFRDTAB2,
    WS_TS_SUMS,

    /* ---- abi_compute.c: ComputeTsBox ---- */
    WS_ABI_TS_FILTERED, /* [n_step][N] filtered density */
    WS_ABI_MEAN_PART,   /* box_mean */
    WS_ABI_TS_MCRIT,
    WS_ABI_TS_MCRIT_R,

    /* ---- ionize_driver.c ---- */
    /* USE_MINI_HALOS: previous delta and the two turnover-mass grids (spectra, scratch, filtered),
     * staged inputs, 2-D tables, per-radius f_coll history in and out */
    WS_MINI_PD_UNF,
    WS_MINI_PD_WORK,
    WS_MINI_PD_FIL,
    WS_MINI_MTA_UNF,
    WS_MINI_MTA_WORK,
    WS_MINI_MTA_FIL,
    WS_MINI_MTM_UNF,
    WS_MINI_MTM_WORK,
    WS_MINI_MTM_FIL,
    WS_MINI_PDENS,
    WS_MINI_MTA,
    WS_MINI_MTM,
    WS_MINI_TABLES,
    WS_MINI_HIST_A,
    WS_MINI_HIST_M,
    WS_MINI_OUT_A,
    WS_MINI_OUT_M,
    /* c21cm_mturn_grids */
    WS_MT_G12,
    WS_MT_ZRE,
    WS_MT_J21,
    WS_MT_VCB,
    WS_MT_OUT_A,
    WS_MT_OUT_M,
    WS_MT_SC,
    WS_MT_PART,

    /* ---- abi_compute.c: ComputeIonizedBox, the turnover grids of a USE_MINI_HALOS run ---- */
    WS_ABI_ION_MTA,
    WS_ABI_ION_MTM,

    /* ---- ts_driver.c ---- */
    /* USE_MINI_HALOS: 2-D tables, filtered turnover grids, mini shell rows, J_21_LW staging */
    WS_TS_MINI_TAB,
    WS_TS_MINI_MCRIT,
    WS_TS_MINI_SHELL,
    WS_TS_MINI_J21,
    WS_TS_MINI_MEAN,
    WS_TS_MCRIT_J21,
    WS_TS_MCRIT_VCB,
    WS_TS_MCRIT_OUT,

    WS_SPHERE_RSQ, /* ionize_driver.c */

    /* ---- halobox_driver.c ---- */
    /* USE_MINI_HALOS (HaloBox.c:245-283, map_mass.c:285-321) */
    WS_HBM_MTA,
    WS_HBM_MTM,
    WS_HBM_TAB,
    WS_HBM_ACC3,
    WS_HBM_OUT4,
    WS_HBM_G12,
    WS_HBM_ZRE,
    WS_HBM_J21,
    WS_HBM_VCB,
    WS_HBM_OUTA,
    WS_HBM_OUTM,
    WS_HBM_SUMS,
    /* abi_compute.c: the turnover grids of ComputeHaloBox and ComputePerturbedHaloCatalog */
    WS_ABI_HB_MTA,
    WS_ABI_HB_MTM,
    /* halo-catalogue branch (deposit_halos) */
    WS_HC_MASS,
    WS_HC_COORD,
    WS_HC_RNG0,
    WS_HC_RNG1,
    WS_HC_RNG2,
    WS_HC_WSFR,
    WS_HC_BINS,

    /* ---- abi_compute.c: test_halo_props, its staged host arrays ---- */
    WS_HP0, /* five catalogue arrays, four feedback grids, the property rows */
    WS_HP_LAST = WS_HP0 + 9,
    /* Eight of the ten lie under slots of other owners.  All are separate entries: test_halo_props uploads
     * what it reads and copies its rows back before it returns. */
    /* fft_native.hip: node tables of the evaluated windows, live from c21hip_wev_prepare to
     * c21hip_wev_release, both inside one ionize or Ts-filter entry */
    WS_WEV_NODES = WS_HP0 + 2,
    WS_WEV_MFP = WS_HP0 + 3,
    /* shard_rccl.c: the exchange buffers of one sharded ComputeTsBox call */
    WS_TSS_SUMS = WS_HP0 + 4,
    WS_TSS_SEND = WS_HP0 + 5,
    WS_TSS_RECV = WS_HP0 + 6,
    WS_TSS_SLAB = WS_HP0 + 7,
    /* ionize_driver.c, fused recombination loop: whalo_sfr of the second radius of a sweep (a work spectrum) */
    WS_SFR_WORK2 = WS_HP0 + 8,
    /* ... and float R per radius index (mean free path of a first crossing), uploaded by every finish */
    WS_R_DEV = WS_HP_LAST,

    /* ---- shard_rccl.c ---- */
    WS_SHARD_RC_MASK,
    WS_SHARD_RC_G12,

    /* ---- ionize_driver.c ---- */
    WS_EUL_XEPEND,  /* banded barrier with an x_e grid: clipped x_e of the undecided cells (sparse) */
    WS_NION_DENSE2, /* closed-form Eulerian loop: second dense f_coll buffer (deferred barrier) */
    WS_GSL_ROW_KIND, /* gsl_stream.c: generator kind per x-row */
    /* shard_rccl.c: the status word a rank out of memory still needs, the slab exchange's bits.  (The status
     * word once shared an id with WS_EUL_XEPEND, whose reallocation freed it.) */
    WS_SHARD_STATUS,
    WS_SHARD_SLABBITS,
    WS_NREC_WORK2, /* fused recombination loop with x_e AND a filtered N_rec: N_rec of the second radius */
    WS_TSS_ROWMAX, /* shard_rccl.c */
    WS_EUL_WORK3,  /* Eulerian table loop, two radii per pass-X sweep: the second set of k-space buffers */
    WS_EUL_WORK4,

    /* ---- lightcone_driver.c ---- */
    WS_LC_TAB,
    WS_LC_BOXES,
    WS_LC_SLAB,
    WS_LC_HUBBLE,
    WS_LC_DVDR,
    /* ---- rsd_driver.c ---- */
    WS_RSD_SCALE,
    WS_RSD_IN,
    WS_RSD_OUT,
    WS_RSD_FLAG,
    WS_RSD_VEL,
    /* ---- angular_driver.c ---- */
    WS_ANG_NHAT,
    WS_ANG_TAB,
    WS_ANG_BOXES,
    WS_ANG_SLAB,
    WS_ANG_FLAG,
    WS_PREFILTER_IN,
    WS_PREFILTER_OUT,
    /* ---- power_driver.c ---- */
    WS_PW_TAB,
    WS_PW_IN,
    WS_PW_PAD,
    WS_PW_SUMS,
    WS_PW_FLAG,
    /* ---- halocat_driver.c ---- */
    WS_PH_IN,
    WS_PH_OUT,
    WS_PH_GRIDS,
    /* ---- dvdr_periodic_driver.c ---- */
    WS_DVP_HUBBLE,
    WS_DVP_BT,
    WS_DVP_VEL,
    WS_DVP_TAU,
    WS_DVP_OUT,
    /* ---- gsl_stream.c: the reference's random streams drawn on the device ---- */
    WS_GSL_DESC,  /* one descriptor per stream that owns rows */
    WS_GSL_STATE, /* per stream: accepted count, carry word, error word, generator state (saved by every launch) */
    WS_GSL_JUMP,  /* jump matrices of cmrg, mrg, taus2 */
    WS_GSL_FLAG,  /* tile-cap flag of a draw; the two counts of c21cm_gsl_accept_pairs */
    WS_GSL_IN,    /* staged host words of c21cm_gsl_accept_pairs */
    WS_GSL_OUT,   /* outputs of the c21cm_gsl_* entries on their way to a host array */
    /* ---- halo_sampler_driver.c ---- */
    WS_HS_TABLES, /* the snapshot's tables (doubles) */
    WS_HS_IN0,    /* staged conditions: five catalogue arrays, or density and overlap */
    WS_HS_IN_LAST = WS_HS_IN0 + 4,
    WS_HS_WORDS, /* four words per condition between pass A and pass B */
    WS_HS_SUMS,  /* kept halos per block of conditions, then their exclusive scan; total and status word */
    WS_HS_OUT0,  /* staged outputs: masses, coordinates, three deviates */
    WS_HS_OUT_LAST = WS_HS_OUT0 + 4,
    /* ---- dexm_driver.c: the DexM halo finder (its transforms run in tsfilter_driver.c's WS_TF_* slots) ---- */
    WS_DX_IN,       /* staged hi-res density */
    WS_DX_DELTA,    /* delta_m of the running rung (dense); then the 0 / 1 mask and its smoothed form */
    WS_DX_MASK,     /* in_halo, bytes */
    WS_DX_FORBID,   /* DEXM_OPTIMIZE: forbidden, bytes */
    WS_DX_STATE,    /* per cell: the candidate's state on the running rung */
    WS_DX_RUNG,     /* per cell: rung + 1 of the halo centred there (16 bits) */
    WS_DX_LIST,     /* the rung's candidates in raster order */
    WS_DX_FOUND,    /* halo cells in the order they were found */
    WS_DX_COUNTS,   /* total, then candidates / halos per compaction workgroup and their exclusive scan */
    WS_DX_COUNTERS, /* decided, accepted, found, last round */
    WS_DX_TABLES,   /* per rung: mass, MtoR(mass) */
    WS_DX_OVERLAP,  /* staged overlap box */
    WS_DX_OUT0,     /* staged outputs: masses, coordinates, three deviates */
    WS_DX_OUT_LAST = WS_DX_OUT0 + 4,
    /* ---- abi_compute.c: ComputeHaloCatalog for CHMF-SAMPLER, between the finder and the sampler ---- */
    WS_ABI_DX_LARGE0, /* the catalogue of large halos: masses, coordinates, three deviates */
    WS_ABI_DX_LARGE_LAST = WS_ABI_DX_LARGE0 + 4,
    WS_ABI_DX_OVERLAP, /* the overlap box */
    /* ---- moments_driver.c ---- */
    WS_MO_TAB,  /* histogram edges, batch offsets */
    WS_MO_IN,   /* staged host field */
    WS_MO_SUMS, /* row sums, means, moments, histogram */
    WS_MO_FLAG,
    /* ---- bispectrum_driver.c ---- */
    WS_BS_TAB,   /* wavenumbers, thresholds, batch offsets, counts, products groups, slots */
    WS_BS_IN,    /* staged host field */
    WS_BS_PAD,   /* the packed chunks and, in place, their half spectra */
    WS_BS_STACK, /* one padded box per shell: float, or double in the indicator pass */
    WS_BS_SUMS,  /* row sums and means of the pack, products partials, outputs */
    WS_BS_FLAG,
    /* ---- bubble_driver.c ---- */
    WS_BU_TAB,    /* histogram edges, batch offsets */
    WS_BU_IN,     /* staged host field */
    WS_BU_MASK,   /* one bit per cell, rows padded to whole 64-bit words */
    WS_BU_PREFIX, /* set bits per chunk of words, their exclusive scan, set bits before every word */
    WS_BU_OUT,    /* histogram, counts, and the per-ray outputs that were asked for */
    WS_BU_FLAG,
    /* ---- cluster_driver.c ---- */
    WS_BC_TAB,    /* histogram edges, batch offsets */
    WS_BC_IN,     /* staged host field */
    WS_BC_MASK,   /* the selection mask and the root mask, one bit per cell each */
    WS_BC_PREFIX, /* set bits per chunk of words, their exclusive scan, set bits before every word */
    WS_BC_LABEL,  /* int32 per cell: the root of its cluster */
    WS_BC_SIZE,   /* int32 per cell: the cells of the cluster rooted there */
    WS_BC_OUT,    /* stats, histograms, root counts, largest-cluster keys, and the cluster lists that were asked for */
    WS_BC_FLAG,
    /* ---- minkowski_driver.c ---- */
    WS_MK_TAB,  /* thresholds (fp64), batch offsets */
    WS_MK_IN,   /* staged host field */
    WS_MK_OUT,  /* the level histograms of the 8 element kinds, then counts */
    WS_MK_FLAG,
    /* ---- granulometry_driver.c ---- */
    WS_GR_TAB,    /* squared radii, batch offsets */
    WS_GR_IN,     /* staged host field */
    WS_GR_MASK,   /* one bit per cell, rows padded to whole 64-bit words */
    WS_GR_PREFIX, /* rank scratch of the mask: set bits per chunk, their scan, set bits before every word */
    WS_GR_D2,     /* int32 per cell: the squared distance transform */
    WS_GR_WORK_A, /* int32 per cell: the two boxes a three-pass transform goes through */
    WS_GR_WORK_B,
    WS_GR_LEVEL,  /* int32 per cell, where asked for */
    WS_GR_OUT,    /* stats, covered, eroded, the erosion histogram, deepest-cell keys */
    WS_GR_FLAG,
    /* ---- observe_driver.c ---- */
    WS_OB_TAB,    /* beam weights, lw per slice and per 64 slices, channel counts */
    WS_OB_IN,     /* staged host field */
    WS_OB_MEANS,  /* partial sums of the slices, then their means */
    WS_OB_WORK_A, /* float per cell: what a pass leaves for the next */
    WS_OB_WORK_B,
    WS_OB_OUT,    /* the result on its way to a host array */
    WS_OB_FLAG,

    WS_COUNT
};

#endif
