"""numpy fp64 restatement of the reference's ComputePerturbedHaloCatalog
(src/py21cmfast/src/PerturbedHaloCatalog.c:25-149) and convert_halo_props (HaloBox.c:781-880, with
set_halo_properties :62-102, the scaling relations scaling_relations.c:209-240,277-283,326-501 and
cic_read_float, map_mass.c:102-140), written from that C.  It takes the explicit scalars of
``c21cm_perturb_halos_grids``: the two displacement factors, the grid dimensions, the box size, the halo
constants (anything with the fields of ``c21cm_halo_consts``) and the optional turnover grids."""

import numpy as np

S_PER_YR = 31556925.9747  # physconst.s_per_yr


def wrap_coord(idx, size):
    """indexing.c:37-58 for an integer array"""
    return np.mod(idx, size)


def wrap_position(pos, size):
    """indexing.c:14-35: subtract, then add, the box length until the position is inside (each step
    rounds; a sum that rounds up to the box length stays there, as in C)"""
    pos = pos.copy()
    while True:
        m = pos >= size
        if not m.any():
            break
        pos[m] -= size
    while True:
        m = pos < 0
        if not m.any():
            break
        pos[m] += size
    return pos


def perturb_coords(coords, vel, vel2, vel_dim, box_size, vdf, vdf2):
    """PerturbedHaloCatalog.c:107-131.  coords [n, 3] float32 (Mpc); vel / vel2: three float32 grids of
    shape vel_dim each (vel2 None: Zel'dovich); box_size: the three wrap lengths.  Returns the fp64
    positions before the store; the catalogue holds their float32."""
    pos = np.asarray(coords, np.float32).astype(np.float64)
    cell_size_inv = vel_dim[0] / box_size[0]
    # pos_to_index: (int)(pos * cell_size_inv + 0.5) truncates towards zero
    ipos = np.trunc(pos * cell_size_inv + 0.5).astype(np.int64)
    for a in range(3):
        ipos[:, a] = wrap_coord(ipos[:, a], vel_dim[a])
    out = np.empty_like(pos)
    for a in range(3):
        p = pos[:, a] + vel[a][ipos[:, 0], ipos[:, 1], ipos[:, 2]].astype(np.float64) * vdf
        if vel2 is not None:
            p = p - vel2[a][ipos[:, 0], ipos[:, 1], ipos[:, 2]].astype(np.float64) * vdf2
        out[:, a] = wrap_position(p, box_size[a])
    return out


def cic_read(box, pos):
    """cic_read_float (map_mass.c:102-140): pos [n, 3] in cells of ``box``; the sum runs in the C order"""
    dim = box.shape
    ip = np.floor(pos).astype(np.int64)
    d = pos - ip
    i0 = [wrap_coord(ip[:, a], dim[a]) for a in range(3)]
    i1 = [wrap_coord(ip[:, a] + 1, dim[a]) for a in range(3)]
    total = np.zeros(len(pos))
    for k in range(8):  # x fastest, then y, then z: the order of cic_indices / cic_weights
        sel = [(k >> a) & 1 for a in range(3)]
        idx = tuple(i1[a] if sel[a] else i0[a] for a in range(3))
        w = ((d[:, 0] if sel[0] else 1.0 - d[:, 0]) * (d[:, 1] if sel[1] else 1.0 - d[:, 1])
             * (d[:, 2] if sel[2] else 1.0 - d[:, 2]))
        total = total + box[idx].astype(np.float64) * w
    return total


def set_halo_properties(m, mturn_a, mturn_m, c, r_star, r_sfr, r_xray):
    """HaloBox.c:62-102 for arrays of halos; c: the ScalingConstants and option flags."""
    with np.errstate(all="ignore"):
        adj = 0.0 if c.scaling_median else c.sigma_star**2 / 2.0
        if c.upper_stellar_turnover and c.alpha_star > c.alpha_upper:
            mu = c.fstar_10 * (c.upper_pivot_ratio / ((m / c.pivot_upper) ** (-c.alpha_star)
                                                      + (m / c.pivot_upper) ** (-c.alpha_upper)))
        else:
            mu = c.fstar_10 * (m / 1e10) ** c.alpha_star
        baryon = c.baryon_ratio
        stars = np.minimum(mu * np.exp(-mturn_a / m + r_star * c.sigma_star - adj), 1.0) * m * baryon
        stars_mini = np.zeros_like(m)
        if c.use_mini_halos:
            mu_m = c.fstar_7 * (m / 1e7) ** c.alpha_star_mini
            f_m = mu_m * np.exp(-mturn_m / m - m / c.acg_thresh + r_star * c.sigma_star - adj)
            stars_mini = np.minimum(f_m, 1.0) * m * baryon
        sigma_sfr = np.zeros_like(m)
        if c.sigma_sfr_lim > 0:
            sigma_sfr = np.maximum(c.sigma_sfr_idx * np.log10((stars + stars_mini) / 1e10) + c.sigma_sfr_lim,
                                   c.sigma_sfr_lim)
        adj_sfr = 0.0 if c.scaling_median else sigma_sfr**2 / 2.0
        fac = np.exp(r_sfr * sigma_sfr - adj_sfr)
        sfr = stars / (c.t_star * c.t_h) * fac
        sfr_mini = stars_mini / (c.t_star * c.t_h) * fac if c.use_mini_halos else np.zeros_like(m)
        xray = np.zeros_like(m)
        if c.use_xray:
            sfr_t, stars_t = sfr + sfr_mini, stars + stars_mini
            term = np.ones_like(m)
            ok = (stars_t > 0) & (sfr_t > 0)
            m0 = 1.28825e10 * (sfr_t[ok] * S_PER_YR) ** 0.56
            term[ok] = (1 + (stars_t[ok] / m0) ** -2.1) ** -0.148
            metal = 1.23 * term * 10 ** (-0.056 * c.redshift + 0.064)

            def lx_on_sfr(lx):
                if c.upper_stellar_turnover:  # lx_on_sfr_doublePL: flat below Z = 0.05, index -0.64 above
                    return lx * (1.0 / ((metal / 0.05) ** (-0.0) + (metal / 0.05) ** 0.64))
                return lx

            mu_x = lx_on_sfr(c.l_x) * (sfr * S_PER_YR)
            if c.use_mini_halos:
                mu_x = mu_x + lx_on_sfr(c.l_x_mini) * (sfr_mini * S_PER_YR)
            adj_x = 0.0 if c.scaling_median else c.sigma_xray**2 / 2.0
            xray = mu_x * np.exp(r_xray * c.sigma_xray - adj_x)
        fesc = np.minimum(c.fesc_10 * (m / 1e10) ** c.alpha_esc, 1.0)
        fesc_mini = np.minimum(c.fesc_7 * (m / 1e7) ** c.alpha_esc, 1.0) if c.use_mini_halos else 0.0
        n_ion = stars * c.pop2_ion * fesc + stars_mini * c.pop3_ion * fesc_mini
        wsfr = sfr * c.pop2_ion * fesc + sfr_mini * c.pop3_ion * fesc_mini
    return dict(halo_masses=m, stellar_masses=stars, stellar_mini=stars_mini, sfr=sfr, sfr_mini=sfr_mini,
                fesc_sfr=wsfr, ion_emissivity=n_ion, xray_emissivity=xray)


def perturbed_halo_catalog(cat, vel, vel2, vel_dim, box_size, vdf, vdf2, consts, hii_dim, dim,
                           log10_mturn_acg=None, log10_mturn_mcg=None):
    """Both functions.  cat: dict(masses, coords, star_rng, sfr_rng, xray_rng).  Returns dict with
    ``pos64`` [n, 3] (fp64, before the store), ``halo_coords`` (their float32), ``live`` (mass != 0),
    ``mturn`` (the two turnover masses of the live halos) and the fp64 property arrays of the live
    halos, in catalogue order."""
    pos64 = perturb_coords(cat["coords"], vel, vel2, vel_dim, box_size, vdf, vdf2)
    stored = pos64.astype(np.float32)
    m = cat["masses"].astype(np.float64)
    live = m != 0
    # HaloBox.c:825-827: the stored float coordinate [Mpc] times HII_DIM / DIM, read as cells
    hp = stored[live].astype(np.float64) * (hii_dim / float(dim))
    ml = m[live]
    if consts.use_mini_halos:
        mta = 10.0 ** cic_read(log10_mturn_acg, hp)
        mtm = 10.0 ** cic_read(log10_mturn_mcg, hp)
    else:
        mta = np.full_like(ml, consts.mturn_a_nofb)
        mtm = np.full_like(ml, consts.mturn_m_nofb)
    props = set_halo_properties(ml, mta, mtm, consts, cat["star_rng"][live].astype(np.float64),
                                cat["sfr_rng"][live].astype(np.float64),
                                cat["xray_rng"][live].astype(np.float64))
    return dict(pos64=pos64, halo_coords=stored, live=live, mturn=(mta, mtm), **props)
