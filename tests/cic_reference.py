"""Plain numpy float64 restatement of the low-resolution ComputePerturbedField density: the
independent high-precision reference the CIC deposit kernels (and the oracle) are held to.

Reference: map_mass.c:23-60 (do_cic_interpolation), :146-208 (move_grid_masses) and
PerturbedField.c:180-282 (normalise_delta_grid, smooth_and_clip_density without smoothing).
Everything is float64: the masses are summed with np.bincount over the 8 CIC corners, the
transform round trip is numpy's double FFT, so the result carries ~1e-15 relative error."""

import os

import numpy as np

FRACT_FLOAT_ERR = 1e-7  # Constants.h: the density floor -1 + FRACT_FLOAT_ERR


def displacement_factors(spec):
    """velocity_displacement_factor[_2LPT] of map_mass.c:160-173, per axis, in hi-res cells."""
    dens_dim = (spec.dim, spec.dim, spec.dim_z)
    box = (spec.box_len, spec.box_len, spec.box_len_z)
    g, gi = spec.growth_factor, spec.init_growth_factor
    d2, id2 = -(3.0 / 7.0) * g * g, -(3.0 / 7.0) * gi * gi
    vdf = [(g - gi) / box[a] * dens_dim[a] for a in range(3)]
    vdf2 = [(d2 - id2) / box[a] * dens_dim[a] for a in range(3)]
    return vdf, vdf2


def deposit_f64(spec, ics, chunk=1 << 22):
    """move_grid_masses onto the low-resolution grid, summed in float64 (map_mass.c:146-208)."""
    dens = ics["hires_density"]
    dens_dim = dens.shape
    vel_dim = out_dim = (spec.hii_dim, spec.hii_dim, spec.hii_dim_z)
    assert dens_dim == (spec.dim, spec.dim, spec.dim_z) and not spec.perturb_on_high_res
    ratio_vel = vel_dim[0] / dens_dim[0]  # dim_ratio_vel = dim_ratio_out (low-res branch)
    ratio_out = out_dim[0] / dens_dim[0]
    vdf, vdf2 = displacement_factors(spec)
    lpt2 = spec.perturb_algorithm == 2
    vel = [ics[f"lowres_v{ax}"] for ax in "xyz"]
    vel2 = [ics[f"lowres_v{ax}_2LPT"] for ax in "xyz"] if lpt2 else None
    # resample_index + wrap_coord (indexing.h:110-114), per axis
    rs = [(np.arange(dens_dim[a]) * ratio_vel + 0.5).astype(np.int64) % vel_dim[a] for a in range(3)]
    nout = int(np.prod(out_dim))
    acc = np.zeros(nout, np.float64)
    flat = dens.reshape(-1)
    for start in range(0, flat.size, chunk):
        t = np.arange(start, min(start + chunk, flat.size), dtype=np.int64)
        src = np.unravel_index(t, dens_dim)
        vi = np.ravel_multi_index([rs[a][src[a]] for a in range(3)], vel_dim)
        lo_idx, dist = [], []
        for a in range(3):
            pos = src[a].astype(np.float64)
            pos += vel[a].reshape(-1)[vi].astype(np.float64) * vdf[a]
            if lpt2:
                pos -= vel2[a].reshape(-1)[vi].astype(np.float64) * vdf2[a]
            pos *= ratio_out
            ip = np.floor(pos)
            dist.append(pos - ip)
            lo_idx.append(ip.astype(np.int64))
        mass = 1.0 + flat[t].astype(np.float64) * spec.init_growth_factor
        for cx in (0, 1):
            for cy in (0, 1):
                for cz in (0, 1):
                    idx = np.ravel_multi_index(
                        [(lo_idx[a] + c) % out_dim[a] for a, c in zip(range(3), (cx, cy, cz))], out_dim)
                    w = mass.copy()
                    for a, c in zip(range(3), (cx, cy, cz)):
                        w *= dist[a] if c else 1.0 - dist[a]
                    acc += np.bincount(idx, weights=w, minlength=nout)
    return acc.reshape(out_dim)


def perturbed_density_f64(spec, ics):
    """Low-resolution PerturbedField density (no smoothing) in float64: deposit, normalise_delta_grid,
    the r2c / c2r round trip with / N, and the floor at -1 + FRACT_FLOAT_ERR."""
    assert not spec.smooth_evolved_density
    acc = deposit_f64(spec, ics)
    mass_factor = acc.size / float(spec.dim * spec.dim * spec.dim_z)  # HII_TOT_NUM_PIXELS / TOT_NUM_PIXELS
    delta = acc * mass_factor - 1.0
    delta = np.fft.irfftn(np.fft.rfftn(delta), s=delta.shape, axes=(0, 1, 2))
    return np.where(delta < -1.0 + FRACT_FLOAT_ERR, -1.0 + FRACT_FLOAT_ERR, delta)


def density_error(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())


def geometry_ics(n, nz, f, hires, disp, seed):
    """Random ICs on an HII n x n x nz / DIM f n x f n x f nz box (hires: DIM 2 n x 2 n x 2 nz, velocities
    on it) whose first-order displacements are `disp` output cells rms per axis.  The first velocity
    plane of every axis -- the one whose F = 2 ... 4 source planes wrap around the box (lo < 0) --
    moves three times as far."""
    from test_oracle_perturb import perturb_spec

    rng = np.random.default_rng(seed)
    r = 2 if hires else f  # perturb_on_high_res: the deposit runs on the DIM = 2 HII_DIM grid (F = 1)
    N, Nz = r * n, r * nz
    L = 1.5 * n
    vshape = (N, N, Nz) if hires else (n, n, nz)
    pre = "hires" if hires else "lowres"
    per_unit = (0.12 - 0.0042) * n / L  # output cells per unit velocity (map_mass.c:165-173)
    ics = {}
    for ax in "xyz":
        v = disp / per_unit * rng.standard_normal(vshape)
        v[0] *= 3.0
        v[:, 0] *= 3.0
        v[:, :, 0] *= 3.0
        ics[f"{pre}_v{ax}"] = v.astype(np.float32)
        ics[f"{pre}_v{ax}_2LPT"] = (0.5 * disp / per_unit * rng.standard_normal(vshape)).astype(np.float32)
    d = (2.0 * rng.standard_normal((N, N, Nz))).astype(np.float32)
    ics["hires_density"] = d - d.mean()
    ics["lowres_density"] = np.zeros((n, n, nz), np.float32)
    spec = perturb_spec(2, dim=N, dim_z=Nz, hii_dim=n, hii_dim_z=nz, box_len=L, box_len_z=L * nz / n,
                        growth_factor=0.12, init_growth_factor=0.0042, keep_3d_velocities=1,
                        dDdt_over_D=2.1e-17, perturb_on_high_res=1 if hires else 0)
    return spec, ics


# (HII_DIM, HII_D_PARA, F = DIM / HII_DIM, hi-res velocities): the cell kernel's tile is 16 x 16 x 24 output
# cells for F >= 2 (15 x 15 x 23 for F = 1), so every output axis is at least that long; 40, 50, 20, 18 and 28
# leave partial 8 x 8 x 16 bricks
CELL_GEOMETRIES = [(40, 40, 1, False), (24, 24, 1, True), (40, 40, 2, False), (40, 24, 2, False),
                   (24, 24, 3, False), (20, 50, 3, False), (24, 24, 4, False), (18, 28, 4, False)]


def oracle_threads():
    """Threads for the oracle in a full-size test: at most the 16 CPUs a GPU job may use."""
    return min(16, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1))


CIC_PATHS = {1: "cell", 2: "tiled", 3: "direct"}


def cic_last_path(api):
    """Which deposit kernel the last ComputePerturbedField ran (c21hip_cic_last_path)."""
    import ctypes as C

    fn = api.load().c21hip_cic_last_path
    fn.restype, fn.argtypes = C.c_int, []
    return CIC_PATHS.get(fn())
