"""numpy / scipy restatement of the reference's redshift-space distortions, written as literally as the
reference code reads, for the RSD tests to compare against (reference: src/py21cmfast/rsds.py
apply_rsds :106-181 and rsds_shift :184-255).

The reference deposits with ``cosmotile.cic.cloud_in_cell_los``, a third-party package whose source is
not part of the reference.  ``cloud_in_cell_los`` below is written from what the reference's
tests/test_rsds.py:113-172 pin down: an integer displacement is ``np.roll``, a periodic shift keeps
every column's sum, a displacement of twice the column empties a non-periodic one.  Standard linear
cloud-in-cell does all three: a cell at x = k + d gives (1 - w) to cell floor(x) and w to the next,
w = x - floor(x); periodic indices wrap, non-periodic ones outside the column are lost."""

from __future__ import annotations

import numpy as np
from scipy.interpolate import RegularGridInterpolator


def cloud_in_cell_los(field, displacement, periodic=False):
    """field, displacement: (n_fine, ncoords); axis 0 is the line of sight (fp64)."""
    n = field.shape[0]
    out = np.zeros(field.shape, np.float64)
    coords = np.broadcast_to(np.arange(field.shape[1]), field.shape)
    x = np.arange(n)[:, None] + np.asarray(displacement, np.float64)
    i = np.floor(x)
    w = x - i
    i = i.astype(np.int64)
    for idx, part in ((i, field * (1.0 - w)), (i + 1, field * w)):
        if periodic:
            np.add.at(out, (np.mod(idx, n), coords), part)
        else:
            ok = (idx >= 0) & (idx < n)
            np.add.at(out, (idx[ok], coords[ok]), part[ok])
    return out


def rsds_shift(field, los_displacement, n_rsd_subcells=4, periodic=False):
    """rsds.py:184-255; field and los_displacement (nslices, ncoords), the displacement in pixels."""
    if field.shape[0] < 2:
        raise ValueError("field must have at least 2 slices")
    if los_displacement.shape != field.shape:
        raise ValueError("field must be an array with the same shape as los_displacement")
    if not isinstance(n_rsd_subcells, int):
        raise ValueError("n_rsd_subcells must be an integer")
    if field.shape[1] == 1:  # RegularGridInterpolator wants two points per axis: shift a twin column
        return rsds_shift(np.repeat(field, 2, axis=1), np.repeat(los_displacement, 2, axis=1),
                          n_rsd_subcells, periodic)[:, :1]

    field = np.asarray(field, np.float64)
    los_displacement = np.asarray(los_displacement, np.float64)
    ang_coords = np.arange(field.shape[1])
    distance = np.arange(field.shape[0])
    distance_plus = np.arange(field.shape[0] + 1)
    if periodic:
        distance_plus_periodic = np.arange(-1, field.shape[0] + 2)
        distance_grid = (distance_plus_periodic[1:] + distance_plus_periodic[:-1]) / 2
        first_slice = los_displacement[-1, :].reshape(1, len(ang_coords))
        last_slice = los_displacement[0, :].reshape(1, len(ang_coords))
        los_displacement = np.concatenate((first_slice, los_displacement, last_slice), axis=0)
    else:
        distance_grid = (distance_plus[1:] + distance_plus[:-1]) / 2

    fine_field = np.repeat(field, n_rsd_subcells, axis=0) / n_rsd_subcells
    distance_fine = np.linspace(distance_plus.min(), distance_plus.max(),
                                1 + n_rsd_subcells * (len(distance_plus) - 1))
    fine_grid = (distance_fine[1:] + distance_fine[:-1]) / 2
    x, y = np.meshgrid(fine_grid, ang_coords, indexing="ij")
    grid = (x.flatten(), y.flatten())
    fine_rsd = RegularGridInterpolator((distance_grid, ang_coords), los_displacement * n_rsd_subcells,
                                       bounds_error=False, fill_value=None, method="linear")(grid).reshape(x.shape)
    fine_field = cloud_in_cell_los(fine_field, fine_rsd, periodic=periodic)
    return np.sum(fine_field.T.reshape(len(ang_coords), len(distance), n_rsd_subcells), axis=-1).T


def apply_rsds(field, los_velocity, hubble, cell, periodic, n_rsd_subcells=4):
    """rsds.py:106-181 with H(z) [1/s] of every slice (or one for a coeval box) and the cell size [Mpc]
    given: the displacement v / H / cell_size in pixels; 2-D (ncoords, nslices) or 3-D, the line of
    sight last."""
    los_displacement = np.asarray(los_velocity, np.float64) / np.asarray(hubble, np.float64) / cell
    shape = field.shape
    f2 = np.asarray(field, np.float64).reshape(-1, shape[-1])
    d2 = los_displacement.reshape(-1, shape[-1])
    out = rsds_shift(f2.T, d2.T, n_rsd_subcells=n_rsd_subcells, periodic=periodic).T
    return out.reshape(shape)
