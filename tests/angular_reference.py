"""numpy / scipy restatement of the reference's angular lightconer, for the angular lightcone tests to
compare against (reference: src/py21cmfast/lightconers.py AngularLightconer :541-701 and
make_lightcone_slices :162-287).

The reference interpolates with ``cosmotile.make_lightcone_slice_interpolator`` /
``make_lightcone_slice_vector_field``, a third-party package whose source is not part of the reference.
The convention written here is the one the reference's own tests imply:

- the unit direction of pixel p is u = (cos b cos l, cos b sin l, sin b), rotated: n = R u;
- its point on the slice at comoving distance d [pixels] is x = d n + origin (box-cell units);
- the value is ``scipy.ndimage.map_coordinates(box, x, order, mode="grid-wrap")`` on the fp64
  redshift-interpolated box of that slice (the whole box first, as make_lightcone_slices does);
- ``los_velocity`` is sum_k v_k(x) n_k, the three interpolated components dotted with n."""

from __future__ import annotations

import numpy as np
from scipy import ndimage

import lightcone_reference as LR

# poles of the periodic B-spline prefilter (Unser 1999): cubic, quintic
POLES = {0: (), 1: (), 3: (np.sqrt(3.0) - 2.0,), 5: (-0.4305753470999737, -0.04309628820326465)}


def directions(latitude, longitude, rotation=None):
    """Rotated unit directions, shape (3, n_pix), fp64."""
    b, lon = np.asarray(latitude, np.float64), np.asarray(longitude, np.float64)
    u = np.stack([np.cos(b) * np.cos(lon), np.cos(b) * np.sin(lon), np.sin(b)])
    if rotation is None:
        return u
    R = np.asarray(rotation.as_matrix() if hasattr(rotation, "as_matrix") else rotation, np.float64)
    return R @ u


def points(nhat, d, origin):
    """x = d n + origin for one slice, shape (3, n_pix)."""
    return d * nhat + np.asarray(origin, np.float64)[:, None]


def interpolate(box, x, order):
    return ndimage.map_coordinates(np.asarray(box, np.float64), x, order=order, mode="grid-wrap")


def fill_slices(lightcones, lc_distances, d_lo, d_hi, cell, boxes_lo, boxes_hi, nhat, origin, order,
                interp_kinds=None):
    """One node pair (drivers/lightcone.py:544-575 with an angular lightconer): every slice between the
    two nodes, every quantity, into ``lightcones[q][:, idx]`` (float32).  ``boxes_*["los_velocity"]`` is
    the triple (velocity_x, velocity_y, velocity_z)."""
    interp_kinds = {"z_reion": "mean_max"} if interp_kinds is None else interp_kinds
    pix = np.asarray(lc_distances) / cell
    dc1, dc2 = d_lo / cell, d_hi / cell
    for idx in LR.slice_indices(lc_distances, d_lo, d_hi, cell):
        lcd = pix[idx]
        x = points(nhat, lcd, origin)
        for q, lc in lightcones.items():
            if q == "los_velocity":
                comps = [interpolate(LR.redshift_interpolation(lcd, a, b, dc1, dc2), x, order)
                         for a, b in zip(boxes_lo[q], boxes_hi[q])]
                lc[:, idx] = sum(c * n for c, n in zip(comps, nhat))
                continue
            box = LR.redshift_interpolation(lcd, boxes_lo[q], boxes_hi[q], dc1, dc2,
                                            kind=interp_kinds.get(q, "mean"))
            lc[:, idx] = interpolate(box, x, order)


def periodic_prefilter_1d(c, z, axis):
    """One pole of the periodic B-spline prefilter along ``axis`` (fp64, in place on a copy): the causal
    and anticausal recursions, each started from its sum over the whole period."""
    c = np.moveaxis(np.array(c, np.float64), axis, 0)
    n = c.shape[0]
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    zn = z ** n
    zi = z ** np.arange(n)
    # causal: c+[0] = sum_i z^i s[-i mod n] / (1 - z^n)
    idx = (-np.arange(n)) % n
    c[0] = np.tensordot(zi, c[idx], axes=(0, 0)) / (1.0 - zn)
    for k in range(1, n):
        c[k] = c[k] + z * c[k - 1]
    # anticausal: c-[n-1] = -z / (1 - z^n) sum_i z^i c+[(n - 1 + i) mod n]
    idx = (n - 1 + np.arange(n)) % n
    last = -z / (1.0 - zn) * np.tensordot(zi, c[idx], axes=(0, 0))
    c[n - 1] = last
    for k in range(n - 2, -1, -1):
        c[k] = z * (c[k + 1] - c[k])
    return np.moveaxis(c, 0, axis)


def periodic_prefilter(box, order):
    """The B-spline coefficients of a periodic box (every axis, every pole): what
    ``scipy.ndimage.spline_filter(box, order, mode="grid-wrap")`` computes."""
    c = np.asarray(box, np.float64)
    for axis in range(c.ndim):
        for z in POLES[order]:
            c = periodic_prefilter_1d(c, z, axis)
    return c
