"""numpy restatement of the reference's rectilinear lightconer, written as literally as the reference
code reads, for the lightcone tests to compare against (reference: src/py21cmfast/lightconers.py
make_lightcone_slices :162-287, redshift_interpolation :295-319, RectilinearLightconer.coeval_subselect
:505-515; rsds.py include_dvdr_in_tau21 :16-103 with periodic = False).  Distances are plain floats:
Mpc for comoving distances, pixels (of ``cell`` Mpc) where the reference converts to pixels."""

from __future__ import annotations

import numpy as np


def coeval_subselect(lcd_pix, coeval, lc_pix, index_offset):
    """RectilinearLightconer.coeval_subselect: the plane that lines the back of the lightcone up with
    the back of the node box, modulo index_offset."""
    lcidx = int(lc_pix.max() - lcd_pix + 1)
    return coeval.take(-lcidx + index_offset, axis=2, mode="wrap")


def subselect_plane(lcd_pix, lc_pix, index_offset, d_para):
    """The index coeval_subselect takes, as a number (numpy's mode="wrap" is Python's modulo)."""
    lcidx = int(lc_pix.max() - lcd_pix + 1)
    return (-lcidx + index_offset) % d_para


def redshift_interpolation(dc, coeval_a, coeval_b, dc_a, dc_b, kind="mean"):
    out = (np.abs(dc_b - dc) * coeval_a.astype(np.float64) + np.abs(dc_a - dc) * coeval_b.astype(np.float64)) / np.abs(
        dc_a - dc_b)
    if kind == "mean_max":
        flag = coeval_a * coeval_b < 0
        out[flag] = np.maximum(coeval_a, coeval_b)[flag]
    elif kind != "mean":
        raise ValueError("kind must be 'mean' or 'mean_max'")
    return out


def slice_indices(lc_distances, d1, d2, cell):
    """lcidx of make_lightcone_slices for the nodes at comoving distances d1, d2 [Mpc]."""
    pix = np.asarray(lc_distances) / cell
    dc1, dc2 = d1 / cell, d2 / cell
    dcmin, dcmax = min(dc1, dc2), max(dc1, dc2)
    return np.nonzero((pix >= dcmin * (1 - 1e-6)) & (pix < dcmax))[0]


def tables(lc_distances, d_lo, d_hi, cell, index_offset, d_para):
    """(indices, planes, w_lo, w_hi, w_norm) slice by slice, as the loop of make_lightcone_slices
    computes them for the pair (c1 = low-redshift node, c2 = high-redshift node)."""
    pix = np.asarray(lc_distances) / cell
    dc1, dc2 = d_lo / cell, d_hi / cell
    idx = slice_indices(lc_distances, d_lo, d_hi, cell)
    planes, w_lo, w_hi = [], [], []
    for i in idx:
        lcd = pix[i]
        planes.append(subselect_plane(lcd, pix, index_offset, d_para))
        w_lo.append(np.abs(dc2 - lcd))
        w_hi.append(np.abs(dc1 - lcd))
    return idx, np.array(planes, int), np.array(w_lo), np.array(w_hi), np.abs(dc1 - dc2)


def fill_slices(lightcones, lc_distances, d_lo, d_hi, cell, boxes_lo, boxes_hi, index_offset,
                interp_kinds=None):
    """One node pair of the node loop (drivers/lightcone.py:544-575): every slice between the two
    nodes, every quantity, written into ``lightcones[q][..., idx]`` (float32)."""
    interp_kinds = {"z_reion": "mean_max"} if interp_kinds is None else interp_kinds
    pix = np.asarray(lc_distances) / cell
    dc1, dc2 = d_lo / cell, d_hi / cell
    for idx in slice_indices(lc_distances, d_lo, d_hi, cell):
        lcd = pix[idx]
        for q, lc in lightcones.items():
            src = "velocity_z" if q == "los_velocity" else q
            b1 = coeval_subselect(lcd, boxes_lo[q], pix, index_offset)
            b2 = coeval_subselect(lcd, boxes_hi[q], pix, index_offset)
            lc[..., idx] = redshift_interpolation(lcd, b1, b2, dc1, dc2, kind=interp_kinds.get(src, "mean"))


def include_dvdr_in_tau21(brightness_temp, los_velocity, hubble, dx, max_dvdr, tau_21=None):
    """rsds.include_dvdr_in_tau21 with periodic = False; ``hubble`` H(z) [1/s] per slice, velocities in
    Mpc/s.  Returns float32."""
    vel_gradient = np.gradient(los_velocity.astype(np.float64), dx, axis=-1, edge_order=2)
    H = np.asarray(hubble, np.float64)
    if tau_21 is None:
        max_v_deriv = max_dvdr * H
        dvdx = np.clip(vel_gradient, -max_v_deriv, max_v_deriv)
        gradient_component = np.abs(1.0 + dvdx / H)
        return (brightness_temp / gradient_component).astype(np.float32)
    tau = np.float64(tau_21)
    gradient_component = np.abs(1.0 + vel_gradient / H)
    with np.errstate(divide="ignore", invalid="ignore"):
        gradient_factor = (1.0 - np.exp(-tau / gradient_component)) / (1.0 - np.exp(-tau))
    gradient_factor = np.float32(np.where(tau < 1e-10, 1.0, gradient_factor))
    return brightness_temp * gradient_factor
