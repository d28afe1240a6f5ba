"""Velocity corrections on the MI355X (reference: src/py21cmfast/rsds.py:16-255).

``include_dvdr_in_tau21``, ``rsds_shift`` and ``apply_rsds`` keep the reference's signatures, argument
checks and messages.  The dv/dr correction is the kernel of ``csrc/hip/dvdr_periodic_kernels.hip`` behind
``grid_api.dvdr_periodic`` (a periodic line of sight: coeval boxes) or of ``lightcone_kernels.hip``
behind ``grid_api.lightcone_dvdr`` (lightcones); the
shift itself is the gfx950 kernel of ``csrc/hip/rsd_kernels.hip`` behind ``grid_api.rsd_shift``.
Per line of sight the displacement ``v / H(z) / cell_size`` [pixels] is interpolated linearly onto
``n_rsd_subcells`` sub-cells per slice (extrapolated past the end slices, or wrapped when
``periodic``), every sub-cell is deposited by linear cloud-in-cell and the sub-cells are summed back.
Velocities are float32 on the device, as the lightcones and boxes that carry them; the
interpolation and the deposit are fp64 and 64-bit fixed point, so the result is bit-reproducible.

Arrays may be numpy (returned as numpy) or torch CUDA tensors (returned on their device).
"""

from __future__ import annotations

import numpy as np

from . import grid_api as api


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _value(a):
    """The numbers of an astropy Quantity (the reference's pixel displacements), else ``a``."""
    return a.value if hasattr(a, "unit") and hasattr(a, "value") else a


def _f32(a):
    if _is_torch(a):
        import torch

        return a.to(torch.float32).contiguous()
    return np.ascontiguousarray(np.asarray(a), np.float32)


def _like(result, ref):
    """``result`` (float32) as the reference's dtype and kind: numpy stays numpy, torch stays torch."""
    if _is_torch(ref):
        return result if result.dtype == ref.dtype else result.to(ref.dtype)
    return result.astype(np.asarray(ref).dtype, copy=False) if np.asarray(ref).dtype.kind == "f" else result


def include_dvdr_in_tau21(brightness_temp, los_velocity, redshifts, inputs, periodic: bool, tau_21=None):
    """The brightness temperature with the velocity-gradient correction (rsds.py:16-103):
    ``brightness_temp`` (2-D ``(ncoords, nslices)`` or 3-D, the line of sight last) and the line-of-sight
    velocity ``los_velocity`` [Mpc/s] of every cell; ``redshifts``: one per slice, or a float (a coeval
    box); ``inputs``: a ``drivers.Inputs``; ``tau_21``: required with USE_TS_FLUCT.  ``periodic``: the
    gradient is the spectral derivative along the last axis, whose length is the period (the reference's
    ``irfftn(1j k_z rfftn(v))``); else ``np.gradient`` with second-order ends.  Returns a new array of the
    kind of ``brightness_temp``; no input is written."""
    if tau_21 is None and inputs.astro_options.USE_TS_FLUCT:
        raise ValueError("tau_21 is not provided, but inputs.astro_options.USE_TS_FLUCT is True!")
    if hasattr(redshifts, "__len__") and len(redshifts) != brightness_temp.shape[-1]:
        raise ValueError("Redshifts must be a float or array with the same size as number of LoS slices")
    if tuple(los_velocity.shape) != tuple(brightness_temp.shape):
        raise ValueError("brightness_temp must be an array with the same shape as los_velocity")
    if brightness_temp.ndim not in (2, 3):
        raise ValueError("brightness_temp must be a 2-D (ncoords, nslices) or 3-D (n, n, nslices) array")
    from .drivers import FlatCosmology

    so, cp = inputs.simulation_options, inputs.cosmo_params
    cosmo = FlatCosmology(cp.hlittle, cp.OMm)
    z = np.broadcast_to(np.asarray(redshifts, np.float64), (brightness_temp.shape[-1],))
    hubble = cosmo.H0_cgs * cosmo.efunc(z)  # 1/s
    cell = float(so.BOX_LEN) / float(so.HII_DIM)  # Mpc
    max_dvdr = float(inputs.astro_params.MAX_DVDR)
    tau = _f32(tau_21) if inputs.astro_options.USE_TS_FLUCT else None
    if periodic:
        out = api.dvdr_periodic(_f32(brightness_temp), _f32(los_velocity), hubble, cell, max_dvdr, tau_21=tau)
    else:  # in place in the library: on a copy
        bt = _f32(brightness_temp)
        out = bt.clone() if _is_torch(bt) else bt.copy()
        api.lightcone_dvdr(out, _f32(los_velocity), hubble, cell, max_dvdr, tau_21=tau)
    return _like(out, brightness_temp)


def rsds_shift(field, los_displacement, n_rsd_subcells: int = 4, periodic: bool = False):
    """Shift the cells of ``field`` (shape ``(nslices, ncoords)``) along the line of sight (axis 0) by
    ``los_displacement`` pixels (same shape; ``v / H(z) / cell_size``), on ``n_rsd_subcells`` sub-cells
    per slice; ``periodic`` wraps the line of sight, else what leaves it is lost (rsds.py:184-255)."""
    los_displacement = _value(los_displacement)
    if field.shape[0] < 2:
        raise ValueError("field must have at least 2 slices")
    if tuple(los_displacement.shape) != tuple(field.shape):
        raise ValueError("field must be an array with the same shape as los_displacement")
    if not isinstance(n_rsd_subcells, (int, np.integer)) or isinstance(n_rsd_subcells, bool):
        raise ValueError("n_rsd_subcells must be an integer")
    if n_rsd_subcells < 1:
        raise ValueError("n_rsd_subcells must be at least 1")
    if field.ndim != 2:
        raise ValueError("field must have shape (nslices, ncoords)")
    # the kernel wants the line of sight last: columns of slices
    f = _f32(field.T)
    d = _f32(los_displacement.T)
    out = api.rsd_shift([f], d, 1.0, n_sub=int(n_rsd_subcells), periodic=periodic)[0]
    return _like(out.T, field)


def apply_rsds(field, los_velocity, redshifts, inputs, periodic: bool, n_rsd_subcells: int = 4):
    """Apply redshift-space distortions to ``field`` (2-D ``(ncoords, nslices)`` or 3-D
    ``(HII_DIM, HII_DIM, nslices)``, the line of sight last) with the line-of-sight velocity
    ``los_velocity`` [Mpc/s] of every cell (rsds.py:106-181).  ``redshifts``: one per slice, or a
    float (a coeval box); ``inputs``: a ``drivers.Inputs`` (cosmology and cell size)."""
    from .drivers import FlatCosmology

    if hasattr(redshifts, "__len__") and len(redshifts) != field.shape[-1]:
        raise ValueError("Redshifts must be a float or array with the same size as number of LoS slices")
    if field.ndim not in (2, 3):
        raise ValueError("field must be a 2-D (ncoords, nslices) or 3-D (n, n, nslices) array")
    if field.shape[-1] < 2:
        raise ValueError("field must have at least 2 slices")
    if tuple(los_velocity.shape) != tuple(field.shape):
        raise ValueError("field must be an array with the same shape as los_displacement")
    if not isinstance(n_rsd_subcells, (int, np.integer)) or isinstance(n_rsd_subcells, bool):
        raise ValueError("n_rsd_subcells must be an integer")
    if n_rsd_subcells < 1:
        raise ValueError("n_rsd_subcells must be at least 1")
    so, cp = inputs.simulation_options, inputs.cosmo_params
    cosmo = FlatCosmology(cp.hlittle, cp.OMm)
    z = np.broadcast_to(np.asarray(redshifts, np.float64), (field.shape[-1],))
    hubble = cosmo.H0_cgs * cosmo.efunc(z)  # 1/s
    cell = float(so.BOX_LEN) / float(so.HII_DIM)  # Mpc
    out = api.rsd_shift([_f32(field)], _f32(los_velocity), 1.0 / (hubble * cell), n_sub=int(n_rsd_subcells),
                        periodic=periodic)[0]
    return _like(out, field)
