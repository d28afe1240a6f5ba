"""Boxes and lightcones as a radio interferometer would image them.

The statistics of ``powerspec`` take the simulation's raw brightness temperature.  The papers they come from (Kakiichi
et al. 2017, Giri et al. 2018, Friedrich et al. 2011) apply them to what an array resolves, in the ``smooth_coeval`` /
``smooth_lightcone`` convention of tools21cm: the mean of every frequency slice is removed (an interferometer does not
measure k_perp = 0), every slice is smoothed with a Gaussian beam whose FWHM is the resolution lambda / B of the
longest baseline B at the slice's redshift, and the line of sight with a top-hat channel matched to that width.
``smooth_lightcone`` and ``smooth_coeval`` do that on the MI355X (``csrc/hip/observe_kernels.hip`` behind
``grid_api.observe_smooth``; the definition is written down at ``c21cm_observe_smooth_grids``, include/c21cm_grid.h,
and its numpy spec is ``tests/observe_reference.py``); their result feeds the ``lightcone_*`` and ``get_*`` statistics
unchanged.  The helpers that turn a baseline into widths in cells are plain numpy.

Arrays may be numpy (results are numpy) or torch CUDA tensors (results are torch tensors on the same device; the field
never visits the host).  Argument errors are ``ValueError`` and are raised before the library is loaded; a non-finite
field value raises ``BackendError`` (InfinityorNaNError).
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from . import grid_api as api
from .powerspec import _cubic_cell, _f32, _lengths, _shape

LAMBDA_21_M = 0.21106114054  # m
NU_21_MHZ = 1420.40575177  # MHz
FWHM_PER_SIGMA = 2.0 * np.sqrt(2.0 * np.log(2.0))
_GUARD = 1e-12  # relative, on the comparisons that decide whether a slice is inside a channel


@functools.lru_cache(maxsize=1)
def _default_cosmo():
    from .drivers import FlatCosmology, Inputs

    cp = Inputs().cosmo_params
    return FlatCosmology(cp.hlittle, cp.OMm)


def _redshifts(redshifts, what="redshifts") -> np.ndarray:
    z = np.asarray(redshifts, np.float64)
    if z.ndim > 1 or not np.all(np.isfinite(z)) or np.any(z < 0):
        raise ValueError(f"{what} must be a scalar or a 1-D array of finite values >= 0")
    return z


def _positive(x, what) -> float:
    if isinstance(x, (bool, np.bool_)) or np.ndim(x) != 0 or not np.isfinite(float(x)) or float(x) <= 0:
        raise ValueError(f"{what} must be a positive, finite number")
    return float(x)


def _widths(width, n: int, what: str) -> np.ndarray:
    w = np.asarray(width, np.float64)
    if w.ndim > 1 or (w.ndim == 1 and w.shape != (n,)):
        raise ValueError(f"{what} must be a scalar or one value per slice ({n})")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"{what} must be finite and >= 0")
    return np.broadcast_to(w, (n,))


def angular_resolution(redshifts, max_baseline_km=2.0):
    """theta = lambda_21 (1 + z) / B in radians: the resolution of an array whose longest baseline is
    ``max_baseline_km``, at the redshifted 21 cm line."""
    z = _redshifts(redshifts)
    b = _positive(max_baseline_km, "max_baseline_km")
    return LAMBDA_21_M * (1.0 + z) / (b * 1000.0)


def beam_fwhm(redshifts, max_baseline_km=2.0, cosmo=None):
    """theta D_c(z) in comoving Mpc, with ``drivers.FlatCosmology.comoving_distance``; the default cosmology is the
    one ``drivers.Inputs()`` carries."""
    theta = angular_resolution(redshifts, max_baseline_km)
    cosmo = _default_cosmo() if cosmo is None else cosmo
    return theta * cosmo.comoving_distance(_redshifts(redshifts))


def beam_sigma_cells(redshifts, cell_size, max_baseline_km=2.0, cosmo=None):
    """The beam's Gaussian sigma in cells of ``cell_size`` [Mpc]: FWHM / (2 sqrt(2 ln 2)) / cell."""
    cell = _positive(cell_size, "cell_size")
    return beam_fwhm(redshifts, max_baseline_km, cosmo) / FWHM_PER_SIGMA / cell


def _windows(x: np.ndarray, width: np.ndarray):
    """below, above: the slices j on either side of s with |x_j - x_s| <= width_s / 2, for monotonic x"""
    n = len(x)
    if n > 1 and x[0] > x[-1]:
        x = -x
    if np.any(np.diff(x) <= 0):
        raise ValueError("the slices must be strictly monotonic along the line of sight")
    half = 0.5 * width + _GUARD * (np.max(np.abs(x)) if n else 0.0)
    s = np.arange(n)
    first = np.searchsorted(x, x - half, side="left")
    last = np.searchsorted(x, x + half, side="right") - 1
    return (s - first).astype(np.int32), (last - s).astype(np.int32)


def los_windows(distances_or_redshifts, width, *, redshifts=False, cosmo=None):
    """The int32 arrays ``(below, above)``: for every slice s the number of slices j < s and j > s with |d_j - d_s| <=
    width_s / 2, d the slices' comoving distances [Mpc] -- given as such, or with ``redshifts=True`` computed from the
    slices' redshifts (``cosmo`` as in ``beam_fwhm``).  ``width``: a scalar or one value per slice, Mpc.  The
    comparison carries a relative guard of 1e-12, so that a slice exactly half a width away is inside."""
    if redshifts:
        z = np.atleast_1d(_redshifts(distances_or_redshifts))
        d = np.asarray((_default_cosmo() if cosmo is None else cosmo).comoving_distance(z), np.float64)
    else:
        d = np.atleast_1d(np.asarray(distances_or_redshifts, np.float64))
        if d.ndim != 1 or not np.all(np.isfinite(d)):
            raise ValueError("distances must be a 1-D array of finite values")
    return _windows(d, _widths(width, len(d), "width"))


def los_windows_mhz(redshifts, channel_width_mhz):
    """``los_windows`` in frequency: the slices with |nu_j - nu_s| <= channel_width / 2, nu = 1420.40575177 / (1 + z)
    MHz.  A channel of fixed width in frequency is longer in Mpc, and holds more slices, at the high-redshift end."""
    z = np.atleast_1d(_redshifts(redshifts))
    return _windows(NU_21_MHZ / (1.0 + z), _widths(channel_width_mhz, len(z), "channel_width_mhz"))


@dataclass
class ObservedField:
    """What ``smooth_lightcone`` and ``smooth_coeval`` return.  ``field``: the smoothed field, of the kind and on the
    device of the input; ``slice_means`` float64 (ns,): the mean of every slice of the input (subtracted or not);
    ``fwhm`` [Mpc], ``sigma_cells``, ``los_below`` and ``los_above`` (ns,), numpy: the beam and the channel of every
    slice as they were passed to the library; ``angular_resolution`` [arcmin] (ns,): the beam as an angle."""

    field: object
    slice_means: object
    fwhm: np.ndarray
    sigma_cells: np.ndarray
    los_below: np.ndarray
    los_above: np.ndarray
    angular_resolution: np.ndarray


def _check_sigma(sigma):
    if np.any(sigma > api.OBSERVE_MAX_SIGMA):
        raise ValueError(f"the beam is {float(np.max(sigma)):.4g} cells wide (sigma); the limit is "
                         f"{api.OBSERVE_MAX_SIGMA:g}")


def _arcmin(fwhm, z, max_baseline_km, given, cosmo):
    if not given:
        return np.degrees(angular_resolution(z, max_baseline_km)) * 60.0
    return np.degrees(fwhm / np.asarray(cosmo.comoving_distance(z), np.float64)) * 60.0


def smooth_lightcone(lightcone, cell_size, redshifts, *, max_baseline_km=2.0, los_ratio=1.0, fwhm=None,
                     los_width=None, channel_width_mhz=None, subtract_mean=True, cosmo=None) -> ObservedField:
    """The rectilinear ``lightcone`` (nx, ny, n_slices) of cells of ``cell_size`` [Mpc] at the resolution of an array
    with a longest baseline of ``max_baseline_km``.  ``redshifts``: those of the slices (``lightconer.lc_redshifts``).
    Per slice: its mean is removed (``subtract_mean``); it is smoothed, wrapping, with a Gaussian of FWHM =
    ``beam_fwhm`` at its redshift, truncated at 4 sigma -- or of ``fwhm`` [Mpc, a scalar or one per slice] where
    given; and it becomes the mean of the slices within half a channel of it along the open line of sight.  The
    channel is ``channel_width_mhz`` [MHz] where given; else ``los_width`` [Mpc, a scalar or per slice; 0 switches
    it off] where given; else ``los_ratio`` times the slice's FWHM.  The slices are ``cell_size`` apart."""
    if lightcone.ndim != 3:
        raise ValueError(f"lightcone must be a 3-D (nx, ny, n_slices) array, got {lightcone.ndim} dimensions")
    nx, ny, ns = _shape(lightcone)
    cell = _positive(cell_size, "cell_size")
    z = _redshifts(redshifts)
    if z.shape != (ns,):
        raise ValueError(f"redshifts must hold one value per slice ({ns}), got shape {z.shape}")
    if channel_width_mhz is not None and los_width is not None:
        raise ValueError("give channel_width_mhz or los_width, not both")
    if isinstance(los_ratio, (bool, np.bool_)) or np.ndim(los_ratio) != 0 or not (
            np.isfinite(float(los_ratio)) and float(los_ratio) >= 0):
        raise ValueError("los_ratio must be a finite number >= 0")
    cosmo = _default_cosmo() if cosmo is None else cosmo
    given = fwhm is not None
    width = np.array(_widths(fwhm, ns, "fwhm")) if given else np.asarray(beam_fwhm(z, max_baseline_km, cosmo))
    sigma = width / FWHM_PER_SIGMA / cell
    _check_sigma(sigma)
    if channel_width_mhz is not None:
        below, above = los_windows_mhz(z, channel_width_mhz)
    else:
        channel = float(los_ratio) * width if los_width is None else _widths(los_width, ns, "los_width")
        below, above = _windows(np.arange(ns) * cell, channel)
    out, means = api.observe_smooth(_f32(lightcone), sigma, below, above, periodic_los=False,
                                    subtract_mean=bool(subtract_mean))
    return ObservedField(field=out, slice_means=means, fwhm=width, sigma_cells=sigma, los_below=below,
                         los_above=above, angular_resolution=_arcmin(width, z, max_baseline_km, given, cosmo))


def smooth_coeval(box, boxlength, redshift, *, max_baseline_km=2.0, los_ratio=1.0, fwhm=None, los_width=None,
                  subtract_mean=True, cosmo=None) -> ObservedField:
    """The coeval ``box`` (nx, ny, nz) in a box of ``boxlength`` (a scalar or 3 lengths) at ``redshift``, as
    ``smooth_lightcone`` with one width for all slices: the line of sight is the last axis and, like the others,
    periodic.  The cells must be square across the line of sight.  The channel spans ``los_width`` [Mpc; 0 switches
    it off] where given, else ``los_ratio`` times the FWHM: floor(width / (2 cell_z)) slices on either side."""
    if box.ndim != 3:
        raise ValueError(f"box must be a 3-D array, got {box.ndim} dimensions")
    shape = _shape(box)
    L = _lengths(boxlength)
    cell = _cubic_cell(L[:2], shape[:2])
    cell_z = L[2] / shape[2]
    z = _redshifts(redshift, "redshift")
    if z.ndim != 0:
        raise ValueError("a coeval box has one redshift")
    if isinstance(los_ratio, (bool, np.bool_)) or np.ndim(los_ratio) != 0 or not (
            np.isfinite(float(los_ratio)) and float(los_ratio) >= 0):
        raise ValueError("los_ratio must be a finite number >= 0")
    cosmo = _default_cosmo() if cosmo is None else cosmo
    given = fwhm is not None
    if given and np.ndim(fwhm) != 0:
        raise ValueError("a coeval box takes one fwhm")
    width = float(_widths(fwhm, 1, "fwhm")[0]) if given else float(beam_fwhm(z, max_baseline_km, cosmo))
    if los_width is not None and np.ndim(los_width) != 0:
        raise ValueError("a coeval box takes one los_width")
    channel = float(los_ratio) * width if los_width is None else float(_widths(los_width, 1, "los_width")[0])
    ns = shape[2]
    half = int(np.floor(channel / (2.0 * cell_z) * (1.0 + _GUARD)))
    if 2 * half + 1 > ns:
        raise ValueError(f"the channel of {channel:.4g} Mpc spans {2 * half + 1} slices, the box has {ns}")
    sigma = np.full(ns, width / FWHM_PER_SIGMA / cell)
    _check_sigma(sigma)
    below = np.full(ns, half, np.int32)
    out, means = api.observe_smooth(_f32(box), sigma, below, below.copy(), periodic_los=True,
                                    subtract_mean=bool(subtract_mean))
    zs = np.full(ns, float(z))
    return ObservedField(field=out, slice_means=means, fwhm=np.full(ns, width), sigma_cells=sigma, los_below=below,
                         los_above=below.copy(),
                         angular_resolution=_arcmin(np.full(ns, width), zs[:1], max_baseline_km, given, cosmo)
                         * np.ones(ns))
