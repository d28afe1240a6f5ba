"""Power spectra of boxes and lightcones, binned on the MI355X.

``get_power`` with its defaults is powerbox's ``get_power(field, boxlength, bins_upto_boxlen=True)``
(restated in ``oracle/powerbox_power.py``): F = (V/N) DFT(f), P = |F|^2 / V, ``int(prod(N)^(1/3) / 2.2)``
linear bins from min|k| to the smallest per-axis maximum of |k|, half-open bins as ``np.digitize``, each
bin the plain mean over the modes of the full grid and ``k`` their mean |k|.  The other options are
written down in ``tests/power_reference.py``, a numpy restatement that is their spec.

The field is transformed in fp32 (rocFFT) and binned in fp64 by the gfx950 kernels of
``csrc/hip/power_kernels.hip`` behind ``grid_api.power_spectrum``; |k| is bit-identical to numpy's, the
counts are exact and two calls give the same bits.  Edges are built here with ``np.linspace`` /
``np.geomspace`` and passed to the kernel.

Arrays may be numpy (results are numpy) or torch CUDA tensors (results are torch tensors on the same
device; the field never visits the host).  Argument errors are ``ValueError``; a non-finite field value
raises ``BackendError`` (InfinityorNaNError).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import grid_api as api


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _f32(a):
    if _is_torch(a):
        import torch

        return a.to(torch.float32).contiguous()
    return np.ascontiguousarray(np.asarray(a), np.float32)


def _shape(a) -> tuple:
    return tuple(int(x) for x in a.shape)


def _lengths(boxlength, dim: int = 3) -> tuple:
    if np.ndim(boxlength) == 0:
        L = (float(boxlength),) * dim
    else:
        L = tuple(float(x) for x in np.asarray(boxlength, np.float64).ravel())
        if len(L) != dim:
            raise ValueError(f"boxlength must be a scalar or {dim} lengths, got {len(L)}")
    if not all(np.isfinite(x) and x > 0 for x in L):
        raise ValueError("box lengths must be positive and finite")
    return L


def k_axis(n: int, length: float) -> np.ndarray:
    """The wavenumbers of one axis in numpy's order: ``fftfreq(n, d=L/n) * 2 pi``."""
    return np.fft.fftfreq(n, d=length / n) * 2.0 * np.pi


def default_nbins(shape) -> int:
    """powerbox's default number of bins for a grid of ``shape``: ``int(prod(N)^(1/dim) / 2.2)``."""
    return int(np.prod(shape) ** (1.0 / len(shape)) / 2.2)


def make_edges(bins, kmin: float, kmax: float, kmin_nonzero: float, log_bins: bool, what: str = "bins"):
    """Bin edges: explicit ``bins`` (1-D, increasing, finite) as given; an int as ``np.linspace(kmin,
    kmax, bins + 1)`` or, with ``log_bins``, ``np.geomspace(kmin_nonzero, kmax, bins + 1)``."""
    if np.ndim(bins) == 0:
        if isinstance(bins, (bool, np.bool_)) or int(bins) != bins:
            raise ValueError(f"{what} must be an integer or an array of edges")
        n = int(bins)
        if n < 1:
            raise ValueError(f"{what} must be >= 1, got {n}")
        if log_bins:
            if not kmin_nonzero > 0 or not kmax > kmin_nonzero:
                raise ValueError(f"log {what} need 0 < the smallest non-zero k < the largest")
            return np.geomspace(kmin_nonzero, kmax, n + 1)
        return np.linspace(kmin, kmax, n + 1)
    e = np.asarray(bins, np.float64)
    if e.ndim != 1 or e.size < 2:
        raise ValueError(f"{what} edges must be a 1-D array of at least 2 values")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError(f"{what} edges must be finite and strictly increasing")
    return e


def spherical_edges(shape, boxlength, bins=None, log_bins=False, bins_upto_boxlen=True):
    """The |k| edges ``get_power`` uses for a grid of ``shape`` (computed from the per-axis wavenumbers:
    |k| never decreases with any |k_i|, so the extremes of the full grid sit on the axes)."""
    axes = [k_axis(n, L) for n, L in zip(shape, _lengths(boxlength, len(shape)))]
    sq = [np.max(k * k) for k in axes]
    if bins_upto_boxlen:
        kmax = min(float(np.sqrt(s)) for s in sq)
    else:
        acc = 0
        for s in sq:
            acc = acc + s
        kmax = float(np.sqrt(acc))
    kmin_nz = min(float(np.sqrt(np.min(k[k != 0] * k[k != 0]))) for k in axes)
    return make_edges(default_nbins(shape) if bins is None else bins, 0.0, kmax, kmin_nz, log_bins)


def cylindrical_edges(shape, boxlength, kperp_bins=None, kpar_bins=None, log_bins=False):
    """The (k_perp, k_par) edges ``get_cylindrical_power`` uses: k_perp from 0 (or its smallest non-zero
    value) to the smaller of max|kx|, max|ky|; k_par = |kz| from 0 (or 2 pi / Lz) to max|kz|; the default
    counts are ``int(sqrt(nx ny) / 2.2)`` and ``int(nz / 2.2)``."""
    L = _lengths(boxlength, 3)
    kx, ky, kz = (k_axis(n, l) for n, l in zip(shape, L))
    perp_max = min(float(np.sqrt(np.max(k * k))) for k in (kx, ky))
    perp_nz = min(float(np.sqrt(np.min(k[k != 0] * k[k != 0]))) for k in (kx, ky))
    par_max = float(np.max(np.abs(kz)))
    par_nz = float(np.min(np.abs(kz[kz != 0])))
    ep = make_edges(default_nbins(shape[:2]) if kperp_bins is None else kperp_bins, 0.0, perp_max, perp_nz,
                    log_bins, "kperp_bins")
    ez = make_edges(default_nbins(shape[2:]) if kpar_bins is None else kpar_bins, 0.0, par_max, par_nz, log_bins,
                    "kpar_bins")
    return ep, ez


def _check_field(field, what="field", deltax2=None):
    if field.ndim != 3:
        raise ValueError(f"{what} must be a 3-D array, got {field.ndim} dimensions")
    if min(_shape(field)) < 2:
        raise ValueError(f"every axis of {what} needs at least 2 cells")
    if deltax2 is not None:
        if _is_torch(deltax2) != _is_torch(field):
            raise ValueError("deltax2 must be the same kind of array (numpy or torch) as the field")
        if _shape(deltax2) != _shape(field):
            raise ValueError(f"deltax2 has shape {_shape(deltax2)}, not that of the field {_shape(field)}")


def get_power(field, boxlength, *, deltax2=None, bins=None, log_bins=False, ignore_zero_mode=False,
              bins_upto_boxlen=True, ignore_kperp_zero=False, ignore_kpar_zero=False, bin_ave=True,
              return_counts=False):
    """Spherically binned power spectrum of the 3-D ``field`` (any shape; the line of sight is the last
    axis) in a box of ``boxlength`` (a scalar or 3 lengths).  Returns ``(power, k[, counts])``: ``k`` the
    mean |k| of each bin, or the edges when ``bin_ave`` is False; empty bins are NaN."""
    _check_field(field, deltax2=deltax2)
    shape = _shape(field)
    L = _lengths(boxlength)
    edges = spherical_edges(shape, L, bins, log_bins, bins_upto_boxlen)
    power, kmean, counts = api.power_spectrum(
        _f32(field), None if deltax2 is None else _f32(deltax2), shape, L, edges,
        ignore_zero_mode=ignore_zero_mode, ignore_kperp_zero=ignore_kperp_zero, ignore_kpar_zero=ignore_kpar_zero)
    k = kmean[0] if bin_ave else _edges_like(edges, power)
    out = (power[0], k)
    return out + (counts[0],) if return_counts else out


def get_cylindrical_power(field, boxlength, *, deltax2=None, kperp_bins=None, kpar_bins=None, log_bins=False,
                          ignore_zero_mode=False, return_counts=False):
    """Cylindrically binned power spectrum: ``(power[n_kperp, n_kpar], kperp, kpar[, counts])`` with
    k_perp = sqrt(kx^2 + ky^2) and k_par = |kz| (the last axis); ``kperp`` / ``kpar`` are the mean
    k_perp / k_par of the modes in each row / column of bins; empty bins are NaN."""
    _check_field(field, deltax2=deltax2)
    shape = _shape(field)
    L = _lengths(boxlength)
    ep, ez = cylindrical_edges(shape, L, kperp_bins, kpar_bins, log_bins)
    power, kmean, counts = api.power_spectrum(
        _f32(field), None if deltax2 is None else _f32(deltax2), shape, L, ep, ez,
        ignore_zero_mode=ignore_zero_mode)
    n = len(ep) - 1
    out = (power[0], kmean[0, :n], kmean[0, n:])
    return out + (counts[0],) if return_counts else out


def _edges_like(edges, ref):
    if _is_torch(ref):
        import torch

        return torch.from_numpy(np.asarray(edges, np.float64)).to(ref.device)
    return np.asarray(edges, np.float64)


@dataclass
class LightconePower:
    """What ``lightcone_power_spectra`` returns: ``power`` (n_chunks, n_bins) or (n_chunks, n_kperp,
    n_kpar); ``k`` (spherical) or ``kperp`` / ``kpar`` (cylindrical); ``chunk_starts`` (first slice of
    each chunk); ``redshifts`` (central redshift of each chunk, when slice redshifts were given);
    ``counts`` (modes per bin, the same for every chunk)."""

    power: object
    chunk_starts: np.ndarray
    counts: object
    k: object = None
    kperp: object = None
    kpar: object = None
    redshifts: np.ndarray | None = None


def lightcone_power_spectra(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                            dimensionless=False, cylindrical=False, **binning):
    """Power spectra of chunks of a rectilinear ``lightcone`` (nx, ny, n_slices; the line of sight last)
    of cells of ``cell_size`` [Mpc]: chunk c is slices ``chunk_starts[c] .. + chunk_length`` (default: nx
    slices, cubic chunks, back to back from slice 0, the remainder dropped), a box of (nx, ny,
    chunk_length) cells.  All chunks go through one batched transform and one binning launch.
    ``dimensionless`` multiplies by k^3 / (2 pi^2) with k the bin's mean |k| (cylindrical: sqrt(kperp^2 +
    kpar^2) of the bin's means).  ``binning``: the keywords of ``get_power`` (or of
    ``get_cylindrical_power`` when ``cylindrical``), ``deltax2`` a second lightcone for cross spectra."""
    if lightcone.ndim != 3:
        raise ValueError(f"lightcone must be a 3-D (nx, ny, n_slices) array, got {lightcone.ndim} dimensions")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n = nx if chunk_length is None else chunk_length
    if isinstance(n, (bool, np.bool_)) or int(n) != n or int(n) < 2:
        raise ValueError("chunk_length must be an integer >= 2")
    n = int(n)
    if n > ns:
        raise ValueError(f"chunk_length {n} is longer than the lightcone ({ns} slices)")
    if chunk_starts is None:
        starts = np.arange(0, ns - n + 1, n, dtype=np.int64)
    else:
        starts = np.asarray(chunk_starts)
        if starts.ndim != 1 or starts.size < 1 or starts.dtype.kind not in "iu":
            raise ValueError("chunk_starts must be a 1-D array of integers")
        starts = starts.astype(np.int64)
        if starts.min() < 0 or starts.max() + n > ns:
            raise ValueError(f"every chunk must lie inside the lightcone's {ns} slices")
    z = None
    if redshifts is not None:
        zs = np.asarray(redshifts, np.float64)
        if zs.shape != (ns,):
            raise ValueError(f"redshifts must hold one value per slice ({ns})")
        z = 0.5 * (zs[starts + (n - 1) // 2] + zs[starts + n // 2])
    deltax2 = binning.pop("deltax2", None)
    if deltax2 is not None:
        if _is_torch(deltax2) != _is_torch(lightcone) or _shape(deltax2) != _shape(lightcone):
            raise ValueError("deltax2 must be an array of the lightcone's kind and shape")
    binning.pop("return_counts", None)  # the counts are always returned here
    shape, L = (nx, ny, n), (nx * dx, ny * dx, n * dx)
    f1 = _f32(lightcone)
    f2 = None if deltax2 is None else _f32(deltax2)
    if cylindrical:
        allowed = {"kperp_bins", "kpar_bins", "log_bins", "ignore_zero_mode"}
    else:
        allowed = {"bins", "log_bins", "ignore_zero_mode", "bins_upto_boxlen", "ignore_kperp_zero",
                   "ignore_kpar_zero", "bin_ave"}
    unknown = set(binning) - allowed
    if unknown:
        raise ValueError(f"unknown binning keywords: {sorted(unknown)}")
    if cylindrical:
        ep, ez = cylindrical_edges(shape, L, binning.get("kperp_bins"), binning.get("kpar_bins"),
                                   binning.get("log_bins", False))
        power, kmean, counts = api.power_spectrum(f1, f2, shape, L, ep, ez, offsets=starts, row_pitch=ns,
                                                  ignore_zero_mode=binning.get("ignore_zero_mode", False))
        m = len(ep) - 1
        res = LightconePower(power=power, chunk_starts=starts, counts=counts[0], kperp=kmean[0, :m],
                             kpar=kmean[0, m:], redshifts=z)
        if dimensionless:
            kk = (res.kperp[:, None] ** 2 + res.kpar[None, :] ** 2) ** 1.5
            res.power = power * (kk / (2 * np.pi**2))[None]
        return res
    edges = spherical_edges(shape, L, binning.get("bins"), binning.get("log_bins", False),
                            binning.get("bins_upto_boxlen", True))
    power, kmean, counts = api.power_spectrum(
        f1, f2, shape, L, edges, offsets=starts, row_pitch=ns,
        ignore_zero_mode=binning.get("ignore_zero_mode", False),
        ignore_kperp_zero=binning.get("ignore_kperp_zero", False),
        ignore_kpar_zero=binning.get("ignore_kpar_zero", False))
    k = kmean[0]
    if dimensionless:
        power = power * (k**3 / (2 * np.pi**2))[None]
    if not binning.get("bin_ave", True):
        k = _edges_like(edges, power)
    return LightconePower(power=power, chunk_starts=starts, counts=counts[0], k=k, redshifts=z)
