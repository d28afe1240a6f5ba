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

Beyond powerbox (the conventions are written down in ``tests/power_stats_reference.py``): ``window`` tapers
the field before the transform, f' = (f - mean) wx[i] wy[j] wz[l], the power divided by <W^2>;
``mu_min`` / ``mu_max`` and ``wedge_slope`` / ``wedge_buffer`` cut the modes of the spherical average;
``return_variance`` adds the population variance of the per-mode power in each bin.  ``get_moments``,
``get_pdf`` and ``lightcone_moments`` are the one-point statistics of a box or of the chunks of a
lightcone (``csrc/hip/moments_kernels.hip``).  ``get_bispectrum`` and ``lightcone_bispectra`` are the three-point
statistic, the FFT estimator over shells in |k| (``csrc/hip/bispectrum_kernels.hip``; its spec is
``tests/bispectrum_reference.py``).  ``get_bubble_sizes`` and ``lightcone_bubble_sizes`` are the morphological
statistic, the mean-free-path bubble size distribution traced ray by ray (``csrc/hip/bubble_kernels.hip``; its
spec is ``tests/bubble_reference.py``); ``get_bubble_clusters`` and ``lightcone_bubble_clusters`` label its
friends-of-friends clusters (``csrc/hip/cluster_kernels.hip``; spec ``tests/cluster_reference.py``);
``get_minkowski_functionals`` and ``lightcone_minkowski_functionals`` count the Minkowski functionals of its
excursion sets at every threshold from one read of the field (``csrc/hip/minkowski_kernels.hip``; spec
``tests/minkowski_reference.py``); ``get_distance_transform``, ``get_granulometry`` and ``lightcone_granulometry``
are its exact Euclidean distance transform and the granulometry size distribution built on it
(``csrc/hip/granulometry_kernels.hip``; spec ``tests/granulometry_reference.py``).

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


_WINDOW_COEFFS = {
    "hann": (0.5, 0.5),
    "blackman": (0.42, 0.50, 0.08),
    "blackmanharris": (0.35875, 0.48829, 0.14128, 0.01168),
}


def taper_window(name: str, n: int) -> np.ndarray:
    """The symmetric cosine-sum window ``name`` ("hann", "blackman" or "blackmanharris") of ``n`` points,
    float64: sum_k a_k cos(k x) over x = -pi .. pi in n - 1 steps (one point: 1)."""
    if name not in _WINDOW_COEFFS:
        raise ValueError(f"unknown window {name!r}; known: {sorted(_WINDOW_COEFFS)}")
    if isinstance(n, (bool, np.bool_)) or int(n) != n or int(n) < 1:
        raise ValueError("a window needs an integer length >= 1")
    n = int(n)
    if n == 1:
        return np.ones(1)
    x = np.linspace(-np.pi, np.pi, n)
    w = np.zeros(n)
    for k, a in enumerate(_WINDOW_COEFFS[name]):
        w += a * np.cos(k * x)
    return w


def _one_window(w, n: int, axis: str):
    if w is None:
        return None
    if isinstance(w, str):
        w = taper_window(w, n)
    else:
        if _is_torch(w):
            w = w.detach().cpu().numpy()
        w = np.array(w, np.float64)
        if w.shape != (n,):
            raise ValueError(f"the {axis} window must be a 1-D array of {n} weights, got shape {w.shape}")
    if not np.all(np.isfinite(w)):
        raise ValueError(f"the {axis} window is not finite")
    if not np.any(w != 0):
        raise ValueError(f"the {axis} window is zero everywhere")
    return w


def resolve_window(window, shape):
    """``window`` as ``get_power`` accepts it -> ``((wx, wy, wz), 1 / <W^2>)`` with each w float64 weights of
    its axis or None, <W^2> = mean(wx^2) mean(wy^2) mean(wz^2) in fp64; ``(None, 1.0)`` without a window."""
    if window is None:
        return None, 1.0
    if isinstance(window, tuple):
        if len(window) != len(shape):
            raise ValueError(f"a window tuple needs one entry per axis ({len(shape)}), got {len(window)}")
        ws = tuple(_one_window(w, n, ax) for w, n, ax in zip(window, shape, "xyz"))
    else:
        ws = (None,) * (len(shape) - 1) + (_one_window(window, shape[-1], "xyz"[len(shape) - 1]),)
    if all(w is None for w in ws):
        return None, 1.0
    mean_w2 = 1.0
    for w in ws:
        if w is not None:
            mean_w2 = mean_w2 * float(np.mean(w * w))
    return ws, 1.0 / mean_w2


def resolve_cuts(mu_min=None, mu_max=None, wedge_slope=None, wedge_buffer=0.0):
    """The cut keywords checked -> ``(mu_range, wedge)`` as ``grid_api.power_spectrum`` takes them: (mu_min,
    mu_max) with the missing side 0 or 1, or None without a mu cut; (slope, buffer), or None without a wedge."""
    def num(x, what):
        if isinstance(x, (bool, np.bool_)) or np.ndim(x) != 0:
            raise ValueError(f"{what} must be a number")
        try:
            x = float(x)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a number") from None
        if not np.isfinite(x):
            raise ValueError(f"{what} must be finite")
        return x

    mu_range = None
    if mu_min is not None or mu_max is not None:
        lo = 0.0 if mu_min is None else num(mu_min, "mu_min")
        hi = 1.0 if mu_max is None else num(mu_max, "mu_max")
        if not (0.0 <= lo <= 1.0 and 0.0 <= hi <= 1.0):
            raise ValueError("mu_min and mu_max must lie in [0, 1]")
        if lo > hi:
            raise ValueError("mu_min must not exceed mu_max")
        mu_range = (lo, hi)
    buf = num(wedge_buffer, "wedge_buffer")
    if buf < 0:
        raise ValueError("wedge_buffer must be >= 0")
    wedge = None
    if wedge_slope is not None:
        slope = num(wedge_slope, "wedge_slope")
        if slope < 0:
            raise ValueError("wedge_slope must be >= 0")
        wedge = (slope, buf)
    elif buf != 0:
        raise ValueError("wedge_buffer needs a wedge_slope")
    return mu_range, wedge


_CUT_KEYS = ("mu_min", "mu_max", "wedge_slope", "wedge_buffer")


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
              return_counts=False, window=None, mu_min=None, mu_max=None, wedge_slope=None, wedge_buffer=0.0,
              return_variance=False):
    """Spherically binned power spectrum of the 3-D ``field`` (any shape; the line of sight is the last
    axis) in a box of ``boxlength`` (a scalar or 3 lengths).  Returns ``(power, k[, counts][, variance])``:
    ``k`` the mean |k| of each bin, or the edges when ``bin_ave`` is False; empty bins are NaN.

    ``window``: None; "hann", "blackman" or "blackmanharris" (``taper_window``) or nz weights, along the
    last axis; or a tuple (wx, wy, wz) of None / name / weights per axis.  The field less its mean is
    multiplied by the weights, the mean does not come back onto k = 0 and the power is divided by <W^2>.
    ``mu_min`` / ``mu_max`` (0 <= mu <= 1, mu = |kz| / |k|) and ``wedge_slope`` / ``wedge_buffer`` (keep
    |kz| - buffer >= slope k_perp) drop modes from the average; they combine with each other and with the
    ignore flags and never move the edges.  ``return_variance``: the population variance of the per-mode
    power over the modes of each bin (at most 1084 bins; 1417 without)."""
    _check_field(field, deltax2=deltax2)
    shape = _shape(field)
    L = _lengths(boxlength)
    edges = spherical_edges(shape, L, bins, log_bins, bins_upto_boxlen)
    windows, inv_w2 = resolve_window(window, shape)
    mu_range, wedge = resolve_cuts(mu_min, mu_max, wedge_slope, wedge_buffer)
    res = api.power_spectrum(
        _f32(field), None if deltax2 is None else _f32(deltax2), shape, L, edges,
        ignore_zero_mode=ignore_zero_mode, ignore_kperp_zero=ignore_kperp_zero, ignore_kpar_zero=ignore_kpar_zero,
        windows=windows, inv_mean_w2=inv_w2, mu_range=mu_range, wedge=wedge, want_variance=return_variance)
    power, kmean, counts = res[:3]
    k = kmean[0] if bin_ave else _edges_like(edges, power)
    out = (power[0], k)
    if return_counts:
        out += (counts[0],)
    if return_variance:
        out += (res[3][0],)
    return out


def get_cylindrical_power(field, boxlength, *, deltax2=None, kperp_bins=None, kpar_bins=None, log_bins=False,
                          ignore_zero_mode=False, return_counts=False, window=None, return_variance=False,
                          **cuts):
    """Cylindrically binned power spectrum: ``(power[n_kperp, n_kpar], kperp, kpar[, counts][, variance])``
    with k_perp = sqrt(kx^2 + ky^2) and k_par = |kz| (the last axis); ``kperp`` / ``kpar`` are the mean
    k_perp / k_par of the modes in each row / column of bins; empty bins are NaN.  ``window`` and
    ``return_variance`` as in ``get_power`` (with the variance at most 877 k_par bins; 1084 without); the mu
    and wedge cuts are for spherical spectra and rejected here."""
    _reject_cuts(cuts)
    _check_field(field, deltax2=deltax2)
    shape = _shape(field)
    L = _lengths(boxlength)
    ep, ez = cylindrical_edges(shape, L, kperp_bins, kpar_bins, log_bins)
    windows, inv_w2 = resolve_window(window, shape)
    res = api.power_spectrum(
        _f32(field), None if deltax2 is None else _f32(deltax2), shape, L, ep, ez,
        ignore_zero_mode=ignore_zero_mode, windows=windows, inv_mean_w2=inv_w2, want_variance=return_variance)
    power, kmean, counts = res[:3]
    n = len(ep) - 1
    out = (power[0], kmean[0, :n], kmean[0, n:])
    if return_counts:
        out += (counts[0],)
    if return_variance:
        out += (res[3][0],)
    return out


def _reject_cuts(kw):
    cut = sorted(set(kw) & set(_CUT_KEYS))
    if cut:
        raise ValueError(f"{', '.join(cut)}: mu and wedge cuts apply to spherical spectra only")
    if kw:
        raise TypeError(f"unexpected keyword arguments: {sorted(kw)}")


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
    ``counts`` (modes per bin, the same for every chunk); ``variance`` (shaped as ``power``: the variance of
    the per-mode power in each bin, with ``return_variance=True``)."""

    power: object
    chunk_starts: np.ndarray
    counts: object
    k: object = None
    kperp: object = None
    kpar: object = None
    redshifts: np.ndarray | None = None
    variance: object = None


def _chunks(ns: int, nx: int, chunk_length, chunk_starts, redshifts):
    """(chunk length, first slices, central redshifts or None) of a lightcone of ``ns`` slices."""
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
    return n, starts, z


def lightcone_power_spectra(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                            dimensionless=False, cylindrical=False, return_variance=False, **binning):
    """Power spectra of chunks of a rectilinear ``lightcone`` (nx, ny, n_slices; the line of sight last)
    of cells of ``cell_size`` [Mpc]: chunk c is slices ``chunk_starts[c] .. + chunk_length`` (default: nx
    slices, cubic chunks, back to back from slice 0, the remainder dropped), a box of (nx, ny,
    chunk_length) cells.  All chunks go through one batched transform and one binning launch.
    ``dimensionless`` multiplies by k^3 / (2 pi^2) with k the bin's mean |k| (cylindrical: sqrt(kperp^2 +
    kpar^2) of the bin's means).  ``binning``: the keywords of ``get_power`` (or of
    ``get_cylindrical_power`` when ``cylindrical``), ``deltax2`` a second lightcone for cross spectra; a
    ``window`` tapers every chunk (its last axis has ``chunk_length`` points).  ``return_variance`` fills
    ``variance``, scaled by the square of the ``dimensionless`` factor."""
    if lightcone.ndim != 3:
        raise ValueError(f"lightcone must be a 3-D (nx, ny, n_slices) array, got {lightcone.ndim} dimensions")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    deltax2 = binning.pop("deltax2", None)
    if deltax2 is not None:
        if _is_torch(deltax2) != _is_torch(lightcone) or _shape(deltax2) != _shape(lightcone):
            raise ValueError("deltax2 must be an array of the lightcone's kind and shape")
    binning.pop("return_counts", None)  # the counts are always returned here
    shape, L = (nx, ny, n), (nx * dx, ny * dx, n * dx)
    f1 = _f32(lightcone)
    f2 = None if deltax2 is None else _f32(deltax2)
    if cylindrical:
        cut = sorted(set(binning) & set(_CUT_KEYS))
        if cut:
            raise ValueError(f"{', '.join(cut)}: mu and wedge cuts apply to spherical spectra only")
        allowed = {"kperp_bins", "kpar_bins", "log_bins", "ignore_zero_mode", "window"}
    else:
        allowed = {"bins", "log_bins", "ignore_zero_mode", "bins_upto_boxlen", "ignore_kperp_zero",
                   "ignore_kpar_zero", "bin_ave", "window", *_CUT_KEYS}
    unknown = set(binning) - allowed
    if unknown:
        raise ValueError(f"unknown binning keywords: {sorted(unknown)}")
    windows, inv_w2 = resolve_window(binning.get("window"), shape)
    extra = dict(windows=windows, inv_mean_w2=inv_w2, want_variance=return_variance)
    if cylindrical:
        ep, ez = cylindrical_edges(shape, L, binning.get("kperp_bins"), binning.get("kpar_bins"),
                                   binning.get("log_bins", False))
        out = api.power_spectrum(f1, f2, shape, L, ep, ez, offsets=starts, row_pitch=ns,
                                 ignore_zero_mode=binning.get("ignore_zero_mode", False), **extra)
        power, kmean, counts = out[:3]
        m = len(ep) - 1
        res = LightconePower(power=power, chunk_starts=starts, counts=counts[0], kperp=kmean[0, :m],
                             kpar=kmean[0, m:], redshifts=z, variance=out[3] if return_variance else None)
        if dimensionless:
            kk = (res.kperp[:, None] ** 2 + res.kpar[None, :] ** 2) ** 1.5
            res.power = power * (kk / (2 * np.pi**2))[None]
            if return_variance:
                res.variance = res.variance * ((kk / (2 * np.pi**2)) ** 2)[None]
        return res
    mu_range, wedge = resolve_cuts(*(binning.get(key, 0.0 if key == "wedge_buffer" else None) for key in _CUT_KEYS))
    edges = spherical_edges(shape, L, binning.get("bins"), binning.get("log_bins", False),
                            binning.get("bins_upto_boxlen", True))
    out = api.power_spectrum(
        f1, f2, shape, L, edges, offsets=starts, row_pitch=ns,
        ignore_zero_mode=binning.get("ignore_zero_mode", False),
        ignore_kperp_zero=binning.get("ignore_kperp_zero", False),
        ignore_kpar_zero=binning.get("ignore_kpar_zero", False), mu_range=mu_range, wedge=wedge, **extra)
    power, kmean, counts = out[:3]
    variance = out[3] if return_variance else None
    k = kmean[0]
    if dimensionless:
        power = power * (k**3 / (2 * np.pi**2))[None]
        if return_variance:
            variance = variance * ((k**3 / (2 * np.pi**2)) ** 2)[None]
    if not binning.get("bin_ave", True):
        k = _edges_like(edges, power)
    return LightconePower(power=power, chunk_starts=starts, counts=counts[0], k=k, redshifts=z, variance=variance)


def _moment_stats(m):
    """(mean, variance, skewness, kurtosis) from the last axis {mean, m2, m3, m4} of ``m``; a constant field
    (m2 = 0) has NaN skewness and kurtosis."""
    mean, m2, m3, m4 = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
    if _is_torch(m):
        return mean, m2, m3 / m2**1.5, m4 / m2**2 - 3.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return mean, m2, m3 / m2**1.5, m4 / m2**2 - 3.0


def get_moments(field):
    """``(mean, variance, skewness, kurtosis)`` of a 3-D ``field``, in fp64 on the device: variance = m2 =
    sum d^2 / N with d = v - mean, skewness = m3 / m2^1.5, kurtosis = m4 / m2^2 - 3 (NaN for a constant
    field).  Scalars: Python floats for numpy input, 0-d tensors on the field's device for torch input."""
    if field.ndim != 3:
        raise ValueError(f"field must be a 3-D array, got {field.ndim} dimensions")
    m, _ = api.field_moments(_f32(field), _shape(field))
    out = _moment_stats(m[0])
    return out if _is_torch(m) else tuple(float(x) for x in out)


def _pdf_edges(bins, value_range, field):
    if np.ndim(bins) == 0:
        if isinstance(bins, (bool, np.bool_)) or int(bins) != bins or int(bins) < 1:
            raise ValueError("bins must be an integer >= 1 or an array of edges")
        if value_range is None:
            if _is_torch(field):
                lo, hi = (float(x) for x in field.aminmax())
            else:
                lo, hi = float(np.min(field)), float(np.max(field))
        else:
            if np.shape(value_range) != (2,):
                raise ValueError("range must be (low, high)")
            lo, hi = float(value_range[0]), float(value_range[1])
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError("the range of the bins is not finite")
        if lo > hi:
            raise ValueError("range needs low <= high")
        if lo == hi:  # as np.histogram
            lo, hi = lo - 0.5, hi + 0.5
        return np.linspace(lo, hi, int(bins) + 1)
    e = np.asarray(bins, np.float64)
    if e.ndim != 1 or e.size < 2:
        raise ValueError("bin edges must be a 1-D array of at least 2 values")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("bin edges must be finite and strictly increasing")
    return e


def _pdf_from_counts(hist, edges, density):
    if not density:
        return hist
    if _is_torch(hist):
        import torch

        widths = torch.from_numpy(np.diff(edges)).to(hist.device)
        return hist.to(torch.float64) / widths / hist.sum(dim=-1, keepdim=True).to(torch.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return hist / np.diff(edges) / hist.sum(axis=-1, keepdims=True)


def get_pdf(field, bins, range=None, density=True):
    """The histogram of a 3-D ``field``: ``(pdf, edges)``.  ``bins``: edges (1-D, increasing), or a count
    for ``np.linspace(*range, bins + 1)`` with ``range`` defaulting to the field's minimum and maximum.
    Bins are half-open as ``np.digitize`` everywhere in this module: a value on the last edge is not
    counted (so the field's maximum falls out of the default range's last bin).  ``density``: counts /
    (kept values x bin width), as ``np.histogram`` normalises; otherwise int64 counts.  At most 4096 bins."""
    if field.ndim != 3:
        raise ValueError(f"field must be a 3-D array, got {field.ndim} dimensions")
    f = _f32(field)
    edges = _pdf_edges(bins, range, f)
    _, hist = api.field_moments(f, _shape(f), edges=edges)
    return _pdf_from_counts(hist[0], edges, density), _edges_like(edges, hist)


@dataclass
class LightconeMoments:
    """What ``lightcone_moments`` returns, one entry per chunk: ``mean``, ``variance``, ``skewness``,
    ``kurtosis``; ``chunk_starts``; ``redshifts`` (when slice redshifts were given); with ``bins``: ``pdf``
    (n_chunks, n_bins) and the ``edges`` all chunks share."""

    mean: object
    variance: object
    skewness: object
    kurtosis: object
    chunk_starts: np.ndarray
    redshifts: np.ndarray | None = None
    pdf: object = None
    edges: object = None


def lightcone_moments(lightcone, *, chunk_length=None, chunk_starts=None, redshifts=None, bins=None, range=None,
                      density=True):
    """One-point statistics of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices), chunked as
    ``lightcone_power_spectra`` chunks it and with its central-redshift rule; all chunks go through one
    launch per pass.  ``bins`` / ``range`` / ``density`` as in ``get_pdf`` (the default range spans the
    whole lightcone)."""
    if lightcone.ndim != 3:
        raise ValueError(f"lightcone must be a 3-D (nx, ny, n_slices) array, got {lightcone.ndim} dimensions")
    nx, ny, ns = _shape(lightcone)
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    f = _f32(lightcone)
    edges = None if bins is None else _pdf_edges(bins, range, f)
    m, hist = api.field_moments(f, (nx, ny, n), offsets=starts, row_pitch=ns, edges=edges)
    mean, var, skew, kurt = _moment_stats(m)
    res = LightconeMoments(mean=mean, variance=var, skewness=skew, kurtosis=kurt, chunk_starts=starts, redshifts=z)
    if edges is not None:
        res.pdf = _pdf_from_counts(hist, edges, density)
        res.edges = _edges_like(edges, hist)
    return res


BISPECTRUM_MAX_BINS = 32


def bispectrum_k_range(shape, boxlength) -> tuple:
    """``(k_min, k_max)`` of the default bispectrum shells: half the largest fundamental, max(2 pi / L) / 2, up to
    (2/3) min(pi n / L) -- two thirds of the smallest Nyquist wavenumber, below which no triplet of modes closes
    modulo the grid and no Nyquist mode is in a shell."""
    L = _lengths(boxlength, len(shape))
    return max(2.0 * np.pi / l for l in L) / 2.0, (2.0 / 3.0) * min(np.pi * int(n) / l for n, l in zip(shape, L))


def bispectrum_edges(shape, boxlength, bins=8, log_bins=False) -> np.ndarray:
    """The shell edges ``get_bispectrum`` uses for a grid of ``shape``: an int gives ``np.linspace(k_min, k_max,
    bins + 1)`` (``log_bins``: ``np.geomspace``) over ``bispectrum_k_range``; an array is taken as the edges.
    Checked either way: 1 to 32 shells, finite and increasing, the first edge > 0 (k = 0 is in no shell), the last
    <= k_max."""
    kmin, kmax = bispectrum_k_range(shape, boxlength)
    e = make_edges(bins, kmin, kmax, kmin, log_bins)
    if not 1 <= len(e) - 1 <= BISPECTRUM_MAX_BINS:
        raise ValueError(f"a bispectrum takes 1 to {BISPECTRUM_MAX_BINS} shells, got {len(e) - 1}")
    if not e[0] > 0:
        raise ValueError("the first edge must be > 0: k = 0 is in no shell")
    if e[-1] > kmax:
        raise ValueError(f"the last edge {e[-1]!r} exceeds k_max = (2/3) min(pi n / L) = {kmax!r}")
    return e


def bispectrum_triangles(edges) -> np.ndarray:
    """Every triangle of shells (b1 <= b2 <= b3) that can hold a closed triplet of modes, ``e[b3] < e[b1 + 1] +
    e[b2 + 1]``, in lexicographic order: int32 (n, 3)."""
    e = np.asarray(edges, np.float64)
    if e.ndim != 1 or e.size < 2:
        raise ValueError("edges must be a 1-D array of at least 2 values")
    n = e.size - 1
    b1, b2, b3 = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    keep = (b1 <= b2) & (b2 <= b3) & (e[b3] < e[b1 + 1] + e[b2 + 1])
    return np.stack([b1[keep], b2[keep], b3[keep]], axis=1).astype(np.int32)


def _check_triangles(triangles, edges) -> np.ndarray:
    if triangles is None:
        return bispectrum_triangles(edges)
    if _is_torch(triangles):
        triangles = triangles.detach().cpu().numpy()
    t = np.asarray(triangles)
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError("triangles must be an (n, 3) array of integers")
    if t.shape[0] < 1:
        raise ValueError("at least one triangle is needed")
    n = len(edges) - 1
    if t.min() < 0 or t.max() >= n or np.any(t[:, 0] > t[:, 1]) or np.any(t[:, 1] > t[:, 2]):
        raise ValueError(f"every triangle needs 0 <= b1 <= b2 <= b3 < {n}")
    return np.ascontiguousarray(t, np.int32)


@dataclass
class Bispectrum:
    """What ``get_bispectrum`` and ``lightcone_bispectra`` return (the latter with a leading chunk axis on
    ``bispectrum``, ``power`` and ``reduced``): ``bispectrum`` (n_tri,) float64, NaN where a triangle holds no
    closed triplet; ``triangles`` (n_tri, 3) shell indices; ``n_triangles`` (n_tri,) int64 closed triplets of modes;
    ``k`` (n_tri, 3) the mean |k| of the three shells; ``power`` / ``n_modes`` (n_bins,) of the shells, as
    ``get_power(bins=edges)``; ``reduced`` B / (P1 P2 + P2 P3 + P3 P1) when asked for; ``edges``; for a lightcone
    ``chunk_starts`` and ``redshifts`` (central redshift of each chunk, when slice redshifts were given)."""

    bispectrum: object
    triangles: object
    n_triangles: object
    k: object
    power: object
    n_modes: object
    edges: object
    reduced: object = None
    chunk_starts: np.ndarray | None = None
    redshifts: np.ndarray | None = None


def _bispectrum_result(f, shape, L, edges, tri, offsets, row_pitch, reduced):
    power, kmean, counts = api.power_spectrum(f, None, shape, L, edges, offsets=offsets, row_pitch=row_pitch)
    B, n_tri = api.bispectrum(f, shape, L, edges, tri, offsets=offsets, row_pitch=row_pitch)
    if _is_torch(B):
        import torch

        idx = torch.from_numpy(tri.astype(np.int64)).to(B.device)
        tri_out = torch.from_numpy(tri.copy()).to(B.device)
    else:
        idx = tri_out = tri
    red = None
    if reduced:
        p1, p2, p3 = power[:, idx[:, 0]], power[:, idx[:, 1]], power[:, idx[:, 2]]
        red = B / (p1 * p2 + p2 * p3 + p3 * p1)
    return Bispectrum(bispectrum=B, triangles=tri_out, n_triangles=n_tri, k=kmean[0][idx], power=power,
                      n_modes=counts[0], edges=_edges_like(edges, B), reduced=red)


def get_bispectrum(field, boxlength, *, bins=8, log_bins=False, triangles=None, reduced=False) -> Bispectrum:
    """The bispectrum of the 3-D ``field`` in a box of ``boxlength`` (a scalar or 3 lengths) by the FFT estimator,
    conventions as ``get_power``: with D the unnormalised DFT, delta_b(x) = sum_{k in shell b} D(k) exp(+i k x) and
    I_b the same sum of ones, B(b1, b2, b3) = (V^2 / N^3) sum_x delta_b1 delta_b2 delta_b3 / sum_x I_b1 I_b2 I_b3.
    ``bins`` / ``log_bins``: the shells (``bispectrum_edges``; a shell is exactly a ``get_power`` bin of the same
    edges); ``triangles``: (n, 3) shell indices b1 <= b2 <= b3, default ``bispectrum_triangles``.  A triangle's
    value does not depend on which others are asked for, and two calls give the same bits.  The device holds one
    padded box per shell (twice that, in fp64, the first time a geometry is seen: the triangle counts)."""
    _check_field(field)
    shape = _shape(field)
    L = _lengths(boxlength)
    edges = bispectrum_edges(shape, L, bins, log_bins)
    tri = _check_triangles(triangles, edges)
    res = _bispectrum_result(_f32(field), shape, L, edges, tri, (0,), None, reduced)
    res.bispectrum, res.power = res.bispectrum[0], res.power[0]
    if reduced:
        res.reduced = res.reduced[0]
    return res


def lightcone_bispectra(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None, bins=8,
                        log_bins=False, triangles=None, reduced=False) -> Bispectrum:
    """Bispectra of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices) of cells of ``cell_size`` [Mpc],
    chunked as ``lightcone_power_spectra`` chunks it and with its central-redshift rule; all chunks go through one
    library call and share the shells, the triangles and their counts.  ``bispectrum``, ``power`` and ``reduced``
    carry a leading chunk axis."""
    if lightcone.ndim != 3:
        raise ValueError(f"lightcone must be a 3-D (nx, ny, n_slices) array, got {lightcone.ndim} dimensions")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    if min(nx, ny) < 2:
        raise ValueError("every axis of a chunk needs at least 2 cells")
    shape, L = (nx, ny, n), (nx * dx, ny * dx, n * dx)
    edges = bispectrum_edges(shape, L, bins, log_bins)
    tri = _check_triangles(triangles, edges)
    res = _bispectrum_result(_f32(lightcone), shape, L, edges, tri, starts, ns, reduced)
    res.chunk_starts, res.redshifts = starts, z
    return res


BUBBLE_MAX_BINS = 4096


def bubble_edges(shape, boxlength, bins=64, log_bins=True, max_length=None) -> np.ndarray:
    """The length edges ``get_bubble_sizes`` uses for a grid of ``shape``: an int gives ``np.geomspace(cell_min,
    max_length, bins + 1)`` (``np.linspace`` without ``log_bins``) from the smallest cell size to ``max_length``
    (default: the largest box length); an array is taken as the edges.  Checked either way: 1 to 4096 bins, finite
    and increasing, the first edge >= 0."""
    L = _lengths(boxlength, len(shape))
    cell_min = min(l / int(n) for l, n in zip(L, shape))
    top = max(L) if max_length is None else float(max_length)
    e = make_edges(bins, cell_min, top, cell_min, log_bins)
    if not 1 <= len(e) - 1 <= BUBBLE_MAX_BINS:
        raise ValueError(f"a bubble size distribution takes 1 to {BUBBLE_MAX_BINS} bins, got {len(e) - 1}")
    if e[0] < 0:
        raise ValueError("the first edge must be >= 0")
    return e


@dataclass
class BubbleSizes:
    """What ``get_bubble_sizes`` and ``lightcone_bubble_sizes`` return (the latter with a leading chunk axis on
    everything but ``edges`` and ``r``): ``edges`` (n_bins + 1,) in length; ``r`` (n_bins,) the geometric bin centres
    sqrt(e_i e_{i+1}); ``hist`` int64 ended rays per bin; ``pdf`` dP/dlnR = hist / (n_ended ln(e_{i+1} / e_i)), NaN
    where no ray ended; ``n_selected`` cells, ``n_ended`` / ``n_capped`` / ``n_escaped`` rays; ``filling_fraction`` =
    n_selected / cells; ``mean_free_path`` the mean of the ended lengths (NaN where no ray ended); with
    ``return_rays`` per ray ``lengths``, ``flags`` (0 ended, 1 capped, 2 escaped; 255 without a selected cell) and
    ``starts`` (flat cell index in the box); for a lightcone ``chunk_starts`` and ``redshifts``."""

    edges: object
    r: object
    hist: object
    pdf: object
    n_selected: object
    n_ended: object
    n_capped: object
    n_escaped: object
    filling_fraction: object
    mean_free_path: object = None
    lengths: object = None
    flags: object = None
    starts: object = None
    chunk_starts: np.ndarray | None = None
    redshifts: np.ndarray | None = None


def _bubble_args(threshold, select, n_rays, seed, directions, periodic, max_length, L):
    if select not in ("below", "above"):
        raise ValueError("select must be 'below' (v < threshold) or 'above' (v >= threshold)")
    if directions not in ("isotropic", "los"):
        raise ValueError("directions must be 'isotropic' or 'los'")
    if isinstance(threshold, (bool, np.bool_)) or np.ndim(threshold) != 0 or not np.isfinite(float(threshold)):
        raise ValueError("threshold must be a finite number")
    if isinstance(n_rays, (bool, np.bool_)) or int(n_rays) != n_rays or not 1 <= int(n_rays) <= 2**31 - 1:
        raise ValueError("n_rays must be an integer in [1, 2^31 - 1]")
    if isinstance(seed, (bool, np.bool_)) or int(seed) != seed or not 0 <= int(seed) < 2**64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if np.ndim(periodic) == 0:
        periodic = (bool(periodic),) * 3
    else:
        periodic = tuple(bool(p) for p in periodic)
        if len(periodic) != 3:
            raise ValueError("periodic must be a bool or three bools")
    max_length = max(L) if max_length is None else float(max_length)
    if not (np.isfinite(max_length) and max_length > 0):
        raise ValueError("max_length must be positive and finite")
    return dict(threshold=float(threshold), select_below=select == "below", n_rays=int(n_rays), seed=int(seed),
                los=directions == "los", periodic=periodic, max_length=max_length)


def _bubble_result(f, shape, L, edges, args, offsets, row_pitch, return_rays):
    out = api.bubble_sizes(f, shape, L, edges, offsets=offsets, row_pitch=row_pitch, return_rays=True, **args)
    hist, stats = out[:2]
    n_cells = float(int(shape[0]) * int(shape[1]) * int(shape[2]))
    e = _edges_like(edges, hist)
    dlnr = _edges_like(np.log(edges[1:] / edges[:-1]) if edges[0] > 0 else
                       np.concatenate([[np.inf], np.log(edges[2:] / edges[1:-1])]), hist)
    r = _edges_like(np.sqrt(edges[:-1] * edges[1:]), hist)
    n_sel, n_end = stats[:, 0], stats[:, 1]
    if _is_torch(hist):
        import torch

        f64 = torch.float64
        pdf = hist.to(f64) / n_end.to(f64)[:, None] / dlnr[None]  # 0 / 0 = NaN where no ray ended
        # a tensor divisor: by a Python scalar torch multiplies with the reciprocal, which is not n_sel / cells
        fill = n_sel.to(f64) / torch.full((), n_cells, dtype=f64, device=hist.device)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            pdf = hist / n_end.astype(np.float64)[:, None] / dlnr[None]
        fill = n_sel / n_cells
    res = BubbleSizes(edges=e, r=r, hist=hist, pdf=pdf, n_selected=n_sel, n_ended=n_end, n_capped=stats[:, 2],
                      n_escaped=stats[:, 3], filling_fraction=fill)
    # the mean free path is the mean of the ended lengths, so the lengths are always asked for
    lengths, flags, starts = out[2:]
    ended = flags == 0
    if _is_torch(hist):
        zero = torch.zeros((), dtype=torch.float64, device=hist.device)
        res.mean_free_path = torch.where(ended, lengths, zero).sum(dim=1) / n_end.to(torch.float64)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            res.mean_free_path = np.where(ended, lengths, 0.0).sum(axis=1) / n_end
    if return_rays:
        res.lengths, res.flags, res.starts = lengths, flags, starts
    return res


_BUBBLE_PER_BOX = ("hist", "pdf", "n_selected", "n_ended", "n_capped", "n_escaped", "filling_fraction",
                   "mean_free_path", "lengths", "flags", "starts")


def get_bubble_sizes(field, boxlength, *, threshold=0.5, select="below", n_rays=1_000_000, seed=0, bins=64,
                     log_bins=True, max_length=None, directions="isotropic", periodic=True,
                     return_rays=False) -> BubbleSizes:
    """The mean-free-path bubble size distribution (Mesinger & Furlanetto 2007) of the 3-D ``field`` in a box of
    ``boxlength`` (a scalar or 3 lengths): ``n_rays`` rays start at random points of the selected phase -- cells with
    ``v < threshold`` (``select="below"``: for a neutral fraction the ionised phase) or ``v >= threshold``
    (``"above"``), every selected cell equally likely -- run in random directions (``directions="isotropic"``, or
    ``"los"``: along +-z) and end at the first cell that is not selected; their lengths are histogrammed into
    ``bins`` (``bubble_edges``: by default 64 log-spaced bins from the smallest cell size to ``max_length``, itself
    by default the largest box length) as dP/dlnR.  A ray that reaches ``max_length`` is capped, and one that leaves
    through an axis that is not ``periodic`` (a bool or three) has escaped; neither is in the histogram.  Rays are
    drawn from ``seed`` with a counter-based generator: ray i is the same whatever ``n_rays``, and two calls give
    the same bytes.  ``return_rays`` adds the per-ray lengths, flags and start cells.  A field without a selected
    cell gives zeros and a NaN pdf."""
    _check_bubble_field(field)
    shape = _shape(field)
    L = _lengths(boxlength)
    args = _bubble_args(threshold, select, n_rays, seed, directions, periodic, max_length, L)
    edges = bubble_edges(shape, L, bins, log_bins, args["max_length"])
    res = _bubble_result(_f32(field), shape, L, edges, args, (0,), None, return_rays)
    for name in _BUBBLE_PER_BOX:
        v = getattr(res, name)
        if v is not None:
            setattr(res, name, v[0])
    return res


def _check_bubble_field(field, what="field"):
    if field.ndim != 3:
        raise ValueError(f"{what} must be a 3-D array, got {field.ndim} dimensions")


def lightcone_bubble_sizes(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                           **kw) -> BubbleSizes:
    """Bubble size distributions of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices) of cells of
    ``cell_size`` [Mpc], chunked as ``lightcone_power_spectra`` chunks it and with its central-redshift rule; all
    chunks go through one library call and share the edges.  The transverse axes are periodic and the line of sight
    is not (a ray that leaves a chunk along it has escaped), so ``periodic`` is not a keyword here; the others are
    those of ``get_bubble_sizes``.  Every per-box entry carries a leading chunk axis."""
    _check_bubble_field(lightcone, "lightcone")
    if "periodic" in kw:
        raise ValueError("periodic is fixed for a lightcone: the transverse axes are, the line of sight is not")
    unknown = set(kw) - {"threshold", "select", "n_rays", "seed", "bins", "log_bins", "max_length", "directions",
                         "return_rays"}
    if unknown:
        raise ValueError(f"unknown keywords: {sorted(unknown)}")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    shape, L = (nx, ny, n), (nx * dx, ny * dx, n * dx)
    args = _bubble_args(kw.get("threshold", 0.5), kw.get("select", "below"), kw.get("n_rays", 1_000_000),
                        kw.get("seed", 0), kw.get("directions", "isotropic"), (True, True, False),
                        kw.get("max_length"), L)
    edges = bubble_edges(shape, L, kw.get("bins", 64), kw.get("log_bins", True), args["max_length"])
    res = _bubble_result(_f32(lightcone), shape, L, edges, args, starts, ns, kw.get("return_rays", False))
    res.chunk_starts, res.redshifts = starts, z
    return res


CLUSTER_DEFAULT_CAPACITY = 2**20  # clusters per box the first call of get_bubble_clusters makes room for


def cluster_edges(shape, bins=32, log_bins=True) -> np.ndarray:
    """The size edges, in cells, ``get_bubble_clusters`` uses for a grid of ``shape`` with N cells: an int gives
    ``np.unique(np.ceil(np.geomspace(1, N + 1, bins + 1)))`` (``np.linspace`` without ``log_bins``) as int64, so a
    small box may get fewer bins than asked for; an array is taken as integer edges.  Checked either way: increasing,
    the first edge >= 1, 1 to 4096 bins."""
    n_cells = int(np.prod([int(n) for n in shape], dtype=np.int64))
    if np.ndim(bins) == 0:
        if isinstance(bins, (bool, np.bool_)) or int(bins) != bins:
            raise ValueError("bins must be an integer or an array of edges")
        if int(bins) < 1:
            raise ValueError(f"bins must be >= 1, got {int(bins)}")
        space = np.geomspace if log_bins else np.linspace
        e = np.unique(np.ceil(space(1, n_cells + 1, int(bins) + 1))).astype(np.int64)
    else:
        raw = np.asarray(bins)
        if raw.ndim != 1 or raw.size < 2:
            raise ValueError("bins must be a 1-D array of at least 2 edges")
        if raw.dtype.kind not in "iu" and not (np.all(np.isfinite(raw)) and np.all(raw == np.round(raw))):
            raise ValueError("cluster size edges must be integers (cells)")
        e = raw.astype(np.int64)
        if np.any(np.diff(e) <= 0):
            raise ValueError("bins must be increasing")
    if not 1 <= len(e) - 1 <= BUBBLE_MAX_BINS:
        raise ValueError(f"a cluster size distribution takes 1 to {BUBBLE_MAX_BINS} bins, got {len(e) - 1}")
    if e[0] < 1:
        raise ValueError("the first edge must be >= 1")
    return e


@dataclass
class BubbleClusters:
    """What ``get_bubble_clusters`` and ``lightcone_bubble_clusters`` return (the latter with a leading chunk axis on
    everything but the edges and ``r_eff``): ``edges`` (n_bins + 1,) int64 in cells; ``volume_edges`` = edges V_cell;
    ``r_eff`` (n_bins,) the radius of the sphere with the volume sqrt(e_i e_{i+1}) V_cell; ``hist_n`` int64 clusters
    per bin and ``hist_cells`` their cells; ``volume_fraction`` = hist_cells / n_selected (NaN without a selected
    cell); ``n_selected`` cells, ``n_clusters``; ``largest_cells``, ``largest_root`` (flat cell index, -1 without a
    selected cell) and ``largest_fraction`` = largest_cells / n_selected, the percolation order parameter;
    ``filling_fraction`` = n_selected / cells; ``mean_volume`` = n_selected V_cell / n_clusters; with
    ``return_labels`` ``labels`` int32 shaped as the box, the root of every cell's cluster or -1; with
    ``return_clusters`` ``roots``, ``sizes`` (cells) and ``volumes`` = sizes V_cell in ascending root; for a
    lightcone ``chunk_starts`` and ``redshifts``."""

    edges: object
    volume_edges: object
    r_eff: object
    hist_n: object
    hist_cells: object
    volume_fraction: object
    n_selected: object
    n_clusters: object
    largest_cells: object
    largest_root: object
    largest_fraction: object
    filling_fraction: object
    mean_volume: object
    labels: object = None
    roots: object = None
    volumes: object = None
    sizes: object = None
    chunk_starts: np.ndarray | None = None
    redshifts: np.ndarray | None = None


def _cluster_args(threshold, select, connectivity, periodic, return_clusters, max_clusters):
    if select not in ("below", "above"):
        raise ValueError("select must be 'below' (v < threshold) or 'above' (v >= threshold)")
    if isinstance(threshold, (bool, np.bool_)) or np.ndim(threshold) != 0 or not np.isfinite(float(threshold)):
        raise ValueError("threshold must be a finite number")
    if isinstance(connectivity, (bool, np.bool_)) or connectivity not in (6, 18, 26):
        raise ValueError("connectivity must be 6 (faces), 18 (and edges) or 26 (and corners)")
    if np.ndim(periodic) == 0:
        periodic = (bool(periodic),) * 3
    else:
        periodic = tuple(bool(p) for p in periodic)
        if len(periodic) != 3:
            raise ValueError("periodic must be a bool or three bools")
    if max_clusters is not None:
        if isinstance(max_clusters, (bool, np.bool_)) or int(max_clusters) != max_clusters or int(max_clusters) < 1:
            raise ValueError("max_clusters must be None or an integer >= 1")
        max_clusters = int(max_clusters)
    return dict(threshold=float(threshold), select_below=select == "below",
                connectivity={6: 1, 18: 2, 26: 3}[connectivity], periodic=periodic), bool(return_clusters), max_clusters


def _cluster_result(f, shape, cell_volume, edges, args, offsets, row_pitch, return_labels, return_clusters,
                    max_clusters):
    def call(capacity):
        return api.bubble_clusters(f, shape, edges, offsets=offsets, row_pitch=row_pitch,
                                   return_labels=return_labels, max_clusters=capacity, **args)

    capacity = 0
    if return_clusters:
        capacity = CLUSTER_DEFAULT_CAPACITY if max_clusters is None else max_clusters
    out = call(capacity)
    stats = out[2]
    most = int(stats[:, 1].max())
    if return_clusters and max_clusters is None and most > capacity:
        capacity = most
        out = call(capacity)
        stats = out[2]
    hist_n, hist_cells = out[:2]
    n_cells = float(int(shape[0]) * int(shape[1]) * int(shape[2]))
    centre = np.sqrt(edges[:-1].astype(np.float64) * edges[1:].astype(np.float64)) * cell_volume
    n_sel, n_cl, big = stats[:, 0], stats[:, 1], stats[:, 2]
    if _is_torch(hist_n):
        import torch

        f64 = torch.float64

        def const(v):
            # a tensor divisor or factor: by a Python scalar torch may multiply with the reciprocal
            return torch.full((), v, dtype=f64, device=hist_n.device)

        def div(a, b):
            return a.to(f64) / b.to(f64)  # 0 / 0 = NaN

        def as_int(e):
            return torch.from_numpy(np.asarray(e, np.int64)).to(hist_n.device)
    else:
        def const(v):
            return np.float64(v)

        def div(a, b):
            with np.errstate(invalid="ignore", divide="ignore"):
                return a.astype(np.float64) / b.astype(np.float64)

        def as_int(e):
            return np.asarray(e, np.int64)

    def f64_of(a):
        return a.to(f64) if _is_torch(a) else a.astype(np.float64)

    res = BubbleClusters(
        edges=as_int(edges), volume_edges=_edges_like(edges.astype(np.float64) * cell_volume, hist_n),
        r_eff=_edges_like(np.cbrt(3.0 * centre / (4.0 * np.pi)), hist_n), hist_n=hist_n, hist_cells=hist_cells,
        volume_fraction=div(hist_cells, n_sel[:, None]), n_selected=n_sel, n_clusters=n_cl, largest_cells=big,
        largest_root=stats[:, 3], largest_fraction=div(big, n_sel), filling_fraction=f64_of(n_sel) / const(n_cells),
        mean_volume=div(n_sel, n_cl) * const(cell_volume))
    rest = list(out[3:])
    if return_labels:
        res.labels = rest.pop(0).reshape((len(offsets),) + tuple(int(n) for n in shape))
    if return_clusters:
        keep = min(most, capacity)  # the largest count over the boxes: shorter lists stay padded with -1 / 0
        res.roots, res.sizes = rest[0][:, :keep], rest[1][:, :keep]
        res.volumes = f64_of(res.sizes) * const(cell_volume)
    return res


_CLUSTER_PER_BOX = ("hist_n", "hist_cells", "volume_fraction", "n_selected", "n_clusters", "largest_cells",
                    "largest_root", "largest_fraction", "filling_fraction", "mean_volume", "labels", "roots",
                    "volumes", "sizes")


def get_bubble_clusters(field, boxlength, *, threshold=0.5, select="below", connectivity=6, periodic=True, bins=32,
                        log_bins=True, return_labels=False, return_clusters=False,
                        max_clusters=None) -> BubbleClusters:
    """The friends-of-friends clusters (Friedrich et al. 2011) of the 3-D ``field`` in a box of ``boxlength`` (a
    scalar or 3 lengths): the cells with ``v < threshold`` (``select="below"``: for a neutral fraction the ionised
    phase) or ``v >= threshold`` (``"above"``) are joined to their selected neighbours -- ``connectivity`` 6 (faces),
    18 (and edges) or 26 (and corners), across the faces of the ``periodic`` axes (a bool or three) -- and the
    clusters are counted by size into ``bins`` (``cluster_edges``: by default up to 32 log-spaced bins in cells), with
    the number of clusters, the largest one and its share of the selected cells (the percolation order parameter).
    A cluster is named by its root, the smallest flat index of its cells.  ``return_labels`` adds the root of every
    cell's cluster (-1 where the cell is not selected); ``return_clusters`` adds the roots, sizes and volumes of the
    clusters in ascending root: all of them with ``max_clusters=None`` (one call with room for 2^20 clusters and, if
    the box has more, one more with the count), or the first ``max_clusters``.  Every count is an integer fixed by
    the mask: two calls give the same bytes.  A field without a selected cell gives zeros, -1 and NaN fractions."""
    _check_bubble_field(field)
    shape = _shape(field)
    L = _lengths(boxlength)
    args, return_clusters, max_clusters = _cluster_args(threshold, select, connectivity, periodic, return_clusters,
                                                        max_clusters)
    edges = cluster_edges(shape, bins, log_bins)
    cell_volume = float(np.prod([l / n for l, n in zip(L, shape)]))
    res = _cluster_result(_f32(field), shape, cell_volume, edges, args, (0,), None, return_labels, return_clusters,
                          max_clusters)
    for name in _CLUSTER_PER_BOX:
        v = getattr(res, name)
        if v is not None:
            setattr(res, name, v[0])
    return res


def lightcone_bubble_clusters(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                              **kw) -> BubbleClusters:
    """Friends-of-friends clusters of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices) of cells of
    ``cell_size`` [Mpc], chunked as ``lightcone_bubble_sizes`` chunks it; all chunks go through one library call and
    share the edges.  The transverse axes are periodic and the line of sight is open, so ``periodic`` is not a
    keyword here; the others are those of ``get_bubble_clusters``.  Every per-box entry carries a leading chunk
    axis; the cluster lists are padded with -1 / 0 to the largest count over the chunks."""
    _check_bubble_field(lightcone, "lightcone")
    if "periodic" in kw:
        raise ValueError("periodic is fixed for a lightcone: the transverse axes are, the line of sight is not")
    unknown = set(kw) - {"threshold", "select", "connectivity", "bins", "log_bins", "return_labels", "return_clusters",
                         "max_clusters"}
    if unknown:
        raise ValueError(f"unknown keywords: {sorted(unknown)}")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    shape = (nx, ny, n)
    args, return_clusters, max_clusters = _cluster_args(
        kw.get("threshold", 0.5), kw.get("select", "below"), kw.get("connectivity", 6), (True, True, False),
        kw.get("return_clusters", False), kw.get("max_clusters"))
    edges = cluster_edges(shape, kw.get("bins", 32), kw.get("log_bins", True))
    res = _cluster_result(_f32(lightcone), shape, dx ** 3, edges, args, starts, ns, kw.get("return_labels", False),
                          return_clusters, max_clusters)
    res.chunk_starts, res.redshifts = starts, z
    return res


MINKOWSKI_MAX_THRESHOLDS = api.MINKOWSKI_MAX_THRESHOLDS


def _min_max(field):
    if _is_torch(field):
        return float(field.min()), float(field.max())
    a = np.asarray(field)
    return float(a.min()), float(a.max())


def minkowski_thresholds(field, n=32) -> np.ndarray:
    """``n`` equally spaced thresholds strictly inside [min, max] of the whole ``field``:
    ``np.linspace(min, max, n + 2)[1:-1]`` in fp64.  A constant (or non-finite) field has none."""
    if isinstance(n, (bool, np.bool_)) or np.ndim(n) != 0 or int(n) != n:
        raise ValueError("the number of thresholds must be an integer")
    if not 1 <= int(n) <= MINKOWSKI_MAX_THRESHOLDS:
        raise ValueError(f"Minkowski functionals take 1 to {MINKOWSKI_MAX_THRESHOLDS} thresholds, got {int(n)}")
    lo, hi = _min_max(field)
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("the field has no finite range to space thresholds in")
    if not hi > lo:
        raise ValueError("a constant field has no thresholds strictly inside its range")
    t = np.linspace(np.float64(lo), np.float64(hi), int(n) + 2)[1:-1]
    if np.any(np.diff(t) <= 0):
        raise ValueError(f"the range of the field is too narrow for {int(n)} distinct thresholds")
    return t


@dataclass
class MinkowskiFunctionals:
    """What ``get_minkowski_functionals`` and ``lightcone_minkowski_functionals`` return (the latter with a leading
    chunk axis on everything but the thresholds).  A box of N cells of volume V_cell has the volume V = N V_cell; its
    cells have the edge lengths l_a and the face areas A_a = V_cell / l_a.  ``thresholds`` (T,) fp64; ``counts`` int64
    (T, 8) = n3 (selected cells), n2x, n2y, n2z (faces of the excursion set perpendicular to an axis), n1x, n1y, n1z
    (edges parallel to one), n0 (vertices); ``n_cells`` = N; ``euler_characteristic`` int64 = n0 - sum n1a + sum n2a -
    n3; ``genus`` = 1 - chi / 2; and the four functionals per unit volume, fp64 (T,): ``v0`` = n3 / N, ``v1`` = (2/9)
    sum_a A_a (n2a - n3) / V, ``v2`` = (2/9) sum_a l_a (n1a - n2b - n2c + n3) / V with b, c the other two axes, ``v3``
    = chi / V.  For cubic cells of edge a these are the Crofton estimators of Schmalzing & Buchert (1997), 2 (n2 - 3
    n3) / (9 a N), 2 (n1 - 2 n2 + 3 n3) / (9 a^2 N) and (n0 - n1 + n2 - n3) / (a^3 N); the lattice correction 2/9 is
    exact only for cubic cells.  For a lightcone also ``chunk_starts`` and ``redshifts``."""

    thresholds: object
    counts: object
    n_cells: int
    euler_characteristic: object
    genus: object
    v0: object
    v1: object
    v2: object
    v3: object
    chunk_starts: np.ndarray | None = None
    redshifts: np.ndarray | None = None


def _minkowski_args(thresholds, select, periodic, field):
    if select not in ("below", "above"):
        raise ValueError("select must be 'below' (v < threshold) or 'above' (v >= threshold)")
    if np.ndim(periodic) == 0:
        periodic = (bool(periodic),) * 3
    else:
        periodic = tuple(bool(p) for p in periodic)
        if len(periodic) != 3:
            raise ValueError("periodic must be a bool or three bools")
    if np.ndim(thresholds) == 0:
        t = minkowski_thresholds(field, thresholds)
    else:
        t = np.array(thresholds, np.float64)
        if t.ndim != 1 or not 1 <= t.size <= MINKOWSKI_MAX_THRESHOLDS:
            raise ValueError(f"thresholds must be an integer or a 1-D array of 1 to {MINKOWSKI_MAX_THRESHOLDS} values")
        if not np.all(np.isfinite(t)) or np.any(np.diff(t) <= 0):
            raise ValueError("thresholds must be finite and strictly increasing")
    return t, dict(select_below=select == "below", periodic=periodic)


def _minkowski_result(f, shape, cell, thresholds, args, offsets, row_pitch) -> MinkowskiFunctionals:
    counts = api.minkowski(f, shape, thresholds, offsets=offsets, row_pitch=row_pitch, **args)
    n_cells = int(shape[0]) * int(shape[1]) * int(shape[2])
    cell_volume = float(np.prod(cell))
    volume = n_cells * cell_volume
    area = [cell_volume / l for l in cell]
    if _is_torch(counts):
        import torch

        def const(v):
            # a tensor divisor or factor: by a Python scalar torch may multiply with the reciprocal
            return torch.full((), v, dtype=torch.float64, device=counts.device)

        def f64_of(a):
            return a.to(torch.float64)
    else:
        def const(v):
            return np.float64(v)

        def f64_of(a):
            return a.astype(np.float64)

    n3, n2, n1, n0 = counts[..., 0], counts[..., 1:4], counts[..., 4:7], counts[..., 7]
    chi = n0 - n1.sum(-1) + n2.sum(-1) - n3
    surface = sum(const(area[a]) * f64_of(n2[..., a] - n3) for a in range(3))
    curvature = sum(const(cell[a]) * f64_of(n1[..., a] - n2[..., (a + 1) % 3] - n2[..., (a + 2) % 3] + n3)
                    for a in range(3))
    return MinkowskiFunctionals(
        thresholds=thresholds, counts=counts, n_cells=n_cells, euler_characteristic=chi,
        genus=const(1.0) - f64_of(chi) / const(2.0), v0=f64_of(n3) / const(float(n_cells)),
        v1=const(2.0) * surface / const(9.0) / const(volume), v2=const(2.0) * curvature / const(9.0) / const(volume),
        v3=f64_of(chi) / const(volume))


_MINKOWSKI_PER_BOX = ("counts", "euler_characteristic", "genus", "v0", "v1", "v2", "v3")


def get_minkowski_functionals(field, boxlength, *, thresholds=32, select="below",
                              periodic=True) -> MinkowskiFunctionals:
    """The Minkowski functionals (Schmalzing & Buchert 1997; for 21-cm fields Gleser et al. 2006, Friedrich et al.
    2011, Yoshiura et al. 2017) of the excursion sets of the 3-D ``field`` in a box of ``boxlength`` (a scalar or 3
    lengths): at every threshold t the cells with ``v < t`` (``select="below"``: for a neutral fraction the ionised
    phase) or ``v >= t`` (``"above"``) form a set whose volume, surface, integrated mean curvature and Euler
    characteristic are counted from the cells, faces, edges and vertices of the cubical complex of the box, which
    wraps on the ``periodic`` axes (a bool or three).  ``thresholds``: an integer (``minkowski_thresholds``: that many
    equally spaced values strictly inside the range of the field) or an increasing 1-D array of at most 255 values;
    all of them are served by one read of the field.  The estimators are written down at ``MinkowskiFunctionals``; for
    cubic cells they are the Crofton estimators of Schmalzing & Buchert, and their lattice correction 2/9 is exact
    only for cubic cells.  Every count is an integer fixed by the field: two calls give the same bytes, and a
    threshold's row does not depend on the other thresholds."""
    _check_bubble_field(field)
    shape = _shape(field)
    L = _lengths(boxlength)
    t, args = _minkowski_args(thresholds, select, periodic, field)
    cell = [l / n for l, n in zip(L, shape)]
    res = _minkowski_result(_f32(field), shape, cell, t, args, (0,), None)
    for name in _MINKOWSKI_PER_BOX:
        setattr(res, name, getattr(res, name)[0])
    return res


def lightcone_minkowski_functionals(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                                    **kw) -> MinkowskiFunctionals:
    """Minkowski functionals of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices) of cells of ``cell_size``
    [Mpc], chunked as ``lightcone_bubble_clusters`` chunks it; all chunks go through one library call.  The transverse
    axes are periodic and the line of sight is open, so ``periodic`` is not a keyword here; the others (``thresholds``,
    ``select``) are those of ``get_minkowski_functionals``.  An integer ``thresholds`` is resolved once over the whole
    lightcone, so the chunks share their thresholds.  Every per-box entry carries a leading chunk axis."""
    _check_bubble_field(lightcone, "lightcone")
    if "periodic" in kw:
        raise ValueError("periodic is fixed for a lightcone: the transverse axes are, the line of sight is not")
    unknown = set(kw) - {"thresholds", "select"}
    if unknown:
        raise ValueError(f"unknown keywords: {sorted(unknown)}")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    t, args = _minkowski_args(kw.get("thresholds", 32), kw.get("select", "below"), (True, True, False), lightcone)
    res = _minkowski_result(_f32(lightcone), (nx, ny, n), [dx, dx, dx], t, args, starts, ns)
    res.chunk_starts, res.redshifts = starts, z
    return res


GRANULOMETRY_MAX_RADII = api.GRANULOMETRY_MAX_RADII
EDT_NONE = api.EDT_NONE


def _periodic3(periodic) -> tuple:
    if np.ndim(periodic) == 0:
        return (bool(periodic),) * 3
    periodic = tuple(bool(p) for p in periodic)
    if len(periodic) != 3:
        raise ValueError("periodic must be a bool or three bools")
    return periodic


def granulometry_radii(shape, n=32, periodic=True) -> np.ndarray:
    """The squared radii, in cells^2, ``get_granulometry`` uses for a grid of ``shape``: the distinct ``floor(r^2)``
    (int64) of ``n`` radii r log-spaced from 1 to the smallest reach of an axis, half its length where it is
    ``periodic`` and its length where it is open.  A small box gets fewer radii than asked for."""
    if isinstance(n, (bool, np.bool_)) or np.ndim(n) != 0 or int(n) != n:
        raise ValueError("the number of radii must be an integer")
    if not 1 <= int(n) <= GRANULOMETRY_MAX_RADII:
        raise ValueError(f"a granulometry takes 1 to {GRANULOMETRY_MAX_RADII} radii, got {int(n)}")
    per = _periodic3(periodic)
    reach = min(int(m) / 2.0 if p else float(int(m)) for m, p in zip(shape, per))
    r = np.geomspace(1.0, max(reach, 1.0), int(n))
    return np.unique(np.floor(r * r).astype(np.int64))


@dataclass
class Granulometry:
    """What ``get_granulometry`` and ``lightcone_granulometry`` return (the latter with a leading chunk axis on
    everything but the radii).  ``radii2`` (K,) int64 the squared radii s in cells^2 and ``radii`` = sqrt(s) cell;
    ``covered`` int64 (K,) the cells inside an inscribed ball with D2 > s and ``eroded`` the cells with D2 > s
    (``c21cm_granulometry_grids``); ``n_selected``; ``filling_fraction`` = n_selected / cells; ``cumulative`` F =
    covered / n_selected, the share of the selected volume that fits a sphere of that radius (NaN without a selected
    cell); ``pdf`` (K - 1,) = (F_k - F_{k+1}) / (ln r_{k+1} - ln r_k) at ``r_mid`` = sqrt(r_k r_{k+1}) (0 at a pair
    that starts at r = 0); ``mean_radius`` = (sum_k (F_k - F_{k+1}) r_mid_k + F_{K-1} r_{K-1}) / F_0;
    ``max_distance`` = sqrt(max D2) cell, the radius of the largest inscribed ball (inf in a box without an unselected
    cell); with ``return_sizes`` ``sizes`` float32 shaped as the box: the largest asked radius at which the cell is
    covered, 0 where it is covered at none, NaN where it is not selected; for a lightcone ``chunk_starts`` and
    ``redshifts``."""

    radii2: object
    radii: object
    r_mid: object
    covered: object
    eroded: object
    n_selected: object
    filling_fraction: object
    cumulative: object
    pdf: object
    mean_radius: object
    max_distance: object
    sizes: object = None
    chunk_starts: np.ndarray | None = None
    redshifts: np.ndarray | None = None


def _cubic_cell(L, shape) -> float:
    cell = [l / n for l, n in zip(L, shape)]
    if any(abs(c - cell[0]) > 1e-9 * cell[0] for c in cell[1:]):
        raise ValueError(f"distance transforms and granulometry need cubic cells, got cells of {cell}")
    return float(cell[0])


def _granulometry_args(threshold, select, periodic):
    if select not in ("below", "above"):
        raise ValueError("select must be 'below' (v < threshold) or 'above' (v >= threshold)")
    if isinstance(threshold, (bool, np.bool_)) or np.ndim(threshold) != 0 or not np.isfinite(float(threshold)):
        raise ValueError("threshold must be a finite number")
    return dict(threshold=float(threshold), select_below=select == "below", periodic=_periodic3(periodic))


def _granulometry_radii2(radii, shape, periodic, cell) -> np.ndarray:
    if np.ndim(radii) == 0:
        return granulometry_radii(shape, radii, periodic)
    r = np.asarray(radii, np.float64)
    if r.ndim != 1 or r.size < 1 or not np.all(np.isfinite(r)) or np.any(r < 0):
        raise ValueError("radii must be an integer or a 1-D array of finite lengths >= 0")
    s = np.unique(np.floor((r / cell) ** 2).astype(np.int64))
    if s.size > GRANULOMETRY_MAX_RADII:
        raise ValueError(f"a granulometry takes at most {GRANULOMETRY_MAX_RADII} distinct radii, got {s.size}")
    return s


def _granulometry_result(f, shape, cell, radii2, args, offsets, row_pitch, return_sizes) -> Granulometry:
    out = api.granulometry(f, shape, radii2, offsets=offsets, row_pitch=row_pitch, return_level=return_sizes, **args)
    covered, eroded, stats = out[:3]
    n_cells = float(int(shape[0]) * int(shape[1]) * int(shape[2]))
    r = np.sqrt(radii2.astype(np.float64)) * cell
    with np.errstate(divide="ignore", invalid="ignore"):
        dln = np.diff(np.log(r))
    r_mid = np.sqrt(r[:-1] * r[1:])
    table = np.concatenate(([np.nan, 0.0], r)).astype(np.float32)  # by level + 1
    if _is_torch(covered):
        import torch

        def dev(a, dtype=np.float64):
            return torch.from_numpy(np.asarray(a, dtype)).to(covered.device)

        def f64_of(a):
            return a.to(torch.float64)

        sqrt, where, inf = torch.sqrt, torch.where, dev(np.inf)

        def lookup(level):
            return dev(table, np.float32)[(level + 1).long()]
    else:
        def dev(a, dtype=np.float64):
            return np.asarray(a, dtype)

        def f64_of(a):
            return a.astype(np.float64)

        sqrt, where, inf = np.sqrt, np.where, np.float64(np.inf)

        def lookup(level):
            return table[level + 1]

    n_sel, deepest = stats[:, 0], stats[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        cum = f64_of(covered) / f64_of(n_sel)[:, None]  # 0 / 0 = NaN
        step = cum[:, :-1] - cum[:, 1:]
        mean = ((step * dev(r_mid)).sum(-1) + cum[:, -1] * dev(r[-1])) / cum[:, 0]
    res = Granulometry(
        radii2=dev(radii2, np.int64), radii=dev(r), r_mid=dev(r_mid), covered=covered, eroded=eroded, n_selected=n_sel,
        filling_fraction=f64_of(n_sel) / dev(n_cells), cumulative=cum, pdf=step / dev(dln), mean_radius=mean,
        max_distance=where(deepest >= EDT_NONE, inf, sqrt(f64_of(deepest)) * dev(cell)))
    if return_sizes:
        res.sizes = lookup(out[3]).reshape((len(offsets),) + tuple(int(n) for n in shape))
    return res


_GRANULOMETRY_PER_BOX = ("covered", "eroded", "n_selected", "filling_fraction", "cumulative", "pdf", "mean_radius",
                         "max_distance", "sizes")


def get_distance_transform(field, boxlength, *, threshold=0.5, select="below", periodic=True, squared=False):
    """The exact Euclidean distance transform of the 3-D ``field`` in a box of ``boxlength`` (a scalar or 3 lengths;
    the cells must be cubic): for every cell with ``v < threshold`` (``select="below"``) or ``v >= threshold``
    (``"above"``) the distance, centre to centre, to the nearest cell that is not selected, with the minimum image on
    the ``periodic`` axes (a bool or three) and nothing beyond an open face -- the convention of
    ``scipy.ndimage.distance_transform_edt``.  Returns float32 distances in the units of ``boxlength`` (0 at
    unselected cells, inf in a box without one), or with ``squared`` the int32 squared distances in cells^2 (2^30 in
    such a box), shaped as the field: numpy for numpy input, torch on its device for a torch CUDA field."""
    _check_bubble_field(field)
    shape = _shape(field)
    cell = _cubic_cell(_lengths(boxlength), shape)
    args = _granulometry_args(threshold, select, periodic)
    d2 = api.granulometry(_f32(field), shape, np.zeros(0, np.int64), return_dist2=True, **args)[3].reshape(shape)
    if squared:
        return d2
    if _is_torch(d2):
        import torch

        d = torch.sqrt(d2.to(torch.float64)) * torch.full((), cell, dtype=torch.float64, device=d2.device)
        return torch.where(d2 >= EDT_NONE, torch.full_like(d, np.inf), d).to(torch.float32)
    return np.where(d2 >= EDT_NONE, np.inf, np.sqrt(d2.astype(np.float64)) * cell).astype(np.float32)


def get_granulometry(field, boxlength, *, threshold=0.5, select="below", radii=32, periodic=True,
                     return_sizes=False) -> Granulometry:
    """The granulometry bubble size distribution (Kakiichi et al. 2017; beside the mean-free-path and
    friends-of-friends estimators in Lin et al. 2016 and Giri et al. 2018) of the 3-D ``field`` in a box of
    ``boxlength`` (a scalar or 3 lengths; the cells must be cubic): the share of the cells with ``v < threshold``
    (``select="below"``: for a neutral fraction the ionised phase) or ``v >= threshold`` (``"above"``) that lies in a
    ball of radius > r which holds selected cells only, for every radius.  A ball is one inscribed at a cell centre:
    its squared radius is the cell's squared distance D2 to the nearest unselected cell (``get_distance_transform``),
    across the faces of the ``periodic`` axes (a bool or three).  ``radii``: an integer (``granulometry_radii``: up to
    that many log-spaced radii) or lengths, turned into the distinct ``floor((r / cell)^2)``.  Everything counted is
    an integer fixed by the mask: two calls give the same bytes, a radius' counts do not depend on the other radii,
    and ``covered`` never grows with the radius.  ``return_sizes`` adds the per-cell radius."""
    _check_bubble_field(field)
    shape = _shape(field)
    cell = _cubic_cell(_lengths(boxlength), shape)
    args = _granulometry_args(threshold, select, periodic)
    radii2 = _granulometry_radii2(radii, shape, args["periodic"], cell)
    res = _granulometry_result(_f32(field), shape, cell, radii2, args, (0,), None, return_sizes)
    for name in _GRANULOMETRY_PER_BOX:
        v = getattr(res, name)
        if v is not None:
            setattr(res, name, v[0])
    return res


def lightcone_granulometry(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, redshifts=None,
                           **kw) -> Granulometry:
    """Granulometry of the chunks of a rectilinear ``lightcone`` (nx, ny, n_slices) of cubic cells of ``cell_size``
    [Mpc], chunked as ``lightcone_bubble_clusters`` chunks it; all chunks go through one library call and share the
    radii.  The transverse axes are periodic and the line of sight is open, so ``periodic`` is not a keyword here; the
    others (``threshold``, ``select``, ``radii``, ``return_sizes``) are those of ``get_granulometry``.  Every per-box
    entry carries a leading chunk axis."""
    _check_bubble_field(lightcone, "lightcone")
    if "periodic" in kw:
        raise ValueError("periodic is fixed for a lightcone: the transverse axes are, the line of sight is not")
    unknown = set(kw) - {"threshold", "select", "radii", "return_sizes"}
    if unknown:
        raise ValueError(f"unknown keywords: {sorted(unknown)}")
    nx, ny, ns = _shape(lightcone)
    dx = float(cell_size)
    if not (np.isfinite(dx) and dx > 0):
        raise ValueError("cell_size must be positive and finite")
    n, starts, z = _chunks(ns, nx, chunk_length, chunk_starts, redshifts)
    shape = (nx, ny, n)
    args = _granulometry_args(kw.get("threshold", 0.5), kw.get("select", "below"), (True, True, False))
    radii2 = _granulometry_radii2(kw.get("radii", 32), shape, args["periodic"], dx)
    res = _granulometry_result(_f32(lightcone), shape, dx, radii2, args, starts, ns, kw.get("return_sizes", False))
    res.chunk_starts, res.redshifts = starts, z
    return res
