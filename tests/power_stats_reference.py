"""Host restatement (numpy, fp64, the full Fourier grid) of what ``21cmfast_amd.powerspec`` adds to the
binning of ``tests/power_reference.py``: taper windows, mu and wedge cuts, the per-bin variance, and the
one-point statistics of boxes and lightcone chunks.  Grids, edges, ``np.digitize`` bins, ignore flags and
chunking are those of ``power_reference`` (imported, not repeated).  The conventions:

* windows: the named ones are the symmetric cosine-sum windows with denominator n - 1, w[i] = sum_k (-1)^k
  a_k cos(2 pi k i / (n - 1)) with a = (0.5, 0.5) "hann", (0.42, 0.5, 0.08) "blackman", (0.35875, 0.48829,
  0.14128, 0.01168) "blackmanharris".  ``window`` is None, a name or nz weights (the last axis only), or a
  tuple (wx, wy, wz) of None / name / weights.  The windowed field is f' = (f - m) wx[i] wy[j] wz[l] with m the
  plain mean of the box; the mean is NOT put back onto k = 0; the power is divided by <W^2> = mean(wx^2)
  mean(wy^2) mean(wz^2).  For cross power both fields are windowed;
* cuts (spherical only), with x = (kx kx + ky ky) + kz kz, every product and sum a separate fp64 operation in
  this order: ``mu_min`` / ``mu_max`` keep a mode iff kz kz >= (mu_min mu_min) x and kz kz <= (mu_max mu_max) x
  (a missing side is 0 or 1); ``wedge_slope`` / ``wedge_buffer`` keep it iff, with a = |kz| - wedge_buffer,
  a >= 0 and a a >= (wedge_slope wedge_slope) (kx kx + ky ky).  Cuts combine with each other and with the
  ignore flags; they never move edges;
* variance: the population variance of the per-mode power over the modes of the full grid in the bin,
  mean(P^2) - mean(P)^2 with P = |F|^2 / V or Re(F F2*) / V per mode (over <W^2> with a window); empty bins are
  NaN; ``dimensionless`` scales it by the square of the factor applied to the power;
* moments: mean, m_p = sum (v - mean)^p / N for p = 2, 3, 4 in two passes over the fp64 cast of the fp32 field;
  variance = m2, skewness = m3 / m2^1.5, kurtosis = m4 / m2^2 - 3; the histogram bin is
  ``np.digitize(v, edges) - 1``, kept when 0 <= bin < n_bins.
"""

from __future__ import annotations

import numpy as np

import power_reference as PR

_COEFFS = {"hann": (0.5, 0.5), "blackman": (0.42, 0.5, 0.08),
           "blackmanharris": (0.35875, 0.48829, 0.14128, 0.01168)}


def taper(name, n):
    if n == 1:
        return np.ones(1)
    i = np.arange(n, dtype=np.float64)
    return sum((-1) ** k * a * np.cos(2.0 * np.pi * k * i / (n - 1)) for k, a in enumerate(_COEFFS[name]))


def window_axes(window, shape):
    """(wx, wy, wz) as fp64 arrays (ones where there is no window), or None without any window."""
    if window is None:
        return None
    if not isinstance(window, tuple):
        window = (None,) * (len(shape) - 1) + (window,)
    if all(w is None for w in window):
        return None
    out = []
    for w, n in zip(window, shape):
        if w is None:
            out.append(np.ones(n))
        elif isinstance(w, str):
            out.append(taper(w, n))
        else:
            out.append(np.asarray(w, np.float64))
    return out


def windowed_spectrum(field, boxlength, deltax2=None, window=None):
    """P on the full grid: ``power_reference.spectrum`` of the windowed fields over <W^2>."""
    ws = window_axes(window, np.shape(field))
    if ws is None:
        return PR.spectrum(field, boxlength, deltax2)
    W = ws[0][:, None, None] * ws[1][None, :, None] * ws[2][None, None, :]
    mean_w2 = np.prod([np.mean(w * w) for w in ws])

    def apply(f):
        f = np.asarray(f, np.float64)
        return (f - f.mean()) * W

    return PR.spectrum(apply(field), boxlength, None if deltax2 is None else apply(deltax2)) / mean_w2


def cut_mask(shape, boxlength, mu_min=None, mu_max=None, wedge_slope=None, wedge_buffer=0.0):
    """True where a mode survives the cuts."""
    _, (kx, ky, kz) = PR._grids(shape, boxlength)
    keep = np.ones(shape, bool)
    perp = kx * kx + ky * ky
    if mu_min is not None or mu_max is not None:
        lo = 0.0 if mu_min is None else float(mu_min)
        hi = 1.0 if mu_max is None else float(mu_max)
        x = perp + kz * kz
        keep &= (kz * kz >= (lo * lo) * x) & (kz * kz <= (hi * hi) * x)
    if wedge_slope is not None:
        s = float(wedge_slope)
        a = np.abs(kz) - float(wedge_buffer)
        keep &= (a >= 0) & (a * a >= (s * s) * perp)
    return keep


def get_power(field, boxlength, *, deltax2=None, bins=None, log_bins=False, ignore_zero_mode=False,
              bins_upto_boxlen=True, ignore_kperp_zero=False, ignore_kpar_zero=False, bin_ave=True, window=None,
              mu_min=None, mu_max=None, wedge_slope=None, wedge_buffer=0.0):
    """``(power, k, counts, variance)``."""
    field = np.asarray(field)
    N = field.shape
    _, (kx, ky, kz) = PR._grids(N, boxlength)
    kmag = np.sqrt((kx * kx + ky * ky) + kz * kz)
    P = windowed_spectrum(field, boxlength, deltax2, window)
    if bins is None:
        bins = int(np.prod(N) ** (1.0 / field.ndim) / 2.2)
    edges = PR._getbins(bins, kmag, log_bins, bins_upto_boxlen)
    keep = cut_mask(N, boxlength, mu_min, mu_max, wedge_slope, wedge_buffer)
    if ignore_zero_mode:
        keep &= kmag != 0
    if ignore_kperp_zero:
        keep &= (kx != 0) | (ky != 0)
    if ignore_kpar_zero:
        keep &= kz != 0
    (p_av, k_av, p2_av), counts = PR._bin(kmag, [P, kmag, P * P], keep, edges)
    return p_av, (k_av if bin_ave else edges), counts, p2_av - p_av * p_av


def get_cylindrical_power(field, boxlength, *, deltax2=None, kperp_bins=None, kpar_bins=None, log_bins=False,
                          ignore_zero_mode=False, window=None):
    """``(power, kperp, kpar, counts, variance)``."""
    P = windowed_spectrum(field, boxlength, deltax2, window)
    kw = dict(kperp_bins=kperp_bins, kpar_bins=kpar_bins, log_bins=log_bins, ignore_zero_mode=ignore_zero_mode,
              return_counts=True)
    p, kp, kz, c = PR.get_cylindrical_power(field, boxlength, spectrum=P, **kw)
    p2 = PR.get_cylindrical_power(field, boxlength, spectrum=P * P, **kw)[0]
    return p, kp, kz, c, p2 - p * p


def lightcone_power_spectra(lightcone, cell_size, *, chunk_length=None, chunk_starts=None, dimensionless=False,
                            cylindrical=False, **binning):
    """A dict: power and variance (n_chunks, ...), k or kperp / kpar, counts, chunk_starts."""
    lc = np.asarray(lightcone)
    nx, ny, ns = lc.shape
    n = nx if chunk_length is None else int(chunk_length)
    starts = np.arange(0, ns - n + 1, n) if chunk_starts is None else np.asarray(chunk_starts, np.int64)
    L = (nx * cell_size, ny * cell_size, n * cell_size)
    d2 = binning.pop("deltax2", None)
    res = {"chunk_starts": starts, "power": [], "variance": []}
    for s in starts:
        kw = dict(binning)
        if d2 is not None:
            kw["deltax2"] = np.asarray(d2)[:, :, s:s + n]
        if cylindrical:
            p, kp, kz, c, v = get_cylindrical_power(lc[:, :, s:s + n], L, **kw)
            fac = (kp[:, None] ** 2 + kz[None, :] ** 2) ** 1.5 / (2 * np.pi**2)
            res.update(kperp=kp, kpar=kz, counts=c)
        else:
            p, k, c, v = get_power(lc[:, :, s:s + n], L, **kw)
            fac = k**3 / (2 * np.pi**2)
            res.update(k=k, counts=c)
        if dimensionless:
            p, v = p * fac, v * fac**2
        res["power"].append(p)
        res["variance"].append(v)
    res["power"], res["variance"] = np.array(res["power"]), np.array(res["variance"])
    return res


def moments(field):
    """``(mean, m2, m3, m4)`` and the scales their errors are measured against, ``(sum|v| / N, sum|d|^p / N)``."""
    v = np.asarray(field, np.float32).astype(np.float64).ravel()
    mean = v.sum() / v.size
    d = v - mean
    m = [mean] + [float((d**p).sum() / v.size) for p in (2, 3, 4)]
    scale = [float(np.abs(v).sum() / v.size)] + [float((np.abs(d) ** p).sum() / v.size) for p in (2, 3, 4)]
    return m, scale


def histogram(field, edges):
    v = np.asarray(field, np.float32).astype(np.float64).ravel()
    b = np.digitize(v, np.asarray(edges, np.float64)) - 1
    n = len(edges) - 1
    return np.bincount(b[(b >= 0) & (b < n)], minlength=n).astype(np.int64)
