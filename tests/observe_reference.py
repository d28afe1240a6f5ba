"""The definition of the telescope-resolution smoothing (``c21cm_observe_smooth_grids``, include/c21cm_grid.h; DESIGN
section 4.11) restated in numpy and fp64: the spec the device kernels are held to.  ``test_observe_host.py`` pins it
against ``scipy.ndimage.gaussian_filter(mode="wrap", truncate=4.0)`` and a plain loop.

Input: a float32 field f[i, j, s] of shape (nx, ny, ns), the line of sight s last.  Per slice a width sigma[s] >= 0 in
cells and two counts below[s], above[s] >= 0.

1. mean     m[s] = the fp64 mean of f[:, :, s]; with ``subtract_mean`` g = float32(float64(f) - m[s]), else g = f.
2. beam     lw = int(4 sigma + 0.5); for lw >= 1, w[d] = exp(-d^2 / (2 sigma^2)), d = 0 .. lw, divided in fp64 by
            w[0] + 2 sum_{d >= 1} w[d] and rounded to fp32; h[i] = sum_{d = -lw .. lw} w[|d|] g[(i + d) mod n] along
            x, then along y.  lw = 0 leaves the slice as it is.  sigma > 128 (lw > 512) is refused.
3. channel  out[i, j, s] = the mean of h over the slices s - below[s] .. s + above[s], clipped to [0, ns - 1] on an
            open line of sight; with ``periodic_los`` wrapped, and below + above + 1 <= ns is required.

Everything after the float32 rounding of g and of the weights is fp64 here; the device works in fp32.
"""

import numpy as np

MAX_SIGMA = 128.0


def half_width(sigma: float) -> int:
    return int(4.0 * float(sigma) + 0.5)


def half_kernel(sigma: float, round_weights: bool = True) -> np.ndarray:
    """w[0 .. lw] as float64: normalised in fp64 and, with ``round_weights``, rounded to fp32; [1.0] for lw = 0"""
    lw = half_width(sigma)
    if lw == 0:
        return np.ones(1)
    d = np.arange(lw + 1, dtype=np.float64)
    w = np.exp(-d * d / (2.0 * float(sigma) ** 2))
    w = w / (w[0] + 2.0 * np.sum(w[1:]))
    return w.astype(np.float32).astype(np.float64) if round_weights else w


def check_args(shape, sigma, below, above, periodic_los):
    nx, ny, ns = shape
    if min(nx, ny, ns) < 1 or nx * ny * ns >= 2**31:
        raise ValueError("bad shape")
    if sigma.shape != (ns,) or below.shape != (ns,) or above.shape != (ns,):
        raise ValueError("one width and two counts per slice")
    if not np.all(np.isfinite(sigma)) or np.any(sigma < 0) or np.any(sigma > MAX_SIGMA):
        raise ValueError("sigma must be finite and in [0, 128]")
    if np.any(below < 0) or np.any(above < 0):
        raise ValueError("counts must be >= 0")
    if periodic_los and np.any(below.astype(np.int64) + above + 1 > ns):
        raise ValueError("a periodic channel must fit the line of sight")


def slice_means(f: np.ndarray) -> np.ndarray:
    return f.astype(np.float64).sum(axis=(0, 1)) / float(f.shape[0] * f.shape[1])


def centre(f: np.ndarray, subtract_mean: bool):
    """(g as float32, m)"""
    m = slice_means(f)
    if not subtract_mean:
        return f.astype(np.float32), m
    return (f.astype(np.float64) - m[None, None, :]).astype(np.float32), m


def wrap_convolve(g: np.ndarray, w: np.ndarray, axis: int) -> np.ndarray:
    """h[i] = sum_d w[|d|] g[(i + d) mod n] along ``axis`` in fp64; the index wraps as often as it has to"""
    g = g.astype(np.float64)
    h = w[0] * g
    for d in range(1, len(w)):
        h = h + w[d] * (np.roll(g, d, axis=axis) + np.roll(g, -d, axis=axis))
    return h


def beam(g: np.ndarray, sigma: np.ndarray, round_weights: bool = True) -> np.ndarray:
    h = np.empty(g.shape, np.float64)
    for s in range(g.shape[2]):
        w = half_kernel(sigma[s], round_weights)
        sl = g[:, :, s].astype(np.float64)
        h[:, :, s] = sl if len(w) == 1 else wrap_convolve(wrap_convolve(sl, w, 0), w, 1)
    return h


def channel(h: np.ndarray, below: np.ndarray, above: np.ndarray, periodic_los: bool) -> np.ndarray:
    ns = h.shape[2]
    out = np.empty(h.shape, np.float64)
    for s in range(ns):
        lo, hi = s - int(below[s]), s + int(above[s])
        if not periodic_los:
            lo, hi = max(lo, 0), min(hi, ns - 1)
        acc = np.zeros(h.shape[:2], np.float64)
        for q in range(lo, hi + 1):
            acc = acc + h[:, :, q % ns]
        out[:, :, s] = acc / float(hi - lo + 1)
    return out


def observe_smooth(f, sigma, below, above, periodic_los=False, subtract_mean=True, round_weights=True):
    """(out float64, m float64, g float32)"""
    f = np.asarray(f, np.float32)
    ns = f.shape[2]
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (ns,))
    below = np.broadcast_to(np.asarray(below, np.int64), (ns,))
    above = np.broadcast_to(np.asarray(above, np.int64), (ns,))
    check_args(f.shape, sigma, below, above, periodic_los)
    if not np.all(np.isfinite(f)):
        raise FloatingPointError("a field value is not finite")
    g, m = centre(f, subtract_mean)
    return channel(beam(g, sigma, round_weights), below, above, periodic_los), m, g
