"""fp64 numpy restatement of the bispectrum estimator of ``21cmfast_amd/powerspec.py``: the
spec the device code is held to.

Conventions are ``get_power``'s: V = Lx Ly Lz, N = nx ny nz, D the unnormalised DFT of the field, wavenumbers
``2 pi fftfreq`` per axis, |k| = sqrt((kx^2 + ky^2) + kz^2), a mode in shell b when e[b] <= |k| < e[b + 1].  For a
triangle of shells (b1, b2, b3), with delta_b(x) = sum_{k in b} D(k) exp(+i k x) and I_b(x) the same sum of ones,

    S = sum_x delta_b1 delta_b2 delta_b3,   n_tri = (1/N) sum_x I_b1 I_b2 I_b3,   B = (V^2 / N^3) S / (N n_tri)

(NaN where n_tri = 0).  ``fft_estimator`` computes this with transforms, ``brute_force`` by enumerating the closed
triplets k1 + k2 + k3 = 0 (modulo the grid) of tiny grids.  Both also return each triangle's scale, (V^2 / N^3)
sum_x |delta_b1 delta_b2 delta_b3| / (N n_tri): what an error in B is measured against.
"""

from __future__ import annotations

import numpy as np


def lengths(boxlength):
    return (float(boxlength),) * 3 if np.ndim(boxlength) == 0 else tuple(float(x) for x in boxlength)


def k_max(shape, boxlength):
    return (2.0 / 3.0) * min(np.pi * n / L for n, L in zip(shape, lengths(boxlength)))


def k_min(boxlength):
    return max(2.0 * np.pi / L for L in lengths(boxlength)) / 2.0


def default_edges(shape, boxlength, bins, log_bins=False):
    lo, hi = k_min(boxlength), k_max(shape, boxlength)
    return np.geomspace(lo, hi, bins + 1) if log_bins else np.linspace(lo, hi, bins + 1)


def all_triangles(n_bins):
    return np.array([(a, b, c) for a in range(n_bins) for b in range(a, n_bins) for c in range(b, n_bins)], np.int32)


def closing_triangles(edges):
    """Every b1 <= b2 <= b3 whose shells can hold a closed triangle: e[b3] < e[b1 + 1] + e[b2 + 1]."""
    e = np.asarray(edges, np.float64)
    t = all_triangles(len(e) - 1)
    return t[e[t[:, 2]] < e[t[:, 0] + 1] + e[t[:, 1] + 1]]


def shell_index(shape, boxlength, edges):
    """The shell of every mode of the full grid (np.digitize - 1; -1 or n_bins outside)."""
    kx, ky, kz = (np.fft.fftfreq(n, d=L / n) * 2.0 * np.pi for n, L in zip(shape, lengths(boxlength)))
    kk = np.sqrt((kx[:, None, None] ** 2 + ky[None, :, None] ** 2) + kz[None, None, :] ** 2)
    return np.digitize(kk, np.asarray(edges, np.float64)) - 1


def _finish(S, A, count, shape, boxlength):
    V, N = float(np.prod(lengths(boxlength))), float(np.prod(shape))
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = (V * V / N**3) / (N * count.astype(np.float64))
        B = np.where(count > 0, S * norm, np.nan)
        scale = np.where(count > 0, A * norm, np.nan)
    return B, count, scale


def fft_estimator(field, boxlength, edges, triangles):
    """``(B, n_triangles, scale)`` of the given (n, 3) triangles by the FFT estimator, everything in fp64."""
    f = np.asarray(field, np.float64)
    shape, N = f.shape, f.size
    shell = shell_index(shape, boxlength, edges)
    D = np.fft.fftn(f)
    n_bins = len(edges) - 1
    delta = [np.fft.ifftn(np.where(shell == b, D, 0.0)).real * N for b in range(n_bins)]
    ind = [np.fft.ifftn((shell == b).astype(np.float64)).real * N for b in range(n_bins)]
    tri = np.asarray(triangles)
    S, A, count = np.empty(len(tri)), np.empty(len(tri)), np.empty(len(tri), np.int64)
    for q, (a, b, c) in enumerate(tri):
        prod = delta[a] * delta[b] * delta[c]
        S[q] = prod.sum()
        A[q] = np.abs(prod).sum()
        count[q] = int(np.rint((ind[a] * ind[b] * ind[c]).sum() / N))
    return _finish(S, A, count, shape, boxlength)


def brute_force(field, boxlength, edges, triangles):
    """The same three arrays from the sum over closed triplets of modes, closure modulo the grid: S = N sum D(k1)
    D(k2) D(k3).  The scale is taken from the transforms (it has no triplet form).  Tiny grids only."""
    f = np.asarray(field, np.float64)
    shape, N = f.shape, f.size
    nx, ny, nz = shape
    shell = shell_index(shape, boxlength, edges)
    D = np.fft.fftn(f)
    n_bins = len(edges) - 1
    members = [np.argwhere(shell == b) for b in range(n_bins)]
    tri = np.asarray(triangles)
    S, count = np.empty(len(tri)), np.empty(len(tri), np.int64)
    for q, (a, b, c) in enumerate(tri):
        total, n = 0.0 + 0.0j, 0
        for m1 in members[a]:
            m2 = members[b]
            m3 = (-(m1[None, :] + m2)) % np.array(shape)[None, :]
            hit = shell[m3[:, 0], m3[:, 1], m3[:, 2]] == c
            n += int(hit.sum())
            total += D[tuple(m1)] * np.sum(D[m2[hit, 0], m2[hit, 1], m2[hit, 2]] * D[m3[hit, 0], m3[hit, 1], m3[hit, 2]])
        S[q] = total.real * N
        count[q] = n
    delta = [np.fft.ifftn(np.where(shell == b, D, 0.0)).real * N for b in range(n_bins)]
    A = np.array([np.abs(delta[a] * delta[b] * delta[c]).sum() for a, b, c in tri])
    return _finish(S, A, count, shape, boxlength)


def plane_wave_field(shape, boxlength, modes, amplitudes, phases):
    """sum_i A_i cos(k_i x + phi_i) with k_i = 2 pi modes[i] / L per axis (integer mode numbers), float64."""
    L = lengths(boxlength)
    x = [np.arange(n) * (l / n) for n, l in zip(shape, L)]
    out = np.zeros(shape)
    for m, a, p in zip(modes, amplitudes, phases):
        k = [2.0 * np.pi * mi / li for mi, li in zip(m, L)]
        out += a * np.cos(k[0] * x[0][:, None, None] + k[1] * x[1][None, :, None] + k[2] * x[2][None, None, :] + p)
    return out


def plane_wave_bispectrum(boxlength, amplitudes, phases, n_tri):
    """B of the triangle that holds the three plane waves (k1 + k2 + k3 = 0, three different shells):
    V^2 A1 A2 A3 cos(phi1 + phi2 + phi3) / (4 n_tri)."""
    V = float(np.prod(lengths(boxlength)))
    return V * V * float(np.prod(amplitudes)) * np.cos(float(np.sum(phases))) / (4.0 * n_tri)
