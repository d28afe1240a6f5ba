"""The k-space windows of filter_box in plain numpy, and the filtered spectrum of a real box.

Restated from the reference's filtering.c (:18-32 top-hat, sharp-k, Gaussian; :80-104 top-hat x
exp(-r / mfp); :106-117 spherical shell; :119-306 multiple scattering; :308-394 filter_box) as
array expressions in float64.  The reference's own narrowings are part of the definition and are
kept: filter_box holds k_x, k_y, k_z and |k|^2 in `float`, takes the root in double, and holds kR
(types 0, 1) or (kR)^2 (type 2) in `float`; R and R_param arrive as `float`.  Everything else --
the window itself, the transform of the box, their product -- is float64 here, so a spectrum from
this module carries none of the float32 transform round-off that the implementations under test do.

test_window_reference.py pins this module against the CPU oracle's C restatement of the same file.
"""

import math

import numpy as np

F32 = np.float32


def _f32(x):
    """Round to float and continue in double (a C `float` variable read back into a double expression)."""
    return np.asarray(x, np.float64).astype(F32).astype(np.float64)


def _sl(x):
    """3 (sin x - x cos x) / x^3 without the small-argument branch (filtering.c:21, 256, 280)."""
    return 3.0 * x ** -3.0 * (np.sin(x) - np.cos(x) * x)


def tophat(kR):
    kR = np.asarray(kR, np.float64)
    safe = np.where(kR < 1e-4, 1.0, kR)
    return np.where(kR < 1e-4, 1 - kR * kR / 10, _sl(safe))


def sharp_k(kR):
    return np.where(np.asarray(kR, np.float64) * 0.413566994 > 1, 0.0, 1.0)


def gaussian(kR_squared):
    return np.exp(-0.643 * 0.643 * np.asarray(kR_squared, np.float64) / 2.0)


def exp_mfp(k, R, mfp):
    """Top-hat times exp(-r / mfp) (Davies & Furlanetto), filtering.c:80-104 with exp_term = exp(-R / mfp)
    formed from the float arguments as filter_box does (:320-322)."""
    R, mfp = float(F32(R)), float(F32(mfp))
    exp_term = math.exp(float(-F32(R) / F32(mfp)))  # float quotient widened: `exp(-R / R_param)` on floats
    kR = np.asarray(k, np.float64) * R
    ratio = mfp / R
    ts_0 = 6 * ratio ** 3 - exp_term * (6 * ratio ** 3 + 6 * ratio ** 2 + 3 * ratio)
    small = ts_0 + (exp_term * (2 * ratio ** 2 + 0.5 * ratio) - 2 * ts_0 * ratio ** 2) * kR * kR
    x = np.where(kR < 1e-4, 1.0, kR)
    f = (x * x * ratio ** 2 + 2 * ratio + 1) * ratio * np.cos(x)
    f = f + (x * x * (ratio ** 2 - ratio ** 3) + ratio + 1) * np.sin(x) / x
    f = f * exp_term
    f = f - 2 * ratio ** 2
    f = f * (-3 * ratio / ((x * ratio) ** 2 + 1) ** 2)
    return np.where(kR < 1e-4, small, f)


def shell(k, R_inner, R_outer):
    R_inner, R_outer = float(F32(R_inner)), float(F32(R_outer))
    k = np.asarray(k, np.float64)
    ki, ko = k * R_inner, k * R_outer
    q = R_inner / R_outer
    small = 1.0 - ko * ko / 10 * (q ** 5 - 1) / (q ** 3 - 1)
    big = ko >= 1e-4
    ki, ko = np.where(big, ki, 1.0), np.where(big, ko, 2.0)
    full = 3.0 / (ko ** 3 - ki ** 3) * (np.sin(ko) - np.cos(ko) * ko - np.sin(ki) + np.cos(ki) * ki)
    return np.where(big, full, small)


# ---- multiple scattering (arXiv:2601.14360), filtering.c:119-306
def ms_mu(x_em):
    z = math.log10(x_em)
    if x_em > 30:
        return 1.0 - 1.0478 * x_em ** -0.7266
    if x_em > 3.0:
        return -0.104 * z ** 5 + 0.4867 * z ** 4 - 0.8217 * z ** 3 + 0.4889 * z * z + 0.264 * z + 0.518
    if x_em > 0.2:
        return -0.0285 * z ** 5 + 0.087 * z ** 4 - 0.1205 * z ** 3 - 0.0456 * z * z + 0.3787 * z + 0.5285
    return 0.3982 * x_em ** 0.1592


def ms_eta(x_em):
    z = math.log10(x_em)
    if x_em > 20.0:
        return 1.0 - 2.804 * x_em ** -1.242
    if x_em > 3.0:
        return 2.17 * z ** 5 - 8.832 * z ** 4 + 13.579 * z ** 3 - 10.04 * z * z + 4.166 * z - 0.17
    if x_em > 0.2:
        return 0.352 * z ** 5 - 0.0516 * z ** 4 - 0.293 * z ** 3 + 0.342 * z * z + 0.582 * z + 0.266
    return 0.4453 * x_em ** 1.296


def ms_alphas_betas(R_inner, R_outer, R_star):
    """(alpha_outer, beta_outer, alpha_inner, beta_inner), filtering.c:162-186."""
    if R_star == 0.0:
        return 1.0, 0.0, 1.0, 1.0
    out = []
    for R in (R_outer, R_inner):
        mu, eta = ms_mu(R / R_star), ms_eta(R / R_star)
        out += [(1.0 / eta - 1.0) / (1.0 / mu - 1.0) ** 2, (1.0 / eta - 1.0) / (1.0 / mu - 1.0)]
    return tuple(out)


def _gamma_inv(x):
    """1 / Gamma(x), zero at the poles."""
    return 0.0 if (x <= 0.0 and x == math.floor(x)) else 1.0 / math.gamma(x)


def _asymptotic_2F3(kR, alpha, beta):
    a1, a2, b1 = (2.0 + alpha) / 2.0, (3.0 + alpha) / 2.0, 5.0 / 2.0
    b2, b3 = (2.0 + alpha + beta) / 2.0, (3.0 + alpha + beta) / 2.0
    if a1 < 20.0:
        g_a1, g_a2 = math.gamma(a1), math.gamma(a2)
        g21, g32 = math.gamma(b2) / g_a1, math.gamma(b3) / g_a2
    else:
        y = beta / 2
        g21 = a1 ** y * math.exp((a1 + y - 0.5) * (y / a1 - y * y / (2.0 * a1 * a1) + y ** 3 / (3.0 * a1 ** 3)) - y)
        g32 = a2 ** y * math.exp((a2 + y - 0.5) * (y / a2 - y * y / (2.0 * a2 * a1) + y ** 3 / (3.0 * a2 ** 3)) - y)
    if alpha < 10.0:
        d1 = (math.pi * math.gamma(a1) * _gamma_inv(b1 - a1) / math.gamma(b2 - a1) / math.gamma(b3 - a1)
              / (kR / 2.0) ** (alpha + 2.0))
        d2 = (-2.0 * math.pi * math.gamma(a2) * _gamma_inv(b1 - a2) * _gamma_inv(b2 - a2) / math.gamma(b3 - a2)
              / (kR / 2.0) ** (alpha + 3.0))
    else:
        d1 = d2 = 0.0
    ph = kR - math.pi * (2.0 + beta) / 2.0
    F = (np.cos(ph) - (1.0 + (alpha - 1.0) * beta) / kR * np.sin(ph)) / (kR / 2) ** (beta + 2)
    return (F + d1 + d2) * 0.75 * g21 * g32


def hyper_2F3(kR, alpha, beta):
    kR = np.asarray(kR, np.float64)
    if beta == 0.0:
        return _sl(np.where(kR == 0, np.nan, kR))
    out = np.empty_like(kR)
    lo = kR < 30.0
    x = kR[lo]
    total, term, live = np.zeros_like(x), np.ones_like(x), np.ones(x.shape, bool)
    for n in range(1, 1000):  # the series, each element stopped by its own 1e-4 criterion as the scalar loop is
        total = np.where(live, total + term, total)
        term = term * (-1.0 / (1.0 + beta / (alpha + 2.0 * n)) / (1.0 + beta / (alpha + 1 + 2.0 * n)) * x * x
                       / (2.0 * n) / (2.0 * n + 3.0))
        live &= ~(np.abs(term) < np.abs(total) * 1e-4)
        if not live.any():
            break
    out[lo] = total
    x = kR[~lo]
    F_ms, F_sl = _asymptotic_2F3(x, alpha, beta), _sl(x)
    out[~lo] = np.where(np.abs(F_ms) < np.abs(F_sl), F_ms, F_sl)
    return out


def multiple_scattering(k, R_inner, R_outer, R_star):
    R_inner, R_outer, R_star = float(F32(R_inner)), float(F32(R_outer)), float(F32(R_star))
    a_o, b_o, a_i, b_i = ms_alphas_betas(R_inner, R_outer, R_star)
    k = np.asarray(k, np.float64)
    W = R_outer ** 3.0 * hyper_2F3(k * R_outer, a_o, b_o) - R_inner ** 3.0 * hyper_2F3(k * R_inner, a_i, b_i)
    return W / (R_outer ** 3.0 - R_inner ** 3.0)


def window(filter_type, k, R, R_param=0.0, R_star=0.0):
    """W of filter_box for modes of magnitude k (float64 array; filter_box's is the double root of its
    float |k|^2): types 0 top-hat, 1 sharp-k, 2 Gaussian, 3 exp-MFP (R_param = mfp), 4 spherical shell and
    5 multiple scattering (R = inner, R_param = outer radius)."""
    k = np.asarray(k, np.float64)
    Rf = float(F32(R))
    if filter_type == 0:
        return tophat(_f32(k * Rf))  # `float kR = sqrt(k_mag_sq) * R`
    if filter_type == 1:
        return sharp_k(_f32(k * Rf))
    if filter_type == 2:  # `float kR = k_mag_sq * R * R`, left to right in float
        ksq = (k * k).astype(F32)
        return gaussian(((ksq * F32(R)) * F32(R)).astype(np.float64))
    if filter_type == 3:
        return exp_mfp(k, R, R_param)
    if filter_type == 4:
        return shell(k, R, R_param)
    if filter_type == 5:
        return multiple_scattering(k, R, R_param, R_star)
    raise ValueError(f"no such filter: {filter_type}")


def k_magnitude(shape, box_len, box_len_z):
    """|k| of every mode of the half spectrum [nx][ny][nz/2+1] as filter_box forms it: components
    2 pi i / box_len (wrapped), 2 pi j / box_len (wrapped; x's box length), 2 pi l / box_len_z, each narrowed
    to float, squares summed in float from the left, root in double."""
    nx, ny, nz = shape
    dkx, dky, dkz = 2.0 * np.pi / box_len, 2.0 * np.pi / box_len, 2.0 * np.pi / box_len_z
    ix, iy = np.arange(nx), np.arange(ny)
    kx = (np.where(ix > nx // 2, ix - nx, ix) * dkx).astype(F32)
    ky = (np.where(iy > ny // 2, iy - ny, iy) * dky).astype(F32)
    kz = (np.arange(nz // 2 + 1) * dkz).astype(F32)
    ksq = (kx * kx)[:, None, None] + (ky * ky)[None, :, None]
    ksq = ksq + (kz * kz)[None, None, :]
    assert ksq.dtype == F32
    return np.sqrt(ksq.astype(np.float64))


def filtered_spectrum(a, box_len, box_len_z, filter_type, R, R_param=0.0, R_star=0.0, spectrum=None,
                      k=None):
    """rfftn(a in float64) W(|k|).  `spectrum` / `k`: rfftn(a.astype(float64)) / k_magnitude(a.shape, ...)
    computed before (both are read, never written)."""
    if spectrum is None:
        spectrum = np.fft.rfftn(np.asarray(a, np.float64))
    if k is None:
        k = k_magnitude(a.shape, box_len, box_len_z)
    assert spectrum.dtype == np.complex128 and k.shape == spectrum.shape
    return spectrum * window(filter_type, k, R, R_param, R_star)
