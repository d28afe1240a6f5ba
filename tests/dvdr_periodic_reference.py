"""fp64 restatement of the periodic dv/dr correction of a coeval box (reference: src/py21cmfast/rsds.py
:16-103, include_dvdr_in_tau21 with periodic = True), written from the formula.

The reference's gradient is ``irfftn(1j k_z rfftn(v))``: only k_z enters, so it is the spectral
derivative of every line along the last axis, ``irfft(1j k rfft(v))`` with ``k = 2 pi rfftfreq(n, dx)``.
Two forms of it live here: the ``rfft`` form and the exact circulant sum that the direct kernel
evaluates.  Velocities in Mpc/s, ``dx`` in Mpc, ``hubble`` H(z) in 1/s (a scalar or one per slice)."""

import numpy as np


def gradient_rfft(v, dx):
    """irfft(1j k rfft(v)) along the last axis, fp64.  For even n the Nyquist mode drops out: 1j k_N X_N
    is purely imaginary and the inverse real transform ignores it."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    k = 2.0 * np.pi * np.fft.rfftfreq(n, dx)
    return np.fft.irfft(1j * k * np.fft.rfft(v, axis=-1), n=n, axis=-1)


def circulant_coefficients(n, dx):
    """d_j of g_j = sum_m d[(j - m) mod n] v_m: d_0 = 0 and, with c = 2 pi / (n dx),
    d_j = (c / 2) (-1)^j cot(pi j / n) for even n, (c / 2) (-1)^j / sin(pi j / n) for odd n."""
    j = np.arange(1, n, dtype=np.float64)
    sign = np.where(np.arange(1, n) % 2, -1.0, 1.0)
    c = 2.0 * np.pi / (n * dx)
    d = np.zeros(n)
    if n % 2:
        d[1:] = 0.5 * c * sign / np.sin(np.pi * j / n)
    else:
        d[1:] = 0.5 * c * sign * np.cos(np.pi * j / n) / np.sin(np.pi * j / n)
        d[n // 2] = 0.0  # cot(pi / 2)
    return d


def gradient_circulant(v, dx):
    """The same gradient as the exact circulant sum, fp64."""
    v = np.asarray(v, np.float64)
    n = v.shape[-1]
    d = circulant_coefficients(n, dx)
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n  # [j, m] -> (j - m) mod n
    return v @ d[idx].T


def taylor_form(brightness_temp, grad, hubble, max_dvdr):
    """bt / |1 + clip(g, +-max_dvdr H) / H| in fp64 (rsds.py:81-87)."""
    H = np.broadcast_to(np.asarray(hubble, np.float64), (np.shape(grad)[-1],))
    mx = max_dvdr * H
    return np.asarray(brightness_temp, np.float64) / np.abs(1.0 + np.clip(grad, -mx, mx) / H)


def tau_factor(tau_21, grad, hubble):
    """(1 - exp(-tau / |1 + g / H|)) / (1 - exp(-tau)) in fp64, 1 where tau < 1e-10 (rsds.py:88-100)."""
    H = np.broadcast_to(np.asarray(hubble, np.float64), (np.shape(grad)[-1],))
    tau = np.asarray(tau_21, np.float64)
    comp = np.abs(1.0 + np.asarray(grad, np.float64) / H)
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = (1.0 - np.exp(-tau / comp)) / (1.0 - np.exp(-tau))
    return np.where(tau < 1e-10, 1.0, fac)


def include_dvdr_in_tau21(brightness_temp, los_velocity, hubble, dx, max_dvdr, tau_21=None, grad=None):
    """The corrected brightness temperature in fp64 (the Taylor form, or with ``tau_21`` the tau form
    whose factor the reference rounds to float32 before it multiplies); ``grad``: a gradient computed
    before, else the ``rfft`` form of ``los_velocity``."""
    g = gradient_rfft(los_velocity, dx) if grad is None else grad
    if tau_21 is None:
        return taylor_form(brightness_temp, g, hubble, max_dvdr)
    return np.asarray(brightness_temp, np.float64) * np.float32(tau_factor(tau_21, g, hubble)).astype(np.float64)
