"""Taper windows, cuts, variance and moments on the host: ``taper_window`` against scipy, self-checks of the
restatement (tests/power_stats_reference.py) that keep the GPU cut tests from passing vacuously, and the
argument errors of every new keyword (raised before the library is loaded)."""

import importlib

import numpy as np
import pytest

import power_reference as PR
import power_stats_reference as SR

PS = importlib.import_module("21cmfast_amd.powerspec")

NAMES = ["blackmanharris", "hann", "blackman"]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [2, 5, 37, 64])
def test_taper_window_equals_scipy(name, n):
    windows = pytest.importorskip("scipy.signal.windows")
    w = PS.taper_window(name, n)
    assert w.dtype == np.float64 and w.shape == (n,)
    np.testing.assert_allclose(w, getattr(windows, name)(n, sym=True), rtol=0, atol=1e-15)
    # the restatement writes the same windows in their textbook form
    np.testing.assert_allclose(SR.taper(name, n), w, rtol=0, atol=1e-15)


def test_resolve_window_forms():
    shape = (4, 5, 6)
    assert PS.resolve_window(None, shape) == (None, 1.0)
    assert PS.resolve_window((None, None, None), shape) == (None, 1.0)
    ws, inv = PS.resolve_window("hann", shape)
    assert ws[0] is None and ws[1] is None
    np.testing.assert_array_equal(ws[2], PS.taper_window("hann", 6))
    assert inv == 1.0 / float(np.mean(ws[2] ** 2))
    a = np.linspace(0.5, 1.5, 5)
    ws, inv = PS.resolve_window(("blackman", a, None), shape)
    np.testing.assert_array_equal(ws[1], a)
    assert ws[2] is None
    assert inv == pytest.approx(1.0 / (np.mean(PS.taper_window("blackman", 4) ** 2) * np.mean(a * a)), rel=1e-15)


def test_reference_variance_equals_a_loop_over_the_bins():
    shape, L = (9, 10, 11), (20.0, 25.0, 30.0)
    f = (np.random.default_rng(3).standard_normal(shape) + 1).astype(np.float32)
    p, k, c, v = SR.get_power(f, L)
    P = PR.spectrum(f, L)
    freq = [np.fft.fftfreq(n, d=l / n) * 2.0 * np.pi for n, l in zip(shape, L)]
    kx, ky, kz = np.meshgrid(*freq, indexing="ij")
    kmag = np.sqrt((kx * kx + ky * ky) + kz * kz)
    edges = np.linspace(kmag.min(), min(np.abs(q).max() for q in freq), len(p) + 1)
    for i in range(len(p)):
        sel = (kmag >= edges[i]) & (kmag < edges[i + 1])
        assert sel.sum() == c[i] and c[i] > 0
        np.testing.assert_allclose(p[i], P[sel].mean(), rtol=1e-12)
        np.testing.assert_allclose(v[i], np.mean((P[sel] - P[sel].mean()) ** 2), rtol=1e-9, atol=1e-12 * p[i] ** 2)
    # without options the restatement is power_reference's
    rp, rk, rc = PR.get_power(f, L, return_counts=True)
    assert np.array_equal(c, rc) and np.array_equal(p, rp) and np.array_equal(k, rk)


CUTS = [
    (dict(mu_min=0.5), 0.553, []),
    (dict(mu_min=0.3, mu_max=0.9), 0.697, []),
    (dict(wedge_slope=0.5), 0.612, []),
    (dict(wedge_slope=1.0, wedge_buffer=0.1), 0.206, [0]),
]


@pytest.mark.parametrize("cut, fraction, empty", CUTS, ids=[",".join(c[0]) for c in CUTS])
def test_reference_cuts_keep_the_expected_modes(cut, fraction, empty):
    shape, L = (33, 35, 37), (70.0, 75.0, 80.0)
    f = (np.random.default_rng(5).standard_normal(shape) + 1).astype(np.float32)
    keep = SR.cut_mask(shape, L, **cut)
    assert abs(keep.mean() - fraction) <= 0.002, keep.mean()
    p, k, c, v = SR.get_power(f, L, **cut)
    assert len(c) == 15
    assert list(np.flatnonzero(c == 0)) == empty
    assert np.array_equal(np.isnan(p), c == 0) and np.array_equal(np.isnan(v), c == 0)
    full = SR.get_power(f, L)[2]
    assert np.all(c <= full) and c.sum() < full.sum()


def test_reference_window_conventions():
    shape, L = (8, 9, 10), 30.0
    f = (np.random.default_rng(2).standard_normal(shape) + 1).astype(np.float32)
    # all-ones weights: the field less its mean, nothing put back onto k = 0
    P1 = SR.windowed_spectrum(f, L, window=np.ones(10))
    P0 = PR.spectrum(f, L)
    assert abs(P1[0, 0, 0]) < 1e-20 * P0.max()
    np.testing.assert_allclose(P1.ravel()[1:], P0.ravel()[1:], rtol=1e-9, atol=1e-12 * P0.max())
    # a constant weight c cancels against <W^2>
    np.testing.assert_allclose(SR.windowed_spectrum(f, L, window=(None, np.full(9, 3.0), None)), P1, rtol=1e-12,
                               atol=1e-12 * P0.max())


def test_reference_moments_and_histogram():
    f = (np.random.default_rng(4).standard_normal((7, 8, 9)) + 1).astype(np.float32)
    (mean, m2, m3, m4), scale = SR.moments(f)
    v = f.astype(np.float64)
    assert mean == pytest.approx(v.mean(), rel=1e-14) and m2 == pytest.approx(v.var(), rel=1e-13)
    assert all(s > 0 for s in scale)
    edges = np.array([-1.0, 0.0, 0.5, 3.0])
    f[0, 0, 0], f[0, 0, 1], f[0, 0, 2] = -1.0, 0.5, 3.0  # on the first, an inner and the last edge
    h = SR.histogram(f, edges)
    ref = np.histogram(f.astype(np.float64)[f < 3.0], edges)[0]
    assert np.array_equal(h, ref)


# ---- argument errors: none of these reaches the library -----------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    api = importlib.import_module("21cmfast_amd.grid_api")

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(api, "load", boom)


F = np.ones((6, 7, 8), np.float32)

BAD_POWER = [
    dict(window="tukey"), dict(window=np.ones(7)), dict(window=np.ones((2, 8))), dict(window=np.zeros(8)),
    dict(window=np.array([1.0] * 7 + [np.nan])), dict(window=("hann", "hann")),
    dict(window=(np.ones(7), None, None)), dict(window=(None, np.full(7, np.inf), None)),
    dict(mu_min=-0.1), dict(mu_max=1.5), dict(mu_min=0.8, mu_max=0.2), dict(mu_min=np.nan), dict(mu_max="x"),
    dict(wedge_slope=-1.0), dict(wedge_slope=np.inf), dict(wedge_slope=1.0, wedge_buffer=-0.1),
    dict(wedge_buffer=0.2), dict(wedge_slope=[1.0, 2.0]),
]


@pytest.mark.parametrize("kw", BAD_POWER, ids=lambda kw: ",".join(f"{k}" for k in kw))
def test_get_power_rejects_bad_options(no_library, kw):
    with pytest.raises(ValueError):
        PS.get_power(F, 10.0, **kw)
    with pytest.raises(ValueError):
        PS.lightcone_power_spectra(np.ones((6, 7, 20), np.float32), 1.0, chunk_length=8, **kw)


@pytest.mark.parametrize("kw", [dict(mu_min=0.5), dict(mu_max=0.5), dict(wedge_slope=1.0), dict(wedge_buffer=0.1)],
                         ids=lambda kw: ",".join(kw))
def test_cylindrical_spectra_reject_cuts(no_library, kw):
    with pytest.raises(ValueError, match="spherical"):
        PS.get_cylindrical_power(F, 10.0, **kw)
    with pytest.raises(ValueError, match="spherical"):
        PS.lightcone_power_spectra(np.ones((6, 7, 20), np.float32), 1.0, chunk_length=8, cylindrical=True, **kw)


def test_cylindrical_spectra_reject_bad_windows(no_library):
    with pytest.raises(ValueError):
        PS.get_cylindrical_power(F, 10.0, window=np.zeros(8))
    with pytest.raises(ValueError):
        PS.get_cylindrical_power(F, 10.0, window="nuttall")
    with pytest.raises(TypeError):
        PS.get_cylindrical_power(F, 10.0, no_such_keyword=1)


def test_moments_and_pdf_reject_bad_arguments(no_library):
    with pytest.raises(ValueError):
        PS.get_moments(np.ones((4, 4), np.float32))
    with pytest.raises(ValueError):
        PS.get_pdf(np.ones((4, 4), np.float32), 8)
    for bins in (0, 2.5, True, [1.0], [0.0, 0.0, 1.0], [0.0, np.nan], np.ones((2, 2))):
        with pytest.raises(ValueError):
            PS.get_pdf(F, bins)
    for rng in ((1.0,), (2.0, 1.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            PS.get_pdf(F, 8, range=rng)
    lc = np.ones((6, 7, 20), np.float32)
    with pytest.raises(ValueError):
        PS.lightcone_moments(lc, chunk_length=30)
    with pytest.raises(ValueError):
        PS.lightcone_moments(lc, chunk_length=8, chunk_starts=[15])
    with pytest.raises(ValueError):
        PS.lightcone_moments(lc, chunk_length=8, redshifts=np.ones(3))
    with pytest.raises(ValueError):
        PS.lightcone_moments(lc, chunk_length=8, bins=0)


def test_power_opts_mirror_matches_the_header(pkg, tmp_path):
    """structs.PowerOpts against the compiler's layout of c21cm_power_opts."""
    import ctypes as C
    import subprocess
    from pathlib import Path

    S = pkg.structs
    root = Path(__file__).resolve().parent.parent
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "c21cm_grid.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(c21cm_power_opts));']
    for field, _ in S.PowerOpts._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(c21cm_power_opts, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        name, value = line.split()
        if name == "size":
            assert C.sizeof(S.PowerOpts) == int(value)
        else:
            assert getattr(S.PowerOpts, name).offset == int(value), name
