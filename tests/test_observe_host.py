"""CPU, no library: pins ``tests/observe_reference.py``, the numpy spec of ``c21cm_observe_smooth_grids`` (DESIGN
section 4.11), against ``scipy.ndimage.gaussian_filter(mode="wrap", truncate=4.0)`` and a plain loop for the channel;
and the host helpers and argument checks of ``21cmfast_amd.observe``, which come before the library is loaded."""

import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
import observe_reference as R  # noqa: E402

OB = importlib.import_module("21cmfast_amd.observe")
LIB = importlib.import_module("21cmfast_amd._lib")
DRV = importlib.import_module("21cmfast_amd.drivers")

SHAPES = [(7, 5, 9), (16, 12, 6), (3, 2, 4)]


def field_of(shape, seed=5):
    return np.random.default_rng(seed).normal(-10.0, 20.0, shape).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_beam_against_scipy(shape):
    """lw reaches 12 on axes of 2 and 3 cells: the index wraps several times.  Limit 1e-13 on values up to 80; scipy
    1.15.3 differs by 1.8e-14, 4e-16 of the largest value"""
    f = field_of(shape)
    sigma = np.linspace(0.3, 3.1, shape[2])
    assert R.half_width(sigma[-1]) == 12
    got = R.beam(f, sigma, round_weights=False)
    for s in range(shape[2]):
        want = ndimage.gaussian_filter(f[:, :, s].astype(np.float64), sigma[s], mode="wrap", truncate=4.0)
        assert np.max(np.abs(got[:, :, s] - want)) <= 1e-13


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_channel_against_a_plain_loop(shape, periodic):
    h = field_of(shape).astype(np.float64)
    ns = shape[2]
    s = np.arange(ns)
    below, above = s % 4, s % 5
    if periodic:
        below, above = np.minimum(below, (ns - 1) // 2), np.minimum(above, ns // 2)
    got = R.channel(h, below, above, periodic)
    for i in range(shape[0]):
        for j in range(shape[1]):
            for k in range(ns):
                if periodic:
                    picks = [h[i, j, q % ns] for q in range(k - below[k], k + above[k] + 1)]
                else:
                    picks = [h[i, j, q] for q in range(k - below[k], k + above[k] + 1) if 0 <= q < ns]
                assert abs(got[i, j, k] - sum(picks) / len(picks)) <= 1e-13
    assert np.array_equal(R.channel(h, 0 * s, 0 * s, periodic), h)


def test_the_whole_chain_and_its_rounding_steps():
    f = field_of((7, 5, 9))
    sigma = np.linspace(0.3, 3.1, 9)
    zero = np.zeros(9, np.int64)
    out, m, g = R.observe_smooth(f, sigma, zero, zero, subtract_mean=True, round_weights=False)
    assert g.dtype == np.float32
    assert np.allclose(m, f.astype(np.float64).mean((0, 1)), rtol=1e-14, atol=0)
    assert np.array_equal(g, (f.astype(np.float64) - m).astype(np.float32))
    for s in range(9):
        want = ndimage.gaussian_filter(g[:, :, s].astype(np.float64), sigma[s], mode="wrap", truncate=4.0)
        assert np.max(np.abs(out[:, :, s] - want)) <= 1e-13
    flat = np.broadcast_to(np.linspace(-3, 3, 9, dtype=np.float32), (7, 5, 9))
    out, m, g = R.observe_smooth(flat, 2.0, 1, 1)
    assert np.all(g == 0) and np.all(out == 0) and np.array_equal(m, flat[0, 0].astype(np.float64))


def test_weights():
    for sigma in (0.125, 0.3, 1.0, 3.1, 17.0, 128.0):
        w = R.half_kernel(sigma, round_weights=False)
        assert len(w) == int(4 * sigma + 0.5) + 1
        assert abs(w[0] + 2.0 * w[1:].sum() - 1.0) <= 1e-15
        w32 = R.half_kernel(sigma)
        assert np.array_equal(w32, w.astype(np.float32).astype(np.float64))
    assert R.half_width(0.1249) == 0 and R.half_width(0.125) == 1 and R.half_width(128.0) == 512
    assert np.array_equal(R.half_kernel(0.12), [1.0])
    f = field_of((4, 3, 2))
    assert np.array_equal(R.beam(f, np.array([0.1, 0.0])), f.astype(np.float64))


def test_reference_argument_errors():
    f = field_of((3, 2, 4))
    zero = np.zeros(4, np.int64)
    for sigma in (-1.0, np.nan, np.inf, 128.5):
        with pytest.raises(ValueError):
            R.observe_smooth(f, sigma, zero, zero)
    with pytest.raises(ValueError):
        R.observe_smooth(f, 1.0, zero - 1, zero)
    with pytest.raises(ValueError):
        R.observe_smooth(f, 1.0, zero + 2, zero + 2, periodic_los=True)
    R.observe_smooth(f, 1.0, zero + 2, zero + 1, periodic_los=True)
    R.observe_smooth(f, 1.0, zero + 9, zero + 9, periodic_los=False)


def test_resolution_helpers():
    assert abs(OB.angular_resolution(9.0, 2.0) - 1.0553e-3) < 5e-8
    assert OB.angular_resolution(9.0) == OB.angular_resolution(9.0, 2.0)
    z = np.array([6.0, 9.0, 12.0])
    cp = DRV.Inputs().cosmo_params
    cosmo = DRV.FlatCosmology(cp.hlittle, cp.OMm)
    want = OB.angular_resolution(z) * cosmo.comoving_distance(z)
    assert np.allclose(OB.beam_fwhm(z), want, rtol=1e-14, atol=0)
    assert np.allclose(OB.beam_fwhm(z, cosmo=cosmo), want, rtol=1e-14, atol=0)
    assert np.allclose(OB.beam_fwhm(z, 0.5), 4.0 * want, rtol=1e-14, atol=0)
    other = DRV.FlatCosmology(0.7, 0.3)
    assert not np.allclose(OB.beam_fwhm(z, cosmo=other), want, rtol=1e-3, atol=0)
    sig = OB.beam_sigma_cells(z, 1.5)
    assert np.allclose(sig, want / (2.0 * np.sqrt(2.0 * np.log(2.0))) / 1.5, rtol=1e-14, atol=0)
    assert np.all(np.diff(want) > 0)  # the beam grows with redshift
    assert 1.5 < sig[0] < sig[-1] < 4.5  # 2 km, 1.5 Mpc cells, z = 6 to 12: beams of 15 to 33 taps


def test_los_windows():
    cell, ns = 1.5, 40
    d = 9000.0 + cell * np.arange(ns)
    s = np.arange(ns)
    for width in (0.0, 1.4, 3.0, 3.1, 7.4, 7.5, 9.0, 200.0):
        k = int(np.floor(width / (2.0 * cell) + 1e-9))
        below, above = OB.los_windows(d, width)
        assert below.dtype == np.int32 and above.dtype == np.int32
        assert np.array_equal(below, np.minimum(k, s)) and np.array_equal(above, np.minimum(k, ns - 1 - s))
        below_r, above_r = OB.los_windows(d[::-1].copy(), width)  # descending distances: the same counts, mirrored
        assert np.array_equal(below_r, np.minimum(k, s)) and np.array_equal(above_r, np.minimum(k, ns - 1 - s))
    width = np.where(s < 20, 3.0, 6.0)
    below, above = OB.los_windows(d, width)
    assert np.array_equal(below[5:20], np.full(15, 1)) and np.array_equal(above[20:35], np.full(15, 2))
    z = np.linspace(6.0, 12.0, 30)
    cosmo = DRV.FlatCosmology(0.7, 0.3)
    a = OB.los_windows(z, 50.0, redshifts=True, cosmo=cosmo)
    b = OB.los_windows(cosmo.comoving_distance(z), 50.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_los_windows_mhz():
    z = np.linspace(6.0, 12.0, 400)
    below, above = OB.los_windows_mhz(z, 1.0)
    nu = 1420.40575177 / (1.0 + z)
    for s in (0, 7, 200, 399):
        inside = np.abs(nu - nu[s]) <= 0.5 * (1 + 1e-12)
        assert below[s] == inside[:s].sum() and above[s] == inside[s + 1:].sum()
    total = below + above
    assert total[350] > total[50] > 0  # a MHz spans more slices at the high-z end
    zero = OB.los_windows_mhz(z, 0.0)
    assert not zero[0].any() and not zero[1].any()


def test_argument_errors_come_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(LIB, "load", no_library)
    monkeypatch.setattr(importlib.import_module("21cmfast_amd.grid_api"), "load", no_library)
    lc = np.zeros((4, 4, 12), np.float32)
    z = np.linspace(7.0, 8.0, 12)
    bad_lightcone = (
        dict(lightcone=np.zeros((4, 4), np.float32)),
        dict(cell_size=0.0), dict(cell_size=np.nan), dict(cell_size=-1.5),
        dict(redshifts=z[:11]), dict(redshifts=np.full(12, np.nan)), dict(redshifts=-z),
        dict(redshifts=np.full(12, 7.0), channel_width_mhz=0.5),  # not monotonic
        dict(max_baseline_km=0.0), dict(max_baseline_km=np.inf), dict(max_baseline_km=True),
        dict(los_ratio=-1.0), dict(los_ratio=np.nan),
        dict(fwhm=-1.0), dict(fwhm=np.nan), dict(fwhm=np.ones(11)), dict(fwhm=np.ones((12, 1))),
        dict(fwhm=1000.0),  # sigma above 128 cells
        dict(los_width=-2.0), dict(los_width=np.ones(5)), dict(los_width=np.inf),
        dict(channel_width_mhz=-0.1), dict(channel_width_mhz=np.ones(13)),
        dict(channel_width_mhz=0.2, los_width=3.0),
    )
    for kw in bad_lightcone:
        args = dict(lightcone=lc, cell_size=1.5, redshifts=z)
        args.update(kw)
        with pytest.raises(ValueError):
            OB.smooth_lightcone(**args)
    box = np.zeros((4, 4, 6), np.float32)
    bad_coeval = (
        dict(box=np.zeros((4, 4), np.float32)),
        dict(boxlength=(6.0, 7.0, 9.0)),  # not square across the line of sight
        dict(boxlength=0.0), dict(boxlength=(6.0, 6.0)),
        dict(redshift=-1.0), dict(redshift=[7.0, 8.0]), dict(redshift=np.nan),
        dict(max_baseline_km=-2.0), dict(los_ratio=-0.5),
        dict(fwhm=[1.0, 2.0]), dict(fwhm=-1.0), dict(fwhm=1000.0),
        dict(los_width=-1.0), dict(los_width=[1.0, 1.0]),
        dict(los_width=12.0),  # 4 slices on either side of a 6-slice box
    )
    for kw in bad_coeval:
        args = dict(box=box, boxlength=(6.0, 6.0, 9.0), redshift=8.0)
        args.update(kw)
        with pytest.raises(ValueError):
            OB.smooth_coeval(**args)
    for call in (lambda: OB.angular_resolution(-1.0), lambda: OB.angular_resolution([[7.0]]),
                 lambda: OB.angular_resolution(7.0, 0.0), lambda: OB.beam_sigma_cells(7.0, 0.0),
                 lambda: OB.los_windows([1.0, 1.0, 2.0], 1.0), lambda: OB.los_windows([1.0, 3.0, 2.0], 1.0),
                 lambda: OB.los_windows([1.0, np.nan], 1.0), lambda: OB.los_windows([1.0, 2.0], -1.0),
                 lambda: OB.los_windows([1.0, 2.0], [1.0, 2.0, 3.0]), lambda: OB.los_windows_mhz([7.0, 7.0], 1.0)):
        with pytest.raises(ValueError):
            call()
    # a well-formed call gets as far as the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        OB.smooth_lightcone(lc, 1.5, z)
    with pytest.raises(AssertionError, match="the library was loaded"):
        OB.smooth_coeval(box, (6.0, 6.0, 9.0), 8.0)
