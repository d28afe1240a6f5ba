"""Power spectra on the host: the restatement (tests/power_reference.py) against the powerbox oracle, the
edge builder of 21cmfast_amd.powerspec against numpy, and the argument errors (raised before any device
work)."""

import importlib

import numpy as np
import pytest

import power_reference as PR
from oracle import powerbox_power as PB

PS = importlib.import_module("21cmfast_amd.powerspec")

SHAPES = [(16, 16, 16), (15, 15, 15), (12, 10, 21), (9, 11, 13)]


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_defaults_equal_the_powerbox_oracle(shape):
    rng = np.random.default_rng(7)
    f = rng.standard_normal(shape).astype(np.float32)
    for L in (100.0, (50.0, 70.0, 90.0)):
        p, k = PR.get_power(f, L)
        po, ko = PB.get_power(f, L)
        np.testing.assert_allclose(k, ko, rtol=1e-12, atol=0)
        np.testing.assert_allclose(p, po, rtol=1e-12, atol=0)
        assert np.array_equal(np.isnan(p), np.isnan(po))


def _kmag(shape, L):
    freq = [np.fft.fftfreq(n, d=l / n) * 2.0 * np.pi for n, l in zip(shape, L)]
    g = np.meshgrid(*freq, indexing="ij")
    return np.sqrt(sum(x * x for x in g)), g


@pytest.mark.parametrize("shape", SHAPES + [(64, 64, 64), (33, 35, 37), (32, 32, 100)])
def test_edge_builder_equals_numpy_bit_for_bit(shape):
    L = (100.0, 77.7, 123.4)
    kmag, (kx, ky, kz) = _kmag(shape, L)
    n = int(np.prod(shape) ** (1.0 / 3) / 2.2)
    upto = min(float(np.min(np.max(kmag, axis=i))) for i in range(3))
    assert np.array_equal(PS.spherical_edges(shape, L), np.linspace(kmag.min(), upto, n + 1))
    assert np.array_equal(PS.spherical_edges(shape, L, bins_upto_boxlen=False),
                          np.linspace(kmag.min(), kmag.max(), n + 1))
    assert np.array_equal(PS.spherical_edges(shape, L, bins=7, log_bins=True),
                          np.geomspace(kmag[kmag > 0].min(), upto, 8))
    # the same edges as the restatement's
    _, e = PR.get_power(np.zeros(shape), L, bins=5, log_bins=True, bin_ave=False)
    assert np.array_equal(PS.spherical_edges(shape, L, bins=5, log_bins=True), e)
    kperp = np.sqrt(kx * kx + ky * ky)[:, :, 0]
    ep, ez = PS.cylindrical_edges(shape, L, log_bins=False)
    assert np.array_equal(ep, np.linspace(0.0, min(float(np.min(np.max(kperp, axis=i))) for i in range(2)),
                                          int(np.sqrt(shape[0] * shape[1]) / 2.2) + 1))
    assert np.array_equal(ez, np.linspace(0.0, np.abs(kz).max(), int(shape[2] / 2.2) + 1))
    ep, ez = PS.cylindrical_edges(shape, L, kperp_bins=4, kpar_bins=3, log_bins=True)
    assert ep[0] == kperp[kperp > 0].min() and ez[0] == np.abs(kz[kz != 0]).min()
    assert np.array_equal(ez, np.geomspace(np.abs(kz[kz != 0]).min(), np.abs(kz).max(), 4))


def test_reference_options_are_self_consistent():
    rng = np.random.default_rng(3)
    f = rng.standard_normal((12, 14, 16))
    p, k, c = PR.get_power(f, 60.0, return_counts=True)
    p0, _, c0 = PR.get_power(f, 60.0, ignore_zero_mode=True, return_counts=True)
    assert c0[0] == c[0] - 1 and np.array_equal(c0[1:], c[1:])
    _, _, ckz = PR.get_power(f, 60.0, ignore_kpar_zero=True, return_counts=True)
    assert ckz.sum() < c.sum()
    pc, _ = PR.get_power(f, 60.0, deltax2=f)
    np.testing.assert_allclose(pc, p, rtol=1e-12)
    P, kp, kz, cc = PR.get_cylindrical_power(f, 60.0, return_counts=True)
    assert P.shape == cc.shape == (len(kp), len(kz))


def test_a_given_spectrum_is_binned_as_the_field_is():
    """``spectrum=`` (one transform, several binnings: the large-shape GPU tests) changes no number, and the
    wavenumber grids kept from the last call follow a change of shape or lengths."""
    rng = np.random.default_rng(8)
    f, g = rng.standard_normal((12, 14, 17)), rng.standard_normal((12, 14, 17))
    for L in ((60.0, 50.0, 70.0), 55.0):
        for d2 in (None, g):
            P = PR.spectrum(f, L, d2)
            for opts in (dict(), dict(log_bins=True, ignore_kperp_zero=True), dict(bins=5, bin_ave=False)):
                a = PR.get_power(f, L, deltax2=d2, return_counts=True, **opts)
                b = PR.get_power(f, L, spectrum=P, return_counts=True, **opts)
                assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
            a = PR.get_cylindrical_power(f, L, deltax2=d2, return_counts=True)
            b = PR.get_cylindrical_power(f, L, spectrum=P, return_counts=True)
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    small = PR.get_power(f[:8, :8, :8], 55.0)
    assert len(small[0]) != len(PR.get_power(f, 55.0)[0])


def test_argument_errors():
    f = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(ValueError, match="3-D"):
        PS.get_power(np.zeros((8, 8)), 10.0)
    with pytest.raises(ValueError, match=">= 1"):
        PS.get_power(f, 10.0, bins=0)
    with pytest.raises(ValueError, match="increasing"):
        PS.get_power(f, 10.0, bins=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="increasing"):
        PS.get_cylindrical_power(f, 10.0, kpar_bins=[2.0, 1.0])
    with pytest.raises(ValueError, match="positive"):
        PS.get_power(f, 0.0)
    with pytest.raises(ValueError, match="positive"):
        PS.get_power(f, (10.0, -1.0, 10.0))
    with pytest.raises(ValueError, match="3 lengths"):
        PS.get_power(f, (10.0, 10.0))
    with pytest.raises(ValueError, match="deltax2"):
        PS.get_power(f, 10.0, deltax2=np.zeros((8, 8, 9), np.float32))
    lc = np.zeros((8, 8, 20), np.float32)
    with pytest.raises(ValueError, match="longer than the lightcone"):
        PS.lightcone_power_spectra(lc, 1.0, chunk_length=21)
    with pytest.raises(ValueError, match="inside the lightcone"):
        PS.lightcone_power_spectra(lc, 1.0, chunk_starts=[0, 15])
    with pytest.raises(ValueError, match="deltax2"):
        PS.lightcone_power_spectra(lc, 1.0, deltax2=np.zeros((8, 8, 21), np.float32))
    with pytest.raises(ValueError, match="unknown binning"):
        PS.lightcone_power_spectra(lc, 1.0, kperp_bins=3)
