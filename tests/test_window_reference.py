"""Pins tests/window_reference.py (numpy, float64) against the CPU oracle's restatement of filtering.c.

The GPU tests of pass X (test_gpu_pass_x_windows.py) compare spectra with window_reference alone; this is
the one place where that module meets the oracle.  Runs without a GPU."""

import numpy as np
import pytest

import window_reference as WR

# (shape, box_len, box_len_z): a cube, and a box whose z cells are NOT the x cells (box_len_z differs from
# box_len nz / nx) and whose y cells share x's box length -- a dk taken from the wrong axis shows
BOXES = [((32, 32, 32), 48.0, 48.0), ((24, 24, 40), 36.0, 0.8 * 36.0 * 40 / 24)]
# every type oracle.filter_grid accepts: (type, R, R_param)
WINDOWS = [(0, 3.0, 0.0), (0, 11.0, 0.0), (1, 2.0, 0.0), (2, 4.0, 0.0), (3, 7.5, 37.66), (3, 9.0, 2.5),
           (4, 5.0, 9.0)]


@pytest.fixture(scope="module")
def boxes():
    out = {}
    for shape, box_len, box_len_z in BOXES:
        a = (np.random.default_rng(11).standard_normal(shape) + 0.5).astype(np.float32)
        out[shape] = (a, np.fft.rfftn(a.astype(np.float64)), WR.k_magnitude(shape, box_len, box_len_z))
    return out


@pytest.mark.parametrize("filter_type,R,R_param", WINDOWS)
@pytest.mark.parametrize("shape,box_len,box_len_z", BOXES)
def test_filtered_spectrum_matches_oracle_filter_grid(oracle, boxes, shape, box_len, box_len_z, filter_type, R,
                                                      R_param):
    a, spectrum, k = boxes[shape]
    got = np.fft.irfftn(WR.filtered_spectrum(a, box_len, box_len_z, filter_type, R, R_param, spectrum=spectrum,
                                             k=k), s=shape, axes=(0, 1, 2))
    ref = oracle.filter_grid(a, box_len, filter_type, R, R_param, box_len_z=box_len_z)
    # the tolerance of the suite's oracle comparisons of filtered boxes (float32 transforms in the oracle)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5 * np.abs(ref).max() + 1e-7)
    assert np.abs(ref).max() > 1e-3  # something was compared


def test_sharp_k_box_removes_modes(boxes):
    """The sharp-k radius of the comparison above cuts inside the grid (else it would pin nothing)."""
    for shape, box_len, box_len_z in BOXES:
        w = WR.window(1, boxes[shape][2], 2.0)
        assert 0.05 < w.mean() < 0.95


@pytest.mark.parametrize("filter_type,R,R_param", WINDOWS)
def test_window_values_match_oracle(oracle, filter_type, R, R_param):
    """Mode by mode: both sides evaluate the same double expressions at the same float-held arguments, so they
    differ by the last bits of pow / sin / cos only.  1e-12 of the window's scale is ~1e4 ulp of room and still
    nine orders below any float32 effect."""
    k = np.concatenate([[0.0, 1e-6, 1e-5 / R, 0.99e-4 / R, 1.01e-4 / R], np.geomspace(1e-3, 40.0, 300)])
    got = WR.window(filter_type, np.sqrt((k * k).astype(np.float32).astype(np.float64)), R, R_param)
    ref = np.array([oracle.window(filter_type, float(x), R, R_param) for x in k])
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("R_in,R_out,R_star", [(2.0, 3.5, 1.7), (8.0, 11.0, 0.6), (20.0, 26.0, 55.0),
                                                (3.0, 4.0, 0.0)])
def test_multiple_scattering_window_matches_oracle(oracle, R_in, R_out, R_star):
    """Type 5 is not served by oracle.filter_grid; its window is pinned value by value.  The series below
    kR = 30 stops at a relative 1e-4, so the two sides agree to rounding only where they stop at the same term:
    they run the same recurrence in the same order, and do."""
    k = np.concatenate([[1e-5], np.geomspace(1e-3, 60.0, 400)])
    kk = np.sqrt((k * k).astype(np.float32).astype(np.float64))
    got = WR.window(5, kk, R_in, R_out, R_star)
    ref = np.array([oracle.filter_window_ms(float(x), R_in, R_out, R_star) for x in k])
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-11 * max(1.0, np.abs(ref).max()))


def test_k_magnitude_axes():
    """k_y takes x's box length, k_z its own; x and y wrap, z does not."""
    k = WR.k_magnitude((8, 6, 10), 16.0, 5.0)
    assert k.shape == (8, 6, 6)
    f = lambda v: float(np.float32(v))  # noqa: E731
    assert k[1, 0, 0] == pytest.approx(f(2 * np.pi / 16.0), rel=1e-7)
    assert k[0, 1, 0] == pytest.approx(f(2 * np.pi / 16.0), rel=1e-7)
    assert k[0, 0, 1] == pytest.approx(f(2 * np.pi / 5.0), rel=1e-7)
    assert k[7, 0, 0] == k[1, 0, 0] and k[0, 5, 0] == k[0, 1, 0]
    assert k[4, 3, 5] == pytest.approx(np.sqrt((np.pi / 2) ** 2 + (3 * np.pi / 8) ** 2 + (2 * np.pi) ** 2),
                                     rel=1e-6)
