"""GPU: ``observe.smooth_lightcone`` / ``observe.smooth_coeval`` / ``grid_api.observe_smooth``
against the numpy spec ``tests/observe_reference.py``, which ``test_observe_host.py`` pins on the CPU.

The tolerance is derived, not measured.  Every pass is a sum of products with weights that sum to 1, so
|out - spec| <= (2 T + n_los + 8) 2^-24 M with T the largest number of taps of the call, n_los its longest channel and
M = max(max|f|, max|g|): T roundings of the pair sums and T of the accumulations per transverse pass (each weighted,
the weights summing to 1, so a pass adds T 2^-24 M at the most), n_los additions along the line of sight, and 8 for the
weights' rounding to fp32, the two "+ 1" of the sums, the division and the mean subtraction.  A misplaced tap gives
errors of order M.  Every cell of every case is compared.

The shapes are the ones at which the kernels can go wrong (a line of sight that ends inside a wave, at its end and one
slice past it; axes shorter than the beam, which then wraps several times; a transverse axis three cells longer than a
workgroup holds at a time; beams on either side of the width at which the beam kernel changes), not the ones where the
science lives.
"""

import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import observe_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

OB = importlib.import_module("21cmfast_amd.observe")
PS = importlib.import_module("21cmfast_amd.powerspec")
API = importlib.import_module("21cmfast_amd.grid_api")
LIB = importlib.import_module("21cmfast_amd._lib")

VALUE_ERROR, NAN_ERROR = 3, 7
EPS = 2.0**-24
SHAPES = [(7, 5, 9), (3, 2, 9), (1, 1, 5), (16, 12, 63), (16, 12, 64), (16, 12, 65), (9, 7, 130), (40, 33, 70),
          "long_x", "long_y"]
SIGMAS = ["rising", "falling", "alternating"]
WINDOWS = ["none", "mod", "whole", "periodic_wrap", "periodic_full"]
SIGMA_MAX = 3.1


def shape_of(shape):
    """the named shapes have one transverse axis three cells longer than a workgroup holds at a time at SIGMA_MAX"""
    if not isinstance(shape, str):
        return shape
    tile = API.observe_geometry()[0] - 2 * R.half_width(SIGMA_MAX)
    return (tile + 3, 2, 3) if shape == "long_x" else (2, tile + 3, 3)


@functools.lru_cache(maxsize=None)
def field_of(shape, seed=5, mean=-10.0, std=20.0):
    f = np.random.default_rng(seed).normal(mean, std, shape).astype(np.float32)
    f.setflags(write=False)
    return f


def sigma_of(mode, ns):
    if mode == "alternating":
        return np.where(np.arange(ns) % 2 == 0, 0.0, SIGMA_MAX)
    rising = np.linspace(0.3, SIGMA_MAX, ns)
    return rising if mode == "rising" else rising[::-1].copy()


def windows_of(mode, ns):
    """(below, above, periodic_los)"""
    s = np.arange(ns)
    if mode == "none":
        return 0 * s, 0 * s, False
    if mode == "mod":
        return s % 4, s % 5, False  # clipped at both ends
    if mode == "whole":
        return 0 * s + ns - 1, 0 * s + ns - 1, False  # the whole line from every slice
    if mode == "periodic_wrap":
        return np.minimum(s % 4, (ns - 1) // 2), np.minimum(s % 5, ns // 2), True
    return 0 * s + (ns - 1) // 2, 0 * s + ns // 2, True  # below + above + 1 = ns


@functools.lru_cache(maxsize=None)
def beam_spec(shape, sigma_mode, subtract_mean):
    """(step 2 in fp64, m, max(max|f|, max|g|)), shared by the windows"""
    f = field_of(shape)
    g, m = R.centre(f, subtract_mean)
    h = R.beam(g, sigma_of(sigma_mode, shape[2]))
    h.setflags(write=False)
    return h, m, float(max(np.max(np.abs(f)), np.max(np.abs(g))))


def bound(sigma, below, above, ns, periodic, M):
    taps = 2 * max(R.half_width(x) for x in sigma) + 1
    lo, hi = np.arange(ns) - below, np.arange(ns) + above
    if not periodic:
        lo, hi = np.maximum(lo, 0), np.minimum(hi, ns - 1)
    return (2 * taps + int(np.max(hi - lo + 1)) + 8) * EPS * M


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("sigma_mode", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_against_the_spec(shape, sigma_mode):
    shape = shape_of(shape)
    ns = shape[2]
    f = field_of(shape)
    sigma = sigma_of(sigma_mode, ns)
    for subtract_mean in (True, False):
        h, m, M = beam_spec(shape, sigma_mode, subtract_mean)
        for window in WINDOWS:
            below, above, periodic = windows_of(window, ns)
            want = R.channel(h, below, above, periodic)
            out, means = API.observe_smooth(f, sigma, below, above, periodic_los=periodic,
                                            subtract_mean=subtract_mean)
            assert out.dtype == np.float32 and out.shape == shape and means.dtype == np.float64
            limit = bound(sigma, below, above, ns, periodic, M)
            err = float(np.max(np.abs(out.astype(np.float64) - want)))
            print(f"{shape} {sigma_mode} {window} mean={subtract_mean}: err {err:.3e} bound {limit:.3e}")
            assert err <= limit, (window, subtract_mean)
            assert np.allclose(means, m, rtol=1e-12, atol=0)


@pytest.mark.parametrize("sigma_max,shape", [(16.0, (123, 2, 3)), (16.2, (123, 2, 3)), (16.0, (2, 5, 66)),
                                             (16.2, (2, 5, 66)), (128.0, (3, 2, 2))])
def test_either_side_of_the_kernel_switch(sigma_max, shape):
    """lw = 64 is the widest beam of the LDS kernel (123 cells: three more than its tile then holds), lw = 65 the
    narrowest of the direct one; lw = 512 on axes of 3 and 2 is the widest beam there is"""
    lds_lw = API.observe_geometry()[1]
    assert R.half_width(16.0) == lds_lw and R.half_width(16.2) == lds_lw + 1 and R.half_width(128.0) == 512
    ns = shape[2]
    f = field_of(shape)
    sigma = np.linspace(1.0, sigma_max, ns)
    zero = np.zeros(ns, np.int64)
    want, m, g = R.observe_smooth(f, sigma, zero, zero)
    out, means = API.observe_smooth(f, sigma)
    M = float(max(np.max(np.abs(f)), np.max(np.abs(g))))
    assert np.max(np.abs(out.astype(np.float64) - want)) <= bound(sigma, zero, zero, ns, False, M)


def test_a_slice_is_the_same_through_either_kernel():
    """slices 0 and 1 of two calls that differ in slice 2 alone, whose lw = 65 sends the second call through the direct
    kernel: the same bytes"""
    f = field_of((40, 33, 3))
    a, _ = API.observe_smooth(f, np.array([0.9, 3.1, 16.0]))
    b, _ = API.observe_smooth(f, np.array([0.9, 3.1, 16.2]))
    assert same_bits(a[:, :, :2].copy(), b[:, :, :2].copy())
    assert not same_bits(a[:, :, 2].copy(), b[:, :, 2].copy())


def test_nothing_to_do_copies_the_field():
    f = field_of((16, 12, 65)).copy()
    f[3, 4, 6], f[0, 0, 0] = -0.0, np.float32(1e-42)  # a negative zero and a denormal keep their bits too
    for sigma in (0.0, 0.1249, np.where(np.arange(65) % 2 == 0, 0.0, 0.12)):
        out, means = API.observe_smooth(f, sigma, subtract_mean=False)
        assert same_bits(out, f)
        assert np.allclose(means, f.astype(np.float64).mean((0, 1)), rtol=1e-12, atol=0)
    # lw = 0 beside slices that are smoothed, and under a channel that holds the slice alone
    sigma = sigma_of("alternating", 65)
    out, _ = API.observe_smooth(f, sigma, np.zeros(65, np.int64), np.arange(65) % 2, subtract_mean=False)
    assert same_bits(out[:, :, ::2].copy(), f[:, :, ::2].copy())


def test_constant_slices_give_exactly_zero():
    shape = (16, 12, 65)
    levels = np.random.default_rng(5).normal(-10.0, 20.0, shape[2]).astype(np.float32)
    f = np.ascontiguousarray(np.broadcast_to(levels, shape))
    for sigma, (below, above, periodic) in ((sigma_of("rising", 65), windows_of("mod", 65)),
                                            (0.0, windows_of("none", 65)),
                                            (sigma_of("alternating", 65), windows_of("periodic_wrap", 65))):
        out, means = API.observe_smooth(f, sigma, below, above, periodic_los=periodic, subtract_mean=True)
        assert np.all(out == 0)
        assert np.array_equal(means, levels.astype(np.float64))


def test_two_calls_and_both_kinds_of_input_give_the_same_bytes():
    import torch

    shape = (40, 33, 70)
    f = field_of(shape)
    sigma = sigma_of("rising", 70)
    below, above, _ = windows_of("mod", 70)
    first = API.observe_smooth(f, sigma, below, above)
    again = API.observe_smooth(f, sigma, below, above)
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
    ft = torch.from_numpy(f.copy()).cuda()
    on_device = API.observe_smooth(ft, sigma, below, above)
    assert on_device[0].device == ft.device and on_device[1].device == ft.device
    assert on_device[0].dtype == torch.float32 and on_device[1].dtype == torch.float64
    assert same_bits(first[0], on_device[0]) and same_bits(first[1], on_device[1])
    assert same_bits(ft, f)  # the input is left as it was


@pytest.mark.parametrize("sigma_mode", ["alternating", "rising"])
def test_a_slice_does_not_depend_on_the_others(sigma_mode):
    shape = (16, 12, 65)
    f = field_of(shape)
    sigma = sigma_of(sigma_mode, 65)
    full, means = API.observe_smooth(f, sigma)
    for s in range(65):
        alone, mean = API.observe_smooth(np.ascontiguousarray(f[:, :, s:s + 1]), sigma[s:s + 1])
        assert same_bits(alone[:, :, 0].copy(), full[:, :, s].copy()), s
        assert mean[0] == means[s]


def test_slice_means():
    for shape in ((40, 33, 70), (300, 2, 3), (1, 1, 5)):  # 300 x 2 rows: more than one part of the reduction
        f = field_of(shape)
        for subtract_mean in (True, False):
            means = API.observe_smooth(f, 1.0, subtract_mean=subtract_mean)[1]
            assert np.allclose(means, f.astype(np.float64).mean((0, 1)), rtol=1e-12, atol=0)


def test_public_functions_call_the_entry_with_the_helpers_arrays():
    import torch

    lc = field_of((16, 16, 40))
    z = np.linspace(6.0, 6.4, 40)
    cell = 1.5
    res = OB.smooth_lightcone(lc, cell, z)
    sigma = OB.beam_sigma_cells(z, cell)
    below, above = OB.los_windows(cell * np.arange(40), OB.beam_fwhm(z))
    assert below.max() >= 1  # the matched channel is on
    want = API.observe_smooth(lc, sigma, below, above)
    assert same_bits(res.field, want[0]) and same_bits(res.slice_means, want[1])
    assert np.array_equal(res.sigma_cells, sigma) and np.array_equal(res.los_below, below)
    assert np.array_equal(res.los_above, above) and np.array_equal(res.fwhm, OB.beam_fwhm(z))
    assert np.allclose(res.angular_resolution, np.degrees(OB.angular_resolution(z)) * 60.0, rtol=1e-14, atol=0)
    mhz = OB.smooth_lightcone(lc, cell, z, channel_width_mhz=1.0, subtract_mean=False, fwhm=3.0)
    below, above = OB.los_windows_mhz(z, 1.0)
    assert below.max() >= 1
    want = API.observe_smooth(lc, 3.0 / OB.FWHM_PER_SIGMA / cell, below, above, subtract_mean=False)
    assert same_bits(mhz.field, want[0])
    off = OB.smooth_lightcone(lc, cell, z, los_width=0.0)
    assert same_bits(off.field, API.observe_smooth(lc, sigma)[0]) and not off.los_below.any()
    on_device = OB.smooth_lightcone(torch.from_numpy(lc.copy()).cuda(), cell, z)
    assert on_device.field.is_cuda and on_device.slice_means.is_cuda and same_bits(on_device.field, res.field)

    box = field_of((16, 16, 16))
    res = OB.smooth_coeval(box, 24.0, 7.0, los_ratio=0.5)
    fwhm = float(OB.beam_fwhm(7.0))
    half = int(np.floor(0.5 * fwhm / (2.0 * 1.5)))
    assert half >= 1
    counts = np.full(16, half, np.int32)
    want = API.observe_smooth(box, fwhm / OB.FWHM_PER_SIGMA / 1.5, counts, counts, periodic_los=True)
    assert same_bits(res.field, want[0]) and same_bits(res.slice_means, want[1])
    assert np.array_equal(res.los_below, counts) and np.array_equal(res.los_above, counts)


def test_power_is_cut_by_the_squared_transform_of_the_kernel():
    n, sigma = 32, 1.5
    f = field_of((n, n, 3), mean=0.0, std=1.0)
    out, _ = API.observe_smooth(f, sigma, subtract_mean=False)
    w = R.half_kernel(sigma)
    k = np.arange(n)
    line = w[0] + 2.0 * sum(w[d] * np.cos(2.0 * np.pi * k * d / n) for d in range(1, len(w)))  # DFT of the wrapped w
    transfer = (line[:, None] * line[None, :]) ** 2
    keep = transfer > 1e-3
    assert keep.sum() > 100
    for s in range(3):
        ratio = np.abs(np.fft.fft2(out[:, :, s].astype(np.float64))) ** 2 / np.abs(
            np.fft.fft2(f[:, :, s].astype(np.float64))) ** 2
        assert np.max(np.abs(ratio[keep] / transfer[keep] - 1.0)) <= 1e-4


def test_the_result_feeds_the_lightcone_statistics():
    lc = field_of((16, 16, 40))
    res = OB.smooth_lightcone(lc, 1.5, np.linspace(6.0, 6.4, 40))
    g = R.centre(lc, True)[0]
    M = float(max(np.max(np.abs(lc)), np.max(np.abs(g))))
    moments = PS.lightcone_moments(res.field)
    assert len(moments.mean) == 2
    assert np.max(np.abs(to_np(moments.mean))) < 10 * EPS * M
    assert np.all(to_np(moments.variance) > 0)


def test_error_paths():
    shape = (7, 5, 9)
    f = field_of(shape).copy()
    zero = np.zeros(9, np.int64)
    untouched = np.full(shape, 7.0, np.float32)

    def refused(code, field, sigma, below=zero, above=zero, periodic=False, out=None):
        out = untouched.copy() if out is None else out
        with pytest.raises(LIB.BackendError) as err:
            API.observe_smooth(field, sigma, below, above, periodic_los=periodic, out=out)
        assert err.value.code == code
        assert "observe:" in str(err.value)
        if out is not field:
            assert np.array_equal(out, untouched)  # nothing is written on an error

    bad = f.copy()
    bad[3, 2, 4] = np.nan
    refused(NAN_ERROR, bad, 1.0)
    bad[3, 2, 4] = np.inf
    refused(NAN_ERROR, bad, 0.0)
    for sigma in (-1.0, np.nan, 129.0):
        one_bad = np.full(9, 1.0)
        one_bad[6] = sigma
        refused(VALUE_ERROR, f, one_bad)
    one_bad = zero.copy()
    one_bad[8] = -1
    refused(VALUE_ERROR, f, 1.0, below=one_bad)
    refused(VALUE_ERROR, f, 1.0, above=one_bad)
    refused(VALUE_ERROR, f, 1.0, below=zero + 5, above=zero + 4, periodic=True)  # ns + 1 slices
    API.observe_smooth(f, 1.0, zero + 4, zero + 4, periodic_los=True)  # ns slices
    refused(VALUE_ERROR, f, 1.0, out=f)
    API.observe_smooth(f, 128.0)  # the widest beam there is
