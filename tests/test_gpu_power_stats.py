"""Taper windows, mu / wedge cuts, per-bin variance and one-point statistics of 21cmfast_amd.powerspec on the
MI355X against the fp64 restatement (tests/power_stats_reference.py).

Tolerances: counts and the NaN pattern exactly, k to 1e-12, power to POWER_RTOL of the restatement (the noise-floor
rule of tests/test_gpu_power.py, copied).  The variance tolerance is a measurement: VAR_RTOL is 4 x the worst
deviation seen over the variance cases below with seeds 3 and 5 (the factor covers the spread between fields),
under the ceiling 6 x POWER_RTOL (var ~ mean^2 for near-Gaussian modes, so an error d in each mode's power reaches
the variance as at most about 6 d).  Observed on an MI355X: see VAR_OBSERVED.  Bins whose reference variance is <=
1e-9 x (reference power)^2 (single modes, conjugate pairs) are compared absolutely against that bound.  Moments:
1e-10 x (sum|v| / N, sum|d|^p / N), from the worst-case summation error (N - 1) 2^-53 = 2.9e-11 at N = 2^18;
histogram counts exactly."""

import ctypes as C
import importlib

import numpy as np
import pytest

import power_stats_reference as SR

pytestmark = pytest.mark.gpu
PS = importlib.import_module("21cmfast_amd.powerspec")
API = importlib.import_module("21cmfast_amd.grid_api")
S = importlib.import_module("21cmfast_amd.structs")

POWER_RTOL = 2e-5
VAR_CEILING = 6 * POWER_RTOL
VAR_OBSERVED = 1.816e-6  # the worst relative deviation of the variance over the cases below (cylindrical, seed 3)
VAR_RTOL = 4 * VAR_OBSERVED
assert VAR_RTOL <= VAR_CEILING

ODD, ODD_L = (33, 35, 37), (70.0, 75.0, 80.0)
LONG, LONG_L = (32, 32, 100), (50.0, 50.0, 156.25)
CUBE, CUBE_L = (64, 64, 64), 100.0
LC_SHAPE, LC_CHUNK, LC_DX = (20, 22, 70), 24, 1.7


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _field(shape, seed=11, mean=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + mean).astype(np.float32)


def check_power(got, ref, rtol=POWER_RTOL, atol_frac=1e-20, what=""):
    got, ref = _np(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    g, r = got[ok], ref[ok]
    noise = atol_frac * np.max(np.abs(r)) if r.size else 0.0
    real = np.abs(r) > noise
    assert np.all(np.abs(g[~real] - r[~real]) <= noise), what
    dev = float(np.max(np.abs(g[real] / r[real] - 1))) if real.any() else 0.0
    print(f"{what}: worst relative power deviation {dev:.2e}")
    assert dev <= rtol, (what, dev)
    return dev


def check_variance(got, ref_var, ref_power, what=""):
    got, rv, rp = _np(got), np.asarray(ref_var), np.asarray(ref_power)
    assert got.shape == rv.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(rv)), what
    ok = ~np.isnan(rv)
    g, v, floor = got[ok], rv[ok], 1e-9 * rp[ok] ** 2
    real = v > floor
    assert real.any(), what
    assert np.all(np.abs(g[~real] - v[~real]) <= floor[~real]), what
    dev = float(np.max(np.abs(g[real] / v[real] - 1)))
    print(f"{what}: worst relative variance deviation {dev:.3e}")
    assert dev <= VAR_CEILING, (what, dev, "above 6 x POWER_RTOL: a bug, not a tolerance")
    assert dev <= VAR_RTOL, (what, dev)
    return dev


def check_spherical(got, ref, what):
    """got: (power, k, counts[, variance]) of the device; ref: (power, k, counts, variance) of the restatement."""
    assert np.array_equal(_np(got[2]), ref[2]), what
    assert np.array_equal(np.isnan(_np(got[0])), ref[2] == 0), what
    np.testing.assert_allclose(_np(got[1]), ref[1], rtol=1e-12, atol=0, err_msg=what)
    check_power(got[0], ref[0], what=what)
    if len(got) > 3:
        check_variance(got[3], ref[3], ref[0], what=what)


# ---- 1. windows --------------------------------------------------------------------------------------------
WINDOW_CASES = {
    "blackmanharris": (ODD, ODD_L, "blackmanharris"),
    "hann": (ODD, ODD_L, "hann"),
    "blackman": (ODD, ODD_L, "blackman"),
    "hann-cube": (CUBE, CUBE_L, "hann"),
    "array": (LONG, LONG_L, 0.25 + np.sin(np.linspace(0.0, np.pi, 100)) ** 2),
    "three-axes": (ODD, ODD_L, ("hann", np.linspace(0.5, 1.5, 35), "blackmanharris")),
    "two-axes": (ODD, ODD_L, ("blackman", None, "hann")),
}


@pytest.mark.parametrize("case", list(WINDOW_CASES))
def test_windowed_power(gpu_lib, case):
    shape, L, window = WINDOW_CASES[case]
    f = _field(shape, seed=5)
    got = PS.get_power(f, L, window=window, return_counts=True)
    check_spherical(got, SR.get_power(f, L, window=window), f"window {case}")


def test_windowed_cross_power(gpu_lib):
    f, g = _field(LONG, 1), _field(LONG, 2)
    h = (f + 0.5 * g).astype(np.float32)
    got = PS.get_power(f, LONG_L, deltax2=h, window="blackmanharris", return_counts=True)
    check_spherical(got, SR.get_power(f, LONG_L, deltax2=h, window="blackmanharris"), "windowed cross")


def test_windowed_cylindrical_power(gpu_lib):
    f = _field(ODD, seed=9)
    p, kp, kz, c = PS.get_cylindrical_power(f, ODD_L, window="hann", return_counts=True)
    rp, rkp, rkz, rc, _ = SR.get_cylindrical_power(f, ODD_L, window="hann")
    assert np.array_equal(c, rc)
    np.testing.assert_allclose(kp, rkp, rtol=1e-12, atol=0)
    np.testing.assert_allclose(kz, rkz, rtol=1e-12, atol=0)
    check_power(p, rp, what="windowed cylindrical")


def test_windowed_lightcone(gpu_lib):
    lc = _field(LC_SHAPE, seed=21)
    got = PS.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, window="blackmanharris")
    ref = SR.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, window="blackmanharris")
    assert list(got.chunk_starts) == [0, 24] and got.power.shape[0] == 2 and got.variance is None
    assert np.array_equal(got.counts, ref["counts"])
    np.testing.assert_allclose(got.k, ref["k"], rtol=1e-12, atol=0)
    for c in range(2):
        check_power(got.power[c], ref["power"][c], what=f"windowed lightcone chunk {c}")


# ---- 2. cuts -----------------------------------------------------------------------------------------------
CUT_CASES = {
    "mu_min": (ODD, ODD_L, dict(mu_min=0.5)),
    "mu_range": (ODD, ODD_L, dict(mu_min=0.3, mu_max=0.9)),
    "wedge": (ODD, ODD_L, dict(wedge_slope=0.5)),
    "wedge-buffer": (ODD, ODD_L, dict(wedge_slope=1.0, wedge_buffer=0.1)),
    "mu_min-long": (LONG, LONG_L, dict(mu_min=0.5)),
    "mu_max-cube": (CUBE, CUBE_L, dict(mu_max=0.6)),
    "wedge,ignore_kpar_zero": (ODD, ODD_L, dict(wedge_slope=0.5, ignore_kpar_zero=True)),
    "mu,wedge,log": (ODD, ODD_L, dict(mu_max=0.95, wedge_slope=0.3, wedge_buffer=0.05, log_bins=True)),
}


@pytest.mark.parametrize("case", list(CUT_CASES))
def test_cuts(gpu_lib, case):
    shape, L, kw = CUT_CASES[case]
    f = _field(shape, seed=5)
    got = PS.get_power(f, L, return_counts=True, **kw)
    ref = SR.get_power(f, L, **kw)
    full = PS.get_power(f, L, return_counts=True)[2]
    assert ref[2].sum() < full.sum(), "the cut removes nothing: the case is vacuous"
    check_spherical(got, ref, f"cut {case}")
    if case == "wedge-buffer":
        assert list(np.flatnonzero(_np(got[2]) == 0)) == [0] and np.isnan(got[0][0])


def test_cut_with_cross_power(gpu_lib):
    f, g = _field(ODD, 1), _field(ODD, 2)
    h = (f + 0.5 * g).astype(np.float32)
    got = PS.get_power(f, ODD_L, deltax2=h, mu_min=0.3, mu_max=0.9, return_counts=True)
    check_spherical(got, SR.get_power(f, ODD_L, deltax2=h, mu_min=0.3, mu_max=0.9), "cut cross")


def test_cut_on_a_lightcone(gpu_lib):
    lc = _field(LC_SHAPE, seed=21)
    got = PS.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, wedge_slope=0.5)
    ref = SR.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, wedge_slope=0.5)
    assert np.array_equal(got.counts, ref["counts"])
    np.testing.assert_allclose(got.k, ref["k"], rtol=1e-12, atol=0)
    for c in range(2):
        check_power(got.power[c], ref["power"][c], what=f"cut lightcone chunk {c}")


# ---- 3. variance -------------------------------------------------------------------------------------------
SEEDS = [3, 5]


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_spherical(gpu_lib, seed):
    for shape, L in ((CUBE, CUBE_L), (ODD, ODD_L)):
        f = _field(shape, seed)
        got = PS.get_power(f, L, return_counts=True, return_variance=True)
        assert len(got) == 4
        check_spherical(got, SR.get_power(f, L), f"variance {shape} seed {seed}")
        p, k, v = PS.get_power(f, L, return_variance=True)
        assert np.array_equal(v, got[3], equal_nan=True) and np.array_equal(p, got[0], equal_nan=True)


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_cylindrical(gpu_lib, seed):
    f = _field(ODD, seed)
    p, kp, kz, c, v = PS.get_cylindrical_power(f, ODD_L, return_counts=True, return_variance=True)
    rp, rkp, rkz, rc, rv = SR.get_cylindrical_power(f, ODD_L)
    assert np.array_equal(c, rc)
    check_power(p, rp, what="variance cylindrical")
    check_variance(v, rv, rp, what=f"variance cylindrical seed {seed}")


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_cross(gpu_lib, seed):
    f, g = _field(LONG, seed), _field(LONG, seed + 100)
    h = (f + 0.5 * g).astype(np.float32)
    got = PS.get_power(f, LONG_L, deltax2=h, return_counts=True, return_variance=True)
    check_spherical(got, SR.get_power(f, LONG_L, deltax2=h), f"variance cross seed {seed}")


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_lightcone(gpu_lib, seed):
    lc = _field(LC_SHAPE, seed)
    for kw in (dict(), dict(dimensionless=True), dict(cylindrical=True, dimensionless=True)):
        got = PS.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, return_variance=True, **kw)
        ref = SR.lightcone_power_spectra(lc, LC_DX, chunk_length=LC_CHUNK, **kw)
        assert got.variance.shape == got.power.shape
        for c in range(2):
            check_power(got.power[c], ref["power"][c], what=f"variance lightcone {kw} chunk {c}")
            check_variance(got.variance[c], ref["variance"][c], ref["power"][c],
                           what=f"variance lightcone {kw} chunk {c} seed {seed}")


@pytest.mark.parametrize("seed", SEEDS)
def test_variance_with_window_and_cut(gpu_lib, seed):
    f = _field(ODD, seed)
    kw = dict(window="blackmanharris", mu_min=0.3, mu_max=0.9)
    got = PS.get_power(f, ODD_L, return_counts=True, return_variance=True, **kw)
    check_spherical(got, SR.get_power(f, ODD_L, **kw), f"variance window cut seed {seed}")


# ---- 4. bits -----------------------------------------------------------------------------------------------
def _same(a, b):
    for x, y in zip(a, b):
        x, y = _np(x), _np(y)
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)


def test_two_calls_give_the_same_bits(gpu_lib):
    f = _field(CUBE, seed=3)
    kw = dict(window="blackmanharris", wedge_slope=0.5, return_counts=True, return_variance=True)
    _same(PS.get_power(f, CUBE_L, **kw), PS.get_power(f, CUBE_L, **kw))
    kw = dict(window="hann", return_counts=True, return_variance=True)
    _same(PS.get_cylindrical_power(f, CUBE_L, **kw), PS.get_cylindrical_power(f, CUBE_L, **kw))


@pytest.mark.parametrize("cyl", [False, True], ids=["spherical", "cylindrical"])
def test_ex_entry_without_options_is_the_plain_entry(gpu_lib, cyl):
    f, g = _field(ODD, 3), _field(ODD, 4)
    if cyl:
        edges = PS.cylindrical_edges(ODD, ODD_L)
    else:
        edges = (PS.spherical_edges(ODD, ODD_L),)
    lc = _field(LC_SHAPE, 6)
    for field, field2, shape, kw in ((f, None, ODD, {}), (f, g, ODD, dict(ignore_zero_mode=True)),
                                     (lc, None, (20, 22, 24), dict(offsets=[0, 24, 40], row_pitch=70))):
        if shape != ODD:
            Ls = tuple(n * LC_DX for n in shape)
            e = PS.cylindrical_edges(shape, Ls) if cyl else (PS.spherical_edges(shape, Ls),)
        else:
            Ls, e = ODD_L, edges
        plain = API.power_spectrum(field, field2, shape, Ls, *e, **kw)
        _same(plain, API.power_spectrum(field, field2, shape, Ls, *e, entry="ex-null", **kw))
        _same(plain, API.power_spectrum(field, field2, shape, Ls, *e, entry="ex", **kw))


# ---- 5. limits ---------------------------------------------------------------------------------------------
def test_variance_bin_limits(gpu_lib):
    pkg = importlib.import_module("21cmfast_amd")
    f = _field((32, 32, 32))
    with pytest.raises(pkg.BackendError, match="1200 .* bins with the variance do not fit"):
        PS.get_power(f, 50.0, bins=1200, return_variance=True)
    p, k, c = PS.get_power(f, 50.0, bins=1200, return_counts=True)
    assert p.shape == (1200,) and c.sum() > 0
    # the LDS budget of one workgroup: 1084 |k| / 877 k_par bins with the variance, 1417 / 1084 without
    p, k, v = PS.get_power(f, 50.0, bins=1084, return_variance=True)
    assert v.shape == (1084,)
    with pytest.raises(pkg.BackendError, match="do not fit"):
        PS.get_power(f, 50.0, bins=1085, return_variance=True)
    assert PS.get_cylindrical_power(f, 50.0, kpar_bins=877, return_variance=True)[3].shape[1] == 877
    with pytest.raises(pkg.BackendError, match="do not fit"):
        PS.get_cylindrical_power(f, 50.0, kpar_bins=878, return_variance=True)
    assert PS.get_cylindrical_power(f, 50.0, kpar_bins=1084)[0].shape[1] == 1084


# ---- 6. moments and PDFs -----------------------------------------------------------------------------------
def check_moments(got, field, what):
    ref, scale = SR.moments(field)
    for name, g, r, s in zip(("mean", "m2", "m3", "m4"), got, ref, scale):
        print(f"{what} {name}: |dev| / scale {abs(float(g) - r) / s:.2e}")
        assert abs(float(g) - r) <= 1e-10 * s, (what, name, float(g), r)


# (70, 65, 9): 4550 rows, more than the 4096 one workgroup of the first level of the box sum takes, the last short
@pytest.mark.parametrize("shape", [ODD, CUBE, (70, 65, 9)])
def test_moments_of_a_box(gpu_lib, shape):
    f = _field(shape, seed=7)
    m, _ = API.field_moments(f, shape)
    check_moments(m[0], f, f"moments {shape}")
    (rm, r2, r3, r4), _ = SR.moments(f)
    mean, var, skew, kurt = PS.get_moments(f)
    assert all(isinstance(x, float) for x in (mean, var, skew, kurt))
    assert mean == m[0, 0] and var == m[0, 1]
    np.testing.assert_allclose(skew, r3 / r2**1.5, rtol=0, atol=1e-9)
    np.testing.assert_allclose(kurt, r4 / r2**2 - 3, rtol=0, atol=1e-9)
    m2, _ = API.field_moments(f, shape)
    assert np.array_equal(m, m2)


def test_moments_and_pdf_of_lightcone_chunks(gpu_lib):
    wide = _field((70, 65, 20), seed=22)  # two chunks of 4550 rows each: the two-level box sum, batched
    res = PS.lightcone_moments(wide, chunk_length=9, bins=[0.0, 1.0, 2.0], density=False)
    for c, s in enumerate((0, 9)):
        chunk = wide[:, :, s:s + 9]
        (rm, r2, r3, r4), _ = SR.moments(chunk)
        check_moments((res.mean[c], res.variance[c], res.skewness[c] * r2**1.5, (res.kurtosis[c] + 3) * r2**2),
                      chunk, f"wide lightcone chunk {c}")
        assert np.array_equal(res.pdf[c], SR.histogram(chunk, [0.0, 1.0, 2.0]))
    lc = _field(LC_SHAPE, seed=21)
    z = np.linspace(6.0, 9.0, LC_SHAPE[2])
    res = PS.lightcone_moments(lc, chunk_length=LC_CHUNK, redshifts=z, bins=16, range=(-2.0, 4.0), density=False)
    assert list(res.chunk_starts) == [0, 24]
    np.testing.assert_array_equal(res.redshifts, 0.5 * (z[[11, 35]] + z[[12, 36]]))
    edges = np.linspace(-2.0, 4.0, 17)
    assert np.array_equal(res.edges, edges)
    for c, s in enumerate((0, 24)):
        chunk = lc[:, :, s:s + LC_CHUNK]
        (rm, r2, r3, r4), _ = SR.moments(chunk)
        check_moments((res.mean[c], res.variance[c], res.skewness[c] * r2**1.5, (res.kurtosis[c] + 3) * r2**2),
                      chunk, f"lightcone chunk {c}")
        assert np.array_equal(res.pdf[c], SR.histogram(chunk, edges))
    plain = PS.lightcone_moments(lc, chunk_length=LC_CHUNK)
    assert plain.pdf is None and np.array_equal(plain.mean, res.mean)
    # the default range spans the whole lightcone; density as np.histogram normalises the kept values
    dens = PS.lightcone_moments(lc, chunk_length=LC_CHUNK, bins=8)
    e = np.linspace(float(lc.min()), float(lc.max()), 9)
    assert np.array_equal(dens.edges, e)
    h = SR.histogram(lc[:, :, :LC_CHUNK], e)
    np.testing.assert_allclose(dens.pdf[0], h / np.diff(e) / h.sum(), rtol=1e-14)


def test_histogram_edges(gpu_lib):
    f = _field(ODD, seed=8)
    edges = np.array([-1.5, -0.25, 0.0, 0.5, 1.0, 1.125, 2.75, 4.0])  # 7 uneven bins, all fp32 values
    f[0, 0, 0], f[5, 6, 7], f[32, 34, 36] = edges[0], edges[3], edges[-1]
    counts, e = PS.get_pdf(f, edges, density=False)
    ref = SR.histogram(f, edges)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref) and np.array_equal(e, edges)
    # half-open: the value on the last edge is dropped, those on the first and the inner edge count upwards
    assert ref.sum() == np.count_nonzero((f >= edges[0]) & (f < edges[-1]))
    g = f.copy()
    g[0, 0, 0], g[5, 6, 7], g[32, 34, 36] = np.nextafter(np.float32(edges[0]), np.float32(-9)), 0.4, 3.9
    moved = PS.get_pdf(g, edges, density=False)[0] - counts
    assert list(moved) == [-1, 0, 1, -1, 0, 0, 1]
    pdf, _ = PS.get_pdf(f, edges)
    v = f.astype(np.float64).ravel()
    np.testing.assert_allclose(pdf, np.histogram(v[v < edges[-1]], edges, density=True)[0], rtol=1e-14)


def test_histogram_of_1024_linear_bins(gpu_lib):
    f = _field(CUBE, seed=9)
    counts, edges = PS.get_pdf(f, 1024, range=(-3.0, 5.0), density=False)
    assert np.array_equal(edges, np.linspace(-3.0, 5.0, 1025))
    assert np.array_equal(counts, SR.histogram(f, edges)) and counts.sum() > 0.99 * f.size
    # the default range is the field's minimum and maximum; the maximum sits on the last edge and is dropped
    counts, edges = PS.get_pdf(f, 1024, density=False)
    assert edges[0] == f.min() and edges[-1] == f.max()
    assert np.array_equal(counts, SR.histogram(f, edges)) and counts.sum() == f.size - np.count_nonzero(f == f.max())
    pkg = importlib.import_module("21cmfast_amd")
    with pytest.raises(pkg.BackendError, match="4097 histogram bins do not fit"):
        PS.get_pdf(f, 4097)
    assert PS.get_pdf(f, 4096, density=False)[0].sum() > 0


def test_constant_field_has_nan_skewness(gpu_lib):
    mean, var, skew, kurt = PS.get_moments(np.full((8, 9, 10), 2.5, np.float32))
    assert mean == 2.5 and var == 0.0 and np.isnan(skew) and np.isnan(kurt)


def _raw_moments(lib, f, n_bins, edges, moments, hist):
    lib.c21cm_field_moments_grids.restype = C.c_int
    lib.c21cm_field_moments_grids.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                              C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    off = np.zeros(1, np.int64)
    return lib.c21cm_field_moments_grids(f.ctypes.data, *f.shape, 1, f.shape[2], off.ctypes.data, n_bins,
                                         edges.ctypes.data, moments.ctypes.data, hist.ctypes.data, None)


def test_moments_nan_is_an_error_and_writes_nothing(gpu_lib):
    pkg = importlib.import_module("21cmfast_amd")
    f = _field((16, 17, 18))
    f[3, 4, 5] = np.nan
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_moments(f)
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_pdf(f, 8, range=(0.0, 1.0))
    edges = np.linspace(-1.0, 3.0, 9)
    moments, hist = np.full(4, -7.0), np.full(8, -7, np.int64)
    status = _raw_moments(gpu_lib, f, 8, edges, moments, hist)
    assert status != 0 and np.all(moments == -7.0) and np.all(hist == -7)
    f[3, 4, 5] = 1.0
    assert _raw_moments(gpu_lib, f, 8, edges, moments, hist) == 0
    assert np.array_equal(hist, SR.histogram(f, edges)) and moments[0] == PS.get_moments(f)[0]


def test_moments_torch_in_torch_out(gpu_lib):
    import torch

    f = _field(ODD, seed=8)
    t = torch.from_numpy(f).to("cuda:0")
    out = PS.get_moments(t)
    assert all(isinstance(x, torch.Tensor) and x.device == t.device and x.dtype == torch.float64 for x in out)
    assert [float(x) for x in out] == list(PS.get_moments(f))
    pdf, edges = PS.get_pdf(t, 32)
    rp, re = PS.get_pdf(f, 32)
    assert isinstance(pdf, torch.Tensor) and pdf.device == t.device and edges.device == t.device
    np.testing.assert_allclose(pdf.cpu().numpy(), rp, rtol=1e-14)
    assert np.array_equal(edges.cpu().numpy(), re)
    lc = torch.from_numpy(_field(LC_SHAPE, 21)).to("cuda:0")
    res = PS.lightcone_moments(lc, chunk_length=LC_CHUNK, bins=8, density=False)
    assert res.mean.device == t.device and res.pdf.device == t.device and res.pdf.dtype == torch.int64
    p, k, c, v = PS.get_power(t, ODD_L, window="hann", mu_min=0.2, return_counts=True, return_variance=True)
    assert all(isinstance(x, torch.Tensor) and x.device == t.device for x in (p, k, c, v))
    _same((p, k, c, v), PS.get_power(f, ODD_L, window="hann", mu_min=0.2, return_counts=True, return_variance=True))


# ---- 7. NaN input with every option on ---------------------------------------------------------------------
def test_power_nan_with_options_is_an_error_and_writes_nothing(gpu_lib):
    pkg = importlib.import_module("21cmfast_amd")
    f = _field((16, 17, 18))
    f[3, 4, 5] = np.nan
    kw = dict(window="blackmanharris", mu_min=0.2, wedge_slope=0.5, return_variance=True)
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_power(f, 50.0, **kw)
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_cylindrical_power(f, 50.0, window="hann", return_variance=True)
    # the raw entry with sentinel-filled outputs
    shape, L = f.shape, (50.0, 50.0, 50.0)
    edges = np.ascontiguousarray(PS.spherical_edges(shape, L))
    nb = len(edges) - 1
    bins = S.PowerBins(cylindrical=0, n_bins=nb, n_bins_par=1, edges=edges.ctypes.data_as(S.c_double_p),
                       edges_par=edges.ctypes.data_as(S.c_double_p))
    wz = PS.taper_window("blackmanharris", shape[2])
    opts = S.PowerOpts(window_z=wz.ctypes.data_as(S.c_double_p), inv_mean_w2=1.0 / float(np.mean(wz * wz)),
                       mu_min_sq=0.04, mu_max_sq=1.0, use_mu=1, wedge_slope_sq=0.25, wedge_buffer=0.0, use_wedge=1,
                       want_variance=1)
    power, kmean, var, counts = np.full(nb, -7.0), np.full(nb, -7.0), np.full(nb, -7.0), np.full(nb, -7, np.int64)
    off = np.zeros(1, np.int64)
    fn = gpu_lib.c21cm_power_spectrum_ex_grids
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_double,
                   C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p]

    def call():
        return fn(f.ctypes.data, None, *shape, 1, shape[2], off.ctypes.data, *L, C.byref(bins), C.byref(opts),
                  power.ctypes.data, kmean.ctypes.data, var.ctypes.data, counts.ctypes.data, None)

    assert call() != 0
    assert all(np.all(a == -7) for a in (power, kmean, var, counts))
    f[3, 4, 5] = 1.0
    assert call() == 0
    got = PS.get_power(f, 50.0, return_counts=True, **kw)
    _same((power, kmean, counts, var), got)
