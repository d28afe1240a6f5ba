"""GPU: ``get_bispectrum`` / ``lightcone_bispectra`` against the fp64 restatement
``tests/bispectrum_reference.py``.

What is exact is asserted exactly: the triangle counts (integers), the NaN pattern, the number of populated
triangles, bit-equality between calls, between a subset of triangles and all of them, between numpy and device
input, and between the chunks of a lightcone and the same boxes one by one.  B itself is compared as |B_dev - B_ref|
/ scale, scale = (V^2 / N^3) sum_x |delta_1 delta_2 delta_3| / (N n_tri) (the restatement returns it), against
BISPECTRUM_TOL below.
"""

import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bispectrum_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

PS = importlib.import_module("21cmfast_amd.powerspec")

POWER_RTOL = 2e-5  # what tests/test_gpu_power.py holds the binned power to
# MEASURED on an MI355X: the worst |B_dev - B_ref| / scale over the ten runs of test_device_matches_restatement (five
# shapes, seeds 3 and 5) was WORST_SEEN, at (33, 35, 37) with seed 3 (per run 2.2e-8 to 2.0e-7, medians over the
# triangles 3e-9 to 3e-8); the bound is four times that -- the margin the variance test of section 4.11 took, for the
# same reason: the bits are the same from run to run, other seeds are not these seeds.  (An fp32 pocketfft emulation
# on a CPU gave 1.2e-7.)  It stays under the sanity ceiling 3 POWER_RTOL: three transformed factors, each held to
# POWER_RTOL in power.
WORST_SEEN = 1.960120e-07
BISPECTRUM_TOL = 4 * WORST_SEEN
CEILING = 3 * POWER_RTOL

# shape, shells, lengths, populated triangles (of all b1 <= b2 <= b3)
CASES = [
    ((16, 16, 16), 5, 100.0, 32),
    ((12, 14, 18), 4, (60.0, 75.0, 80.0), 19),
    ((33, 35, 37), 8, (70.0, 75.0, 80.0), 98),
    ((32, 32, 100), 8, (50.0, 50.0, 156.25), 98),
    ((64, 64, 64), 12, 100.0, 269),
]
SEEDS = (3, 5)


def make_field(shape, seed):
    g = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return (g + np.float32(0.5) * g * g).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(case, seed):
    shape, n_bins, L, _ = CASES[case]
    f = make_field(shape, seed)
    edges = R.default_edges(shape, L, n_bins)
    tri = R.all_triangles(n_bins)
    B, counts, scale = R.fft_estimator(f, L, edges, tri)
    for a in (f, edges, tri, B, counts, scale):
        a.setflags(write=False)
    return f, edges, tri, B, counts, scale


def same_bits(a, b):
    a, b = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_bound_is_recorded_and_sane():
    assert WORST_SEEN is not None and BISPECTRUM_TOL == 4 * WORST_SEEN
    assert 0 < BISPECTRUM_TOL < CEILING


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=[str(c[0]) for c in CASES])
def test_device_matches_restatement(gpu_lib, case, seed):
    shape, n_bins, L, populated = CASES[case]
    f, edges, tri, B, counts, scale = reference(case, seed)
    res = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri)
    assert np.array_equal(res.edges, edges) and np.array_equal(res.triangles, tri)
    assert res.n_triangles.dtype == np.int64 and np.array_equal(res.n_triangles, counts)
    assert np.array_equal(np.isnan(res.bispectrum), counts == 0)
    assert int((res.n_triangles > 0).sum()) == populated == len(PS.bispectrum_triangles(edges))
    ok = counts > 0
    dev = np.abs(res.bispectrum - B)[ok] / scale[ok]
    print(f"bispectrum {shape} seed {seed}: worst |B_dev - B_ref| / scale = {dev.max():.3e}, "
          f"worst |B| / scale = {np.max(np.abs(B[ok]) / scale[ok]):.3f}")
    assert BISPECTRUM_TOL is not None and BISPECTRUM_TOL < CEILING
    assert dev.max() <= BISPECTRUM_TOL
    # the shells are get_power's bins
    shell = R.shell_index(shape, L, edges)
    assert np.array_equal(res.n_modes, np.bincount(shell[(shell >= 0) & (shell < n_bins)], minlength=n_bins))
    power, k = PS.get_power(f, L, bins=edges)
    assert same_bits(res.power, power) and same_bits(res.k, k[tri])


def test_default_triangles_and_reduced(gpu_lib):
    shape, n_bins, L, populated = CASES[0]
    f, edges, tri, B, counts, scale = reference(0, 3)
    every = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri)
    res = PS.get_bispectrum(f, L, bins=n_bins, reduced=True)
    keep = counts > 0
    assert np.array_equal(res.triangles, tri[keep]) and len(res.triangles) == populated
    assert same_bits(res.bispectrum, every.bispectrum[keep])
    p = res.power[res.triangles]
    assert np.array_equal(res.reduced, res.bispectrum / (p[:, 0] * p[:, 1] + p[:, 1] * p[:, 2] + p[:, 2] * p[:, 0]))
    assert every.reduced is None


def test_plane_waves_known_answer(gpu_lib):
    shape, L = (32, 32, 32), 100.0
    modes = [(2, 1, 0), (3, -4, 2), (-5, 3, -2)]
    amps, phases = (1.5, 0.7, 1.1), (0.3, -1.1, 0.5)
    f = R.plane_wave_field(shape, L, modes, amps, phases).astype(np.float32)
    edges = PS.bispectrum_edges(shape, L, 8)
    shells = sorted(int(np.digitize(2 * np.pi / L * np.linalg.norm(m), edges)) - 1 for m in modes)
    assert len(set(shells)) == 3 and shells[0] >= 0 and shells[2] < 8
    res = PS.get_bispectrum(f, L, bins=8, triangles=[shells])
    _, n_ref, scale = R.fft_estimator(f, L, edges, [shells])
    want = R.plane_wave_bispectrum(L, amps, phases, n_ref[0])
    assert res.n_triangles[0] == n_ref[0] > 0
    assert abs(want) / scale[0] > 0.3  # of order one: a relative error is a fair measure here
    rel = abs(res.bispectrum[0] - want) / abs(want)
    print(f"plane waves: B = {res.bispectrum[0]:.9e}, analytic {want:.9e}, relative error {rel:.3e}")
    assert rel <= BISPECTRUM_TOL


def test_subset_two_calls_and_device_input_give_the_same_bits(gpu_lib):
    import torch

    shape, n_bins, L, _ = CASES[2]
    f, edges, tri, B, counts, scale = reference(2, 3)
    every = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri)
    again = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri)
    assert same_bits(every.bispectrum, again.bispectrum) and same_bits(every.n_triangles, again.n_triangles)
    pick = [q for q, t in enumerate(tri.tolist()) if t[0] == t[1] == t[2]] + [1, 7, 30, 31, 64, 100, 119]
    pick = np.array(pick[::-1])  # and not in sorted order
    sub = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri[pick])
    assert same_bits(sub.bispectrum, every.bispectrum[pick]) and same_bits(sub.n_triangles, every.n_triangles[pick])
    one = PS.get_bispectrum(f, L, bins=n_bins, triangles=tri[pick[:1]])
    assert same_bits(one.bispectrum, every.bispectrum[pick[:1]])
    d = PS.get_bispectrum(torch.from_numpy(f.copy()).to("cuda:0"), L, bins=n_bins, triangles=tri)
    for name in ("bispectrum", "triangles", "n_triangles", "k", "power", "n_modes", "edges"):
        t = getattr(d, name)
        assert isinstance(t, torch.Tensor) and t.device.type == "cuda", name
        assert same_bits(t, getattr(every, name)), name


def test_bin_limit(gpu_lib):
    api = importlib.import_module("21cmfast_amd.grid_api")
    lib = importlib.import_module("21cmfast_amd._lib")
    shape, L = (48, 48, 48), 100.0
    f = make_field(shape, 3)
    kmin, kmax = PS.bispectrum_k_range(shape, L)
    edges = np.linspace(kmin, kmax, 33)
    closing = PS.bispectrum_triangles(edges)
    tri = np.array([(0, 0, b) for b in range(32)] + closing[np.linspace(0, len(closing) - 1, 32).astype(int)].tolist(),
                   np.int32)
    assert len(tri) == 64
    res = PS.get_bispectrum(f, L, bins=edges, triangles=tri)
    B, counts, scale = R.fft_estimator(f, L, edges, tri)
    assert np.array_equal(res.n_triangles, counts) and np.array_equal(np.isnan(res.bispectrum), counts == 0)
    ok = counts > 0
    assert ok.sum() >= 30  # shell 0 of 32 holds no mode at all: every (0, 0, b3) is NaN
    assert np.max(np.abs(res.bispectrum - B)[ok] / scale[ok]) <= BISPECTRUM_TOL
    with pytest.raises(ValueError):
        PS.get_bispectrum(f, L, bins=33)
    with pytest.raises(lib.BackendError) as err:
        api.bispectrum(f, shape, (L, L, L), np.linspace(kmin, kmax, 34), tri)
    assert err.value.code == 3


def test_library_argument_errors(gpu_lib):
    api = importlib.import_module("21cmfast_amd.grid_api")
    lib = importlib.import_module("21cmfast_amd._lib")
    shape, L = (12, 12, 12), (10.0, 10.0, 10.0)
    f = make_field(shape, 3)
    kmin, kmax = PS.bispectrum_k_range(shape, L)
    good_e, good_t = np.linspace(kmin, kmax, 4), np.array([[0, 1, 2]], np.int32)
    for e, t in (([0.0, 1.0, 2.0], good_t), ([1.0, 1.0, 2.0], good_t), ([1.0, np.nan, 2.0], good_t),
                 ([1.0, 2.0, np.nextafter(kmax, np.inf)], good_t), (good_e, [[1, 0, 2]]), (good_e, [[0, 1, 3]]),
                 (good_e, [[-1, 1, 2]])):
        with pytest.raises(lib.BackendError) as err:
            api.bispectrum(f, shape, L, np.asarray(e, np.float64), np.asarray(t, np.int32))
        assert err.value.code == 3
    out, counts = api.bispectrum(f, shape, L, good_e, good_t)
    assert out.shape == (1, 1) and counts.shape == (1,)


def test_geometry_cache(gpu_lib):
    (sa, na, La, _), (sb, nb, Lb, _) = CASES[0], CASES[1]
    fa, _, ta, _, ca, _ = reference(0, 3)
    fb, _, tb, _, cb, _ = reference(1, 3)
    first = PS.get_bispectrum(fa, La, bins=na, triangles=ta)
    assert np.array_equal(first.n_triangles, ca)
    assert np.array_equal(PS.get_bispectrum(fb, Lb, bins=nb, triangles=tb).n_triangles, cb)
    back = PS.get_bispectrum(fa, La, bins=na, triangles=ta)
    assert np.array_equal(back.n_triangles, ca) and same_bits(back.bispectrum, first.bispectrum)
    # the same shape and edges in a longer box is another geometry: the counts stay, B scales as V^2
    e2 = PS.bispectrum_edges(sa, 2 * La, na)
    twice = PS.get_bispectrum(fa, 2 * La, bins=na, triangles=ta)
    assert np.array_equal(twice.edges, e2) and np.array_equal(twice.n_triangles, ca)
    ok = ca > 0
    assert np.allclose(twice.bispectrum[ok], 64 * first.bispectrum[ok], rtol=1e-12)


def test_lightcone_chunks(gpu_lib):
    api = importlib.import_module("21cmfast_amd.grid_api")
    big = make_field((16, 16, 60), 5)
    lc = np.ascontiguousarray(big[:, :, 5:53])
    z = np.linspace(6.0, 9.0, 48)
    res = PS.lightcone_bispectra(lc, 2.0, redshifts=z, bins=5, reduced=True)
    assert res.bispectrum.shape == (3, len(res.triangles)) and res.power.shape == (3, 5)
    assert np.array_equal(res.chunk_starts, [0, 16, 32]) and res.redshifts.shape == (3,)
    for c, s in enumerate(res.chunk_starts):
        one = PS.get_bispectrum(lc[:, :, s:s + 16], 32.0, bins=5, reduced=True)
        assert same_bits(one.bispectrum, res.bispectrum[c]) and same_bits(one.reduced, res.reduced[c])
        assert same_bits(one.power, res.power[c]) and same_bits(one.n_triangles, res.n_triangles)
        assert same_bits(one.k, res.k)
    assert not np.array_equal(res.bispectrum[0], res.bispectrum[1])
    # the strided view itself, and the parent array read through row_pitch
    view = PS.lightcone_bispectra(big[:, :, 5:53], 2.0, bins=5)
    assert same_bits(view.bispectrum, res.bispectrum)
    B, n = api.bispectrum(big, (16, 16, 16), (32.0,) * 3, res.edges, res.triangles, offsets=5 + res.chunk_starts,
                          row_pitch=60)
    assert same_bits(B, res.bispectrum) and same_bits(n, res.n_triangles)
    # overlapping chunks of another length
    odd = PS.lightcone_bispectra(lc, 2.0, chunk_length=20, chunk_starts=[0, 9, 28], bins=4)
    for c, s in enumerate((0, 9, 28)):
        assert same_bits(PS.get_bispectrum(lc[:, :, s:s + 20], (32.0, 32.0, 40.0), bins=4).bispectrum, odd.bispectrum[c])


def test_non_finite_input(gpu_lib):
    lib = importlib.import_module("21cmfast_amd._lib")
    f = make_field((16, 16, 16), 3).copy()
    f[3, 4, 5] = np.nan
    with pytest.raises(lib.BackendError) as err:
        PS.get_bispectrum(f, 100.0, bins=5)
    assert err.value.code == 7
    # the bispectrum entry itself (get_bispectrum meets the power spectrum's check first)
    api = importlib.import_module("21cmfast_amd.grid_api")
    edges = PS.bispectrum_edges((16, 16, 16), 100.0, 5)
    with pytest.raises(lib.BackendError) as err:
        api.bispectrum(f, (16, 16, 16), (100.0,) * 3, edges, PS.bispectrum_triangles(edges))
    assert err.value.code == 7 and "bispectrum" in str(err.value)
    lc = make_field((16, 16, 48), 3).copy()
    lc[1, 2, 40] = np.inf
    with pytest.raises(lib.BackendError) as err:
        PS.lightcone_bispectra(lc, 2.0, bins=5)
    assert err.value.code == 7
