"""Host checks of the bispectrum (no GPU): the fp64 restatement ``tests/bispectrum_reference.py``
-- the spec of the device code -- against a brute-force sum over closed triplets of modes and against the known
answer for three plane waves; the edges and triangles ``21cmfast_amd/powerspec.py`` builds; and its argument errors,
raised before the library is loaded."""

import importlib
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bispectrum_reference as R  # noqa: E402

PS = importlib.import_module("21cmfast_amd.powerspec")
ROOT = Path(__file__).resolve().parent.parent

# the device cases of tests/test_gpu_bispectrum.py: shape, shells, lengths, triangles kept of all
GPU_CASES = [
    ((16, 16, 16), 5, 100.0, 32, 35),
    ((12, 14, 18), 4, (60.0, 75.0, 80.0), 19, 20),
    ((33, 35, 37), 8, (70.0, 75.0, 80.0), 98, 120),
    ((32, 32, 100), 8, (50.0, 50.0, 156.25), 98, 120),
    ((64, 64, 64), 12, 100.0, 269, 364),
]


@pytest.mark.parametrize("shape,L,n_bins", [((8, 8, 8), 100.0, 3), ((6, 7, 8), (60.0, 75.0, 80.0), 3),
                                            ((12, 10, 9), (90.0, 80.0, 70.0), 4)], ids=str)
def test_fft_estimator_equals_brute_force(shape, L, n_bins):
    f = np.random.default_rng(11).standard_normal(shape)
    f = f + 0.5 * f * f
    edges = R.default_edges(shape, L, n_bins)
    tri = R.all_triangles(n_bins)
    B1, c1, s1 = R.fft_estimator(f, L, edges, tri)
    B2, c2, s2 = R.brute_force(f, L, edges, tri)
    assert np.array_equal(c1, c2)
    assert np.array_equal(np.isnan(B1), c1 == 0) and np.array_equal(np.isnan(B2), c1 == 0)
    ok = c1 > 0
    assert ok.sum() >= 8
    assert np.max(np.abs(B1 - B2)[ok] / s1[ok]) < 1e-12
    assert np.allclose(s1[ok], s2[ok], rtol=1e-12)


def test_known_triangle_counts():
    edges = R.default_edges((8, 8, 8), 100.0, 3)
    _, counts, _ = R.fft_estimator(np.random.default_rng(2).standard_normal((8, 8, 8)), 100.0, edges,
                                   R.all_triangles(3))
    assert counts.tolist() == [0, 24, 6, 48, 48, 144, 48, 192, 264, 552]


def test_plane_waves_known_answer():
    shape, L = (16, 16, 16), 100.0
    modes = [(1, 0, 0), (1, 2, 0), (-2, -2, 0)]  # |m| = 1, 2.24, 2.83: three different shells of width 0.83
    amps, phases = (1.5, 0.7, 1.1), (0.3, -1.1, 0.5)
    f = R.plane_wave_field(shape, L, modes, amps, phases)
    edges = R.default_edges(shape, L, 5)
    shells = [int(np.digitize(2 * np.pi / L * np.linalg.norm(m), edges)) - 1 for m in modes]
    assert sorted(set(shells)) == sorted(shells) and min(shells) >= 0 and max(shells) < 5
    tri = np.array([sorted(shells)], np.int32)
    B, n, scale = R.fft_estimator(f, L, edges, tri)
    want = R.plane_wave_bispectrum(L, amps, phases, n[0])
    assert n[0] > 0 and abs(want) / scale[0] > 0.1
    assert abs(B[0] - want) < 1e-12 * scale[0]
    # every other triangle holds no signal
    others = np.array([t for t in R.all_triangles(5).tolist() if t != tri[0].tolist()], np.int32)
    Bo, no, so = R.fft_estimator(f, L, edges, others)
    assert np.all(np.abs(Bo[no > 0]) < 1e-9 * abs(want))


@pytest.mark.parametrize("shape,L", [((16, 16, 16), 100.0), ((12, 14, 18), (60.0, 75.0, 80.0)),
                                     ((33, 35, 37), (70.0, 75.0, 80.0))], ids=str)
def test_bispectrum_edges_formula(shape, L):
    Ls = R.lengths(L)
    kmin = max(2 * np.pi / l for l in Ls) / 2
    kmax = (2.0 / 3.0) * min(np.pi * n / l for n, l in zip(shape, Ls))
    assert PS.bispectrum_k_range(shape, L) == (kmin, kmax)
    assert np.array_equal(PS.bispectrum_edges(shape, L), np.linspace(kmin, kmax, 9))
    assert np.array_equal(PS.bispectrum_edges(shape, L, 5), np.linspace(kmin, kmax, 6))
    assert np.array_equal(PS.bispectrum_edges(shape, L, 6, log_bins=True), np.geomspace(kmin, kmax, 7))
    mine = np.array([0.5 * kmax, 0.75 * kmax, kmax])
    assert np.array_equal(PS.bispectrum_edges(shape, L, mine), mine)
    assert np.array_equal(PS.bispectrum_edges(shape, L, 5), R.default_edges(shape, L, 5))
    # no Nyquist mode below k_max, on any axis
    assert kmax < min(np.pi * n / l for n, l in zip(shape, Ls))


@pytest.mark.parametrize("shape,n_bins,L,kept,total", GPU_CASES, ids=lambda v: str(v))
def test_bispectrum_triangles_keeps_the_populated_ones(shape, n_bins, L, kept, total):
    edges = PS.bispectrum_edges(shape, L, n_bins)
    tri = PS.bispectrum_triangles(edges)
    assert tri.dtype == np.int32 and tri.shape == (kept, 3)
    assert tri.tolist() == sorted(tri.tolist()) and np.array_equal(tri, R.closing_triangles(edges))
    every = R.all_triangles(n_bins)
    assert len(every) == total
    if np.prod(shape) <= 40000:  # the populated triangles, by transforms of the shell indicators
        _, counts, _ = R.fft_estimator(np.zeros(shape), L, edges, every)
        assert every[counts > 0].tolist() == tri.tolist()


def test_mirror_of_the_bins_struct_matches_the_compiler(tmp_path):
    S = importlib.import_module("21cmfast_amd.structs")
    import ctypes as C

    src = tmp_path / "layout.c"
    fields = [n for n, _ in S.BispecBins._fields_]
    body = "".join(f'printf("%zu\\n", offsetof(c21cm_bispec_bins, {n}));' for n in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c21cm_grid.h"\nint main(void){'
                   'printf("%zu\\n", sizeof(c21cm_bispec_bins));' + body + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(S.BispecBins)] + [getattr(S.BispecBins, n).offset for n in fields]


@pytest.fixture
def no_library(monkeypatch):
    api = importlib.import_module("21cmfast_amd.grid_api")

    def boom(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(api, "load", boom)


F = np.ones((12, 12, 12), np.float32)
KMAX = (2.0 / 3.0) * (np.pi * 12 / 10.0)
BAD = [
    dict(bins=0), dict(bins=33), dict(bins=2.5), dict(bins=True), dict(bins=np.linspace(0.5, KMAX, 34)),
    dict(bins=[1.0]), dict(bins=[1.0, np.nan, 2.0]), dict(bins=[1.0, np.inf]), dict(bins=[1.0, 1.0, 2.0]),
    dict(bins=[2.0, 1.0]), dict(bins=np.ones((2, 2))),
    dict(bins=[0.0, 1.0, 2.0]), dict(bins=[-1.0, 1.0]),
    dict(bins=[1.0, 2.0, np.nextafter(KMAX, np.inf)]),
    dict(triangles=np.zeros((0, 3), np.int32)), dict(triangles=[0, 0, 0]), dict(triangles=[[0, 1]]),
    dict(triangles=[[0.0, 1.0, 2.0]]), dict(triangles=[[0, 1, 8]]), dict(triangles=[[-1, 1, 2]]),
    dict(triangles=[[1, 0, 2]]), dict(triangles=[[0, 2, 1]]),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: ",".join(f"{k}={np.shape(v) or v}" for k, v in kw.items()))
def test_bispectrum_rejects_bad_arguments(no_library, kw):
    with pytest.raises(ValueError):
        PS.get_bispectrum(F, 10.0, **kw)
    with pytest.raises(ValueError):
        PS.lightcone_bispectra(np.ones((12, 12, 30), np.float32), 10.0 / 12, chunk_length=12, **kw)


def test_bispectrum_rejects_bad_fields_and_chunks(no_library):
    with pytest.raises(ValueError):
        PS.get_bispectrum(np.ones((12, 12), np.float32), 10.0)
    with pytest.raises(ValueError):
        PS.get_bispectrum(np.ones((2, 12, 12, 12), np.float32), 10.0)
    with pytest.raises(ValueError):
        PS.get_bispectrum(F, (10.0, 10.0))
    lc = np.ones((12, 12, 30), np.float32)
    with pytest.raises(ValueError):
        PS.lightcone_bispectra(lc[0], 1.0)
    for kw in (dict(chunk_length=1), dict(chunk_length=31), dict(chunk_length=2.5), dict(chunk_starts=[25]),
               dict(chunk_starts=[-1]), dict(chunk_starts=[0.5]), dict(chunk_starts=[[0]]), dict(redshifts=np.ones(29))):
        with pytest.raises(ValueError):
            PS.lightcone_bispectra(lc, 1.0, **kw)
    with pytest.raises(ValueError):
        PS.lightcone_bispectra(lc, 0.0)


def test_bispectrum_triangles_and_edges_need_no_library(no_library):
    e = PS.bispectrum_edges((12, 12, 12), 10.0, 4)
    assert PS.bispectrum_triangles(e).shape[1] == 3
