"""CPU, no library: pins ``tests/granulometry_reference.py``, the numpy spec of ``c21cm_granulometry_grids`` (DESIGN
section 4.11), against scipy's distance transform, brute-force forms of the definitions and hand-known sets; and the
default radii and argument checks of the Python layer, which come before the library is loaded."""

import importlib
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
import granulometry_reference as R  # noqa: E402

PS = importlib.import_module("21cmfast_amd.powerspec")
LIB = importlib.import_module("21cmfast_amd._lib")

RADII2 = [0, 1, 2, 4, 5, 8, 9, 13, 16, 25, 36]
PERIODIC = [(True, True, True), (True, True, False), (False, False, False), (True, False, True)]


@pytest.mark.parametrize("shape,balls", [((12, 10, 14), 3), ((16, 16, 64), 12), ((9, 7, 70), 6)])
def test_open_boxes_against_scipy(shape, balls):
    for seed in (1, 2):
        mask = R.ball_mask(shape, balls, seed, periodic=False)
        want = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int32)
        assert np.array_equal(R.dist2(mask, False), want)
        assert np.array_equal(R.dist2(~mask, False), np.rint(ndimage.distance_transform_edt(~mask) ** 2))


@pytest.mark.parametrize("per", PERIODIC)
@pytest.mark.parametrize("shape,balls", [((12, 10, 14), 3), ((5, 16, 33), 4), ((2, 1, 9), 1)])
def test_periodic_boxes_against_a_tiling(shape, balls, per):
    """a periodic axis tiled three times and left open: the centre tile sees every minimum image"""
    mask = R.ball_mask(shape, balls, 5, r_max=4.0, periodic=per)
    reps = tuple(3 if p else 1 for p in per)
    tiled = np.rint(ndimage.distance_transform_edt(np.tile(mask, reps)) ** 2)
    centre = tuple(slice(n, 2 * n) if p else slice(0, n) for n, p in zip(shape, per))
    assert np.array_equal(R.dist2(mask, per), tiled[centre])
    assert np.array_equal(R.dist2(mask, per), R.dist2_brute(mask, per))


@pytest.mark.parametrize("per", PERIODIC)
@pytest.mark.parametrize("shape,balls", [((12, 10, 14), 3), ((16, 16, 64), 12)])
def test_covered_is_the_thresholded_local_thickness(shape, balls, per):
    mask = R.ball_mask(shape, balls, 11, periodic=per)
    res = R.granulometry(mask, RADII2, per)
    thick = R.local_thickness(res["dist2"], per)
    for k, s in enumerate(RADII2):
        assert np.array_equal(R.covered_mask(res["dist2"], s, per), thick > s), s
        assert res["covered"][k] == int((thick > s).sum())
    # the level counts the radii below the local thickness
    want = np.where(mask, sum((thick > s).astype(np.int32) for s in RADII2), -1)
    assert np.array_equal(res["level"], want)


@pytest.mark.parametrize("shape,balls", [((16, 16, 64), 12), ((33, 31, 70), 40), ((8, 8, 130), 10)])
def test_monotone_and_complete_at_zero(shape, balls):
    mask = R.ball_mask(shape, balls, 17)
    res = R.granulometry(mask, RADII2, True)
    assert res["covered"][0] == res["eroded"][0] == int(mask.sum()) == res["stats"][0]
    assert np.all(np.diff(res["covered"]) <= 0) and np.all(np.diff(res["eroded"]) <= 0)
    assert np.all(res["eroded"] <= res["covered"])
    # the condition of the GPU tests: the radii resolve the distribution
    assert np.sum((res["covered"] > 0) & (res["covered"] < res["stats"][0])) >= 5
    # a row does not depend on the other radii
    part = R.granulometry(mask, RADII2[3:8:2], True)
    assert part["covered"].tolist() == res["covered"][3:8:2].tolist()


def test_two_slabs():
    mask = np.zeros((6, 5, 40), bool)
    mask[:, :, 3:8] = True
    mask[:, :, 15:24] = True
    res = R.granulometry(mask, [0, 3, 4, 8, 9, 15, 16, 24, 25], (True, True, False))
    assert res["eroded"].tolist() == [420, 300, 180, 180, 90, 90, 30, 30, 0]
    assert res["covered"].tolist() == [420, 420, 420, 420, 270, 270, 270, 270, 0]
    assert res["stats"].tolist() == [420, 25, 19, 6 * 5 * 40 - 420]


def test_full_box():
    res = R.granulometry(np.ones((4, 5, 6), bool), [0, 7, 1000, 2**30 - 1], True)
    assert np.all(res["dist2"] == R.NONE)
    assert res["covered"].tolist() == [120] * 4 and res["eroded"].tolist() == [120] * 4
    assert res["stats"].tolist() == [120, R.NONE, 0, 0] and np.all(res["level"] == 4)


def test_empty_selection():
    res = R.granulometry(np.zeros((4, 5, 6), bool), [0, 1, 4], (True, False, True))
    assert res["covered"].tolist() == [0, 0, 0] and res["eroded"].tolist() == [0, 0, 0]
    assert np.all(res["dist2"] == 0) and np.all(res["level"] == -1)
    assert res["stats"].tolist() == [0, 0, -1, 120]


def test_one_unselected_cell():
    shape, p = (7, 4, 10), (5, 0, 8)
    mask = np.ones(shape, bool)
    mask[p] = False
    idx = np.indices(shape)
    want = sum(np.minimum(np.abs(idx[a] - p[a]), shape[a] - np.abs(idx[a] - p[a])) ** 2 for a in range(3))
    assert np.array_equal(R.dist2(mask, True), want)


def test_default_radii():
    s = PS.granulometry_radii((64, 64, 64), 32)
    assert s.dtype == np.int64 and s[0] == 1 and s[-1] == 32 * 32 and np.all(np.diff(s) > 0) and len(s) <= 32
    want = np.unique(np.floor(np.geomspace(1.0, 32.0, 32) ** 2).astype(np.int64))
    assert s.tolist() == want.tolist()
    # half a periodic axis, the whole of an open one: the shortest reach wins
    assert PS.granulometry_radii((8, 8, 40), 8, (True, True, False))[-1] == 16
    assert PS.granulometry_radii((8, 8, 40), 8, False)[-1] == 64
    assert PS.granulometry_radii((40, 40, 6), 8, (True, True, False))[-1] == 36
    assert PS.granulometry_radii((1, 1, 1), 5).tolist() == [1]
    for n in (0, 256, 2.5, True):
        with pytest.raises(ValueError):
            PS.granulometry_radii((8, 8, 8), n)


def test_argument_errors_come_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(LIB, "load", no_library)
    monkeypatch.setattr(importlib.import_module("21cmfast_amd.grid_api"), "load", no_library)
    f = np.arange(64, dtype=np.float32).reshape(4, 4, 4)
    lc = np.arange(192, dtype=np.float32).reshape(4, 4, 12)
    for kw in (dict(select="between"), dict(threshold=np.nan), dict(threshold=True), dict(radii=0), dict(radii=256),
               dict(radii=[]), dict(radii=[1.0, np.inf]), dict(radii=[-1.0]), dict(radii=np.zeros((2, 2))),
               dict(radii=np.arange(300.0))):
        with pytest.raises(ValueError):
            PS.get_granulometry(f, 4.0, **kw)
        with pytest.raises(ValueError):
            PS.lightcone_granulometry(lc, 1.0, **kw)
    for per in ((True, True), (True,) * 4):
        with pytest.raises(ValueError):
            PS.get_granulometry(f, 4.0, periodic=per)
        with pytest.raises(ValueError):
            PS.get_distance_transform(f, 4.0, periodic=per)
    for call in (PS.get_granulometry, PS.get_distance_transform):
        with pytest.raises(ValueError):
            call(np.zeros((4, 4), np.float32), 4.0)
        with pytest.raises(ValueError):
            call(f, (4.0, 4.0))
        with pytest.raises(ValueError):
            call(f, (4.0, 4.0, 4.0 * (1 + 1e-6)))  # cells must be cubic
        with pytest.raises(ValueError):
            call(np.zeros((4, 4, 8), np.float32), 4.0)
    with pytest.raises(ValueError):
        PS.lightcone_granulometry(lc, 1.0, periodic=True)
    with pytest.raises(ValueError):
        PS.lightcone_granulometry(lc, 1.0, connectivity=6)
    with pytest.raises(ValueError):
        PS.lightcone_granulometry(lc, 0.0)
    with pytest.raises(ValueError):
        PS.lightcone_granulometry(lc, 1.0, chunk_length=13)
    API = importlib.import_module("21cmfast_amd.grid_api")
    for radii2 in ([1, 1], [4, 1], [-1], [0.5], np.arange(256), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            API.granulometry(f, (4, 4, 4), radii2)
    with pytest.raises(ValueError):
        API.granulometry(f, (4, 4, 8), [1])  # the box does not lie inside the field
    with pytest.raises(ValueError):
        API.granulometry(np.zeros(40000, np.float32), (1, 1, 2**15), [1], row_pitch=2**15)  # the 2^30 bound
