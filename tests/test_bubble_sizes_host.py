"""Host checks of the mean-free-path bubble size estimator (no GPU): the numpy restatement
``tests/bubble_reference.py`` -- the spec of the device code -- pinned to answers it cannot influence: ray-box exit
distances of a cuboid, the closed-form chord distribution of a slab, the start cells, and line-of-sight chords; and the
argument errors ``21cmfast_amd/powerspec.py`` raises before the library is loaded.

The slab: a plane-parallel selected layer of thickness w, a start uniform in it, an isotropic direction.  The path to
the face is z' / |mu| with z' uniform on (0, w) and |mu| uniform on (0, 1), so P(L > l) = E[max(0, 1 - l |mu| / w)] =
1 - l / (2 w) for l <= w and w / (2 l) beyond.
"""

import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bubble_reference as R  # noqa: E402

PS = importlib.import_module("21cmfast_amd.powerspec")


@functools.lru_cache(maxsize=None)
def cuboid_reference():
    res = R.trace(R.cuboid_mask(), R.cuboid_lengths(), R.CUBOID_RAYS, R.CUBOID_SEED, max_length=100.0)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def test_cuboid_rays_end_at_the_box_exit():
    R.check_cuboid(cuboid_reference())


def test_slab_follows_the_closed_form():
    res = R.trace(R.slab_mask(), R.SLAB_SHAPE, R.SLAB_RAYS, R.SLAB_SEED, max_length=R.SLAB_MAX)
    R.check_slab(res["lengths"], res["flags"], float(R.SLAB_Z[1] - R.SLAB_Z[0]), R.SLAB_MAX, R.SLAB_RAYS)


def test_start_cells_are_the_kth_selected():
    rng = np.random.default_rng(3)
    mask = rng.random((7, 5, 9)) < 0.05
    n = 5000
    res = R.trace(mask, (7.0, 5.0, 9.0), n, seed=11, box_index=2)
    u_cell = R.draws(n, 11, 2)[0]
    sel = np.flatnonzero(mask)
    k = np.minimum((u_cell * sel.size).astype(np.int64), sel.size - 1)
    assert np.array_equal(res["starts"], sel[k])
    # uniform over the selected cells: every one is hit, none outside
    assert set(np.unique(res["starts"])) == set(sel)
    # the start point lies in the start cell
    idx = np.stack(np.unravel_index(res["starts"], mask.shape), axis=1)
    assert np.all(np.floor(res["p0"]) == idx)


def test_los_chords_are_the_distance_to_the_slab_face():
    n = 4000
    res = R.trace(R.slab_mask(), R.SLAB_SHAPE, n, seed=5, directions="los", max_length=R.SLAB_MAX)
    z = res["p0"][:, 2]
    up = res["d"][:, 2] > 0
    assert np.all(np.abs(res["d"][:, 2]) == 1.0) and np.all(res["d"][:, :2] == 0.0)
    assert 0.4 < up.mean() < 0.6
    want = np.where(up, R.SLAB_Z[1] - z, z - R.SLAB_Z[0])
    assert np.all(res["flags"] == R.ENDED)
    assert np.array_equal(res["lengths"], want)


def test_no_selected_cell_and_all_selected():
    res = R.trace(np.zeros((4, 4, 4), bool), (4.0, 4.0, 4.0), 10)
    assert np.all(np.isnan(res["lengths"])) and np.all(res["flags"] == R.NO_CELL) and np.all(res["starts"] == -1)
    assert np.array_equal(R.stats(res), [0, 0, 0, 0])
    res = R.trace(np.ones((4, 4, 4), bool), (4.0, 4.0, 4.0), 100)
    assert np.all(res["flags"] == R.CAPPED) and np.all(res["lengths"] == 4.0)
    res = R.trace(np.ones((4, 4, 4), bool), (4.0, 4.0, 4.0), 100, periodic=(True, True, False), max_length=50.0)
    # a ray leaves through a z face, or is too flat to get there within max_length
    want = R.aabb_exit(res["p0"], res["d"], np.array([-np.inf, -np.inf, 0.0]), np.array([np.inf, np.inf, 4.0]))
    esc = want < 50.0
    assert esc.sum() > 90
    assert np.array_equal(res["flags"], np.where(esc, R.ESCAPED, R.CAPPED))
    assert np.allclose(res["lengths"], np.where(esc, want, 50.0), rtol=1e-12, atol=0)


def test_a_ray_does_not_depend_on_n_rays():
    mask = np.random.default_rng(1).random((9, 7, 11)) < 0.5
    a = R.trace(mask, (9.0, 7.0, 11.0), 50, seed=4)
    b = R.trace(mask, (9.0, 7.0, 11.0), 500, seed=4)
    for key in ("lengths", "flags", "starts"):
        assert np.array_equal(a[key], b[key][:50])


def test_default_edges_and_argument_errors():
    e = PS.bubble_edges((8, 8, 16), (8.0, 16.0, 16.0), 10, True, 16.0)
    assert np.array_equal(e, np.geomspace(1.0, 16.0, 11))
    e = PS.bubble_edges((8, 8, 16), 16.0, 4, False, 8.0)
    assert np.array_equal(e, np.linspace(1.0, 8.0, 5))
    f = np.zeros((4, 4, 4), np.float32)
    for kw in (dict(n_rays=0), dict(n_rays=2**31), dict(max_length=0.0), dict(max_length=np.inf),
               dict(bins=np.array([1.0, 0.5])), dict(bins=np.array([-1.0, 2.0])), dict(select="between"),
               dict(directions="up"), dict(periodic=(True, True)), dict(threshold=np.nan), dict(seed=-1)):
        with pytest.raises(ValueError):
            PS.get_bubble_sizes(f, 4.0, **kw)
    with pytest.raises(ValueError):
        PS.get_bubble_sizes(np.zeros((4, 4)), 4.0)
    with pytest.raises(ValueError):
        PS.lightcone_bubble_sizes(np.zeros((4, 4, 12), np.float32), 1.0, periodic=True)
