"""Host checks of the friends-of-friends cluster estimator (no GPU): the numpy restatement
``tests/cluster_reference.py`` -- the spec of the device code -- pinned to answers it cannot influence: its plain
union-find against scipy's labelling, invariance under shifts of a periodic box, and masks whose clusters are known;
and the argument errors ``21cmfast_amd/powerspec.py`` raises before the library is loaded.
"""

import importlib
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cluster_reference as R  # noqa: E402

PS = importlib.import_module("21cmfast_amd.powerspec")
LIB = importlib.import_module("21cmfast_amd._lib")

PERIODIC = list(itertools.product((False, True), repeat=3))


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


@pytest.mark.parametrize("shape", [(7, 5, 9), (4, 1, 6), (2, 2, 2)])
@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_simple_equals_fast(shape, connectivity):
    rng = np.random.default_rng(sum(shape) + connectivity)
    for fill in (0.2, 0.35, 0.7):
        mask = rng.random(shape) < fill
        for per in PERIODIC:
            assert same(R.label_simple(mask, connectivity, per), R.label_fast(mask, connectivity, per)), (fill, per)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_fast_without_periodic_axes_is_scipys_partition(connectivity):
    mask = np.random.default_rng(5).random((11, 9, 13)) < 0.3
    labels, roots, sizes, stats = R.label_fast(mask, connectivity, False)
    lab, n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, connectivity))
    assert stats[1] == n == roots.size and stats[0] == mask.sum()
    # the same partition: a one-to-one map between the two namings
    pairs = np.unique(np.stack([labels[mask], lab[mask]], axis=1), axis=0)
    assert len(pairs) == n and len(np.unique(pairs[:, 0])) == n and len(np.unique(pairs[:, 1])) == n
    assert np.all(labels[~mask] == -1)
    # a root is the smallest flat index of its cluster
    flat = labels.ravel()
    assert np.array_equal(roots, np.flatnonzero(flat == np.arange(flat.size)))
    assert np.array_equal(np.sort(sizes), np.sort(np.bincount(lab[mask])[1:]))


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_sizes_are_invariant_under_rolls_of_a_periodic_box(connectivity):
    mask = np.random.default_rng(8).random((6, 7, 5)) < 0.3
    want = np.sort(R.label_simple(mask, connectivity, True)[2])
    for shift in ((1, 0, 0), (0, 3, 0), (0, 0, 2), (5, 6, 4)):
        got = R.label_simple(np.roll(mask, shift, (0, 1, 2)), connectivity, True)[2]
        assert np.array_equal(np.sort(got), want)


def test_checkerboard():
    shape = (4, 6, 8)
    i, j, k = np.indices(shape)
    mask = (i + j + k) % 2 == 0
    n = mask.size
    for fn in (R.label_simple, R.label_fast):
        for per in (True, False):
            labels, roots, sizes, stats = fn(mask, 1, per)
            assert stats.tolist() == [n // 2, n // 2, 1, 0] and np.all(sizes == 1)
            assert np.array_equal(roots, np.flatnonzero(mask.ravel()))
            for c in (2, 3):
                assert fn(mask, c, per)[3].tolist() == [n // 2, 1, n // 2, 0]


def test_edge_and_corner_contacts():
    edge = np.zeros((4, 4, 4), bool)
    edge[1, 1, 1] = edge[1, 2, 2] = True
    corner = np.zeros((4, 4, 4), bool)
    corner[1, 1, 1] = corner[2, 2, 2] = True
    for fn in (R.label_simple, R.label_fast):
        assert [int(fn(edge, c, True)[3][1]) for c in (1, 2, 3)] == [2, 1, 1]
        assert [int(fn(corner, c, True)[3][1]) for c in (1, 2, 3)] == [2, 2, 1]


def test_slabs_at_the_two_ends_join_through_the_wrap():
    mask = np.zeros((3, 3, 8), bool)
    mask[:, :, 0] = mask[:, :, -1] = True
    for fn in (R.label_simple, R.label_fast):
        labels, roots, sizes, stats = fn(mask, 1, (False, False, True))
        assert stats.tolist() == [18, 1, 18, 0] and roots.tolist() == [0] and sizes.tolist() == [18]
        assert np.all(labels[mask] == 0)
        labels, roots, sizes, stats = fn(mask, 1, (True, True, False))
        assert stats.tolist() == [18, 2, 9, 0] and roots.tolist() == [0, 7] and sizes.tolist() == [9, 9]


def test_all_and_none_selected():
    for fn in (R.label_simple, R.label_fast):
        labels, roots, sizes, stats = fn(np.ones((3, 4, 5), bool), 1, True)
        assert stats.tolist() == [60, 1, 60, 0] and roots.tolist() == [0] and np.all(labels == 0)
        labels, roots, sizes, stats = fn(np.zeros((3, 4, 5), bool), 3, True)
        assert stats.tolist() == [0, 0, 0, -1] and roots.size == 0 and sizes.size == 0 and np.all(labels == -1)


def test_histograms():
    hist_n, hist_cells = R.histograms([1, 1, 2, 5, 9, 10], [1, 2, 5, 10])
    assert hist_n.tolist() == [2, 1, 2] and hist_cells.tolist() == [2, 2, 14]


def test_default_edges_and_argument_errors(monkeypatch):
    e = PS.cluster_edges((8, 8, 16))
    assert e.dtype == np.int64
    assert np.array_equal(e, np.unique(np.ceil(np.geomspace(1, 1025, 33))).astype(np.int64))
    assert e[0] == 1 and e[-1] == 1025 and len(e) < 33  # the first log steps collapse onto the same integers
    assert np.array_equal(PS.cluster_edges((2, 2, 2), 4, False), [1, 3, 5, 7, 9])
    assert np.array_equal(PS.cluster_edges((2, 2, 2), np.array([1, 2, 9])), [1, 2, 9])

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(LIB, "load", no_library)
    monkeypatch.setattr(importlib.import_module("21cmfast_amd.grid_api"), "load", no_library)
    f = np.zeros((4, 4, 4), np.float32)
    for kw in (dict(connectivity=4), dict(select="between"), dict(threshold=np.nan), dict(periodic=(True, True)),
               dict(bins=np.array([4, 2, 1])), dict(bins=np.array([0, 2])), dict(bins=np.arange(1, 4099)),
               dict(max_clusters=0)):
        with pytest.raises(ValueError):
            PS.get_bubble_clusters(f, 4.0, **kw)
        with pytest.raises(ValueError):
            PS.lightcone_bubble_clusters(np.zeros((4, 4, 12), np.float32), 1.0, **kw)
    with pytest.raises(ValueError):
        PS.get_bubble_clusters(np.zeros((4, 4)), 4.0)
    with pytest.raises(ValueError):
        PS.lightcone_bubble_clusters(np.zeros((4, 4, 12), np.float32), 1.0, periodic=True)
    with pytest.raises(ValueError):
        PS.lightcone_bubble_clusters(np.zeros((4, 4, 12), np.float32), 1.0, n_rays=10)
