"""GPU: ``get_bubble_clusters`` / ``lightcone_bubble_clusters`` / ``grid_api.bubble_clusters``
against the numpy restatement ``tests/cluster_reference.py``.

Everything is an integer fixed by the mask, so everything is compared for equality: labels, roots, sizes, the four
stats and both histograms.  The shapes are the ones at which the kernels can go wrong (partial and tail mask words,
one-cell and two-cell periodic axes, a word boundary, many roots, one hot root), not the ones where the science lives.
"""

import ctypes as C
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cluster_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

PS = importlib.import_module("21cmfast_amd.powerspec")
API = importlib.import_module("21cmfast_amd.grid_api")
LIB = importlib.import_module("21cmfast_amd._lib")

VALUE_ERROR, NAN_ERROR = 3, 7
CONNECTIVITY = {1: 6, 2: 18, 3: 26}
# quantiles of a unit Gaussian: fills near 0.2, 0.3116 (the site-percolation threshold of the cubic lattice) and 0.6
THRESHOLDS = (-0.8416, -0.4914, 0.2533)
RANDOM_SHAPES = [(12, 10, 14), (16, 16, 64), (9, 7, 70), (8, 8, 130), (33, 31, 70)]
SIMPLE_CELLS = 2000  # label_simple up to here, label_fast beyond (the host tests hold the two to each other)


def make_field(shape, seed):
    """A correlated Gaussian field (a white one summed over the 7-point stencil, periodic), unit variance: the field
    of the bubble size tests"""
    g = np.random.default_rng(seed).standard_normal(shape)
    f = g.copy()
    for ax in range(3):
        f += np.roll(g, 1, ax) + np.roll(g, -1, ax)
    return (f / np.sqrt(7.0)).astype(np.float32)


def field_of(mask):
    """0 where the mask is set, 1 elsewhere: selected by the default threshold 0.5"""
    return np.where(mask, 0.0, 1.0).astype(np.float32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def reference(mask, c, per):
    fn = R.label_simple if mask.size <= SIMPLE_CELLS else R.label_fast
    return fn(mask, c, per)


def assert_matches(res, ref, edges=None):
    """a one-box result of get_bubble_clusters (labels and clusters asked for) against (labels, roots, sizes, stats)"""
    labels, roots, sizes, stats = ref
    got = [int(to_np(x)) for x in (res.n_selected, res.n_clusters, res.largest_cells, res.largest_root)]
    assert got == stats.tolist()
    lab = to_np(res.labels)
    assert lab.dtype == np.int32 and np.array_equal(lab, labels)
    assert to_np(res.roots).dtype == np.int64 and np.array_equal(to_np(res.roots), roots)
    assert np.array_equal(to_np(res.sizes), sizes)
    hist_n, hist_cells = R.histograms(sizes, to_np(res.edges) if edges is None else edges)
    assert np.array_equal(to_np(res.hist_n), hist_n) and np.array_equal(to_np(res.hist_cells), hist_cells)


def run(field, c, per, **kw):
    return PS.get_bubble_clusters(field, 1.0, connectivity=CONNECTIVITY[c], periodic=per, return_labels=True,
                                  return_clusters=True, **kw)


@functools.lru_cache(maxsize=None)
def random_field(shape):
    f = make_field(shape, 17)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("per", [(True, True, True), (True, True, False)], ids=["periodic", "open_z"])
@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_boxes(shape, c, per):
    f = random_field(shape)
    for t in THRESHOLDS:
        mask = R.select_mask(f, t)
        assert 0.1 < mask.mean() < 0.7
        assert_matches(run(f, c, per, threshold=t), reference(mask, c, per))
    # the other side of the threshold
    assert_matches(run(f, c, per, threshold=THRESHOLDS[1], select="above"),
                   reference(R.select_mask(f, THRESHOLDS[1], False), c, per))


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 1), (2, 2, 2), (1, 1, 130), (3, 1, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_degenerate_axes(shape, c):
    rng = np.random.default_rng(3)
    for mask in (np.ones(shape, bool), rng.random(shape) < 0.5, rng.random(shape) < 0.5):
        for per in (True, False, (True, False, True)):
            assert_matches(run(field_of(mask), c, per), R.label_simple(mask, c, per))


ADV = (16, 16, 64)


def serpentine():
    """One cell wide (two cells per row), through every row in boustrophedon order, z following a triangle wave:
    consecutive rows share one z, so the path is one chain from cell 0"""
    mask = np.zeros(ADV, bool)
    for k in range(ADV[0] * ADV[1]):
        x, y = divmod(k, ADV[1])
        if x % 2:
            y = ADV[1] - 1 - y
        s = k % 124
        s = s if s <= 62 else 124 - s
        mask[x, y, s:s + 2] = True
    return mask


def checkerboard():
    i, j, k = np.indices(ADV)
    return (i + j + k) % 2 == 0


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("name", ["serpentine", "serpentine_reversed", "checkerboard", "all", "none", "single"])
def test_adversarial_masks(name, c):
    n = int(np.prod(ADV))
    if name == "serpentine":
        mask = serpentine()
    elif name == "serpentine_reversed":
        mask = serpentine()[::-1, ::-1, ::-1].copy()
    elif name == "checkerboard":
        mask = checkerboard()
    elif name == "all":
        mask = np.ones(ADV, bool)
    elif name == "none":
        mask = np.zeros(ADV, bool)
    else:
        mask = np.zeros(ADV, bool)
        mask[5, 7, 63] = True
    for per in (False, True):
        ref = R.label_fast(mask, c, per)
        res = run(field_of(mask), c, per)
        assert_matches(res, ref)
        stats = ref[3].tolist()
        if name.startswith("serpentine"):
            assert stats[:3] == [512, 1, 512]
            assert stats[3] == (0 if name == "serpentine" else int(np.flatnonzero(mask.ravel())[0]))
        elif name == "checkerboard":
            assert stats == ([n // 2, n // 2, 1, 0] if c == 1 else [n // 2, 1, n // 2, 0])
        elif name == "all":
            assert stats == [n, 1, n, 0]
        elif name == "none":
            assert stats == [0, 0, 0, -1]
        else:
            assert stats == [1, 1, 1, (5 * 16 + 7) * 64 + 63]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_clusters_that_meet_only_through_a_wrap(axis):
    mask = np.zeros(ADV, bool)
    lo, hi = [3, 4, 5], [3, 4, 5]
    lo[axis], hi[axis] = 0, ADV[axis] - 1
    mask[tuple(lo)] = mask[tuple(hi)] = True
    for c in (1, 2, 3):
        per = [False] * 3
        res = run(field_of(mask), c, tuple(per))
        assert_matches(res, R.label_simple(mask, c, tuple(per)))
        assert int(res.n_clusters) == 2
        per[axis] = True
        res = run(field_of(mask), c, tuple(per))
        assert_matches(res, R.label_simple(mask, c, tuple(per)))
        assert int(res.n_clusters) == 1 and int(res.largest_cells) == 2
        # every axis but this one periodic: still two
        other = tuple(a != axis for a in range(3))
        assert int(run(field_of(mask), c, other).n_clusters) == 2


def test_edge_and_corner_contacts_across_a_word_boundary():
    shape = (8, 8, 130)
    for second, want in (((1, 2, 64), [2, 1, 1]), ((2, 2, 64), [2, 2, 1]), ((1, 1, 64), [1, 1, 1])):
        mask = np.zeros(shape, bool)
        mask[1, 1, 63] = mask[second] = True
        for c in (1, 2, 3):
            res = run(field_of(mask), c, True)
            assert_matches(res, R.label_fast(mask, c, True))
            assert int(res.n_clusters) == want[c - 1]


BIG = (160, 144, 200)
# scipy.ndimage.label of the mask below, nothing periodic: clusters and the largest one, per connectivity
BIG_SELECTED = 1436926
BIG_KNOWN = {1: (247232, 60527), 2: (2442, 1434064), 3: (200, 1436693)}


@functools.lru_cache(maxsize=None)
def big_mask():
    mask = np.random.default_rng(7).random(BIG) < 0.3116
    mask.setflags(write=False)
    return mask


@pytest.mark.parametrize("per", [False, True], ids=["open", "periodic"])
@pytest.mark.parametrize("c", [1, 2, 3])
def test_one_larger_box(c, per):
    """white noise at the percolation threshold: many roots at 6, one hot root at 18 and 26"""
    mask = big_mask()
    ref = R.label_fast(mask, c, per)
    assert ref[3][0] == mask.sum()
    res = run(field_of(mask), c, per)
    assert_matches(res, ref)
    if not per and int(mask.sum()) == BIG_SELECTED:  # the generator gave the mask the figures were recorded for
        assert (int(res.n_clusters), int(res.largest_cells)) == BIG_KNOWN[c]


@pytest.mark.parametrize("c", [1, 3])
def test_lightcone_chunks(c):
    lc = make_field((16, 16, 111), 23)
    t = THRESHOLDS[1]
    res = PS.lightcone_bubble_clusters(lc, 1.5, chunk_length=37, threshold=t, connectivity=CONNECTIVITY[c],
                                       return_labels=True, return_clusters=True, bins=12)
    assert res.chunk_starts.tolist() == [0, 37, 74]
    assert res.labels.shape == (3, 16, 16, 37)
    counts = []
    for i, s in enumerate(res.chunk_starts):
        mask = R.select_mask(lc[:, :, s:s + 37], t)
        labels, roots, sizes, stats = R.label_fast(mask, c, (True, True, False))
        k = roots.size
        counts.append(k)
        assert np.array_equal(res.labels[i], labels)
        assert [int(res.n_selected[i]), int(res.n_clusters[i]), int(res.largest_cells[i]),
                int(res.largest_root[i])] == stats.tolist()
        assert np.array_equal(res.roots[i, :k], roots) and np.array_equal(res.sizes[i, :k], sizes)
        assert np.all(res.roots[i, k:] == -1) and np.all(res.sizes[i, k:] == 0)
        hist_n, hist_cells = R.histograms(sizes, res.edges)
        assert np.array_equal(res.hist_n[i], hist_n) and np.array_equal(res.hist_cells[i], hist_cells)
        assert res.filling_fraction[i] == stats[0] / mask.size
        assert res.largest_fraction[i] == stats[2] / stats[0]
        assert np.array_equal(res.volumes[i], res.sizes[i] * 1.5 ** 3)
    assert res.roots.shape == (3, max(counts)) and len(set(counts)) > 1


def test_capacity(monkeypatch):
    f = random_field((9, 7, 70))
    t = THRESHOLDS[0]
    mask = R.select_mask(f, t)
    labels, roots, sizes, stats = reference(mask, 1, True)
    n = roots.size
    assert n > 8
    edges = PS.cluster_edges(f.shape)
    for cap in (1, n, n + 5):
        out = API.bubble_clusters(f, f.shape, edges, threshold=t, max_clusters=cap)
        assert len(out) == 5
        assert out[2][0].tolist() == stats.tolist()  # the true count whatever the capacity
        k = min(cap, n)
        assert out[3].shape == (1, cap) and out[3].dtype == np.int64 and out[4].dtype == np.int64
        assert np.array_equal(out[3][0, :k], roots[:k]) and np.array_equal(out[4][0, :k], sizes[:k])
        assert np.all(out[3][0, k:] == -1) and np.all(out[4][0, k:] == 0)
    # more clusters than the first call makes room for: the second call
    calls = []
    real = API.bubble_clusters

    def counted(*a, **kw):
        calls.append(kw["max_clusters"])
        return real(*a, **kw)

    monkeypatch.setattr(PS, "CLUSTER_DEFAULT_CAPACITY", 8)
    monkeypatch.setattr(API, "bubble_clusters", counted)
    res = PS.get_bubble_clusters(f, 1.0, threshold=t, return_clusters=True)
    assert calls == [8, n]
    assert np.array_equal(res.roots, roots) and np.array_equal(res.sizes, sizes)
    # an explicit capacity: one call, the first clusters
    del calls[:]
    res = PS.get_bubble_clusters(f, 1.0, threshold=t, return_clusters=True, max_clusters=3)
    assert calls == [3] and np.array_equal(res.roots, roots[:3]) and int(res.n_clusters) == n


def test_the_most_bins_and_bins_that_leave_sizes_out():
    f = random_field((16, 16, 64))
    t = THRESHOLDS[0]
    sizes, stats = reference(R.select_mask(f, t), 1, True)[2:]
    assert sizes.max() > 40 and sizes.min() == 1
    for edges in (np.arange(1, 4098), np.array([2, 3, 40]), np.array([1, 2**40])):  # 4096 bins; sizes below and above
        hist_n, hist_cells, got = API.bubble_clusters(f, f.shape, edges, threshold=t)
        want_n, want_cells = R.histograms(sizes, edges)
        assert hist_n.shape == (1, len(edges) - 1)
        assert np.array_equal(hist_n[0], want_n) and np.array_equal(hist_cells[0], want_cells)
        assert got[0].tolist() == stats.tolist()


def test_same_bytes_twice_and_from_the_device():
    import torch

    f = random_field((33, 31, 70))
    kw = dict(threshold=THRESHOLDS[1], connectivity=2, periodic=(True, False, True), return_labels=True,
              max_clusters=4096)
    edges = PS.cluster_edges(f.shape, 16)
    a = API.bubble_clusters(f, f.shape, edges, **kw)
    b = API.bubble_clusters(f, f.shape, edges, **kw)
    d = API.bubble_clusters(torch.from_numpy(np.array(f)).cuda(), f.shape, edges, **kw)
    assert len(a) == len(b) == len(d) == 6
    for x, y, z in zip(a, b, d):
        assert isinstance(x, np.ndarray) and z.is_cuda
        assert same_bits(x, y) and same_bits(x, z)
    kw["return_labels"], kw["max_clusters"] = False, 0
    plain = API.bubble_clusters(f, f.shape, edges, **kw)
    assert len(plain) == 3
    for x, y in zip(plain, a[:3]):
        assert same_bits(x, y)
    # the high-level entry keeps a device field's results on the device
    res = PS.get_bubble_clusters(torch.from_numpy(np.array(f)).cuda(), 70.0, threshold=THRESHOLDS[1],
                                 connectivity=18, periodic=(True, False, True), return_labels=True,
                                 return_clusters=True)
    assert res.labels.is_cuda and res.volume_fraction.is_cuda and res.volumes.is_cuda
    assert same_bits(res.labels.reshape(1, -1), a[3])
    n = int(a[2][0, 1])
    assert same_bits(res.roots, a[4][0, :n])


SENTINEL = -77


def raw_call(field_ptr, shape, *, n_batch=1, row_pitch=None, offsets=(0,), threshold=0.5, select_below=1,
             connectivity=1, periodic_mask=7, edges=(1, 2, 100), hist_n=True, hist_cells=True, stats=True,
             labels=False, max_clusters=0, roots=False, sizes=False, null_edges=False, null_offsets=False):
    """the C entry with nothing checked on the way: (status, the output arrays, pre-filled with SENTINEL)"""
    lib = LIB.load()
    nx, ny, nz = shape
    edges = np.asarray(edges, np.int64)
    n_bins = len(edges) - 1
    offsets = np.asarray(offsets, np.int64)
    small = nx * ny * nz < 2**20
    out = {}
    for name, want, n, dtype in (("hist_n", hist_n, max(n_bins, 1), np.int64),
                                 ("hist_cells", hist_cells, max(n_bins, 1), np.int64), ("stats", stats, 4, np.int64),
                                 ("labels", labels, nx * ny * nz if small else 1, np.int32),
                                 ("roots", roots, max(max_clusters, 1), np.int64),
                                 ("sizes", sizes, max(max_clusters, 1), np.int64)):
        out[name] = np.full((max(n_batch, 1), n), SENTINEL, dtype) if want else None

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    status = lib.c21cm_bubble_clusters_grids(
        field_ptr, nx, ny, nz, n_batch, nz if row_pitch is None else row_pitch,
        None if null_offsets else ptr(offsets), threshold, select_below, connectivity, periodic_mask, n_bins,
        None if null_edges else ptr(edges), ptr(out["hist_n"]), ptr(out["hist_cells"]), ptr(out["stats"]),
        ptr(out["labels"]), max_clusters, ptr(out["roots"]), ptr(out["sizes"]), None)
    return status, out


def untouched(out):
    return all(v is None or np.all(v == SENTINEL) for v in out.values())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_writes_nothing(bad):
    f = np.array(random_field((12, 10, 14)))
    f[7, 3, 13] = bad
    status, out = raw_call(f.ctypes.data_as(C.c_void_p), f.shape, labels=True, max_clusters=50, roots=True, sizes=True)
    assert status == NAN_ERROR and "not finite" in LIB.last_error()
    assert untouched(out)
    with pytest.raises(LIB.BackendError) as err:
        PS.get_bubble_clusters(f, 1.0)
    assert err.value.code == NAN_ERROR
    # and the next call is clean
    f[7, 3, 13] = 0.0
    status, out = raw_call(f.ctypes.data_as(C.c_void_p), f.shape, labels=True)
    assert status == 0 and not untouched(out)
    assert np.array_equal(out["labels"].reshape(f.shape), R.label_simple(R.select_mask(f, 0.5), 1, True)[0])


def test_argument_errors_of_the_c_entry():
    """every check comes before any access: the field is a pointer nothing may follow"""
    fake = C.c_void_p(0x1000)
    ok = (4, 4, 4)
    cases = [
        dict(shape=(1, 2, 2**30)),  # nx ny nz = 2^31
        dict(shape=(2**16, 2**16, 1)),
        dict(shape=(0, 4, 4)), dict(shape=(4, 4, -1)),
        dict(roots=True, max_clusters=4), dict(sizes=True, max_clusters=4),  # only one of the cluster arrays
        dict(roots=True, sizes=True, max_clusters=0), dict(roots=True, sizes=True, max_clusters=-1),
        dict(n_batch=0), dict(n_batch=65536, offsets=np.zeros(65536, np.int64)),
        dict(row_pitch=3), dict(offsets=(-1,)),
        dict(threshold=float("nan")), dict(threshold=float("inf")),
        dict(connectivity=0), dict(connectivity=4), dict(periodic_mask=-1), dict(periodic_mask=8),
        dict(edges=(1,)), dict(edges=np.arange(1, 4099)), dict(edges=(1, 5, 5)), dict(edges=(3, 2)),
        dict(edges=(0, 2)),
        dict(hist_n=False), dict(hist_cells=False), dict(stats=False), dict(null_edges=True),
        dict(null_offsets=True),
    ]
    for kw in cases:
        shape = kw.pop("shape", ok)
        status, out = raw_call(fake, shape, **kw)
        assert status == VALUE_ERROR, kw
        assert LIB.last_error().startswith("bubble clusters:"), kw
        assert untouched(out), kw
    status, out = raw_call(None, ok)
    assert status == VALUE_ERROR and untouched(out)
