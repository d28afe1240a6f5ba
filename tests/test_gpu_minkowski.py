"""GPU: ``get_minkowski_functionals`` / ``lightcone_minkowski_functionals`` / ``grid_api.minkowski`` (DESIGN section
4.11) against the numpy restatement ``tests/minkowski_reference.py``, which takes one mask per threshold where the
device code takes every threshold from one pass over the levels of the cells.

Everything is an integer fixed by the field, so everything is compared for equality.  The shapes are the ones at which
the kernel can go wrong (a z range that ends inside a wave, at its end, and one cell past it; fewer rows than a
workgroup holds and more; more than one x segment; one-cell and two-cell periodic axes), not the ones where the
science lives.
"""

import ctypes as C
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import minkowski_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

PS = importlib.import_module("21cmfast_amd.powerspec")
API = importlib.import_module("21cmfast_amd.grid_api")
LIB = importlib.import_module("21cmfast_amd._lib")

VALUE_ERROR, NAN_ERROR = 3, 7
THRESHOLDS = [-0.8416, -0.4914, 0.0, 0.2533, 1.2]
RANDOM_SHAPES = [(12, 10, 14), (16, 16, 64), (9, 7, 70), (8, 8, 130), (33, 31, 70)]
PERIODIC = {"periodic": (True, True, True), "open_z": (True, True, False), "open": (False, False, False),
            "open_y": (True, False, True)}
ADV = (16, 16, 64)


def make_field(shape, seed):
    """A correlated Gaussian field (a white one summed over the 7-point stencil, periodic), unit variance: the field
    of the bubble size tests"""
    g = np.random.default_rng(seed).standard_normal(shape)
    f = g.copy()
    for ax in range(3):
        f += np.roll(g, 1, ax) + np.roll(g, -1, ax)
    return (f / np.sqrt(7.0)).astype(np.float32)


def field_of(mask):
    """0 where the mask is set, 1 elsewhere: selected below the threshold 0.5"""
    return np.where(mask, 0.0, 1.0).astype(np.float32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def random_field(shape):
    f = make_field(shape, 17)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def tied_field(shape):
    f = (np.round(random_field(shape) * 4) / 4).astype(np.float32)
    f.setflags(write=False)
    return f


def assert_rows(got, field, thresholds, below, per):
    got = to_np(got)
    assert got.dtype == np.int64 and got.shape == (len(thresholds), 8)
    for i, t in enumerate(thresholds):
        want = R.counts(R.select_mask(field, t, below), per)
        assert got[i].tolist() == want.tolist(), (i, t)


@pytest.mark.parametrize("select", ["below", "above"])
@pytest.mark.parametrize("per", list(PERIODIC), ids=list(PERIODIC))
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_boxes(shape, per, select):
    f = random_field(shape)
    res = PS.get_minkowski_functionals(f, 1.0, thresholds=THRESHOLDS, select=select, periodic=PERIODIC[per])
    assert_rows(res.counts, f, THRESHOLDS, select == "below", PERIODIC[per])
    assert 0.1 < float(res.v0[0 if select == "below" else 3]) < 0.7


@pytest.mark.parametrize("select", ["below", "above"])
@pytest.mark.parametrize("per", list(PERIODIC), ids=list(PERIODIC))
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ties(shape, per, select):
    f = tied_field(shape)
    t = [-1.0, -0.5, 0.0, 0.25, 1.25]
    assert all(np.any(f == np.float32(x)) for x in t)
    res = PS.get_minkowski_functionals(f, 1.0, thresholds=t, select=select, periodic=PERIODIC[per])
    assert_rows(res.counts, f, t, select == "below", PERIODIC[per])


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 5, 1), (2, 2, 2), (1, 1, 130), (3, 1, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_degenerate_axes(shape):
    rng = np.random.default_rng(3)
    for mask in (np.ones(shape, bool), rng.random(shape) < 0.5, rng.random(shape) < 0.5):
        for per in (True, False, (True, False, True)):
            for select, m in (("below", mask), ("above", ~mask)):
                res = PS.get_minkowski_functionals(field_of(mask), 1.0, thresholds=[0.5], select=select, periodic=per)
                assert to_np(res.counts)[0].tolist() == R.counts(m, per).tolist(), (per, select)


@pytest.mark.parametrize("shape", [(1, 33000, 3), (70, 530, 66)], ids=lambda s: "x".join(map(str, s)))
def test_many_tiles(shape):
    """a workgroup takes a tile of 32 x 16 x 64 sites at a time and a launch has at most 2048 workgroups per box: a
    box of 2063 tiles, so that workgroups take a second one, and one of 3 x 34 x 2 tiles cut short on every axis"""
    f = make_field(shape, 5)
    for per in ((True, True, True), (False, False, False)):
        got = API.minkowski(f, shape, THRESHOLDS[1:4], periodic=per)
        assert_rows(got[0], f, THRESHOLDS[1:4], True, per)


def test_threshold_counts():
    f = random_field(ADV)
    for below in (True, False):
        one = API.minkowski(f, ADV, [0.1], select_below=below)
        assert one.shape == (1, 1, 8)
        assert_rows(one[0], f, [0.1], below, True)
        many = PS.minkowski_thresholds(f, 255)
        full = API.minkowski(f, ADV, many, select_below=below, periodic=(True, False, True))
        assert full.shape == (1, 255, 8)
        pick = [0, 1, 63, 127, 128, 200, 254]
        part = API.minkowski(f, ADV, many[pick], select_below=below, periodic=(True, False, True))
        assert np.array_equal(part[0], full[0, pick])  # a row does not depend on the other thresholds
        assert_rows(part[0], f, many[pick], below, (True, False, True))
        # a set grows with the threshold below, shrinks above
        assert np.all(np.diff(full[0], axis=0) * (1 if below else -1) >= 0)
    # thresholds outside the field's range: the empty and the full set
    lo, hi = float(f.min()) - 1.0, float(f.max()) + 1.0
    n = f.size
    for per, full_row in ((True, [n, n, n, n, n, n, n, n]), (False, R.counts(np.ones(ADV, bool), False).tolist())):
        got = API.minkowski(f, ADV, [lo - 1.0, lo, hi, hi + 1.0], select_below=True, periodic=(per,) * 3)[0]
        assert got.tolist() == [[0] * 8, [0] * 8, full_row, full_row]
        got = API.minkowski(f, ADV, [lo - 1.0, lo, hi, hi + 1.0], select_below=False, periodic=(per,) * 3)[0]
        assert got.tolist() == [full_row, full_row, [0] * 8, [0] * 8]


KNOWN = R.known_shapes()


@pytest.mark.parametrize("case", KNOWN, ids=[c[0] for c in KNOWN])
def test_known_shapes(case):
    name, mask, per, want, chi, n0 = case
    res = PS.get_minkowski_functionals(field_of(mask), 2.0, thresholds=[0.5], periodic=per)
    got = to_np(res.counts)[0]
    assert got.tolist() == R.counts(mask, per).tolist()
    if want is not None:
        assert got.tolist() == want
    assert int(res.euler_characteristic[0]) == chi and float(res.genus[0]) == 1.0 - chi / 2.0
    if n0 is not None:
        assert int(got[7]) == n0
    # the complement from the other side of the threshold
    res = PS.get_minkowski_functionals(field_of(mask), 2.0, thresholds=[0.5], select="above", periodic=per)
    assert to_np(res.counts)[0].tolist() == R.counts(~mask, per).tolist()


@pytest.mark.parametrize("name", ["checkerboard", "constant", "ramp"])
def test_adversarial_for_the_aggregation(name):
    i, j, k = np.indices(ADV)
    if name == "checkerboard":  # two values: every lane of a wave adds to one of two counters
        f = ((i + j + k) % 2).astype(np.float32)
        t = np.array([0.5])
    elif name == "constant":  # one counter per element kind
        f = np.full(ADV, 0.25, np.float32)
        t = np.array([0.0, 0.25, 0.5])
    else:  # a different level in every cell of a wave
        f = (k * 4 + (i + j) % 4).astype(np.float32)
        t = np.arange(255) + 0.5
        assert len(np.unique(R.levels(f, t)[3, 5])) == 64
    for per in (True, False):
        for below in (True, False):
            got = API.minkowski(f, ADV, t, select_below=below, periodic=(per,) * 3)[0]
            rows = range(len(t)) if len(t) < 10 else (0, 1, 2, 100, 127, 128, 253, 254)
            for r in rows:
                assert got[r].tolist() == R.counts(R.select_mask(f, t[r], below), per).tolist(), (per, below, r)


@pytest.mark.parametrize("select", ["below", "above"])
@pytest.mark.parametrize("per", [(True, True, True), (True, False, True)], ids=["periodic", "open_y"])
def test_n3_is_the_cluster_code_n_selected(per, select):
    f = random_field((9, 7, 70))
    res = PS.get_minkowski_functionals(f, 1.0, thresholds=THRESHOLDS, select=select, periodic=per)
    for i, t in enumerate(THRESHOLDS):
        cl = PS.get_bubble_clusters(f, 1.0, threshold=t, select=select, periodic=per)
        assert int(res.counts[i, 0]) == int(cl.n_selected)


def test_lightcone_chunks():
    lc = make_field((8, 8, 150), 23)
    starts = np.array([0, 20, 37, 110])
    z = np.linspace(6.0, 9.0, 150)
    res = PS.lightcone_minkowski_functionals(lc, 1.5, chunk_length=40, chunk_starts=starts, redshifts=z,
                                             thresholds=THRESHOLDS, select="above")
    assert res.chunk_starts.tolist() == starts.tolist() and res.redshifts.shape == (4,)
    assert res.counts.shape == (4, 5, 8) and res.v2.shape == (4, 5) and res.n_cells == 8 * 8 * 40
    for i, s in enumerate(starts):
        chunk = np.ascontiguousarray(lc[:, :, s:s + 40])
        one = PS.get_minkowski_functionals(chunk, (12.0, 12.0, 60.0), thresholds=THRESHOLDS, select="above",
                                           periodic=(True, True, False))
        assert_rows(res.counts[i], chunk, THRESHOLDS, False, (True, True, False))
        for name in ("counts", "euler_characteristic", "genus", "v0", "v1", "v2", "v3"):
            assert same_bits(getattr(res, name)[i], getattr(one, name)), name
        want = R.functionals(res.counts[i], (8, 8, 40), (12.0, 12.0, 60.0))
        np.testing.assert_allclose(res.v1[i], want["v1"], rtol=1e-14)
        np.testing.assert_allclose(res.v2[i], want["v2"], rtol=1e-14, atol=1e-18)
        np.testing.assert_allclose(res.v3[i], want["v3"], rtol=1e-14, atol=1e-18)
        assert np.array_equal(res.euler_characteristic[i], want["chi"])
    # an integer is resolved once over the whole lightcone
    auto = PS.lightcone_minkowski_functionals(lc, 1.5, chunk_length=40, chunk_starts=starts, thresholds=7)
    assert np.array_equal(auto.thresholds, PS.minkowski_thresholds(lc, 7)) and auto.counts.shape == (4, 7, 8)


def test_placement_and_determinism():
    import torch

    f = random_field((33, 31, 70))
    t = PS.minkowski_thresholds(f, 32)
    kw = dict(select_below=False, periodic=(True, False, True))
    a = API.minkowski(f, f.shape, t, **kw)
    b = API.minkowski(f, f.shape, t, **kw)
    d_f = torch.from_numpy(np.array(f)).cuda()
    d = API.minkowski(d_f, f.shape, t, **kw)
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and d.is_cuda and d.dtype == torch.int64
    assert same_bits(a, b) and same_bits(a, d)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        e = API.minkowski(d_f, f.shape, t, stream=stream.cuda_stream, **kw)
    stream.synchronize()
    assert same_bits(a, e)
    # the high-level entry keeps a device field's results on the device, in fp64 from the integer counts
    res = PS.get_minkowski_functionals(d_f, (33.0, 62.0, 35.0), thresholds=t, select="above",
                                       periodic=(True, False, True))
    host = PS.get_minkowski_functionals(f, (33.0, 62.0, 35.0), thresholds=t, select="above",
                                        periodic=(True, False, True))
    for name in ("counts", "euler_characteristic", "genus", "v0", "v1", "v2", "v3"):
        x = getattr(res, name)
        assert x.is_cuda and x.dtype == (torch.int64 if name in ("counts", "euler_characteristic") else torch.float64)
        assert same_bits(x, getattr(host, name)), name
    assert same_bits(res.counts, a[0])
    want = R.functionals(a[0], f.shape, (33.0, 62.0, 35.0))
    for name in ("v0", "v1", "v2", "v3"):
        np.testing.assert_allclose(getattr(host, name), want[name], rtol=1e-14, atol=1e-18)


SENTINEL = -77


def raw_call(field_ptr, shape, *, n_batch=1, row_pitch=None, offsets=(0,), thresholds=(0.25, 0.5), n_thresholds=None,
             select_below=1, periodic_mask=7, counts=True, null_thresholds=False, null_offsets=False):
    """the C entry with nothing checked on the way: (status, counts pre-filled with SENTINEL)"""
    lib = LIB.load()
    nx, ny, nz = shape
    thresholds = np.asarray(thresholds, np.float64)
    n_thr = len(thresholds) if n_thresholds is None else n_thresholds
    offsets = np.asarray(offsets, np.int64)
    out = np.full((max(n_batch, 1), max(len(thresholds), 1), 8), SENTINEL, np.int64) if counts else None

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    status = lib.c21cm_minkowski_grids(field_ptr, nx, ny, nz, n_batch, nz if row_pitch is None else row_pitch,
                                       None if null_offsets else ptr(offsets), n_thr,
                                       None if null_thresholds else ptr(thresholds), select_below, periodic_mask,
                                       ptr(out), None)
    return status, out


def untouched(out):
    return out is None or bool(np.all(out == SENTINEL))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_value_writes_nothing(bad):
    f = np.array(random_field((12, 10, 14)))
    f[7, 3, 13] = bad
    status, out = raw_call(f.ctypes.data_as(C.c_void_p), f.shape)
    assert status == NAN_ERROR and "not finite" in LIB.last_error()
    assert untouched(out)
    with pytest.raises(LIB.BackendError) as err:
        PS.get_minkowski_functionals(f, 1.0, thresholds=[0.0])
    assert err.value.code == NAN_ERROR
    # and the next call is clean
    f[7, 3, 13] = 0.0
    status, out = raw_call(f.ctypes.data_as(C.c_void_p), f.shape)
    assert status == 0 and not untouched(out)
    assert_rows(out[0], f, [0.25, 0.5], True, True)


def test_argument_errors_of_the_c_entry():
    """every check comes before any access: the field is a pointer nothing may follow"""
    fake = C.c_void_p(0x1000)
    ok = (4, 4, 4)
    cases = [
        dict(shape=(1, 2, 2**30)),  # nx ny nz = 2^31
        dict(shape=(2**16, 2**16, 1)),
        dict(shape=(0, 4, 4)), dict(shape=(4, 4, -1)),
        dict(n_batch=0), dict(n_batch=65536, offsets=np.zeros(65536, np.int64)),
        dict(row_pitch=3), dict(offsets=(-1,)),
        dict(n_thresholds=0), dict(n_thresholds=-1), dict(thresholds=np.arange(256.0)),
        dict(thresholds=(0.5, float("nan"))), dict(thresholds=(float("-inf"), 0.5)), dict(thresholds=(0.5, float("inf"))),
        dict(thresholds=(0.5, 0.5)), dict(thresholds=(0.5, 0.25)),
        dict(periodic_mask=-1), dict(periodic_mask=8),
        dict(counts=False), dict(null_thresholds=True), dict(null_offsets=True),
    ]
    for kw in cases:
        shape = kw.pop("shape", ok)
        status, out = raw_call(fake, shape, **kw)
        assert status == VALUE_ERROR, kw
        assert LIB.last_error().startswith("minkowski:"), kw
        assert untouched(out), kw
    status, out = raw_call(None, ok)
    assert status == VALUE_ERROR and untouched(out)
