"""GPU: ``get_bubble_sizes`` / ``lightcone_bubble_sizes`` against the numpy restatement
``tests/bubble_reference.py``, ray for ray, and against closed forms.

Start cells and flags are integers and must be equal.  Lengths must agree to rtol 1e-12 except for at most max(1,
1e-4 n_rays) rays per case: the device's sincos and numpy's cos / sin may differ in the last bit, which moves a length
by a few ulp (inside the tolerance) and can flip a tie between two axes (outside it) -- the allowance the sampler
tests make for the same reason.  The histogram is compared with ``np.digitize`` of the device's own lengths, exactly,
so it is tested apart from libm.
"""

import ctypes as C
import functools
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bubble_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

PS = importlib.import_module("21cmfast_amd.powerspec")
API = importlib.import_module("21cmfast_amd.grid_api")
LIB = importlib.import_module("21cmfast_amd._lib")

RTOL = 1e-12
N_MAX = 20000
N_RAYS = (1, 1000, N_MAX)
SEED = 12345
THRESHOLD = 0.3

# name -> shape of a box (or of the lightcone), box lengths (or the cell size), chunk length (lightcone only)
CASES = {
    "partial_word": ((12, 10, 14), (18.0, 20.0, 10.5), None),  # non-cubic cells
    "one_word": ((16, 16, 64), (16.0, 16.0, 64.0), None),
    "tail_word_70": ((9, 7, 70), (9.0, 7.0, 70.0), None),
    "tail_word_130": ((8, 8, 130), (12.0, 12.0, 195.0), None),
    "lightcone": ((16, 16, 111), 1.5, 37),  # row_pitch 111, chunks at 0, 37, 74: unaligned rows, open z
}


def make_field(shape, seed):
    """A correlated Gaussian field (a white one summed over the 7-point stencil, periodic), unit variance"""
    g = np.random.default_rng(seed).standard_normal(shape)
    f = g.copy()
    for ax in range(3):
        f += np.roll(g, 1, ax) + np.roll(g, -1, ax)
    return (f / np.sqrt(7.0)).astype(np.float32)


def to_np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def same_bits(a, b):
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def freeze(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """field, a list (one per box) of the restatement's rays at N_MAX, the box shape, its lengths, its periodicity"""
    shape, L, chunk = CASES[name]
    f = make_field(shape, 17)
    f.setflags(write=False)
    if chunk is None:
        boxes, per = [f], (True, True, True)
        box_shape, lengths = shape, L
    else:
        boxes, per = [f[:, :, s:s + chunk] for s in range(0, shape[2] - chunk + 1, chunk)], (True, True, False)
        box_shape, lengths = (shape[0], shape[1], chunk), (shape[0] * L, shape[1] * L, chunk * L)
    refs = [freeze(R.trace(R.select_mask(b, THRESHOLD), lengths, N_MAX, SEED, box_index=i, periodic=per))
            for i, b in enumerate(boxes)]
    return f, refs, box_shape, lengths, per


def device_run(name, n_rays, on_device=False):
    shape, L, chunk = CASES[name]
    f = case_reference(name)[0]
    if on_device:
        import torch

        f = torch.from_numpy(np.array(f)).cuda()
    kw = dict(threshold=THRESHOLD, n_rays=n_rays, seed=SEED, bins=24, return_rays=True)
    if chunk is None:
        res = PS.get_bubble_sizes(f, L, **kw)
        for key in PS._BUBBLE_PER_BOX:
            setattr(res, key, getattr(res, key)[None])
        return res
    return PS.lightcone_bubble_sizes(f, L, chunk_length=chunk, **kw)


@functools.lru_cache(maxsize=None)
def device_max(name):
    return device_run(name, N_MAX)


def assert_rays_match(lengths, flags, starts, ref, n):
    """device rays 0 .. n - 1 of one box against the restatement's"""
    assert np.array_equal(starts, ref["starts"][:n])
    assert np.array_equal(flags, ref["flags"][:n])
    want = ref["lengths"][:n]
    off = ~(np.abs(lengths - want) <= RTOL * np.abs(want))
    print(f"rays {n}: {off.sum()} outside rtol {RTOL}; worst relative "
          f"{np.max(np.abs(lengths - want) / np.abs(want)):.3e}")
    assert off.sum() <= max(1, int(1e-4 * n))


@pytest.mark.parametrize("n_rays", N_RAYS)
@pytest.mark.parametrize("name", list(CASES))
def test_ray_for_ray(name, n_rays):
    f, refs, box_shape, lengths, per = case_reference(name)
    res = device_run(name, n_rays)
    edges = to_np(res.edges)
    n_cells = float(np.prod(box_shape))
    for b, ref in enumerate(refs):
        ln, fl, st = to_np(res.lengths[b]), to_np(res.flags[b]), to_np(res.starts[b])
        assert ln.shape == (n_rays,) and fl.dtype == np.uint8 and st.dtype == np.int64
        assert_rays_match(ln, fl, st, ref, n_rays)
        # the histogram and the counts against the device's own rays, exactly
        assert np.array_equal(to_np(res.hist[b]), R.histogram(ln, fl, edges))
        counts = [ref["n_sel"], np.sum(fl == R.ENDED), np.sum(fl == R.CAPPED), np.sum(fl == R.ESCAPED)]
        got = [int(to_np(x)[b]) for x in (res.n_selected, res.n_ended, res.n_capped, res.n_escaped)]
        assert got == counts and sum(got[1:]) == n_rays
        assert float(to_np(res.filling_fraction)[b]) == ref["n_sel"] / n_cells
        ended = fl == R.ENDED
        if ended.any():
            assert np.isclose(float(to_np(res.mean_free_path)[b]), ln[ended].mean(), rtol=1e-12)
    if name == "lightcone":
        assert len(refs) == 3 and np.array_equal(res.chunk_starts, [0, 37, 74])
        if n_rays == N_MAX:
            assert all(int(x) > 0 for x in to_np(res.n_escaped))
    # a repeated call gives the same bytes, and so does a call with another n_rays for the rays they share
    again = device_run(name, n_rays)
    big = device_max(name)
    for key in ("hist", "lengths", "flags", "starts", "n_ended", "n_capped", "n_escaped", "pdf"):
        assert same_bits(getattr(res, key), getattr(again, key)), key
    for key in ("lengths", "flags", "starts"):
        assert same_bits(to_np(getattr(res, key)), to_np(getattr(big, key))[:, :n_rays].copy()), key


@pytest.mark.parametrize("name", ["partial_word", "lightcone"])
def test_numpy_and_device_arrays_agree(name):
    host, dev = device_max(name), device_run(name, N_MAX, on_device=True)
    import torch

    for key in ("edges", "r", "hist", "pdf", "n_selected", "n_ended", "n_capped", "n_escaped", "filling_fraction",
                "lengths", "flags", "starts"):
        assert isinstance(getattr(dev, key), torch.Tensor) and getattr(dev, key).is_cuda, key
        assert same_bits(getattr(host, key), getattr(dev, key)), key
    # the mean is summed on the host or on the device: the same to rounding
    assert np.allclose(to_np(host.mean_free_path), to_np(dev.mean_free_path), rtol=1e-12, atol=0)


def test_los_rays_match():
    f, refs, box_shape, lengths, per = case_reference("tail_word_70")
    res = PS.get_bubble_sizes(f, lengths, threshold=THRESHOLD, n_rays=5000, seed=3, directions="los",
                              periodic=(True, False, False), return_rays=True, bins=8)
    ref = R.trace(R.select_mask(f, THRESHOLD), lengths, 5000, 3, directions="los", periodic=(True, False, False))
    # no sincos: every length is equal
    assert np.array_equal(res.starts, ref["starts"]) and np.array_equal(res.flags, ref["flags"])
    assert np.array_equal(res.lengths, ref["lengths"])
    assert res.n_escaped > 0


def test_select_above_is_the_complement():
    f = case_reference("partial_word")[0]
    L = CASES["partial_word"][1]
    res = PS.get_bubble_sizes(f, L, threshold=THRESHOLD, select="above", n_rays=2000, seed=9, return_rays=True)
    ref = R.trace(R.select_mask(f, THRESHOLD, "above"), L, 2000, 9)
    assert res.n_selected == f.size - R.select_mask(f, THRESHOLD).sum()
    assert_rays_match(res.lengths, res.flags, res.starts, ref, 2000)


# ---- analytic, on the device ----
def test_slab_closed_form():
    f = np.where(R.slab_mask(), 0.0, 1.0).astype(np.float32)
    res = PS.get_bubble_sizes(f, R.SLAB_SHAPE, n_rays=R.SLAB_RAYS, seed=R.SLAB_SEED, max_length=R.SLAB_MAX,
                              return_rays=True)
    sig = R.check_slab(res.lengths, res.flags, float(R.SLAB_Z[1] - R.SLAB_Z[0]), R.SLAB_MAX, R.SLAB_RAYS)
    print("slab, deviations in sigma:", np.round(sig, 2))
    assert res.n_capped + res.n_ended == R.SLAB_RAYS


def test_slab_with_several_periodic_wraps():
    f = np.where(R.slab_mask(), 0.0, 1.0).astype(np.float32)
    max_length = 5.0 * max(R.SLAB_SHAPE)
    res = PS.get_bubble_sizes(f, R.SLAB_SHAPE, n_rays=R.SLAB_RAYS, seed=R.SLAB_SEED + 1, max_length=max_length,
                              return_rays=True)
    sig = R.check_slab(res.lengths, res.flags, float(R.SLAB_Z[1] - R.SLAB_Z[0]), max_length, R.SLAB_RAYS)
    print("slab with wraps, deviations in sigma:", np.round(sig, 2))
    assert res.lengths[res.flags == R.ENDED].max() > 3.0 * max(R.SLAB_SHAPE)  # rays that went round more than once


def test_cuboid_rays_end_at_the_box_exit():
    f = np.where(R.cuboid_mask(), 0.0, 1.0).astype(np.float32)
    res = PS.get_bubble_sizes(f, R.cuboid_lengths(), n_rays=R.CUBOID_RAYS, seed=R.CUBOID_SEED, max_length=100.0,
                              return_rays=True)
    # the geometry (p0, d) is the restatement's: the same draws; the exit distance does not depend on any traversal
    ref = R.trace(R.cuboid_mask(), R.cuboid_lengths(), R.CUBOID_RAYS, R.CUBOID_SEED, max_length=100.0)
    assert np.array_equal(res.starts, ref["starts"])
    worst = R.check_cuboid(dict(p0=ref["p0"], d=ref["d"], flags=res.flags, lengths=res.lengths))
    print(f"cuboid: worst relative deviation from the exit distance {worst:.3e}")


# ---- edges ----
def test_one_selected_cell():
    shape, cell = (5, 6, 7), np.array([1.0, 0.5, 2.0])
    f = np.ones(shape, np.float32)
    f[2, 3, 4] = 0.0
    res = PS.get_bubble_sizes(f, tuple(np.array(shape) * cell), n_rays=3000, seed=2, return_rays=True)
    ref = R.trace(f < 0.5, tuple(np.array(shape) * cell), 3000, 2)
    assert res.n_selected == 1 and res.n_ended == 3000
    assert np.all(res.starts == np.ravel_multi_index((2, 3, 4), shape))
    want = R.aabb_exit(ref["p0"], ref["d"], np.array([2, 3, 4]) * cell, np.array([3, 4, 5]) * cell)
    assert np.all(np.abs(res.lengths - want) <= RTOL * want)


def test_no_selected_cell():
    res = PS.get_bubble_sizes(np.ones((6, 5, 9), np.float32), 10.0, n_rays=100, return_rays=True)
    assert res.n_selected == 0 and res.n_ended == 0 and res.n_capped == 0 and res.n_escaped == 0
    assert not res.hist.any() and res.filling_fraction == 0.0
    assert np.all(np.isnan(res.lengths)) and np.all(res.flags == 255) and np.all(res.starts == -1)
    assert np.all(np.isnan(res.pdf)) and np.isnan(res.mean_free_path)


def test_all_selected_and_periodic():
    res = PS.get_bubble_sizes(np.zeros((6, 5, 9), np.float32), 10.0, n_rays=1000, return_rays=True)
    assert res.n_selected == 270 and res.n_capped == 1000 and res.n_ended == 0 and res.n_escaped == 0
    assert not res.hist.any() and np.all(np.isnan(res.pdf)) and res.filling_fraction == 1.0
    assert np.all(res.flags == R.CAPPED) and np.all(res.lengths == 10.0)


def raw_call(field, *, n_rays=10, edges=(1.0, 2.0, 4.0), max_length=8.0, null=None):
    """c21cm_bubble_sizes_grids on a host box with pre-filled outputs: (status, outputs)"""
    lib = LIB.load()
    nx, ny, nz = field.shape
    edges = np.array(edges, np.float64)
    n_bins = len(edges) - 1
    off = np.zeros(1, np.int64)
    n = max(n_rays, 1) if n_rays < 2**31 else 1
    out = dict(hist=np.full((1, n_bins), -7, np.int64), stats=np.full((1, 4), -7, np.int64),
               lengths=np.full((1, n), -7.0), flags=np.full((1, n), 77, np.uint8), starts=np.full((1, n), -7, np.int64))
    ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
    ptr.update(field=field.ctypes.data_as(C.c_void_p), offsets=off.ctypes.data_as(C.c_void_p),
               edges=edges.ctypes.data_as(C.c_void_p))
    if null:
        ptr[null] = None
    status = lib.c21cm_bubble_sizes_grids(ptr["field"], nx, ny, nz, 1, nz, ptr["offsets"], 8.0, 8.0, 8.0, 0.5, 1, n_rays,
                                          0, 0, 7, max_length, n_bins, ptr["edges"], ptr["hist"], ptr["stats"],
                                          ptr["lengths"], ptr["flags"], ptr["starts"], None)
    return status, out


def untouched(out):
    return (np.all(out["hist"] == -7) and np.all(out["stats"] == -7) and np.all(out["lengths"] == -7.0)
            and np.all(out["flags"] == 77) and np.all(out["starts"] == -7))


def test_nan_in_the_field():
    f = np.zeros((8, 8, 8), np.float32)
    status, out = raw_call(f)
    assert status == 0 and not untouched(out)
    for bad in (np.nan, np.inf):
        f[3, 4, 5] = bad
        status, out = raw_call(f)
        assert status == 7 and "not finite" in LIB.last_error()
        assert untouched(out)
    with pytest.raises(LIB.BackendError, match="InfinityorNaNError"):
        PS.get_bubble_sizes(f, 8.0, n_rays=10)


@pytest.mark.parametrize("kw", [dict(n_rays=0), dict(n_rays=-3), dict(n_rays=2**31), dict(edges=(1.0, 1.0, 2.0)),
                                dict(edges=(2.0, 1.0, 4.0)), dict(edges=(-1.0, 1.0, 2.0)), dict(max_length=0.0),
                                dict(max_length=-1.0), dict(null="field"), dict(null="offsets"), dict(null="edges"),
                                dict(null="hist"), dict(null="stats")], ids=str)
def test_value_errors(kw):
    status, out = raw_call(np.zeros((8, 8, 8), np.float32), **kw)
    assert status == 3 and LIB.last_error().startswith("bubble sizes:")
    assert untouched(out)


# ---- shape ----
def test_production_shape():
    n, n_rays, n_check = 256, 1_000_000, 4096
    f = make_field((n, n, n), 5)
    res = PS.get_bubble_sizes(f, 300.0, threshold=0.0, n_rays=n_rays, seed=1)
    mask = R.select_mask(f, 0.0)
    assert int(res.n_selected) == int(mask.sum())
    assert res.n_ended + res.n_capped + res.n_escaped == n_rays and res.n_escaped == 0
    assert res.filling_fraction == mask.mean()
    assert res.hist.sum() <= res.n_ended
    few = PS.get_bubble_sizes(f, 300.0, threshold=0.0, n_rays=n_check, seed=1, return_rays=True)
    ref = R.trace(mask, (300.0,) * 3, n_check, 1)
    assert_rays_match(few.lengths, few.flags, few.starts, ref, n_check)
