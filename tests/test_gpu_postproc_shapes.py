"""The lightcone, RSD, angular and power kernels at the shapes production runs take (csrc/hip/lightcone_kernels.hip,
rsd_kernels.hip, angular_lightcone_kernels.hip, power_kernels.hip, csrc/host/power_driver.c).

The kernel tests of test_gpu_lightcone.py, test_gpu_rsds.py, test_gpu_angular_lightcone.py and test_gpu_power.py
run at toy shapes, where every launch fits one pass of its grid.  Here each test first works out the launch
geometry from the constants of the sources (read from the source files, so a change of kMaxBlocks,
PW_MODES_PER_WG or PW_MIN_WGS changes what is asserted) and asserts that the path is entered:

* slab, dv/dr, angular sampler: grid-stride trips, n_cols * run > kBlock * kMaxBlocks;
* RSD shift: more column groups than kMaxBlocks, so a workgroup re-zeroes its accumulators and goes round again;
  several columns per workgroup with a ragged last group in a late round; displacements of many box lengths;
* prefilter: the truncated start sums, L >= horizon(z);
* power: >= 16 trips of the base loop per wave, all four waves busy, > 256 workgroups per k_perp group for the
  strided sum (spherical), every binning option, cross power, cylindrical, lightcone chunks;
* run_lightcone at HII_DIM = 128: the dv/dr and RSD launches of a whole run cross both limits.

References: the fp64 restatements tests/*_reference.py and, for the prefilter, scipy.ndimage.spline_filter itself.
Tolerances are those of the small-shape tests."""

import ctypes as C
import importlib
import re
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest
import scipy.fft
from scipy import ndimage
from scipy.spatial.transform import Rotation

import angular_reference as AR
import lightcone_reference as LR
import power_reference as PR
import rsd_reference as RR
from test_gpu_angular_lightcone import on_device, pair_tables, to_host
from test_gpu_lightcone import run_case
from test_gpu_power import POWER_RTOL, check_power
from test_gpu_rsds import assert_close_per_column
from test_gpu_run_coeval import DATA

pytestmark = pytest.mark.gpu
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
PS = importlib.import_module("21cmfast_amd.powerspec")

CSRC = Path(__file__).resolve().parent.parent / "21cmfast_amd" / "csrc"
WORKERS = 16


def source_constant(path, pattern):
    """An integer constant of the sources, e.g. ``constexpr int kMaxBlocks = 256 * 8;``"""
    m = re.search(pattern, (CSRC / path).read_text())
    assert m, f"{pattern} not found in {path}"
    expr = m.group(1)
    assert re.fullmatch(r"[0-9 *+()]+", expr), expr
    return int(eval(expr))  # digits, *, + and brackets only


def launch_limit(hip_file):
    """kBlock * kMaxBlocks of a kernel file: the items one pass of the capped grid covers"""
    block = source_constant(f"hip/{hip_file}", r"constexpr int kBlock = ([^;]+);")
    blocks = source_constant(f"hip/{hip_file}", r"constexpr int kMaxBlocks = ([^;]+);")
    return block, blocks


# ------------------------------------------------------------------------------ lightcone slabs, dv/dr
# (HII_DIM, HII_D_PARA, n_slices, node positions in slices): runs of 1, 10, 14 and 46 (> HII_D_PARA) slices;
# slices 0-2 and 74-79 belong to no pair
BIG_SLABS = {"256": (256, 40, 80, [2.5, 3.5, 13.5, 27.5, 73.5]), "200": (200, 40, 80, [2.5, 3.5, 13.5, 27.5, 73.5])}


@pytest.mark.parametrize("case", sorted(BIG_SLABS))
def test_slab_kernel_grid_stride(gpu_lib, case):
    n, d_para, n_slices, nodes = BIG_SLABS[case]
    block, blocks = launch_limit("lightcone_kernels.hip")
    got, want, runs = run_case(n, d_para, n_slices, nodes, seed=23, device=True)
    assert sorted(runs) == [1, 10, 14, 46] and max(runs) > d_para != n
    strided = [r for r in runs if n * n * r > block * blocks]
    print(f"\nslab {n}^2: items per pair {[n * n * r for r in runs]}, one pass covers {block * blocks}")
    assert len(strided) >= 2 and 46 in strided, "the longer pairs take grid-stride trips"
    if case == "200":  # the last trip is partial
        assert all((n * n * r) % (block * blocks) for r in strided)
    for k in want:
        np.testing.assert_array_max_ulp(got[k], want[k], maxulp=1)
        assert not got[k][..., :3].any() and not got[k][..., 74:].any(), k  # outside every pair: untouched
        assert got[k][..., 3:74].any(axis=(0, 1)).all(), k
    assert np.any(got["z_reion"] == -1.0) and np.all(np.isfinite(got["z_reion"]))


@pytest.mark.parametrize("use_ts", [False, True], ids=["taylor", "tau21"])
def test_dvdr_kernel_grid_stride(gpu_lib, use_ts):
    import torch

    n, n_slices, dx = 256, 700, 2.0
    block, blocks = launch_limit("lightcone_kernels.hip")
    trips = -(-n * n * n_slices // (block * blocks))
    print(f"\ndv/dr: {n * n * n_slices} items, {trips} trips of {block * blocks}")
    assert n * n * n_slices > block * blocks and (n * n * n_slices) % (block * blocks)
    rng = np.random.default_rng(41 + use_ts)
    H = 2.2e-18 * (1 + np.linspace(18, 6, n_slices)) ** 1.5 / 19 ** 1.5
    vel = rng.standard_normal((n, n, n_slices), dtype=np.float32) * (0.3 * H * dx).astype(np.float32)
    bt = rng.standard_normal((n, n, n_slices), dtype=np.float32) * np.float32(20)
    tau = None
    if use_ts:
        tau = np.abs(rng.standard_normal((n, n, n_slices), dtype=np.float32)) * np.float32(0.05)
        tau[0, :, :] = 1e-11  # below the 1e-10 threshold
        tau[-1, :, :] = 0.0
    t0 = time.perf_counter()
    want = LR.include_dvdr_in_tau21(bt, vel, H, dx, 0.2, tau_21=tau)
    print(f"host reference {time.perf_counter() - t0:.1f} s")
    d_bt = torch.from_numpy(bt).cuda()
    api.lightcone_dvdr(d_bt, torch.from_numpy(vel).cuda(), H, dx, 0.2,
                       tau_21=None if tau is None else torch.from_numpy(tau).cuda())
    got = d_bt.cpu().numpy()
    # the whole array, so the first and last slice of the first and last column with it
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-30)
    for col in ((0, 0), (n - 1, n - 1)):
        np.testing.assert_allclose(got[col][[0, -1]], want[col][[0, -1]], rtol=1e-6, atol=1e-30)
    if use_ts:
        np.testing.assert_array_equal(got[0], bt[0])
        np.testing.assert_array_equal(got[-1], bt[-1])
    assert not np.array_equal(got[1:-1], bt[1:-1])


# ------------------------------------------------------------------------------ RSD shift
def rsd_cpb(lib, n, nf):
    """columns per workgroup and LDS bytes, as the launch computes them"""
    lib.c21hip_rsd_lds_bytes.restype = C.c_size_t
    lib.c21hip_rsd_lds_bytes.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
    cpb = C.c_int(0)
    lib.c21hip_rsd_lds_bytes(n, nf, C.byref(cpb))
    return cpb.value


def rsd_reference(field, disp, m, periodic, chunk=2048):
    """RR.rsds_shift of (n_cols, n) arrays, the columns in independent chunks (a column's result depends
    on no other column: the restatement interpolates the displacement at integer column coordinates)."""
    bounds = [(a, min(a + chunk, field.shape[0])) for a in range(0, field.shape[0], chunk)]
    if len(bounds) > 1 and bounds[-1][1] - bounds[-1][0] == 1:  # no one-column tail
        bounds[-2:] = [(bounds[-2][0], bounds[-1][1])]

    def one(ab):
        a, b = ab
        return RR.rsds_shift(field[a:b].T.astype(np.float64), disp[a:b].T, n_rsd_subcells=m, periodic=periodic).T

    with ThreadPoolExecutor(WORKERS) as ex:
        return np.concatenate(list(ex.map(one, bounds)))


def rsd_inputs(rng, n_cols, n, nf):
    fields = [rng.standard_normal((n_cols, n), dtype=np.float32) * np.float32(10.0 ** rng.uniform(-3, 3))
              for _ in range(nf)]
    vel = rng.standard_normal((n_cols, n), dtype=np.float32) * np.float32(1e-17)  # Mpc/s, as los_velocity
    scale = rng.uniform(1.0e17, 4.0e17, n)  # pixels per Mpc/s: a few pixels of displacement
    return fields, vel, scale


# n_sub, periodic, fields: both periodicities, 1 and 4 sub-cells, 1 and 3 fields
@pytest.mark.parametrize("m,periodic,nf", [(4, True, 3), (1, False, 1), (4, False, 1)],
                         ids=["m4_per_f3", "m1_open_f1", "m4_open_f1"])
def test_rsd_many_rounds_per_workgroup(gpu_lib, m, periodic, nf):
    import torch

    n_cols, n = 256 * 256, 256
    _, blocks = launch_limit("rsd_kernels.hip")
    cpb = rsd_cpb(gpu_lib, n, nf)
    groups = -(-n_cols // cpb)
    print(f"\nrsd: cpb = {cpb}, groups = {groups} > {blocks}: {groups // blocks} rounds per workgroup")
    assert cpb == 1 and groups > blocks and groups // blocks >= 16
    rng = np.random.default_rng(97 + m + nf)
    fields, vel, scale = rsd_inputs(rng, n_cols, n, nf)
    got = api.rsd_shift(fields, vel, scale, n_sub=m, periodic=periodic)
    disp = vel.astype(np.float64) * scale
    t0 = time.perf_counter()
    for q in range(nf):
        want = rsd_reference(fields[q], disp, m, periodic)
        assert_close_per_column(got[q], want, fields[q], f"field {q}")
    print(f"host reference {time.perf_counter() - t0:.1f} s")
    if nf == 3:  # two runs and host-staged against device inputs: the same bits (staging: n_host_in * 64 MiB)
        again = api.rsd_shift(fields, vel, scale, n_sub=m, periodic=periodic)
        dev = api.rsd_shift([torch.from_numpy(f).cuda() for f in fields], torch.from_numpy(vel).cuda(), scale,
                            n_sub=m, periodic=periodic)
        for q in range(nf):
            np.testing.assert_array_equal(got[q], again[q])
            np.testing.assert_array_equal(got[q], dev[q].cpu().numpy())


@pytest.mark.parametrize("n,n_cols", [(17, 40003), (100, 5001), (255, 2500)])
def test_rsd_ragged_last_group_in_a_late_round(gpu_lib, n, n_cols):
    nf, m = 3, 4
    _, blocks = launch_limit("rsd_kernels.hip")
    cpb = rsd_cpb(gpu_lib, n, nf)
    groups = -(-n_cols // cpb)
    print(f"\nrsd n = {n}: cpb = {cpb}, {n_cols} columns, {groups} groups, last group {n_cols % cpb or cpb} columns")
    assert n_cols > blocks * cpb and groups > blocks
    if n < 128:  # several columns per workgroup, the last group short
        assert cpb > 1 and n_cols % cpb
    for periodic in (False, True):
        rng = np.random.default_rng(n + periodic)
        fields, vel, scale = rsd_inputs(rng, n_cols, n, nf)
        got = api.rsd_shift(fields, vel, scale, n_sub=m, periodic=periodic)
        disp = vel.astype(np.float64) * scale
        for q in range(nf):
            want = rsd_reference(fields[q], disp, m, periodic)
            assert_close_per_column(got[q], want, fields[q], f"field {q} periodic {periodic}")


def test_rsd_displacements_of_many_box_lengths(gpu_lib):
    """Periodic, |x| up to ~1e6 fine cells, and whole columns displaced by 2^39 pixels = 2^41 fine cells, beyond the
    2^40 above which the kernel reduces x with fmod.  Those columns move as a whole (every slice by the same power
    of two), so x = k + 2^41 is exact on both sides; a displacement that varied along such a column would be
    quantised to 2^-12 fine cells, far more than the tolerance, in the restatement as much as in the kernel."""
    n_cols, n, m = 4099, 60, 4
    rng = np.random.default_rng(77)
    field = rng.random((n_cols, n), dtype=np.float32) + np.float32(0.5)
    vel = rng.standard_normal((n_cols, n), dtype=np.float32) * np.float32(6.0e4)  # pixels: scale 1
    huge = [0, 1234, n_cols - 1]
    vel[huge] = np.float32(2.0 ** 39)
    vel[1] = np.float32(-2.0 ** 39 - 2.0 ** 20)
    huge.append(1)
    disp = vel.astype(np.float64)
    x = np.abs(disp) * m
    assert x[huge].min() > 2.0 ** 40 and 5e5 < np.delete(x, huge, axis=0).max() < 2e6
    got = api.rsd_shift([field], vel, 1.0, n_sub=m, periodic=True)[0]
    want = rsd_reference(field, disp, m, True)
    assert_close_per_column(got, want, field, "far displacements")
    np.testing.assert_allclose(got.sum(axis=-1, dtype=np.float64), field.sum(axis=-1, dtype=np.float64), rtol=1e-6)
    for c in huge:  # a whole number of pixels: a roll
        shift = int(disp[c, 0] % n)
        np.testing.assert_allclose(got[c], np.roll(field[c], shift), rtol=1e-6)


# ------------------------------------------------------------------------------ angular sampler
# no half-integer component: a pixel whose direction has a zero component is no rounding tie at order 0
ANG_ORIGIN = (3.25, -17.3, 1234.1)
ANG_ROT = Rotation.from_euler("Y", -np.pi / 2)  # like_rectilinear's: the grid looks along +z


def grid_sky(side=256, width=0.25):
    """the regular (latitude, longitude) grid of AngularLightconer.like_rectilinear, side^2 pixels"""
    a = np.linspace(0.0, width, side)
    lat, lon = np.meshgrid(a[::-1], a, indexing="ij")
    return lat.ravel(), lon.ravel()


def ang_ties(nhat, dist, origin):
    """(n_pix, n_slices) mask of points within 1e-9 of a rounding tie (order 0), as test_gpu_angular_lightcone.ties"""
    x = np.stack([AR.points(nhat, d, origin) for d in dist], axis=-1)
    return np.any(np.abs(x - np.floor(x) - 0.5) < 1e-9, axis=0)


ANG_CASES = [(0, (64, 64)), (1, (64, 64)), (3, (64, 64)), (5, (64, 64)),
             (0, (48, 80)), (1, (48, 80)), (3, (48, 80)), (5, (48, 80)), (1, (128, 128))]


@pytest.mark.parametrize("case", ANG_CASES, ids=[f"o{c[0]}_{c[1][0]}x{c[1][1]}" for c in ANG_CASES])
def test_angular_sampler_grid_stride(gpu_lib, case):
    order, (n, d_para) = case
    block, blocks = launch_limit("angular_lightcone_kernels.hip")
    rng = np.random.default_rng(300 + order + n)
    lat, lon = grid_sky()
    nhat = AR.directions(lat, lon, ANG_ROT)
    n_pix, n_slices = len(lat), 12
    lcd = 300.0 + 1.5 * np.arange(n_slices)
    d_lo, d_hi = lcd[1] - 0.25, lcd[10] + 0.5
    idx, dist, w_lo, w_hi, w_norm = pair_tables(lcd, d_lo, d_hi)
    run = len(idx)
    print(f"\nangular: {n_pix} pixels x {run} slices = {n_pix * run} items, one pass covers {block * blocks}")
    assert list(idx) == list(range(1, 11)) and n_pix * run > block * blocks and (n_pix * run) % (block * blocks)
    # most pixels read taps that wrap on no axis
    x = np.stack([AR.points(nhat, d, ANG_ORIGIN) for d in dist], axis=-1)
    first = np.floor(x) - order // 2
    inside = (np.mod(first, np.array([n, n, d_para])[:, None, None]) + order
              < np.array([n, n, d_para])[:, None, None]).all(axis=0)
    assert inside.mean() > 0.5

    names = ["density"] + (["z_reion"] if order <= 1 else []) + ["los_velocity"]
    lo, hi = {}, {}
    for k in names:
        scale = 10.0 ** rng.uniform(-2, 2)
        shape = (3, n, n, d_para) if k == "los_velocity" else (n, n, d_para)
        a = rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)
        b = rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)
        lo[k], hi[k] = (tuple(a), tuple(b)) if k == "los_velocity" else (a, b)
    want = {k: np.zeros((n_pix, n_slices), np.float32) for k in names}
    t0 = time.perf_counter()
    AR.fill_slices(want, lcd, d_lo, d_hi, 1.0, lo, hi, nhat, ANG_ORIGIN, order)
    print(f"host reference {time.perf_counter() - t0:.1f} s")

    def coefficients(d):
        if order < 3:
            return {k: (tuple(on_device(c) for c in v) if isinstance(v, tuple) else on_device(v)) for k, v in d.items()}
        return {k: (tuple(api.spline_prefilter([on_device(c) for c in v], order)) if isinstance(v, tuple) else
                    api.spline_prefilter([on_device(v)], order)[0]) for k, v in d.items()}

    got = {k: on_device(np.zeros((n_pix, n_slices), np.float32)) for k in names}
    api.lightcone_angular(got, coefficients(lo), coefficients(hi), int(idx[0]), dist, w_lo, w_hi, w_norm,
                          on_device(nhat), ANG_ORIGIN, order=order, mean_max=("z_reion",))
    keep = np.zeros((n_pix, n_slices), bool)
    keep[:, idx] = True
    if order == 0:  # the tie mask is a hole in the comparison: it stays a negligible share of it
        tie = ang_ties(nhat, lcd[idx], ANG_ORIGIN)
        print(f"rounding ties masked: {tie.sum()} of {tie.size}")
        assert tie.mean() <= 1e-4
        keep[:, idx] &= ~tie
    tol = 1e-6 if order <= 1 else 1e-5
    for k in names:
        g = to_host(got[k])
        assert not g[:, :1].any() and not g[:, 11:].any(), k  # only the slices of the pair
        boxes = lo[k] + hi[k] if isinstance(lo[k], tuple) else (lo[k], hi[k])
        scale = max(np.abs(a).max() for a in boxes)
        err = np.abs(g.astype(np.float64) - want[k])[keep]
        print(f"{k}: worst error {err.max() / scale:.3g} of max|field|")
        assert err.max() <= tol * scale, f"{k}: {err.max() / scale:.3g} of max|field|"


# ------------------------------------------------------------------------------ prefilter
def horizon(z):
    """the taps of the truncated start sums: |z|^h < 1e-18 (prefilter_pole, angular_lightcone_kernels.hip)"""
    return int(np.ceil(-18.0 * np.log(10.0) / np.log(abs(z))))


PREFILTER_SHAPES = [(32, 32, 32), (50, 50, 50), (64, 64, 64), (40, 64, 96), (128, 128, 128)]


@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prefilter_truncated_start_sums(gpu_lib, shape, order):
    """Worst deviation from scipy's fp64 coefficients in units of max|coefficients|, over the ten cases on an
    MI355X: device 1.05e-7 to 1.64e-7, scipy with fp32 storage (output=float32: every axis stored in fp32, as
    the device stores every pass) 7.0e-8 to 8.6e-8; the bound is the 2e-6 of the small-shape test.  Both are
    printed.  The far end of a truncated sum weighs 1e-18: one tap more or fewer there is invisible in fp32, a
    shift of the taps by one cell is not."""
    poles = AR.POLES[order]
    assert [horizon(z) for z in AR.POLES[3] + AR.POLES[5]] == [32, 50, 14]
    truncated = [(L, horizon(z)) for L in shape for z in poles if L >= horizon(z)]
    print(f"\nprefilter {shape} order {order}: truncated (L, horizon) {sorted(set(truncated))}")
    assert truncated, "some axis and pole takes the truncated start"
    if min(shape) >= 50 or order == 3:
        assert len(truncated) == 3 * len(poles), "every axis and pole does"
    box = np.random.default_rng(sum(shape) + order).standard_normal(shape, dtype=np.float32)
    want = ndimage.spline_filter(box.astype(np.float64), order=order, mode="grid-wrap")
    scale = np.abs(want).max()
    second = AR.periodic_prefilter(box, order)
    assert np.abs(second - want).max() <= 1e-12 * scale
    stored32 = ndimage.spline_filter(box.astype(np.float64), order=order, mode="grid-wrap", output=np.float32)
    d32 = np.abs(stored32.astype(np.float64) - want).max() / scale
    out = api.spline_prefilter([on_device(box)], order)[0]
    c = on_device(box)
    api.spline_prefilter([c], order, out=[c])  # in place
    got = to_host(out)
    np.testing.assert_array_equal(got, to_host(c))
    dev = np.abs(got.astype(np.float64) - want).max() / scale
    print(f"device {dev:.3g}, scipy with fp32 storage {d32:.3g} of max|coefficients|")
    assert dev <= 2e-6
    np.testing.assert_allclose(got, second, rtol=0, atol=2e-6 * scale)


# ------------------------------------------------------------------------------ power spectra
def power_geometry(shape, n_batch, n_used):
    """(rows per workgroup, modes per workgroup, trips of the base loop per wave) as power_driver.c lays a launch
    out: rpw = min(PW_MODES_PER_WG / nh, ceil(n_used n_batch / PW_MIN_WGS)); a wave takes 64 modes per trip and
    the four waves of a workgroup stride by 256"""
    per_wg = source_constant("host/power_driver.c", r"#define PW_MODES_PER_WG (\d+)")
    min_wgs = source_constant("host/power_driver.c", r"#define PW_MIN_WGS (\d+)")
    nh = shape[2] // 2 + 1
    rpw = max(1, min(per_wg // nh, -(-n_used * n_batch // min_wgs)))
    return rpw, rpw * nh, -(-rpw * nh // 256)


def assert_spherical_geometry(shape, n_batch=1, what=""):
    rpw, modes, trips = power_geometry(shape, n_batch, shape[0] * shape[1])
    n_wg = -(-shape[0] * shape[1] // rpw)
    print(f"\n{what} {shape}: rpw = {rpw}, {modes} modes per workgroup, trips per wave = {trips}, n_wg = {n_wg}")
    assert trips >= 16 and n_wg > 256


def assert_cylindrical_geometry(shape, L, n_batch=1, what="", **edge_opts):
    ep, _ = PS.cylindrical_edges(shape, L, **edge_opts)
    kx, ky = PS.k_axis(shape[0], L[0]), PS.k_axis(shape[1], L[1])
    g = np.digitize(np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2), ep) - 1
    n_used = int(np.count_nonzero((g >= 0) & (g < len(ep) - 1)))
    rpw, modes, trips = power_geometry(shape, n_batch, n_used)
    print(f"\n{what} cylindrical {shape}: {n_used} rows, rpw = {rpw}, {modes} modes per workgroup, trips = {trips}")
    assert trips >= 16


def white(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) + np.float32(1.0)


def red(shape, seed):
    """a Gaussian field with P(k) ~ k^-3, built in fp64, plus a mean of 20: the shape of a brightness-temperature box"""
    rng = np.random.default_rng(seed)
    ft = scipy.fft.rfftn(rng.standard_normal(shape), workers=WORKERS)
    k = [np.fft.fftfreq(n) for n in shape[:2]] + [np.fft.rfftfreq(shape[2])]
    k2 = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    k2[0, 0, 0] = np.inf
    f = scipy.fft.irfftn(ft * k2 ** -0.75, s=shape, workers=WORKERS)
    return (f * (10.0 / f.std()) + 20.0).astype(np.float32)


def full_spectrum_fp32(field, L):
    """P on the full grid from scipy's single-precision transform of the fp32 field (scipy.fft keeps fp32): what an
    fp32 transform that is not the code under test gives.  The half spectrum is unfolded with P(-k) = P(k)."""
    ft = scipy.fft.rfftn(field, workers=WORKERS)
    assert ft.dtype == np.complex64
    nx, ny, nz = field.shape
    V = float(np.prod(L))
    half = (ft.real.astype(np.float64) ** 2 + ft.imag.astype(np.float64) ** 2) * (V / field.size ** 2)
    full = np.empty(field.shape)
    full[:, :, :nz // 2 + 1] = half
    i, j = (-np.arange(nx)) % nx, (-np.arange(ny)) % ny
    l = nz - np.arange(nz // 2 + 1, nz)
    full[:, :, nz // 2 + 1:] = half[i][:, j][:, :, l]
    return full


def check_spherical(f, L, P, what, rtol=POWER_RTOL, **opts):
    deltax2 = opts.pop("deltax2", None)
    got = PS.get_power(f, L, return_counts=True, deltax2=deltax2, **opts)
    ref = PR.get_power(f, L, return_counts=True, spectrum=P, **opts)
    assert np.array_equal(got[2], ref[2]), what
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-12, atol=0, err_msg=what)
    return check_power(got[0], ref[0], rtol=rtol, what=what)


def check_cylindrical(f, L, P, what, rtol=POWER_RTOL, **opts):
    deltax2 = opts.pop("deltax2", None)
    p, kp, kz, c = PS.get_cylindrical_power(f, L, return_counts=True, deltax2=deltax2, **opts)
    rp, rkp, rkz, rc = PR.get_cylindrical_power(f, L, return_counts=True, spectrum=P, **opts)
    assert np.array_equal(c, rc), what
    np.testing.assert_allclose(kp, rkp, rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(kz, rkz, rtol=1e-12, atol=0, err_msg=what)
    return check_power(p, rp, rtol=rtol, what=what)


SPHERICAL_OPTIONS = [  # those of test_gpu_power.test_get_power_options
    dict(log_bins=True), dict(bins=np.array([0.0, 0.1, 0.25, 0.5, 1.0, 1.7])), dict(bins=9),
    dict(ignore_zero_mode=True), dict(ignore_kperp_zero=True), dict(ignore_kpar_zero=True),
    dict(bins_upto_boxlen=False), dict(bin_ave=False),
]
CYLINDRICAL_OPTIONS = [dict(), dict(log_bins=True, ignore_zero_mode=True),
                       dict(kperp_bins=[0.0, 0.3, 0.9, 2.0, 2.6], kpar_bins=4)]


def test_power_256_every_option(gpu_lib):
    shape, L = (256, 256, 256), (300.0, 300.0, 300.0)
    assert_spherical_geometry(shape, what="white")
    f = white(shape, 11)
    t0 = time.perf_counter()
    P = PR.spectrum(f, L)
    check_spherical(f, L, P, "256 defaults")
    for opts in SPHERICAL_OPTIONS:
        check_spherical(f, L, P, f"256 {sorted(opts)}", **opts)
    for opts in CYLINDRICAL_OPTIONS:
        edge_opts = {k: v for k, v in opts.items() if k != "ignore_zero_mode"}
        assert_cylindrical_geometry(shape, L, what=str(sorted(opts)), **edge_opts)
        check_cylindrical(f, L, P, f"256 cylindrical {sorted(opts)}", **opts)
    g = (np.float32(0.5) * f + white(shape, 12)).astype(np.float32)
    Pc = PR.spectrum(f, L, g)
    check_spherical(f, L, Pc, "256 cross", deltax2=g)
    check_cylindrical(f, L, Pc, "256 cylindrical cross", deltax2=g)
    print(f"host reference and device, all options: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("shape,L", [((512, 512, 64), (600.0, 600.0, 75.0)), ((221, 216, 251), (330.0, 320.0, 390.0))],
                         ids=["512x512x64", "221x216x251"])
def test_power_noncubic(gpu_lib, shape, L):
    """White noise + 1 at POWER_RTOL.  The bins of a handful of modes beside the axes through k = 0 are where an
    fp32 transform that keeps the mean in misses it at these sizes: scipy's fp32 transform of the (221, 216, 251)
    field is off by 3.2e-5 in one cylindrical bin and 6.2e-5 in the lowest log bins, and so was the device
    (3.2e-5, 5.2e-5) until the pack took the mean out (now 7.8e-7, 4.9e-7 on an MI355X)."""
    assert_spherical_geometry(shape, what="white")
    f = white(shape, 5)
    P = PR.spectrum(f, L)
    check_spherical(f, L, P, f"{shape} defaults")
    # log bins: the first bins hold 2 to 4 modes next to the mode of the mean
    check_spherical(f, L, P, f"{shape} log", log_bins=True, ignore_kperp_zero=True)
    assert_cylindrical_geometry(shape, L, what="default")
    check_cylindrical(f, L, P, f"{shape} cylindrical")
    g = (f * np.float32(0.5) + white(shape, 6)).astype(np.float32)
    check_spherical(f, L, PR.spectrum(f, L, g), f"{shape} cross", deltax2=g)


@pytest.mark.parametrize("shape,L", [((256, 256, 256), (300.0, 300.0, 300.0)), ((221, 216, 251), (330.0, 320.0, 390.0))],
                         ids=["256", "221x216x251"])
def test_power_red_field(gpu_lib, shape, L):
    """A k^-3 field with a mean of 20: the low-power bins show the fp32 transform.  d32 is the worst per-bin relative
    deviation of scipy's fp32 transform (binned by the restatement) from the fp64 restatement; the device's worst
    bin must stay within 4 d32 (rocFFT factorises and orders its operations differently).  The bound is on the
    worst bin: one bin's deviation is a sum of rounding errors that can cancel to nearly nothing in either transform,
    so the ratio of two independent transforms in a single bin has no bound.  Both figures are printed; on an MI355X
    (d32, device): 256^3 spherical 1.90e-7, 1.63e-7; cylindrical 3.35e-6, 2.06e-6; (221, 216, 251) spherical
    1.09e-7, 2.36e-7; cylindrical 1.34e-4, 1.43e-5."""
    assert_spherical_geometry(shape, what="red")
    f = red(shape, 31)
    P64, P32 = PR.spectrum(f, L), full_spectrum_fp32(f, L)
    for what, ref in (("spherical", PR.get_power), ("cylindrical", PR.get_cylindrical_power)):
        p64, p32 = ref(f, L, spectrum=P64)[0], ref(f, L, spectrum=P32)[0]
        ok = ~np.isnan(p64)
        d32 = float(np.max(np.abs(p32[ok] / p64[ok] - 1)))
        got = (PS.get_power if what == "spherical" else PS.get_cylindrical_power)(f, L)[0]
        dev = float(np.max(np.abs(got[ok] / p64[ok] - 1)))
        print(f"\nred {shape} {what}: d32 = {d32:.3e}, device = {dev:.3e}, ratio {dev / d32:.2f}")
        assert dev <= 4 * d32, (what, dev, d32)
        # counts and k exactly, the power through check_power as for white noise
        (check_spherical if what == "spherical" else check_cylindrical)(f, L, P64, f"red {what}", rtol=4 * d32)


@pytest.mark.parametrize("cylindrical", [False, True], ids=["spherical", "cylindrical"])
def test_power_lightcone_chunks(gpu_lib, cylindrical):
    shape, cell = (128, 128, 1024), 1.5
    starts, n = [0, 64, 100, 400, 640, 896], 128  # overlapping chunks, the last one ends at the last slice
    chunk = (shape[0], shape[1], n)
    if cylindrical:
        assert_cylindrical_geometry(chunk, tuple(cell * x for x in chunk), n_batch=len(starts), what="lightcone")
    else:
        rpw, modes, trips = power_geometry(chunk, len(starts), shape[0] * shape[1])
        print(f"\nlightcone chunks: rpw = {rpw}, {modes} modes per workgroup, trips per wave = {trips}")
        assert trips >= 16
    lc = white(shape, 21)
    z = np.linspace(6.0, 12.0, shape[2])
    got = PS.lightcone_power_spectra(lc, cell, redshifts=z, chunk_starts=starts, cylindrical=cylindrical)
    ref = PR.lightcone_power_spectra(lc, cell, redshifts=z, chunk_starts=starts, cylindrical=cylindrical)
    assert np.array_equal(got.chunk_starts, ref["chunk_starts"])
    np.testing.assert_array_equal(got.redshifts, ref["redshifts"])
    assert np.array_equal(got.counts, ref["counts"])
    if cylindrical:
        np.testing.assert_allclose(got.kperp, ref["kperp"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got.kpar, ref["kpar"], rtol=1e-12, atol=0)
    else:
        np.testing.assert_allclose(got.k, ref["k"], rtol=1e-12, atol=0)
    assert got.power.shape[0] == len(starts)
    for c in range(len(starts)):
        check_power(got.power[c], ref["power"][c], what=f"chunk {c}")


# ------------------------------------------------------------------------------ end to end
def test_run_lightcone_128_dvdr_and_rsds(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    n, cell = 128, 1.5
    kw = dict(HII_DIM=n, DIM=2 * n, BOX_LEN=n * cell, N_THREADS=2, ZPRIME_STEP_FACTOR=1.04, SOURCE_MODEL=1,
              USE_TS_FLUCT=False, Z_HEAT_MAX=20.0, USE_LYA_HEATING=False, HII_FILTER=0, KEEP_3D_VELOCITIES=True)
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 20.0)
    z0, z1 = nodes[-1] + 0.15, nodes[0] - 0.15
    so = D.Inputs(**kw).simulation_options
    q = ("density", "neutral_fraction", "brightness_temp")
    base = set(q) | {"los_velocity"}
    max_dvdr = D.Inputs(**kw).astro_params.MAX_DVDR

    def run(lcn, **o):
        res = D.run_lightcone(D.Inputs(random_seed=3, **kw), lcn, nodes, data_path=DATA, lib=gpu_lib, device="cuda", **o)
        return {k: to_host(v) for k, v in res["lightcones"].items()}

    rect = D.RectilinearLightconer.between_redshifts(z0, z1, cell, quantities=q)
    rect_plain = D.RectilinearLightconer.between_redshifts(z0, z1, cell, quantities=q + ("los_velocity",))
    ang = D.AngularLightconer.like_rectilinear(so, z0, z1, quantities=q, interpolation_order=3)
    ang_plain = D.AngularLightconer.like_rectilinear(so, z0, z1, quantities=q + ("los_velocity",),
                                                     interpolation_order=3)
    n_slices = len(rect.lc_distances)
    block, blocks = launch_limit("lightcone_kernels.hip")
    _, rsd_blocks = launch_limit("rsd_kernels.hip")
    cpb = rsd_cpb(gpu_lib, n_slices, len(base))
    print(f"\n{n}^2 columns x {n_slices} slices = {n * n * n_slices} dv/dr items; rsd cpb = {cpb}, "
          f"{-(-n * n // cpb)} groups")
    assert n_slices > 32 and len(ang.lc_distances) == n_slices
    assert n * n * n_slices > block * blocks and -(-n * n // cpb) > rsd_blocks
    for name, lcn, plain_lcn in (("rectilinear", rect, rect_plain), ("angular", ang, ang_plain)):
        got = run(lcn, apply_rsds=True)
        plain = run(plain_lcn, include_dvdr_in_tau21=False)
        assert set(got) == base | {k + "_with_rsds" for k in base}, name
        assert got["brightness_temp"].shape[-1] == n_slices and got["brightness_temp"].size == n * n * n_slices
        for k in base - {"brightness_temp"}:
            np.testing.assert_array_equal(got[k], plain[k], err_msg=f"{name} {k}")
        H = lcn.cosmo.H0_cgs * lcn.cosmo.efunc(lcn.lc_redshifts)
        want_bt = LR.include_dvdr_in_tau21(plain["brightness_temp"], plain["los_velocity"], H, cell, max_dvdr)
        np.testing.assert_allclose(got["brightness_temp"], want_bt, rtol=1e-6, atol=1e-6, err_msg=name)
        assert not np.array_equal(got["brightness_temp"], plain["brightness_temp"])
        corrected = dict(plain, brightness_temp=got["brightness_temp"])
        for k in base:
            cols = corrected[k].reshape(-1, n_slices)
            disp = plain["los_velocity"].reshape(-1, n_slices).astype(np.float64) / H / cell
            want = rsd_reference(cols, disp, 4, False).reshape(corrected[k].shape)
            assert_close_per_column(got[k + "_with_rsds"], want, corrected[k], f"{name} {k}")
            if k != "los_velocity":
                assert not np.array_equal(got[k + "_with_rsds"], got[k]), k
