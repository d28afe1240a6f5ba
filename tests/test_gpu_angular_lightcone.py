"""Angular lightcones on the MI355X (csrc/hip/angular_lightcone_kernels.hip, csrc/host/angular_driver.c,
grid_api.lightcone_angular / spline_prefilter, drivers.AngularLightconer through run_lightcone).

Kernel level, on seeded random node boxes, against the scipy restatement (tests/angular_reference.py):
orders 0, 1, 3 and 5 (3 and 5 through the device prefilter); directions on a Fibonacci sphere with both
poles and longitudes 0 and 2pi, rotated, at distances far outside the box and a non-zero origin; cubic
and NON_CUBIC_FACTOR boxes; 1, 3 and 17 fields (two launches); mean_max; host and device arrays mixed;
the projected velocity; bit-reproducibility; non-finite boxes.  End to end: the 3-D velocities of
run_coeval, and run_lightcone with a like_rectilinear angular lightconer beside a rectilinear one."""

import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import angular_reference as AR
import lightcone_reference as LR
import rsd_reference as RR
from test_gpu_rsds import assert_close_per_column
from test_gpu_run_coeval import DATA

pytestmark = pytest.mark.gpu
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
pkg = importlib.import_module("21cmfast_amd")

ROT = Rotation.from_euler("xyz", [0.4, -1.2, 2.3])
ORIGIN = (3.25, -17.5, 1234.0)


def sky(n=56):
    """a Fibonacci sphere, both poles, longitudes 0 and 2pi"""
    k = np.arange(n) + 0.5
    lat = np.concatenate([np.arcsin(1 - 2 * k / n), [np.pi / 2, -np.pi / 2, 0.3, -0.7]])
    lon = np.concatenate([np.mod(np.pi * (1 + 5**0.5) * k, 2 * np.pi), [0.4, 2.0, 0.0, 2 * np.pi]])
    return lat, lon


def pair_tables(lcd, d_lo, d_hi):
    """(idx, distances, w_lo, w_hi, w_norm) of the slices between two nodes (cell = 1)"""
    idx = LR.slice_indices(lcd, d_lo, d_hi, 1.0)
    return idx, lcd[idx], np.abs(d_hi - lcd[idx]), np.abs(d_lo - lcd[idx]), abs(d_lo - d_hi)


def on_device(a):
    import torch

    return torch.from_numpy(a).cuda()


def to_host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def run_kernel(lcs, lo, hi, lcd, d_lo, d_hi, nhat, order, mean_max=("z_reion",)):
    idx, dist, w_lo, w_hi, w_norm = pair_tables(lcd, d_lo, d_hi)
    if order >= 3:
        lo = {k: (tuple(api.spline_prefilter(list(v), order)) if isinstance(v, tuple) else
                  api.spline_prefilter([v], order)[0]) for k, v in lo.items()}
        hi = {k: (tuple(api.spline_prefilter(list(v), order)) if isinstance(v, tuple) else
                  api.spline_prefilter([v], order)[0]) for k, v in hi.items()}
    api.lightcone_angular(lcs, lo, hi, int(idx[0]), dist, w_lo, w_hi, w_norm, nhat, ORIGIN, order=order,
                          mean_max=mean_max)
    return idx


def ties(nhat, dist):
    """(n_pix, n_slices) mask of points within 1e-9 of a rounding tie (order 0)"""
    x = np.stack([AR.points(nhat, d, ORIGIN) for d in dist], axis=-1)
    return np.any(np.abs(x - np.floor(x) - 0.5) < 1e-9, axis=0)


CASES = [  # order, (HII_DIM, HII_D_PARA), fields
    (0, (12, 12), 3), (0, (10, 15), 17), (1, (12, 12), 17), (1, (10, 15), 3),
    (3, (12, 12), 1), (3, (10, 15), 3), (5, (12, 12), 3), (5, (8, 12), 1),
]


@pytest.mark.parametrize("case", CASES, ids=[f"o{c[0]}_{c[1][0]}x{c[1][1]}_f{c[2]}" for c in CASES])
def test_kernel_matches_restatement(gpu_lib, case):
    order, (n, d_para), nf = case
    rng = np.random.default_rng(100 + order * 7 + nf)
    lat, lon = sky()
    nhat = AR.directions(lat, lon, ROT)
    n_pix, n_slices = len(lat), 40
    lcd = 300.0 + 1.5 * np.arange(n_slices)  # cells: far outside the box
    d_lo, d_hi = lcd[3] - 0.25, lcd[33] + 0.5
    names = ["z_reion" if (q == 0 and order <= 1) else f"f{q}" for q in range(nf)]
    lo, hi = {}, {}
    for k in names:
        scale = 10.0 ** rng.uniform(-2, 2)
        lo[k] = (rng.standard_normal((n, n, d_para)) * scale).astype(np.float32)
        hi[k] = (rng.standard_normal((n, n, d_para)) * scale).astype(np.float32)
    want = {k: np.zeros((n_pix, n_slices), np.float32) for k in names}
    AR.fill_slices(want, lcd, d_lo, d_hi, 1.0, lo, hi, nhat, ORIGIN, order)
    # every other field, box and lightcone lives on the device; nhat too when there are several fields
    got = {k: (on_device(np.zeros((n_pix, n_slices), np.float32)) if q % 2 else np.zeros((n_pix, n_slices), np.float32))
           for q, k in enumerate(names)}
    lo_in = {k: (on_device(v) if q % 3 == 1 else v) for q, (k, v) in enumerate(lo.items())}
    hi_in = {k: (on_device(v) if q % 3 == 2 else v) for q, (k, v) in enumerate(hi.items())}
    idx = run_kernel(got, lo_in, hi_in, lcd, d_lo, d_hi, on_device(nhat) if nf > 1 else nhat, order)
    assert list(idx) == list(range(3, 34))
    keep = np.zeros((n_pix, n_slices), bool)
    keep[:, idx] = True
    if order == 0:
        keep[:, idx] &= ~ties(nhat, lcd[idx])
    tol = (1e-6 if order <= 1 else 1e-5)
    for k in names:
        g = to_host(got[k])
        assert not g[:, :3].any() and not g[:, 34:].any(), k  # only the slices of the pair
        scale = max(np.abs(lo[k]).max(), np.abs(hi[k]).max())
        err = np.abs(g.astype(np.float64) - want[k])[keep]
        assert err.max() <= tol * scale, f"{k}: {err.max() / scale:.3g} of max|field|"


@pytest.mark.parametrize("order", [0, 1, 3])
def test_projected_velocity(gpu_lib, order):
    rng = np.random.default_rng(9)
    lat, lon = sky()
    nhat = AR.directions(lat, lon, ROT)
    n_pix, n_slices, n, d_para = len(lat), 12, 9, 14
    lcd = 500.0 + np.arange(n_slices, dtype=float)
    d_lo, d_hi = 499.0, 512.0
    lo = tuple((rng.standard_normal((n, n, d_para)) * 1e-17).astype(np.float32) for _ in range(3))
    hi = tuple((rng.standard_normal((n, n, d_para)) * 1e-17).astype(np.float32) for _ in range(3))
    want = {"los_velocity": np.zeros((n_pix, n_slices), np.float32)}
    AR.fill_slices(want, lcd, d_lo, d_hi, 1.0, {"los_velocity": lo}, {"los_velocity": hi}, nhat, ORIGIN, order)
    got = {"los_velocity": np.zeros((n_pix, n_slices), np.float32), "density": np.zeros((n_pix, n_slices), np.float32)}
    run_kernel(got, {"los_velocity": lo, "density": lo[0]}, {"los_velocity": hi, "density": hi[0]}, lcd, d_lo, d_hi,
               on_device(nhat), order)
    keep = ~ties(nhat, lcd) if order == 0 else np.ones((n_pix, n_slices), bool)
    scale = max(max(np.abs(a).max() for a in lo), max(np.abs(a).max() for a in hi))
    tol = 1e-6 if order <= 1 else 1e-5
    assert np.abs(got["los_velocity"].astype(np.float64) - want["los_velocity"])[keep].max() <= tol * scale
    # a uniform vector field: v . n (order 0 exactly, the others to round-off)
    v = (0.5, -1.25, 2.0)
    uni = tuple(np.full((n, n, d_para), c, np.float32) for c in v)
    got = {"los_velocity": np.zeros((n_pix, n_slices), np.float32)}
    run_kernel(got, {"los_velocity": uni}, {"los_velocity": uni}, lcd, d_lo, d_hi, on_device(nhat), order)
    exact = np.broadcast_to(np.float32(np.einsum("k,kp->p", np.array(v), nhat))[:, None], (n_pix, n_slices))
    if order == 0:
        np.testing.assert_array_equal(got["los_velocity"], exact)
    else:
        np.testing.assert_allclose(got["los_velocity"], exact, rtol=0, atol=1e-6 * 2.0)


def test_reproducible_and_non_finite_boxes(gpu_lib):
    rng = np.random.default_rng(3)
    lat, lon = sky()
    nhat_h = AR.directions(lat, lon, ROT)
    nhat = on_device(nhat_h)
    lcd = 50.0 + np.arange(20.0)
    box = {k: on_device(rng.standard_normal((8, 8, 8)).astype(np.float32)) for k in ("a", "b")}
    outs = []
    for _ in range(2):
        out = {"a": on_device(np.zeros((len(lat), 20), np.float32)), "b": on_device(np.zeros((len(lat), 20), np.float32))}
        run_kernel(out, box, box, lcd, 49.5, 70.0, nhat, 3)
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    # a NaN read by a pixel's taps, and anywhere in a box that is prefiltered
    x = AR.points(nhat_h, lcd[0], ORIGIN)[:, 0]
    bad = box["a"].cpu().numpy()
    bad[tuple(np.mod(np.floor(x).astype(int), 8))] = np.nan
    out = {"a": np.zeros((len(lat), 20), np.float32)}
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        run_kernel(out, {"a": bad}, {"a": box["a"]}, lcd, 49.5, 70.0, nhat, 1)
    inf = box["b"].cpu().numpy()
    inf[7, 0, 3] = np.inf
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        api.spline_prefilter([inf], 5)
    with pytest.raises(pkg.BackendError, match="ValueError"):  # mean_max needs order 0 or 1
        api.lightcone_angular({"z_reion": out["a"]}, {"z_reion": box["a"]}, {"z_reion": box["a"]}, 0,
                              [50.0], [1.0], [1.0], 2.0, nhat, order=3)
    # the prefilter against scipy's, on the device and in place
    c = on_device(box["b"].cpu().numpy())
    api.spline_prefilter([c], 3, out=[c])
    want = AR.periodic_prefilter(box["b"].cpu().numpy(), 3)
    np.testing.assert_allclose(c.cpu().numpy(), want, rtol=0, atol=2e-6 * np.abs(want).max())


def e2e_setup(ts):
    kw = dict(HII_DIM=32, DIM=64, BOX_LEN=64.0, N_THREADS=2, ZPRIME_STEP_FACTOR=1.04, SOURCE_MODEL=1,
              USE_TS_FLUCT=ts, Z_HEAT_MAX=20.0, USE_LYA_HEATING=False, HII_FILTER=0, KEEP_3D_VELOCITIES=True)
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 20.0)
    return kw, nodes, nodes[-1] + 0.15, nodes[0] - 0.15


def test_run_coeval_returns_3d_velocities(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    kw, _, _, _ = e2e_setup(False)
    on = D.run_coeval(D.Inputs(random_seed=4, **kw), [18.0], data_path=DATA, lib=gpu_lib)[18.0]
    kw["KEEP_3D_VELOCITIES"] = False
    off = D.run_coeval(D.Inputs(random_seed=4, **kw), [18.0], data_path=DATA, lib=gpu_lib)[18.0]
    assert "velocity_x" not in off and "velocity_y" not in off
    for k in ("velocity_x", "velocity_y"):
        assert on[k].shape == on["velocity_z"].shape and np.isfinite(on[k]).all() and np.abs(on[k]).max() > 0
    for k in ("density", "velocity_z", "brightness_temp"):
        np.testing.assert_array_equal(on[k], off[k], err_msg=k)
    # the three components are different fields of comparable size
    assert not np.array_equal(on["velocity_x"], on["velocity_y"])
    assert 0.2 < on["velocity_x"].std() / on["velocity_z"].std() < 5


def test_like_rectilinear_against_rectilinear(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    kw, _, _, _ = e2e_setup(False)
    # lower redshifts than the other runs: over the lightcone the angular grid widens by ~6 %, so the two
    # lightcones part at the far end (no evolution: any node redshifts will do)
    nodes = D.get_logspaced_redshifts(8.0, 1.04, 10.0)
    z0, z1 = nodes[-1] + 0.02, nodes[0] - 0.02
    inputs = D.Inputs(random_seed=3, **kw)
    q = ("brightness_temp", "density")
    rect = D.RectilinearLightconer.between_redshifts(z0, z1, 2.0, quantities=q)
    ang = D.AngularLightconer.like_rectilinear(inputs.simulation_options, z0, z1, quantities=q)
    np.testing.assert_array_equal(ang.lc_distances, rect.lc_distances)
    r = D.run_lightcone(inputs, rect, nodes, data_path=DATA, lib=gpu_lib, include_dvdr_in_tau21=False)
    a = D.run_lightcone(D.Inputs(random_seed=3, **kw), ang, nodes, data_path=DATA, lib=gpu_lib, device="cuda",
                        include_dvdr_in_tau21=False)
    n = 32
    assert set(a["lightcones"]) == set(q)
    np.testing.assert_array_equal(a["latitude"], ang.latitude)
    np.testing.assert_array_equal(a["longitude"], ang.longitude)
    np.testing.assert_array_equal(a["lightcone_distances"], r["lightcone_distances"])
    for k in q:
        np.testing.assert_array_equal(a["global_quantities"][k], r["global_quantities"][k])
    rbt = r["lightcones"]["brightness_temp"]
    abt = a["lightcones"]["brightness_temp"].cpu().numpy().reshape(rbt.shape)
    # the reference's test_ang_lightcone (tests/test_high_level_io.py:153-190)
    full0 = np.corrcoef(rbt[:, :, 0].flatten(), abt[:, :, 0].flatten())[0, 1]
    fullz = np.corrcoef(rbt[:, :, -1].flatten(), abt[:, :, -1].flatten())[0, 1]
    assert full0 > fullz and full0 > 0.5, (full0, fullz)
    top = np.corrcoef(rbt[:n // 2, :n // 2, 0].flatten(), abt[:n // 2, :n // 2, 0].flatten())[0, 1]
    bottom = np.corrcoef(rbt[n // 2:, n // 2:, 0].flatten(), abt[n // 2:, n // 2:, 0].flatten())[0, 1]
    assert top > bottom, (top, bottom)
    # pixel (b, l) = (0, 0) of the lowest slice is box cell (0, 0, 0) interpolated between its nodes,
    # which is where the rectilinear lightcone's lowest slice sits (plane 0)
    pair = [(lo, hi) for lo, hi in zip(nodes[1:], nodes[:-1]) if rect.slab_tables(lo, hi, 2.0, n) is not None
            and rect.slab_tables(lo, hi, 2.0, n)[0] == 0]
    assert pair and rect.slab_tables(*pair[0], 2.0, n)[1][0] == 0
    p = (n - 1) * n
    assert ang.latitude[p] == 0 and ang.longitude[p] == 0
    for k in q:
        assert a["lightcones"][k][p, 0].item() == r["lightcones"][k][0, 0, 0], k


@pytest.mark.parametrize("ts", [False, True])
def test_run_lightcone_dvdr_and_rsds(gpu_lib, monkeypatch, ts):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    kw, nodes, z0, z1 = e2e_setup(ts)
    so = D.Inputs(**kw).simulation_options
    q = ("density", "neutral_fraction", "brightness_temp")
    extra = ("los_velocity",) + (("tau_21",) if ts else ())
    ang = D.AngularLightconer.like_rectilinear(so, z0, z1, quantities=q)
    plain_lc = D.AngularLightconer.like_rectilinear(so, z0, z1, quantities=q + extra)
    on = D.run_lightcone(D.Inputs(random_seed=3, **kw), ang, nodes, data_path=DATA, lib=gpu_lib, device="cuda",
                         apply_rsds=True)
    plain = D.run_lightcone(D.Inputs(random_seed=3, **kw), plain_lc, nodes, data_path=DATA, lib=gpu_lib,
                            include_dvdr_in_tau21=False)
    base = set(q) | set(extra)
    got = {k: v.cpu().numpy() for k, v in on["lightcones"].items()}
    assert set(got) == base | {k + "_with_rsds" for k in base}
    assert got["brightness_temp"].shape == (32 * 32, len(ang.lc_distances))
    for k in base - {"brightness_temp"}:
        np.testing.assert_array_equal(got[k], plain["lightcones"][k], err_msg=k)
    H = ang.cosmo.H0_cgs * ang.cosmo.efunc(ang.lc_redshifts)
    pl = plain["lightcones"]
    want_bt = LR.include_dvdr_in_tau21(pl["brightness_temp"], pl["los_velocity"], H, 2.0,
                                       D.Inputs(**kw).astro_params.MAX_DVDR, tau_21=pl["tau_21"] if ts else None)
    np.testing.assert_allclose(got["brightness_temp"], want_bt, rtol=1e-6, atol=1e-6)
    assert not np.array_equal(got["brightness_temp"], pl["brightness_temp"])
    corrected = dict(pl, brightness_temp=got["brightness_temp"])
    for k in base:
        want = RR.apply_rsds(corrected[k], pl["los_velocity"], H, 2.0, periodic=False)
        assert_close_per_column(got[k + "_with_rsds"], want, corrected[k], k)
        if k != "los_velocity":
            assert not np.array_equal(got[k + "_with_rsds"], got[k]), k
    if ts:
        assert np.abs(got["tau_21"]).max() > 0
