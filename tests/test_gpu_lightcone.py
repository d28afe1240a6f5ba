"""Rectilinear lightcones on the MI355X (csrc/hip/lightcone_kernels.hip, csrc/host/lightcone_driver.c,
drivers.run_lightcone).

Kernel level, on seeded synthetic boxes, against the numpy restatement of the reference's lightconer
(tests/lightcone_reference.py): the slab kernel within 1 fp32 ulp over cubic, odd, non-cubic boxes,
runs of one slice and runs longer than HII_D_PARA, mean_max sign cases; the dv/dr kernel at rtol 1e-6
in both branches; host and device pointers bit-identical; malformed specs rejected.

End to end, against the reference's own lightcone fixtures (tests/golden/reference/power_spectra_*.h5,
group ``lightcone``): run_lightcone with the fixtures' inputs (TESTRUN of test_gpu_run_coeval.py,
nodes of get_node_z(18, lc=True), the lightconer of produce_integration_test_data.py:395-426), the
binned power of every lightcone field and the global means of every node."""

import ctypes as C
import importlib
import time

import numpy as np
import pytest

import lightcone_reference as LR
import refpin as RP
from test_gpu_run_coeval import DATA, TESTRUN

pytestmark = pytest.mark.gpu
D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")
api = importlib.import_module("21cmfast_amd.grid_api")


def synthetic(rng, n, d_para, fields):
    out = {}
    for k in fields:
        a = rng.standard_normal((n, n, d_para)).astype(np.float32)
        if k == "z_reion":  # -1 where not yet ionised, else a redshift; some tiny and mixed values
            a = np.where(a > 0.3, np.float32(-1.0), (8 + 4 * np.abs(a)).astype(np.float32)).astype(np.float32)
            a[0, 0, :3] = (1e-30, -1e-30, 0.0)  # fp32 product underflows / is zero: no flag
        out[k] = a
    return out


def run_case(n, d_para, n_slices, node_slices, seed, device):
    """Lightcone of n_slices slices, one cell apart; node distances at the given fractional slice
    positions.  Returns (got, want) dicts."""
    import torch

    rng = np.random.default_rng(seed)
    cell = 1.5
    lcd = 1000.0 + cell * np.arange(n_slices)
    fields = ("density", "z_reion", "brightness_temp")
    nodes = [1000.0 + cell * s for s in node_slices]  # ascending distance = descending redshift
    boxes = [synthetic(rng, n, d_para, fields) for _ in nodes]
    want = {k: np.zeros((n, n, n_slices), np.float32) for k in fields}
    got = {k: np.zeros((n, n, n_slices), np.float32) for k in fields}
    if device:
        got = {k: torch.from_numpy(v).cuda() for k, v in got.items()}
    offset = n_slices
    runs = []
    for j in range(len(nodes) - 1):  # high-redshift pair first, as the node loop goes
        hi_i, lo_i = len(nodes) - 1 - j, len(nodes) - 2 - j
        d_lo, d_hi = nodes[lo_i], nodes[hi_i]
        LR.fill_slices(want, lcd, d_lo, d_hi, cell, boxes[lo_i], boxes[hi_i], offset)
        idx, plane, w_lo, w_hi, w_norm = LR.tables(lcd, d_lo, d_hi, cell, offset, d_para)
        if len(idx) == 0:
            continue
        runs.append(len(idx))
        src_lo, src_hi = boxes[lo_i], boxes[hi_i]
        if device:
            src_lo = {k: torch.from_numpy(v).cuda() for k, v in src_lo.items()}
            src_hi = {k: torch.from_numpy(v).cuda() for k, v in src_hi.items()}
        api.lightcone_slices(got, src_lo, src_hi, int(idx[0]), plane, w_lo, w_hi, w_norm)
    if device:
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
    return got, want, runs


# (HII_DIM, HII_D_PARA, n_slices, node positions in slices)
SLAB_CASES = {
    "cubic50": (50, 50, 88, [-0.4, 20.3, 55.7, 87.6]),
    "odd37": (37, 37, 23, [-0.2, 7.5, 22.5]),
    "noncubic": (24, 29, 61, [-0.5, 30.2, 60.9]),
    "run_of_one": (16, 16, 9, [-0.5, 0.5, 1.5, 8.5]),
    "longer_than_d_para": (12, 5, 40, [-0.5, 39.5]),
}


@pytest.mark.parametrize("case", sorted(SLAB_CASES))
def test_slab_kernel_matches_restatement(gpu_lib, case):
    n, d_para, n_slices, nodes = SLAB_CASES[case]
    got, want, runs = run_case(n, d_para, n_slices, nodes, seed=11, device=True)
    if case == "run_of_one":
        assert 1 in runs
    if case == "longer_than_d_para":
        assert max(runs) > d_para
    for k in want:
        np.testing.assert_array_max_ulp(got[k], want[k], maxulp=1)
    # mean_max: every flagged cell took the larger node value, nothing else did
    assert np.any(got["z_reion"] == -1.0) and np.all(np.isfinite(got["z_reion"]))
    host, _, _ = run_case(n, d_para, n_slices, nodes, seed=11, device=False)
    for k in want:  # host pointers: staged, same kernel, same bits
        np.testing.assert_array_equal(host[k], got[k])


def test_slab_kernel_mean_max_sign_cases(gpu_lib):
    import torch

    a = np.array([[[-1.0, 9.0, -1.0, 9.0, 1e-30, 0.0, 7.0, -2.0]]], np.float32)
    b = np.array([[[-1.0, -1.0, 10.0, 10.0, -1e-30, -1.0, 0.0, -3.0]]], np.float32)
    a, b = np.repeat(a, 2, 0).repeat(2, 1), np.repeat(b, 2, 0).repeat(2, 1)
    d = a.shape[2]
    lc = torch.zeros((2, 2, d), dtype=torch.float32, device="cuda")
    plane = np.arange(d, dtype=np.int32)
    w_lo, w_hi = np.full(d, 0.25), np.full(d, 0.75)
    api.lightcone_slices({"z_reion": lc}, {"z_reion": torch.from_numpy(a).cuda()},
                         {"z_reion": torch.from_numpy(b).cuda()}, 0, plane, w_lo, w_hi, 1.0)
    got = lc.cpu().numpy()[0, 0]
    mean = np.float32(0.25 * a[0, 0].astype(np.float64) + 0.75 * b[0, 0].astype(np.float64))
    want = np.where(a[0, 0] * b[0, 0] < 0, np.maximum(a[0, 0], b[0, 0]), mean)
    np.testing.assert_array_equal(got, want)
    assert got[1] == 9.0 and got[2] == 10.0 and got[0] == -1.0 and got[4] == mean[4]


@pytest.mark.parametrize("use_ts", [False, True])
@pytest.mark.parametrize("n_slices", [3, 64])
def test_dvdr_kernel_matches_restatement(gpu_lib, use_ts, n_slices):
    import torch

    rng = np.random.default_rng(5 + n_slices)
    n, dx = 20, 2.0
    H = 2.2e-18 * (1 + np.linspace(18, 12, n_slices)) ** 1.5 / 19 ** 1.5
    # gradients of order H: the clip at 0.2 H engages in part of the cells
    vel = (rng.standard_normal((n, n, n_slices)) * 0.3 * H * dx).astype(np.float32)
    bt = (rng.standard_normal((n, n, n_slices)) * 20).astype(np.float32)
    tau = (np.abs(rng.standard_normal((n, n, n_slices))) * 0.05).astype(np.float32) if use_ts else None
    if use_ts:
        tau[0, :, :] = 1e-11  # below the 1e-10 threshold
        tau[1, :, :] = 0.0
    want = LR.include_dvdr_in_tau21(bt, vel, H, dx, 0.2, tau_21=tau)
    if not use_ts:  # the clip does engage
        g = np.gradient(vel.astype(np.float64), dx, axis=-1, edge_order=2)
        assert np.mean(np.abs(g) > 0.2 * H) > 0.1
    d_bt = torch.from_numpy(bt).cuda()
    api.lightcone_dvdr(d_bt, torch.from_numpy(vel).cuda(), H, dx, 0.2,
                       tau_21=None if tau is None else torch.from_numpy(tau).cuda())
    got = d_bt.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-30)
    if use_ts:
        np.testing.assert_array_equal(got[:2], bt[:2])
    h_bt = bt.copy()
    api.lightcone_dvdr(h_bt, vel, H, dx, 0.2, tau_21=tau)
    np.testing.assert_array_equal(h_bt, got)


def test_malformed_specs_are_rejected(gpu_lib):
    lib = gpu_lib
    lib.c21cm_last_error.restype = C.c_char_p
    box = np.zeros((4, 4, 6), np.float32)
    lc = np.zeros((4, 4, 10), np.float32)
    ptr = lambda a: (C.c_void_p * 1)(a.ctypes.data)  # noqa: E731
    plane = np.array([0, 1, 2], np.int32)
    w = np.ones(3)

    def slab(**kw):
        spec = dict(hii_dim=4, hii_d_para=6, n_slices=10, i0=2, i1=5, n_fields=1, mean_max=0,
                    plane=plane.ctypes.data_as(C.POINTER(C.c_int)), w_lo=w.ctypes.data_as(S.c_double_p),
                    w_hi=w.ctypes.data_as(S.c_double_p), w_norm=2.0)
        spec.update(kw)
        st = lib.c21cm_lightcone_slab_grids(C.byref(S.LightconeSpec(**spec)), ptr(box), ptr(box), ptr(lc), None)
        return st, lib.c21cm_last_error().decode()

    assert slab()[0] == 0
    for kw, msg in [(dict(n_slices=0, i0=0, i1=0), "zero slices"), (dict(i1=11), "outside the lightcone"),
                    (dict(i0=5, i1=5), "empty"), (dict(n_fields=17), "n_fields"),
                    (dict(w_norm=0.0), "w_norm"), (dict(hii_d_para=2), "plane index 2")]:
        st, err = slab(**kw)
        assert st == 3 and msg in err, (kw, err)
    bad = np.array([0, 6, 1], np.int32)
    st, err = slab(plane=bad.ctypes.data_as(C.POINTER(C.c_int)))
    assert st == 3 and "plane index 6 of slice 3" in err
    hub = np.full(10, 1e-18)

    def dvdr(n_slices=10, tau=None, **kw):
        spec = dict(hii_dim=4, n_slices=n_slices, dx=2.0, max_dvdr=0.2, use_ts_fluct=0,
                    hubble=hub.ctypes.data_as(S.c_double_p))
        spec.update(kw)
        a = np.zeros((4, 4, n_slices), np.float32)
        st = lib.c21cm_lightcone_dvdr_grids(C.byref(S.DvdrSpec(**spec)), C.c_void_p(a.ctypes.data),
                                            C.c_void_p(a.ctypes.data), tau, None)
        return st, lib.c21cm_last_error().decode()

    assert dvdr()[0] == 0
    for kw, msg in [(dict(n_slices=2), "at least 3 slices"), (dict(use_ts_fluct=1), "tau_21"),
                    (dict(dx=0.0), "dx"), (dict(hubble=None), "H(z)")]:
        st, err = dvdr(**kw)
        assert st == 3 and msg in err, (kw, err)
    with pytest.raises(ValueError, match="one H"):
        api.lightcone_dvdr(np.zeros((4, 4, 5), np.float32), np.zeros((4, 4, 5), np.float32), hub, 2.0, 0.2)


# ------------------------------------------------------------------------------ end to end
FIXTURE_OPTS = {
    "simple": dict(SOURCE_MODEL=1),
    "no-mdz": dict(SOURCE_MODEL=0),
    "fixed_halogrids": dict(SOURCE_MODEL=2),
    "homo": dict(SOURCE_MODEL=1, RECOMB_MODEL=1, CELL_RECOMB=True, R_BUBBLE_MAX=50.0),
    "inhomo": dict(SOURCE_MODEL=1, RECOMB_MODEL=2, R_BUBBLE_MAX=50.0),
    "ts": dict(SOURCE_MODEL=1, USE_TS_FLUCT=True),
    "ts_nomdz": dict(SOURCE_MODEL=0, USE_TS_FLUCT=True),
    "multiple_scattering": dict(SOURCE_MODEL=2, USE_TS_FLUCT=True, LYA_MULTIPLE_SCATTERING=True),
}
# worst relative deviation of the binned lightcone power allowed per field; default 2e-3 (the coeval
# pins of test_gpu_run_coeval.py), density 4e-4
POWER_TOL = {"density": 4e-4}
GLOBAL_RTOL = {"brightness_temp": 1e-3, "neutral_fraction": 2e-5}


def fixture_run(lib, name, device):
    inputs = D.Inputs(random_seed=RP.SEED, **{**TESTRUN, **FIXTURE_OPTS[name]})
    evolution = inputs.evolution_required
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 35.0 if evolution else 20.0)
    f = RP.fixture("power_spectra", name)
    fields = [k[len("power_"):] for k in f.keys("lightcone") if k.startswith("power_")]
    lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.2, nodes[0] - 0.2, RP.BOX_LEN / RP.HII_DIM,
                                                   quantities=fields)
    t0 = time.perf_counter()
    res = D.run_lightcone(inputs, lc, nodes, data_path=DATA, device=device, lib=lib)
    return inputs, lc, res, f, fields, time.perf_counter() - t0


@pytest.mark.parametrize("name", list(FIXTURE_OPTS))
def test_run_lightcone_reproduces_reference_fixture(gpu_lib, monkeypatch, name):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    device = "cuda" if name in ("simple", "fixed_halogrids", "ts", "homo") else None
    inputs, lc, res, f, fields, wall = fixture_run(gpu_lib, name, device)
    dims = lc.lightcone_dimensions(inputs.simulation_options)
    worst, large = {}, {}
    for k in fields:
        a = res["lightcones"][k]
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        assert a.shape == lc.get_shape(inputs.simulation_options) and np.isfinite(a).all(), k
        p, kk = RP.get_power(a, dims)
        np.testing.assert_allclose(kk, f["lightcone/k"], rtol=1e-12)
        ref = f[f"lightcone/power_{k}"]
        # Fields that are constant in these runs (Gamma_12 and, homogeneous recombinations, the
        # recombination count are 0 before reionisation; z_reion is -1 everywhere when no cell has
        # ionised): the fixture's bins are 0 or the round-off of the transform of a constant,
        # <= 1e-20 of its largest bin.  Those bins are compared absolutely, the others relatively.
        noise = 1e-20 * np.max(np.abs(ref))
        real = np.abs(ref) > noise
        assert np.all(np.abs(p[~real]) <= noise), (k, p[~real], ref[~real])
        dev = np.where(real, np.abs(p / np.where(real, ref, 1.0) - 1), 0.0)
        worst[k], large[k] = float(np.max(dev)), float(np.max(dev[:5]))
    gdev = {}
    for k in ("brightness_temp", "neutral_fraction"):
        ref = f[f"lightcone/global_{k}"]
        got = res["global_quantities"][k]
        assert len(got) == len(ref) == len(res["node_redshifts"])
        gdev[k] = float(np.max(np.abs(got / ref - 1)))
    print(f"\n{name}: {len(res['node_redshifts'])} nodes, {wall:.1f} s, device={device}")
    print("  power, worst relative deviation:", {k: f"{v:.2e}" for k, v in worst.items()})
    print("  power, five largest scales     :", {k: f"{v:.2e}" for k, v in large.items()})
    print("  globals, worst relative        :", {k: f"{v:.2e}" for k, v in gdev.items()})
    failures = []
    for k in fields:
        if name == "ts_nomdz":  # the wider pin of the coeval box (test_gpu_reference_fixtures_ts.py)
            if large[k] >= 4e-3 or worst[k] >= 1.5e-2:
                failures.append(k)
        elif worst[k] >= POWER_TOL.get(k, 2e-3):
            failures.append(k)
    for k, v in gdev.items():
        if v >= GLOBAL_RTOL[k] * (2 if name == "ts_nomdz" else 1):
            failures.append(f"global_{k}")
    assert not failures, failures


def test_device_and_host_lightcones_are_bit_identical_and_dvdr_is_the_only_change(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    kw = dict(HII_DIM=32, DIM=64, BOX_LEN=64.0, N_THREADS=2, ZPRIME_STEP_FACTOR=1.04, SOURCE_MODEL=1,
              USE_TS_FLUCT=True, Z_HEAT_MAX=20.0, USE_LYA_HEATING=False, HII_FILTER=0)
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 20.0)
    q = ("density", "z_reion", "neutral_fraction", "brightness_temp", "spin_temperature")
    lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.1, nodes[0] - 0.1, 2.0, quantities=q)
    on = D.run_lightcone(D.Inputs(random_seed=3, **kw), lc, nodes, data_path=DATA, device="cuda", lib=gpu_lib)
    off = D.run_lightcone(D.Inputs(random_seed=3, **kw), lc, nodes, data_path=DATA, device=None, lib=gpu_lib)
    plain = D.run_lightcone(D.Inputs(random_seed=3, **kw), lc, nodes, data_path=DATA, device=None, lib=gpu_lib,
                            include_dvdr_in_tau21=False)
    assert set(on["lightcones"]) == set(q) | {"los_velocity", "tau_21"}
    assert set(plain["lightcones"]) == set(q)
    for k, v in on["lightcones"].items():
        np.testing.assert_array_equal(v.cpu().numpy(), off["lightcones"][k], err_msg=k)
    for k in q:
        if k != "brightness_temp":
            np.testing.assert_array_equal(plain["lightcones"][k], off["lightcones"][k], err_msg=k)
        np.testing.assert_array_equal(on["global_quantities"][k], off["global_quantities"][k])
    # the uncorrected lightcone, corrected by the restatement, is the corrected one
    H = lc.cosmo.H0_cgs * lc.cosmo.efunc(on["lightcone_redshifts"])
    want = LR.include_dvdr_in_tau21(plain["lightcones"]["brightness_temp"], off["lightcones"]["los_velocity"], H,
                                    2.0, D.Inputs(**kw).astro_params.MAX_DVDR, tau_21=off["lightcones"]["tau_21"])
    np.testing.assert_allclose(off["lightcones"]["brightness_temp"], want, rtol=1e-6, atol=1e-6)
    assert not np.array_equal(off["lightcones"]["brightness_temp"], plain["lightcones"]["brightness_temp"])
