"""Redshift-space distortions on the MI355X (csrc/hip/rsd_kernels.hip, csrc/host/rsd_driver.c,
grid_api.rsd_shift, 21cmfast_amd/rsds.py, run_lightcone(apply_rsds=True)).

Kernel level, on seeded random fields and velocities, against the numpy restatement of the reference's
rsds_shift (tests/rsd_reference.py): short and long columns, 1 / 2 / 4 / 5 sub-cells, both
periodicities, 1, 3 and 17 fields (two launches); the reference's own properties (integer shifts are
np.roll, periodic sums are kept, a 2n shift empties a column); bit-reproducibility and host / device
parity; non-finite inputs reported.  End to end: run_lightcone(apply_rsds=True) with and without
USE_TS_FLUCT and with a buffer, and apply_rsds on a run_coeval brightness-temperature box."""

import importlib

import numpy as np
import pytest

import rsd_reference as RR
from test_gpu_run_coeval import DATA

pytestmark = pytest.mark.gpu
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
rsds = importlib.import_module("21cmfast_amd.rsds")
pkg = importlib.import_module("21cmfast_amd")


def random_case(rng, n_cols, n, nf):
    fields = [(rng.standard_normal((n_cols, n)) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32) for _ in range(nf)]
    vel = (rng.standard_normal((n_cols, n)) * 1e-17).astype(np.float32)  # Mpc/s, as los_velocity
    scale = rng.uniform(1.0e17, 4.0e17, n)  # pixels per Mpc/s: a few pixels of displacement
    return fields, vel, scale


def assert_close_per_column(got, want, field, what=""):
    tol = 2e-6 * np.abs(field).max(axis=-1, keepdims=True)
    err = np.abs(np.asarray(got, np.float64) - want)
    assert (err <= tol).all(), f"{what}: worst {float((err / np.maximum(tol, 1e-300)).max())} x tolerance"


CASES = [  # n_slices, n_sub, periodic, n_fields, n_cols
    (2, 1, False, 1, 40), (2, 4, True, 3, 40), (3, 5, False, 17, 40), (3, 2, True, 1, 40),
    (64, 1, True, 3, 40), (64, 4, False, 17, 24), (64, 5, True, 1, 40), (64, 2, False, 3, 40),
    (64, 4, True, 17, 24), (2048, 4, False, 3, 6), (2048, 5, True, 1, 6), (2500, 2, False, 17, 3),
    (4000, 4, False, 1, 4), (20000, 1, True, 3, 2),
]


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_m{c[1]}_{'per' if c[2] else 'open'}_f{c[3]}" for c in CASES])
def test_kernel_matches_restatement(gpu_lib, case):
    n, m, periodic, nf, n_cols = case
    rng = np.random.default_rng(n * 31 + m * 7 + nf)
    fields, vel, scale = random_case(rng, n_cols, n, nf)
    got = api.rsd_shift(fields, vel, scale, n_sub=m, periodic=periodic)
    disp = vel.astype(np.float64) * scale
    for q in range(nf):
        want = RR.rsds_shift(fields[q].T.astype(np.float64), disp.T, n_rsd_subcells=m, periodic=periodic).T
        assert_close_per_column(got[q], want, fields[q], f"field {q}")


@pytest.mark.parametrize("m", [1, 2])
def test_integer_shifts_are_rolls(gpu_lib, m):
    rng = np.random.default_rng(12345)
    box_in = rng.random((10, 5)).astype(np.float32)
    for v in range(-10, 11):
        got = rsds.rsds_shift(box_in, v * np.ones_like(box_in), n_rsd_subcells=m, periodic=True)
        np.testing.assert_allclose(got, np.roll(box_in, v, axis=0), rtol=1e-6, err_msg=str(v))


@pytest.mark.parametrize("m", [1, 2, 4, 5])
def test_periodic_sums_are_kept_and_a_2n_shift_empties_the_column(gpu_lib, m):
    rng = np.random.default_rng(m)
    box_in = rng.random((300, 64)).astype(np.float32)
    disp = (rng.standard_normal(box_in.shape) * 5).astype(np.float32)
    got = rsds.rsds_shift(box_in, disp, n_rsd_subcells=m, periodic=True)
    np.testing.assert_allclose(got.sum(axis=0, dtype=np.float64), box_in.sum(axis=0, dtype=np.float64), rtol=1e-6)
    gone = rsds.rsds_shift(np.ones((10, 5), np.float32), np.full((10, 5), 20.0, np.float32), n_rsd_subcells=m)
    assert not gone.any()


def test_reproducible_and_host_device_parity(gpu_lib):
    import torch

    rng = np.random.default_rng(11)
    fields, vel, scale = random_case(rng, 300, 700, 3)
    a = api.rsd_shift(fields, vel, scale, n_sub=4)
    b = api.rsd_shift(fields, vel, scale, n_sub=4)
    dev = api.rsd_shift([torch.from_numpy(f).cuda() for f in fields], torch.from_numpy(vel).cuda(), scale, n_sub=4)
    mixed = api.rsd_shift([fields[0], torch.from_numpy(fields[1]).cuda(), fields[2]], vel, scale, n_sub=4)
    for q in range(3):
        np.testing.assert_array_equal(a[q], b[q])
        np.testing.assert_array_equal(a[q], dev[q].cpu().numpy())
        np.testing.assert_array_equal(a[q], mixed[q] if q != 1 else mixed[q].cpu().numpy())
    # in place, on the host and on the device; the velocity shifted as one of the fields, in place
    inplace = [f.copy() for f in fields]
    api.rsd_shift(inplace, vel, scale, n_sub=4, out=inplace)
    v_dev = torch.from_numpy(vel).cuda()
    f_dev = [torch.from_numpy(f).cuda() for f in fields] + [v_dev]
    api.rsd_shift(f_dev, v_dev, scale, n_sub=4, out=f_dev)
    v_ref = api.rsd_shift([vel], vel, scale, n_sub=4)[0]
    for q in range(3):
        np.testing.assert_array_equal(a[q], inplace[q])
        np.testing.assert_array_equal(a[q], f_dev[q].cpu().numpy())
    np.testing.assert_array_equal(v_ref, f_dev[3].cpu().numpy())


def test_non_finite_inputs_and_bad_shapes_are_errors(gpu_lib):
    rng = np.random.default_rng(5)
    fields, vel, scale = random_case(rng, 8, 50, 2)
    bad_v = vel.copy()
    bad_v[3, 17] = np.nan
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        api.rsd_shift(fields, bad_v, scale)
    bad_f = fields[1].copy()
    bad_f[0, 0] = np.inf
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        api.rsd_shift([fields[0], bad_f], vel, scale)
    with pytest.raises(pkg.BackendError, match="ValueError"):
        api.rsd_shift([f[:, :1].copy() for f in fields], vel[:, :1].copy(), scale[:1])
    with pytest.raises(pkg.BackendError, match="ValueError"):
        api.rsd_shift(fields, vel, scale, n_sub=0)
    long_col = np.zeros((1, 30000), np.float32)
    with pytest.raises(pkg.BackendError, match="ValueError"):  # more accumulators than the LDS holds
        api.rsd_shift([long_col], long_col, 1.0)


def lightcone_setup(ts):
    kw = dict(HII_DIM=32, DIM=64, BOX_LEN=64.0, N_THREADS=2, ZPRIME_STEP_FACTOR=1.04, SOURCE_MODEL=1,
              USE_TS_FLUCT=ts, Z_HEAT_MAX=20.0, USE_LYA_HEATING=False, HII_FILTER=0)
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 20.0)
    q = ("density", "neutral_fraction", "brightness_temp")
    lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.15, nodes[0] - 0.15, 2.0, quantities=q)
    return kw, nodes, lc


def want_rsds(lcs, lc, m=4):
    H = lc.cosmo.H0_cgs * lc.cosmo.efunc(lc.lc_redshifts)
    return {k: RR.apply_rsds(v, lcs["los_velocity"], H, 2.0, periodic=False, n_rsd_subcells=m)
            for k, v in lcs.items()}


@pytest.mark.parametrize("ts", [False, True])
def test_run_lightcone_with_rsds(gpu_lib, monkeypatch, ts):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    kw, nodes, lc = lightcone_setup(ts)
    assert len(nodes) >= 3

    def run(lcn=lc, **o):
        return D.run_lightcone(D.Inputs(random_seed=3, **kw), lcn, nodes, data_path=DATA, lib=gpu_lib, **o)

    plain = run()
    host = run(apply_rsds=True)
    dev = run(apply_rsds=True, device="cuda")
    base = set(lc.quantities) | {"los_velocity"} | ({"tau_21"} if ts else set())
    assert set(plain["lightcones"]) == base
    assert set(host["lightcones"]) == base | {k + "_with_rsds" for k in base}
    for k, v in host["lightcones"].items():
        np.testing.assert_array_equal(v, dev["lightcones"][k].cpu().numpy(), err_msg=k)
    for k in base:
        np.testing.assert_array_equal(host["lightcones"][k], plain["lightcones"][k], err_msg=k)
    np.testing.assert_array_equal(host["lightcone_distances"], lc.lc_distances)
    want = want_rsds(plain["lightcones"], lc)
    for k in base:
        got = host["lightcones"][k + "_with_rsds"]
        assert_close_per_column(got, want[k], plain["lightcones"][k], k)
        if k != "los_velocity":
            assert not np.array_equal(got, plain["lightcones"][k]), k

    # a buffer of 3 slices at both ends: built on the extended lightconer, shifted, then trimmed
    buf = run(apply_rsds=True, rsd_buffer_slices=(3, 3))
    ext = lc.extended(3, 3)
    ext_plain = run(lcn=ext)
    n = len(lc.lc_distances)
    np.testing.assert_array_equal(buf["lightcone_distances"], lc.lc_distances)
    np.testing.assert_array_equal(buf["lightcone_redshifts"], lc.lc_redshifts)
    want = want_rsds(ext_plain["lightcones"], ext)
    for k in base:
        np.testing.assert_array_equal(buf["lightcones"][k], ext_plain["lightcones"][k][..., 3:3 + n], err_msg=k)
        assert buf["lightcones"][k + "_with_rsds"].shape[-1] == n
        assert_close_per_column(buf["lightcones"][k + "_with_rsds"], want[k][..., 3:3 + n],
                                ext_plain["lightcones"][k][..., 3:3 + n], k)


def test_apply_rsds_on_a_coeval_box(gpu_lib, monkeypatch):
    import torch

    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    inputs = D.Inputs(random_seed=4, HII_DIM=32, DIM=64, BOX_LEN=64.0, N_THREADS=2, SOURCE_MODEL=1, HII_FILTER=0)
    snap = D.run_coeval(inputs, [18.0], data_path=DATA, lib=gpu_lib)[18.0]
    bt, vz = np.asarray(snap["brightness_temp"]), np.asarray(snap["velocity_z"])
    got = rsds.apply_rsds(bt, vz, 18.0, inputs, periodic=True)
    cosmo = D.FlatCosmology(inputs.cosmo_params.hlittle, inputs.cosmo_params.OMm)
    want = RR.apply_rsds(bt, vz, cosmo.H0_cgs * cosmo.efunc(18.0), 2.0, periodic=True)
    assert got.shape == bt.shape and got.dtype == np.float32
    assert_close_per_column(got, want, bt, "brightness_temp")
    np.testing.assert_allclose(got.sum(axis=-1, dtype=np.float64), bt.sum(axis=-1, dtype=np.float64), rtol=1e-5,
                               atol=1e-6 * np.abs(bt).max())
    dev = rsds.apply_rsds(torch.from_numpy(bt).cuda(), torch.from_numpy(vz).cuda(), 18.0, inputs, periodic=True)
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)
