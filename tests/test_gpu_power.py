"""21cmfast_amd.powerspec on the MI355X against the host restatement (tests/power_reference.py), the
reference's fixtures through the device spectrum, bit parity between calls, numpy / torch round trips and
the NaN error.

Tolerances: counts exactly, k to 1e-12 (|k| is numpy's to the bit, the sums are fp64), power to
POWER_RTOL of the restatement's fp64 spectrum (the transform is fp32; observed worst deviation is printed).
Bins whose power is <= 1e-20 of the largest are compared absolutely, as tests/test_gpu_lightcone.py does."""

import importlib
from pathlib import Path

import numpy as np
import pytest

import power_reference as PR
import refpin as RP

pytestmark = pytest.mark.gpu
PS = importlib.import_module("21cmfast_amd.powerspec")
D = importlib.import_module("21cmfast_amd.drivers")
DATA = Path(__file__).parent / "golden" / "reference" / "_data"

POWER_RTOL = 2e-5
SHAPES = [(64, 64, 64), (50, 50, 50), (96, 96, 96), (32, 32, 100), (33, 35, 37)]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _field(shape, seed=11, mean=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + mean).astype(np.float32)


def check_power(got, ref, rtol=POWER_RTOL, atol_frac=1e-20, what=""):
    got, ref = _np(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    g, r = got[ok], ref[ok]
    noise = atol_frac * np.max(np.abs(r)) if r.size else 0.0
    real = np.abs(r) > noise
    assert np.all(np.abs(g[~real] - r[~real]) <= noise), what
    dev = float(np.max(np.abs(g[real] / r[real] - 1))) if real.any() else 0.0
    print(f"{what}: worst relative power deviation {dev:.2e}")
    assert dev <= rtol, (what, dev)
    return dev


def check_all(got, ref, what):
    p, k, c = got
    rp, rk, rc = ref
    assert np.array_equal(_np(c), rc), what
    np.testing.assert_allclose(_np(k), rk, rtol=1e-12, atol=0, err_msg=what)
    return check_power(p, rp, what=what)


@pytest.mark.parametrize("shape", SHAPES)
def test_get_power_defaults_equal_the_restatement(gpu_lib, shape):
    f = _field(shape)
    L = (100.0, 80.0, 120.0) if len(set(shape)) > 1 else 100.0
    got = PS.get_power(f, L, return_counts=True)
    ref = PR.get_power(f, L, return_counts=True)
    check_all(got, ref, f"{shape}")
    assert isinstance(got[0], np.ndarray) and got[0].dtype == np.float64 and got[2].dtype == np.int64


@pytest.mark.parametrize("opts", [
    dict(log_bins=True), dict(bins=np.array([0.0, 0.1, 0.25, 0.5, 1.0, 1.7])), dict(bins=9),
    dict(ignore_zero_mode=True), dict(ignore_kperp_zero=True), dict(ignore_kpar_zero=True),
    dict(bins_upto_boxlen=False), dict(bin_ave=False),
], ids=lambda o: ",".join(o))
def test_get_power_options(gpu_lib, opts):
    shape, L = (33, 35, 37), (70.0, 75.0, 80.0)
    f = _field(shape, seed=5)
    got = PS.get_power(f, L, return_counts=True, **opts)
    ref = PR.get_power(f, L, return_counts=True, **opts)
    check_all(got, ref, str(opts))


def test_cross_power(gpu_lib):
    shape, L = (32, 32, 100), (50.0, 50.0, 156.25)
    f, g = _field(shape, 1), _field(shape, 2)
    h = (f + 0.5 * g).astype(np.float32)
    got = PS.get_power(f, L, deltax2=h, return_counts=True)
    ref = PR.get_power(f, L, deltax2=h, return_counts=True)
    check_all(got, ref, "cross")


@pytest.mark.parametrize("opts", [dict(), dict(log_bins=True, ignore_zero_mode=True),
                                  dict(kperp_bins=[0.0, 0.3, 0.9, 2.0], kpar_bins=4)], ids=["default", "log", "edges"])
def test_cylindrical_power(gpu_lib, opts):
    shape, L = (33, 35, 37), (70.0, 75.0, 80.0)
    f = _field(shape, seed=9)
    p, kp, kz, c = PS.get_cylindrical_power(f, L, return_counts=True, **opts)
    rp, rkp, rkz, rc = PR.get_cylindrical_power(f, L, return_counts=True, **opts)
    assert np.array_equal(c, rc)
    np.testing.assert_allclose(kp, rkp, rtol=1e-12, atol=0)
    np.testing.assert_allclose(kz, rkz, rtol=1e-12, atol=0)
    check_power(p, rp, what=f"cylindrical {opts}")
    # cross power through the cylindrical path as well
    g = (f * 0.5 + 0.25).astype(np.float32)
    pc = PS.get_cylindrical_power(f, L, deltax2=g, **opts)[0]
    check_power(pc, PR.get_cylindrical_power(f, L, deltax2=g, **opts)[0], what="cylindrical cross")


def test_two_calls_give_the_same_bits(gpu_lib):
    f = _field((96, 96, 96), seed=3)
    a = PS.get_power(f, 100.0, return_counts=True)
    b = PS.get_power(f, 100.0, return_counts=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)
    lc = _field((32, 32, 160), seed=4)
    a = PS.lightcone_power_spectra(lc, 2.0, cylindrical=True)
    b = PS.lightcone_power_spectra(lc, 2.0, cylindrical=True)
    assert np.array_equal(a.power, b.power, equal_nan=True) and np.array_equal(a.kperp, b.kperp, equal_nan=True)


def test_torch_in_torch_out(gpu_lib):
    import torch

    f = _field((50, 50, 50), seed=8)
    t = torch.from_numpy(f).to("cuda:0")
    p, k, c = PS.get_power(t, 100.0, return_counts=True)
    assert all(isinstance(x, torch.Tensor) and x.device == t.device for x in (p, k, c))
    ref = PS.get_power(f, 100.0, return_counts=True)
    for x, y in zip((p, k, c), ref):
        assert np.array_equal(x.cpu().numpy(), y, equal_nan=True)
    e = PS.get_power(t, 100.0, bin_ave=False)[1]
    assert isinstance(e, torch.Tensor) and e.device == t.device
    pc = PS.get_cylindrical_power(t, 100.0)[0]
    assert isinstance(pc, torch.Tensor) and pc.device == t.device
    lc = PS.lightcone_power_spectra(torch.from_numpy(_field((32, 32, 96))).to("cuda:0"), 1.5, dimensionless=True)
    assert isinstance(lc.power, torch.Tensor) and lc.power.device == t.device


def test_nan_input_is_an_error(gpu_lib):
    pkg = importlib.import_module("21cmfast_amd")
    f = _field((32, 32, 32))
    f[3, 4, 5] = np.nan
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_power(f, 50.0)
    f[3, 4, 5] = np.inf
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_cylindrical_power(f, 50.0)
    g = _field((32, 32, 32))
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.get_power(g, 50.0, deltax2=f)
    lc = _field((16, 16, 64))
    lc[1, 1, 40] = np.nan
    with pytest.raises(pkg.BackendError, match="InfinityorNaN"):
        PS.lightcone_power_spectra(lc, 1.0)
    # the NaN is outside every chunk: a spectrum
    assert np.isfinite(PS.lightcone_power_spectra(lc, 1.0, chunk_starts=[0, 20]).k).all()


@pytest.mark.parametrize("kw", [
    dict(), dict(chunk_length=24), dict(chunk_starts=[0, 5, 37], chunk_length=20), dict(dimensionless=True),
    dict(cylindrical=True), dict(cylindrical=True, dimensionless=True, kpar_bins=5),
    dict(log_bins=True, ignore_kpar_zero=True),
], ids=["cubic", "noncubic", "starts", "dimensionless", "cyl", "cyl-dimless", "log"])
def test_lightcone_chunks_equal_the_restatement(gpu_lib, kw):
    lc = _field((24, 20, 100), seed=21)
    z = np.linspace(6.0, 9.0, 100)
    got = PS.lightcone_power_spectra(lc, 1.7, redshifts=z, **kw)
    ref = PR.lightcone_power_spectra(lc, 1.7, redshifts=z, **kw)
    assert np.array_equal(got.chunk_starts, ref["chunk_starts"])
    np.testing.assert_array_equal(got.redshifts, ref["redshifts"])
    assert np.array_equal(got.counts, ref["counts"])
    if kw.get("cylindrical"):
        np.testing.assert_allclose(got.kperp, ref["kperp"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got.kpar, ref["kpar"], rtol=1e-12, atol=0)
    else:
        np.testing.assert_allclose(got.k, ref["k"], rtol=1e-12, atol=0)
    assert got.power.shape[0] == len(ref["chunk_starts"])
    for c in range(got.power.shape[0]):
        check_power(got.power[c], ref["power"][c], what=f"chunk {c} {kw}")


# ---- the reference's fixtures through the device spectrum --------------------------------------------
TESTRUN = dict(HII_DIM=RP.HII_DIM, DIM=RP.DIM, BOX_LEN=RP.BOX_LEN, N_THREADS=2,
               ZPRIME_STEP_FACTOR=1.04, HII_FILTER=0, USE_EXP_FILTER=False, CELL_RECOMB=False,
               USE_UPPER_STELLAR_TURNOVER=False, USE_LYA_HEATING=False)  # as tests/test_gpu_run_coeval.py


def test_device_spectrum_reproduces_coeval_fixture(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    inputs = D.Inputs(random_seed=RP.SEED, **{**TESTRUN, "SOURCE_MODEL": 1})
    snap = D.run_coeval(inputs, [18.0], data_path=DATA, device="cuda", lib=gpu_lib)[18.0]
    f = RP.fixture("power_spectra", "simple")
    # the host-binned tests' tolerances (tests/test_gpu_run_coeval.py): density 4e-4, the others 2e-3
    for key, tol in (("density", 4e-4), ("brightness_temp", 2e-3)):
        p, k = PS.get_power(snap[key], RP.BOX_LEN)
        p, k = _np(p), _np(k)
        np.testing.assert_allclose(k, f["coeval/k"], rtol=1e-12)
        dev = float(np.max(np.abs(p / f[f"coeval/power_{key}"] - 1)))
        print(key, dev)
        assert dev < tol, key


def test_device_spectrum_reproduces_lightcone_fixture(gpu_lib, monkeypatch):
    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    inputs = D.Inputs(random_seed=RP.SEED, **{**TESTRUN, "SOURCE_MODEL": 1})
    nodes = D.get_logspaced_redshifts(18.0, 1.04, 35.0 if inputs.evolution_required else 20.0)
    lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.2, nodes[0] - 0.2, RP.BOX_LEN / RP.HII_DIM,
                                                   quantities=["brightness_temp"])
    res = D.run_lightcone(inputs, lc, nodes, data_path=DATA, device="cuda", lib=gpu_lib)
    f = RP.fixture("power_spectra", "simple")
    a = res["lightcones"]["brightness_temp"]
    dims = lc.lightcone_dimensions(inputs.simulation_options)
    p, k = PS.get_power(a, dims)
    p, k = _np(p), _np(k)
    np.testing.assert_allclose(k, f["lightcone/k"], rtol=1e-12)
    dev = float(np.max(np.abs(p / f["lightcone/power_brightness_temp"] - 1)))
    print("lightcone brightness_temp", dev)
    assert dev < 2e-3
