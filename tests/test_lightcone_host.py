"""CPU checks of the lightcone path: the numpy restatement the GPU tests compare against gives known
answers (tests/lightcone_reference.py), run_lightcone validates its arguments as the reference's
validate_options does before any GPU work, and the ctypes mirrors of the two new specs agree with
the C layout of include/c21cm_grid.h."""

import ctypes as C
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lightcone_reference as LR

D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")
ROOT = Path(__file__).resolve().parent.parent


def test_interpolation_known_answers():
    a = np.array([1.0, -2.0, 3.0, -1.0, 0.0], np.float32)
    b = np.array([3.0, 4.0, -5.0, -3.0, 2.0], np.float32)
    # on the low node, on the high node, half way
    np.testing.assert_array_equal(LR.redshift_interpolation(10.0, a, b, 10.0, 12.0), a)
    np.testing.assert_array_equal(LR.redshift_interpolation(12.0, a, b, 10.0, 12.0), b)
    np.testing.assert_allclose(LR.redshift_interpolation(11.0, a, b, 10.0, 12.0), (a + b) / 2)
    # mean_max: where the two differ in sign (z_reion = -1 not yet ionised) the larger value
    got = LR.redshift_interpolation(11.5, a, b, 10.0, 12.0, kind="mean_max")
    np.testing.assert_allclose(got, [2.5, 4.0, 3.0, -2.5, 1.5])
    with pytest.raises(ValueError):
        LR.redshift_interpolation(11.0, a, b, 10.0, 12.0, kind="nearest")


def test_gradient_of_a_linear_ramp_is_constant_at_both_ends():
    n, dx, H = 9, 2.0, 2.2e-18
    slope = 0.05 * H  # well inside the clip
    v = np.broadcast_to(slope * dx * np.arange(n), (2, 3, n)).astype(np.float64).astype(np.float32)
    g = np.gradient(v.astype(np.float64), dx, axis=-1, edge_order=2)
    np.testing.assert_allclose(g, slope, rtol=1e-6)  # one-sided second order is exact on a line
    bt = np.full(v.shape, 20.0, np.float32)
    got = LR.include_dvdr_in_tau21(bt, v, np.full(n, H), dx, 0.2)
    np.testing.assert_allclose(got, 20.0 / (1.0 + 0.05), rtol=1e-6)


def test_clip_engages():
    n, dx, H, max_dvdr = 6, 2.0, 2.2e-18, 0.2
    for sign in (1.0, -1.0):
        v = (sign * 3.0 * H * dx * np.arange(n) * np.ones((1, 1, 1))).astype(np.float32)  # dv/dx = 3 H
        got = LR.include_dvdr_in_tau21(np.ones(v.shape, np.float32), v, np.full(n, H), dx, max_dvdr)
        np.testing.assert_allclose(got, 1.0 / abs(1.0 + sign * max_dvdr), rtol=1e-6)


def test_tau21_form_and_its_small_tau_limit():
    n, dx, H = 5, 2.0, 2.2e-18
    v = (0.1 * H * dx * np.arange(n) * np.ones((2, 1, 1))).astype(np.float32)
    bt = np.full(v.shape, 10.0, np.float32)
    tau = np.full(v.shape, 0.5, np.float32)
    tau[0, 0, 1] = 5e-11  # below 1e-10: the factor is 1
    tau[0, 0, 2] = 0.0    # 0/0 in the formula: the factor is 1
    got = LR.include_dvdr_in_tau21(bt, v, np.full(n, H), dx, 0.2, tau_21=tau)
    assert got[0, 0, 1] == 10.0 and got[0, 0, 2] == 10.0
    want = np.float32((1 - np.exp(-0.5 / 1.1)) / (1 - np.exp(-0.5)))
    np.testing.assert_allclose(got[1], 10.0 * want, rtol=1e-6)
    assert np.isfinite(got).all()


def test_fill_slices_wraps_planes():
    """A run longer than the node box takes planes again, modulo HII_D_PARA."""
    cell, d_para = 1.0, 4
    lcd = 100.0 + np.arange(10.0)
    lo = {"density": np.arange(2 * 2 * d_para, dtype=np.float32).reshape(2, 2, d_para)}
    hi = {"density": lo["density"] + 100}
    lcs = {"density": np.zeros((2, 2, 10), np.float32)}
    LR.fill_slices(lcs, lcd, 100.0, 110.0, cell, lo, hi, index_offset=10)
    planes = [(-int(lcd.max() - d + 1) + 10) % d_para for d in lcd]
    assert planes == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    w = (lcd - 100.0) / 10.0
    np.testing.assert_allclose(lcs["density"][0, 1], lo["density"][0, 1, planes] + 100 * w, rtol=1e-6)


def test_new_spec_mirrors_match_compiler_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "c21cm_grid.h"', "int main(void){"]
    pairs = {"c21cm_lightcone_spec": S.LightconeSpec, "c21cm_dvdr_spec": S.DvdrSpec}
    for name, cls in pairs.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines.append('printf("max_fields x %d\\n", C21CM_LC_MAX_FIELDS);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    api = importlib.import_module("21cmfast_amd.grid_api")
    for line in out.strip().splitlines():
        name, field, value = line.split()
        if name == "max_fields":
            assert api.LC_MAX_FIELDS == int(value)
        elif field == "size":
            assert C.sizeof(pairs[name]) == int(value), name
        else:
            assert getattr(pairs[name], field).offset == int(value), f"{name}.{field}"


def small_inputs(**kw):
    return D.Inputs(HII_DIM=16, DIM=32, BOX_LEN=32.0, SOURCE_MODEL=1, **kw)


def test_run_lightcone_validates_before_any_gpu_work():
    """validate_options (lightconers.py:336-372) and _check_desired_arrays_exist: ValueError, raised
    before the library is loaded (lib=None here, and no GPU is needed to get there)."""
    nodes = (20.0, 19.0, 18.0)
    ok = D.RectilinearLightconer.between_redshifts(18.2, 19.8, 2.0, quantities=("brightness_temp", "density"))
    with pytest.raises(ValueError, match="not inside the node"):
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(17.5, 19.0, 2.0), nodes)
    with pytest.raises(ValueError, match="not inside the node"):
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(18.5, 20.5, 2.0), nodes)
    with pytest.raises(ValueError, match="spin_temperature"):  # no USE_TS_FLUCT: no spin temperature
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(
            18.2, 19.8, 2.0, quantities=("brightness_temp", "spin_temperature")), nodes)
    with pytest.raises(ValueError, match="cumulative_recombinations"):  # no recombination model
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(
            18.2, 19.8, 2.0, quantities=("cumulative_recombinations",)), nodes)
    with pytest.raises(ValueError, match="request it"):
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(
            18.2, 19.8, 2.0, quantities=("density",)), nodes)
    with pytest.raises(ValueError, match="cosmology"):
        D.run_lightcone(small_inputs(), D.RectilinearLightconer.between_redshifts(
            18.2, 19.8, 2.0, cosmo=D.FlatCosmology(0.7, 0.3)), nodes)
    with pytest.raises(ValueError, match="two node"):
        D.run_lightcone(small_inputs(), ok, (18.0,))
    fields = D.lightcone_fields(small_inputs(USE_TS_FLUCT=True, RECOMB_MODEL=2))
    assert {"spin_temperature", "tau_21", "cumulative_recombinations", "z_reion", "los_velocity"} <= fields
    assert "n_ion" not in fields and "n_ion" in D.lightcone_fields(D.Inputs(SOURCE_MODEL=2))
