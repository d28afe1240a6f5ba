"""CPU checks of the coeval velocity corrections: ``rsds.include_dvdr_in_tau21`` and the three ``Coeval``
methods validate their arguments with the reference's messages before the library is loaded (no GPU is
needed to get there), the fp64 restatement the GPU tests compare against (tests/dvdr_periodic_reference.py)
gives known answers in both of its forms, and the ctypes mirror of the new spec agrees with the C layout
of include/c21cm_grid.h."""

import ctypes as C
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvdr_periodic_reference as PR

D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")
rsds = importlib.import_module("21cmfast_amd.rsds")
ROOT = Path(__file__).resolve().parent.parent


def small_inputs(**kw):
    return D.Inputs(HII_DIM=10, DIM=20, BOX_LEN=20.0, SOURCE_MODEL=1, **kw)


@pytest.mark.parametrize("periodic", [True, False])
def test_include_dvdr_argument_checks(periodic):
    """The reference's shapes (5 x 5 x 10 ones) and its three messages, in its order."""
    ones = np.ones((5, 5, 10), np.float32)
    with pytest.raises(ValueError, match="tau_21 is not provided, but inputs.astro_options.USE_TS_FLUCT is True!"):
        rsds.include_dvdr_in_tau21(ones, ones, 8.0, small_inputs(USE_TS_FLUCT=True), periodic=periodic)
    with pytest.raises(ValueError,
                       match="Redshifts must be a float or array with the same size as number of LoS slices"):
        rsds.include_dvdr_in_tau21(ones, ones, np.array([8.0, 9.0]), small_inputs(), periodic=periodic)
    with pytest.raises(ValueError, match="brightness_temp must be an array with the same shape as los_velocity"):
        rsds.include_dvdr_in_tau21(ones, ones[..., :-1], 8.0, small_inputs(), periodic=periodic)
    # the order: a missing tau_21 is reported before the redshifts, the redshifts before the shapes
    with pytest.raises(ValueError, match="tau_21 is not provided"):
        rsds.include_dvdr_in_tau21(ones, ones[..., :-1], np.array([8.0, 9.0]), small_inputs(USE_TS_FLUCT=True),
                                   periodic=periodic)
    with pytest.raises(ValueError, match="Redshifts must be"):
        rsds.include_dvdr_in_tau21(ones, ones[..., :-1], np.array([8.0, 9.0]), small_inputs(), periodic=periodic)


def test_coeval_methods_argument_checks():
    ones = np.ones((5, 5, 10), np.float32)
    coeval = D.Coeval(small_inputs(), 8.0, {"brightness_temp": ones, "velocity_z": ones, "density": ones})
    assert coeval.brightness_temp is ones and coeval.redshift == 8.0
    with pytest.raises(AttributeError):
        coeval.velocity_x
    calls = (lambda ax: coeval.include_dvdr_in_tau21(axis=ax), lambda ax: coeval.apply_rsds(axis=ax),
             lambda ax: coeval.apply_velocity_corrections(axis=ax))
    for call in calls:
        with pytest.raises(ValueError) as err:
            call("x")
        assert str(err.value) == ("You asked for axis = 'x', but the coeval doesn't have velocity_x! Set "
                                  "matter_options.KEEP_3D_VELOCITIES=True next time you call run_coeval if you "
                                  "wish to set axis=`x'.")
        with pytest.raises(ValueError) as err:
            call("w")
        assert str(err.value) == "`axis` can only be `x`, `y` or `z`."
    # with a spin temperature the snapshot must carry tau_21
    ts = D.Coeval(small_inputs(USE_TS_FLUCT=True), 8.0, {"brightness_temp": ones, "velocity_z": ones})
    for call in (ts.include_dvdr_in_tau21, ts.apply_velocity_corrections):
        with pytest.raises(ValueError, match=r'keep=\(\.\.\., "tau_21"\) to run_coeval'):
            call()
    # from_result keys the snapshot as run_coeval does: by the float32 redshift
    result = {float(np.float32(8.1)): {"brightness_temp": ones}, "history": []}
    assert D.Coeval.from_result(result, 8.1, small_inputs()).brightness_temp is ones


@pytest.mark.parametrize("n", [3, 4, 5, 8, 12, 35, 50, 64])
def test_circulant_form_equals_rfft_form(n):
    rng = np.random.default_rng(n)
    v = rng.standard_normal((7, n))
    a, b = PR.gradient_rfft(v, 1.5), PR.gradient_circulant(v, 1.5)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("n", [2, 8, 50, 64])
def test_nyquist_line_has_zero_gradient(n):
    v = 3.0 * (-1.0) ** np.arange(n)
    scale = 3.0 * np.pi / 1.5  # the amplitude times the Nyquist wavenumber
    assert np.abs(PR.gradient_rfft(v, 1.5)).max() <= 1e-13 * scale
    assert np.abs(PR.gradient_circulant(v, 1.5)).max() <= 1e-13 * scale


@pytest.mark.parametrize("n,mode", [(5, 1), (12, 5), (35, 17), (64, 3), (64, 31)])
def test_single_sine_mode_has_its_analytic_derivative(n, mode):
    dx = 2.0
    x = dx * np.arange(n)
    k = 2.0 * np.pi * mode / (n * dx)
    v, want = np.sin(k * x + 0.3), k * np.cos(k * x + 0.3)
    for grad in (PR.gradient_rfft, PR.gradient_circulant):
        assert np.abs(grad(v, dx) - want).max() <= 1e-12 * k


def test_restatement_forms():
    H, n = 2.2e-18, 6
    g = np.array([0.1, -0.1, 0.5, -0.5, 0.0, 0.19]) * H
    bt = np.full(n, 10.0)
    np.testing.assert_allclose(PR.taylor_form(bt, g, H, 0.2), 10.0 / np.array([1.1, 0.9, 1.2, 0.8, 1.0, 1.19]),
                               rtol=1e-14)
    tau = np.array([0.5, 5e-11, 0.0, 0.5, 0.5, 0.5])
    fac = PR.tau_factor(tau, g, H)
    assert fac[1] == 1.0 and fac[2] == 1.0 and fac[4] == 1.0
    np.testing.assert_allclose(fac[0], (1 - np.exp(-0.5 / 1.1)) / (1 - np.exp(-0.5)), rtol=1e-14)


def test_periodic_spec_mirror_matches_compiler_layout(tmp_path):
    name, cls = "c21cm_dvdr_periodic_spec", S.DvdrPeriodicSpec
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "c21cm_grid.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({name}));']
    for field, _ in cls._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof({name}, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        field, value = line.split()
        if field == "size":
            assert C.sizeof(cls) == int(value)
        else:
            assert getattr(cls, field).offset == int(value), field
            seen += 1
    assert seen == 7
