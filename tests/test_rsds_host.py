"""CPU checks of the redshift-space distortions: the numpy restatement the GPU tests compare against
passes the reference's own TestRSDsShift cases (tests/test_rsds.py:113-172 of the reference), the
public functions and run_lightcone(apply_rsds=True) reject bad arguments before any GPU work, and the
ctypes mirror of c21cm_rsd_spec agrees with the C layout of include/c21cm_grid.h."""

import ctypes as C
import importlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rsd_reference as RR

D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")
rsds = importlib.import_module("21cmfast_amd.rsds")
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n_rsd_subcells", [1, 2, 4, 5])
def test_restatement_conserves_mass_periodic(n_rsd_subcells):
    rng = np.random.default_rng(12345)
    box_in = rng.random((10, 5))
    box_out = RR.rsds_shift(box_in, rng.random((10, 5)), n_rsd_subcells=n_rsd_subcells, periodic=True)
    np.testing.assert_allclose(box_out.sum(axis=0), box_in.sum(axis=0))


@pytest.mark.parametrize("n_rsd_subcells", [1, 2])
@pytest.mark.parametrize("velocity", range(-10, 11))
def test_restatement_integer_shift_is_roll(n_rsd_subcells, velocity):
    rng = np.random.default_rng(12345)
    box_in = rng.random((10, 5))
    box_out = RR.rsds_shift(box_in, velocity * np.ones_like(box_in), n_rsd_subcells=n_rsd_subcells, periodic=True)
    np.testing.assert_allclose(box_out, np.roll(box_in, velocity, axis=0))


@pytest.mark.parametrize("n_rsd_subcells", [1, 2, 5])
def test_restatement_large_displacement_empties_the_column(n_rsd_subcells):
    box_in = np.ones((10, 5))
    box_out = RR.rsds_shift(box_in, 20 * np.ones_like(box_in), n_rsd_subcells=n_rsd_subcells, periodic=False)
    np.testing.assert_allclose(box_out, 0)


@pytest.mark.parametrize("periodic", [False, True])
def test_restatement_3d_equals_2d(periodic):
    rng = np.random.default_rng(7)
    field = rng.normal(size=(4, 4, 12))
    vel = rng.normal(size=field.shape) * 1e-17
    hubble = np.linspace(2e-17, 3e-17, 12)
    got3 = RR.apply_rsds(field, vel, hubble, 1.5, periodic)
    got2 = RR.apply_rsds(field.reshape(16, 12), vel.reshape(16, 12), hubble, 1.5, periodic)
    np.testing.assert_array_equal(got3.reshape(16, 12), got2)


def test_restatement_non_periodic_extrapolates_the_end_intervals():
    """Sub-cells beyond the first and last slice centres take the displacement of the end interval's
    line (RegularGridInterpolator with fill_value=None): a linear ramp stays a line."""
    n, m = 6, 4
    disp = (0.01 * np.arange(n))[:, None] * np.ones((1, 2))
    field = np.zeros((n, 2))
    field[0] = 1.0  # the first slice's sub-cells sit at 0.125 and 0.375, before the first node (0.5)
    got = RR.rsds_shift(field, disp, n_rsd_subcells=m)
    fine_pos = (np.arange(m) + 0.5) / m
    fine_disp = m * 0.01 * (fine_pos - 0.5)  # negative: extrapolated below the first node
    x = np.arange(m) + fine_disp
    lost = sum(0.25 * (1 - (xi - np.floor(xi))) for xi in x if xi < 0)
    np.testing.assert_allclose(got[:, 0].sum(), 1.0 - lost)
    assert lost > 0


def test_public_functions_validate_before_any_gpu_work():
    f = np.zeros((1, 4), np.float32)
    with pytest.raises(ValueError, match="at least 2 slices"):
        rsds.rsds_shift(f, f)
    with pytest.raises(ValueError, match="same shape as los_displacement"):
        rsds.rsds_shift(np.zeros((3, 4)), np.zeros((3, 5)))
    with pytest.raises(ValueError, match="n_rsd_subcells must be an integer"):
        rsds.rsds_shift(np.zeros((3, 4)), np.zeros((3, 4)), n_rsd_subcells=2.0)
    inputs = D.Inputs(HII_DIM=4, DIM=8, BOX_LEN=8.0)
    box = np.zeros((4, 4, 6), np.float32)
    with pytest.raises(ValueError, match="Redshifts must be a float or array"):
        rsds.apply_rsds(box, box, np.ones(5), inputs, periodic=False)
    with pytest.raises(ValueError, match="same shape as los_displacement"):
        rsds.apply_rsds(box, box[..., :5], 10.0, inputs, periodic=True)
    with pytest.raises(ValueError, match="n_rsd_subcells must be an integer"):
        rsds.apply_rsds(box, box, 10.0, inputs, periodic=True, n_rsd_subcells="4")
    with pytest.raises(ValueError, match="at least 2 slices"):
        rsds.apply_rsds(box[..., :1], box[..., :1], 10.0, inputs, periodic=True)


def small_inputs(**kw):
    return D.Inputs(HII_DIM=16, DIM=32, BOX_LEN=32.0, SOURCE_MODEL=1, **kw)


def test_run_lightcone_rsd_arguments_are_checked_before_any_gpu_work():
    nodes = (20.0, 19.0, 18.0)
    lcn = D.RectilinearLightconer.between_redshifts(18.2, 19.8, 2.0)
    with pytest.raises(ValueError, match="n_rsd_subcells must be an integer"):
        D.run_lightcone(small_inputs(), lcn, nodes, apply_rsds=True, n_rsd_subcells=2.5)
    with pytest.raises(ValueError, match="at least 1"):
        D.run_lightcone(small_inputs(), lcn, nodes, apply_rsds=True, n_rsd_subcells=0)
    with pytest.raises(ValueError, match="rsd_buffer_slices"):
        D.run_lightcone(small_inputs(), lcn, nodes, apply_rsds=True, rsd_buffer_slices=(-1, 0))
    # a buffer past the node redshifts is the existing range error
    with pytest.raises(ValueError, match="not inside the node"):
        D.run_lightcone(small_inputs(), lcn, nodes, apply_rsds=True, rsd_buffer_slices=(0, 400))
    with pytest.raises(ValueError, match="not inside the node"):
        D.run_lightcone(small_inputs(), lcn, nodes, apply_rsds=True, rsd_buffer_slices=(400, 0))


def test_lightconer_extension_keeps_the_requested_slices():
    lcn = D.RectilinearLightconer.between_redshifts(8.0, 9.0, 1.5, quantities=("density",), index_offset=7)
    ext = lcn.extended(3, 2)
    d = lcn.lc_distances
    assert len(ext.lc_distances) == len(d) + 5
    np.testing.assert_array_equal(ext.lc_distances[3:-2], d)
    np.testing.assert_allclose(np.diff(ext.lc_distances), 1.5, rtol=1e-9)
    assert ext.index_offset == 7 and ext.quantities == ("density",) and ext.cosmo is lcn.cosmo
    assert lcn.extended(0, 0) is lcn


def test_rsd_spec_mirror_matches_compiler_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "c21cm_grid.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(c21cm_rsd_spec));']
    for field, _ in S.RsdSpec._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(c21cm_rsd_spec, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        field, value = line.split()
        if field == "size":
            assert C.sizeof(S.RsdSpec) == int(value)
        else:
            assert getattr(S.RsdSpec, field).offset == int(value), field
