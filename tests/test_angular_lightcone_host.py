"""CPU checks of the angular lightcone (drivers.AngularLightconer): the reference's constructor
errors and rotation equality, like_rectilinear's geometry, the restatement the GPU tests compare against
(tests/angular_reference.py) on known answers, its periodic prefilter against scipy's, run_lightcone's
argument errors before any GPU work, and the ctypes mirror of the new spec against the C layout."""

import ctypes as C
import importlib
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.transform import Rotation

import angular_reference as AR

D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")
ROOT = Path(__file__).resolve().parent.parent


def sky(n=48):
    """n directions on a Fibonacci sphere, longitudes in [0, 2pi)"""
    k = np.arange(n) + 0.5
    lat = np.arcsin(1 - 2 * k / n)
    lon = np.mod(np.pi * (1 + 5**0.5) * k, 2 * np.pi)
    return lat, lon


def test_constructor_errors_are_the_reference_ones():
    lat, lon = sky()
    d = np.linspace(6000.0, 6100.0, 10)
    with pytest.raises(ValueError, match="longitude must be 1-dimensional"):
        D.AngularLightconer(lat, lon[None, :], d)
    with pytest.raises(ValueError, match=re.escape("longitude must be in the range [0, 2pi]")):
        D.AngularLightconer(lat, lon + 2 * np.pi, d)
    with pytest.raises(ValueError, match=re.escape("longitude must be in the range [0, 2pi]")):
        D.AngularLightconer(lat, lon - 1.0, d)
    with pytest.raises(ValueError, match="longitude and latitude must have the same shape"):
        D.AngularLightconer(lat[None, :], lon, d)
    with pytest.raises(ValueError, match="interpolation_order"):
        D.AngularLightconer(lat, lon, d, interpolation_order=2)
    with pytest.raises(ValueError, match="origin"):
        D.AngularLightconer(lat, lon, d, origin=(0.0, 1.0))
    with pytest.raises(ValueError, match="rotation"):
        D.AngularLightconer(lat, lon, d, rotation=np.diag([1.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="lc_distances"):
        D.AngularLightconer(lat, lon, [])
    # both ends of the longitude range are allowed
    lc = D.AngularLightconer(np.zeros(2), np.array([0.0, 2 * np.pi]), d)
    assert lc.get_shape() == (2, 10)


def test_rotation_equality():
    lat, lon = sky()
    lc1 = D.AngularLightconer.between_redshifts(6.0, 7.0, 2.0, latitude=lat, longitude=lon)
    lc2 = D.AngularLightconer.between_redshifts(6.0, 7.0, 2.0, latitude=lat, longitude=lon)
    assert lc1 == lc2
    rot = Rotation.from_euler("z", np.pi / 2)
    lc3 = D.AngularLightconer.between_redshifts(6.0, 7.0, 2.0, latitude=lat, longitude=lon, rotation=rot)
    assert lc1 != lc3
    lc4 = D.AngularLightconer.between_redshifts(6.0, 7.0, 2.0, latitude=lat, longitude=lon,
                                                rotation=rot.as_matrix() + 1e-12)
    assert lc3 == lc4  # allclose, as _rotation_eq
    assert lc3 != D.AngularLightconer.between_redshifts(6.0, 7.0, 2.0, latitude=lat, longitude=lon,
                                                        rotation=Rotation.from_euler("z", np.pi / 3))
    assert lc1 != lc1.extended(1, 0) and lc1.extended(0, 0) is lc1


def test_like_rectilinear_geometry():
    inputs = D.Inputs(HII_DIM=16, DIM=32, BOX_LEN=32.0)
    so = inputs.simulation_options
    lc = D.AngularLightconer.like_rectilinear(so, 8.0, 8.5)
    d0 = lc.cosmo.comoving_distance(8.0)
    bsr = 32.0 / d0
    np.testing.assert_array_equal(lc.longitude.reshape(16, 16)[0], np.linspace(0, bsr, 16))
    np.testing.assert_array_equal(lc.latitude.reshape(16, 16)[:, 0], np.linspace(0, bsr, 16)[::-1])
    np.testing.assert_array_equal(lc.origin, [0.0, 0.0, -d0 / 2.0])
    np.testing.assert_allclose(lc.rotation, Rotation.from_euler("Y", -np.pi / 2).as_matrix(), atol=1e-15)
    assert lc.lc_distances[0] == d0
    np.testing.assert_allclose(np.diff(lc.lc_distances), 2.0)
    assert lc.get_shape(so) == (256, len(lc.lc_distances))
    # (b, l) = (0, 0) is pixel (15, 0) of the grid: direction +z, and on the lowest slice the box origin
    p = 15 * 16
    assert lc.latitude[p] == 0 and lc.longitude[p] == 0
    np.testing.assert_array_equal(lc.nhat[:, p], [0.0, 0.0, 1.0])
    np.testing.assert_array_equal(AR.points(lc.nhat, lc.lc_distances[0] / 2.0, lc.origin)[:, p], 0.0)
    # the restatement's directions agree with the lightconer's
    np.testing.assert_allclose(AR.directions(lc.latitude, lc.longitude, Rotation.from_euler("Y", -np.pi / 2)),
                               lc.nhat, atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(lc.nhat, axis=0), 1.0, rtol=1e-15)


def test_slice_selection_is_the_rectilinear_one():
    inputs = D.Inputs(HII_DIM=16, DIM=32, BOX_LEN=32.0)
    ang = D.AngularLightconer.like_rectilinear(inputs.simulation_options, 8.0, 9.0)
    rect = D.RectilinearLightconer(ang.lc_distances)
    for z_lo, z_hi in ((8.0, 8.3), (8.3, 8.7), (8.7, 9.0), (9.5, 9.9)):
        a, r = ang.angular_tables(z_lo, z_hi, 2.0), rect.slab_tables(z_lo, z_hi, 2.0, 16)
        if r is None:
            assert a is None
            continue
        assert a[0] == r[0] and len(a[1]) == len(r[1])
        for x, y in zip(a[2:], r[2:]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(a[1], ang.lc_distances[a[0]:a[0] + len(a[1])] / 2.0)


@pytest.mark.parametrize("order", [0, 1, 3, 5])
def test_restatement_uniform_box_and_integer_points(order):
    rng = np.random.default_rng(order)
    lat, lon = sky(40)
    nhat = AR.directions(lat, lon, Rotation.from_euler("xyz", [0.3, -1.1, 2.0]))
    lcs = {"density": np.zeros((40, 6), np.float32)}
    lo = {"density": np.full((6, 6, 9), 2.5, np.float32)}
    hi = {"density": np.full((6, 6, 9), 2.5, np.float32)}
    AR.fill_slices(lcs, 100.0 + 2.0 * np.arange(6), 99.0, 120.0, 2.0, lo, hi, nhat, (3.0, -7.5, 1e3), order)
    np.testing.assert_allclose(lcs["density"], 2.5, rtol=1e-12)
    # integer points: the cell values (orders 3 and 5 through their prefilter: to round-off)
    box = rng.standard_normal((5, 7, 6))
    x = rng.integers(-40, 40, (3, 50)).astype(float)
    got = AR.interpolate(box, x, order)
    want = box[tuple(np.mod(x.astype(int), np.array(box.shape)[:, None]))]
    if order <= 1:
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, atol=1e-12)


@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("shape", [(8, 8, 12), (5, 7, 3), (1, 4, 9), (16, 16, 16)])
def test_prefilter_restatement_is_scipy_grid_wrap(order, shape):
    box = np.random.default_rng(7).standard_normal(shape)
    want = ndimage.spline_filter(box, order, mode="grid-wrap", output=np.float64)
    np.testing.assert_allclose(AR.periodic_prefilter(box, order), want, atol=1e-14 * np.abs(want).max())


@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("shape", [(32, 32, 32), (50, 50, 50), (64, 64, 64), (40, 64, 96), (128, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_prefilter_restatement_is_scipy_grid_wrap_at_production_sizes(order, shape):
    """Lines of 32 cells and more, where the device truncates its start sums (the horizon is 32 cells for the
    cubic pole, 50 and 14 for the quintic ones) and the restatement, which sums the whole period, does not:
    the GPU tests compare against either, so the two are held together here."""
    box = np.random.default_rng(sum(shape) + order).standard_normal(shape, dtype=np.float32)
    want = ndimage.spline_filter(box.astype(np.float64), order=order, mode="grid-wrap")
    np.testing.assert_allclose(AR.periodic_prefilter(box, order), want, rtol=0, atol=1e-12 * np.abs(want).max())


def small_inputs(**kw):
    return D.Inputs(HII_DIM=16, DIM=32, BOX_LEN=32.0, SOURCE_MODEL=1, **kw)


def test_run_lightcone_validates_before_any_gpu_work():
    """ValueError before the library is loaded (no GPU is needed to get there)."""
    nodes = (20.0, 19.0, 18.0)
    so = small_inputs().simulation_options

    def ang(**kw):
        return D.AngularLightconer.like_rectilinear(so, 18.2, 19.8, **kw)

    msg = "To account for RSDs or velocity corrections in an angular lightcone, you need to set"
    with pytest.raises(ValueError, match=msg):  # dv/dr is on by default
        D.run_lightcone(small_inputs(), ang(), nodes)
    with pytest.raises(ValueError, match=msg):
        D.run_lightcone(small_inputs(), ang(), nodes, include_dvdr_in_tau21=False, apply_rsds=True)
    with pytest.raises(ValueError, match=msg):
        D.run_lightcone(small_inputs(), ang(quantities=("density", "los_velocity")), nodes,
                        include_dvdr_in_tau21=False)
    with pytest.raises(ValueError, match="mean_max"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True),
                        ang(quantities=("brightness_temp", "z_reion"), interpolation_order=3), nodes)
    with pytest.raises(ValueError, match="not inside the node"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True), D.AngularLightconer.like_rectilinear(
            so, 17.5, 19.0), nodes)
    with pytest.raises(ValueError, match="spin_temperature"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True), ang(quantities=("brightness_temp",
                                                                               "spin_temperature")), nodes)
    with pytest.raises(ValueError, match="request it"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True), ang(quantities=("density",)), nodes)
    with pytest.raises(ValueError, match="cosmology"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True), ang(cosmo=D.FlatCosmology(0.7, 0.3)), nodes)
    with pytest.raises(ValueError, match="n_rsd_subcells"):
        D.run_lightcone(small_inputs(KEEP_3D_VELOCITIES=True), ang(), nodes, apply_rsds=True, n_rsd_subcells=0)
    with pytest.raises(TypeError, match="lightconer"):
        D.run_lightcone(small_inputs(), object(), nodes)
    assert {"velocity_x", "velocity_y"} <= D.lightcone_fields(small_inputs(KEEP_3D_VELOCITIES=True))
    assert "velocity_x" not in D.lightcone_fields(small_inputs())


def test_angular_spec_mirror_matches_compiler_layout(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "c21cm_grid.h"', "int main(void){"]
    name, cls = "c21cm_angular_spec", S.AngularSpec
    lines.append(f'printf("size %zu\\n", sizeof({name}));')
    for field, _ in cls._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof({name}, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        field, value = line.split()
        if field == "size":
            assert C.sizeof(cls) == int(value)
        else:
            assert getattr(cls, field).offset == int(value), field
