"""The DexM radius ladder on the host (csrc/host/halo_sampler_tables.c: c21cm_dexm_ladder; no GPU needed)
against the numpy walk of tests/dexm_reference.py, which keeps the reference's float variables
(HaloCatalog.c:81-200): R re-rounded to float32 after every multiply and divide by the double DELTA_R_FACTOR,
M and delta_crit float32.  Rungs, masses and barriers are compared bit for bit."""

import ctypes as C
import importlib

import numpy as np
import pytest

import dexm_reference as D

f64 = C.c_double


@pytest.fixture(scope="module")
def host(pkg):
    lib = pkg.load()
    for name in ("dicke", "sigma_z0", "c21_MtoR", "c21_RtoM"):
        getattr(lib, name).restype = f64
        getattr(lib, name).argtypes = [f64]
    lib.c21cm_dexm_is_empty.argtypes = [f64]
    lib.c21cm_dexm_ladder.restype = C.c_int
    lib.c21cm_dexm_ladder.argtypes = [f64, C.c_void_p]
    lib.c21hip_get_error.restype = C.c_char_p
    return lib


def broadcast(lib, S, source=4, hii=32, box=128.0, matter=None, **sim):
    keep = dict(so=S.default_simulation_options(HII_DIM=hii, DIM=2 * hii, BOX_LEN=box, SAMPLER_MIN_MASS=5e8, **sim),
                mo=S.default_matter_options(SOURCE_MODEL=source, **(matter or {})), cp=S.default_cosmo_params(),
                ap=S.default_astro_params(), ao=S.default_astro_options(), ct=S.default_cosmo_tables())
    lib.Broadcast_struct_global_all(*[C.byref(keep[k]) for k in ("so", "mo", "cp", "ap", "ao", "ct")])
    lib.init_ps()
    lib._keep_dexm_host = keep
    return keep


@pytest.mark.parametrize("source", [4, 3])
@pytest.mark.parametrize("hii,box", [(32, 128.0), (64, 96.0)])
def test_ladder_against_the_numpy_walk(pkg, host, hii, box, source):
    """two boxes, both source models (M_MIN from HII_DIM or from DIM), redshifts with skipped rungs only at
    the top, with everything skipped, and in between"""
    S = pkg.structs
    keep = broadcast(host, S, source, hii=hii, box=box, DEXM_R_OVERLAP=1.5, DEXM_OPTIMIZE_MINMASS=3e11,
                     matter=dict(HALO_FILTER=1, DEXM_OPTIMIZE=True))
    so = keep["so"]
    n_skipped = []
    for z in (6.0, 10.0, 16.0):
        kept, skipped, growth = D.ladder(host, so, source == 4, z)
        n_skipped.append(skipped)
        spec = S.FindHalosSpec()
        assert host.c21cm_dexm_ladder(z, C.byref(spec)) == 0, host.c21hip_get_error()
        assert spec.n_R == len(kept)
        assert (spec.n_R == 0) == bool(host.c21cm_dexm_is_empty(z))
        for name, column in zip(("R", "mass", "delta_crit"), zip(*kept) if kept else ([], [], [])):
            got = np.array(getattr(spec, name)[:spec.n_R], np.float32)
            assert np.array_equal(got.view(np.uint32), np.array(column, np.float32).view(np.uint32)), (name, z)
        assert spec.growth == float(growth)
        assert (spec.dim, spec.dim_z, spec.halo_filter, spec.optimize) == (2 * hii, 2 * hii, 1, 1)
        assert (spec.hii_dim, spec.hii_dim_z) == ((hii, hii) if source == 4 else (0, 0))
        assert (spec.box_len, spec.r_overlap, spec.optimize_minmass) == (box, 1.5, 3e11)
        assert spec.rtom_unit == host.c21_RtoM(1.0) and spec.redshift == z
    assert max(n_skipped) > 0  # the 7 sigma skip was exercised


def test_parameters_that_describe_no_box_return_at_once(pkg, host):
    S = pkg.structs
    spec = S.FindHalosSpec()
    for change in (dict(BOX_LEN=float("inf")), dict(BOX_LEN=float("nan")), dict(BOX_LEN=1e30),
                   dict(DELTA_R_FACTOR=1.0 + 1e-9), dict(DELTA_R_FACTOR=float("nan"))):
        keep = broadcast(host, S)
        for k, v in change.items():
            setattr(keep["so"], k, v)
        assert host.c21cm_dexm_ladder(11.0, C.byref(spec)) == 3, change
        assert "no box" in host.c21hip_get_error().decode()
    keep = broadcast(host, S)
    keep["cp"].OMm = float("nan")
    assert host.c21cm_dexm_ladder(11.0, C.byref(spec)) == 3
    assert host.c21cm_dexm_ladder(11.0, None) == 3


def test_more_rungs_than_the_spec_holds_is_a_value_error(pkg, host):
    """DELTA_R_FACTOR = 1.001: thousands of steps between the cell and the box, far more than 256 kept"""
    S = pkg.structs
    broadcast(host, S, DELTA_R_FACTOR=1.001)
    spec = S.FindHalosSpec()
    assert not host.c21cm_dexm_is_empty(6.0)
    assert host.c21cm_dexm_ladder(6.0, C.byref(spec)) == 3
    assert str(S.MAX_DEXM_RADII) in host.c21hip_get_error().decode()
    broadcast(host, S)
    assert host.c21cm_dexm_ladder(6.0, C.byref(spec)) == 0 and 0 < spec.n_R <= S.MAX_DEXM_RADII
