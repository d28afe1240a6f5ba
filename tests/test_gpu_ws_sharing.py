"""GPU: entries whose workspace slots share an id (csrc/hip/ws_slots.h, the `WS_B = WS_A` lines) do not
disturb each other.  For each pair: A, B, A again -- the second A must reproduce the first bit for bit --
and then B, A, B.  All arrays are host (numpy) arrays, so every staging slot is taken, and each pair runs at
two sizes so that each entry's buffers are the larger ones once: the shared slot is then reallocated between
the two calls that are compared, which is where a stale pointer would show."""

import importlib

import numpy as np
import pytest

from recomb_helpers import inputs, recomb_spec
from test_gpu_halobox_catalogue import _bind_test_halo_props, random_catalogue
from test_gpu_perturb import random_ics as perturb_ics
from test_oracle_brightness import fields
from test_oracle_halobox import halobox_spec, make_tables
from test_oracle_halobox import random_ics as halobox_ics
from test_oracle_perturb import perturb_spec

pytestmark = pytest.mark.gpu
S = importlib.import_module("21cmfast_amd.structs")
W = importlib.import_module("21cmfast_amd.workloads")


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def check_pair(a, b):
    """a, b: callables returning a dict of arrays / scalars."""
    for first, second in ((a, b), (b, a)):
        want = first()
        second()
        got = first()
        assert want.keys() == got.keys()
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def perturb_call(api, n, N, hires):
    ics = perturb_ics(n, N, seed=n, hires_vel=hires)
    spec = perturb_spec(2, dim=N, dim_z=N, hii_dim=n, hii_dim_z=n, box_len=1.5 * n, box_len_z=1.5 * n,
                        growth_factor=0.12, init_growth_factor=0.0042, keep_3d_velocities=1, dDdt_over_D=2.1e-17,
                        perturb_on_high_res=int(hires))
    return lambda: api.perturb_grids(spec, ics)


def ionize_outputs(buf, rep):
    names = ("neutral_fraction", "z_reion", "kinetic_temperature", "ionisation_rate_G12", "mean_free_path",
             "cumulative_recombinations")
    out = {k: np.array(getattr(buf, k)) for k in names if getattr(buf, k) is not None}
    out["global_xH"] = rep.global_xH
    return out


def ionize_ts_call(api, n):
    """Lagrangian sources with the x_e grid of a spin-temperature run: takes WS_XE_WORK and WS_PARTIALS."""
    spec = W.ionize_spec(n, r_bubble_max=12.0, use_ts_fluct=1)
    d = inputs((n, n, n), seed=5, ts=True)

    def call():
        buf, _, rep = api.ionize_grids(spec, d["density"], d["n_ion"], xe=d["xe"], Tneutral=d["Tneutral"])
        return ionize_outputs(buf, rep)

    return call


def ionize_fused_recomb_call(api, n, nz):
    """The fused recombination loop with two radii per sweep: takes WS_SFR_WORK2, WS_R_DEV and the node tables
    of the evaluated windows."""
    spec = recomb_spec(n, model=2, cell_recomb=1, r_bubble_max=20.0, hii_dim_z=nz)
    d = inputs((n, n, nz), seed=77)

    def call():
        buf, _, rep = api.ionize_grids(spec, d["density"], n_ion=d["n_ion"], whalo_sfr=d["whalo_sfr"],
                                       prev_nrec=d["prev_nrec"], prev_z_reion=d["prev_z_reion"])
        flags = api.ionize_last_loop_flags()
        assert flags & 2 and flags & 32, flags  # the fused recombination loop, two radii per sweep
        return ionize_outputs(buf, rep)

    return call


def brightness_call(api, n):
    density, xH, Ts = fields(n=n, seed=11)
    spec = S.brightness_spec(density.size, 7.6, use_ts_fluct=True)
    return lambda: api.brightness_grids(spec, density, xH, Ts)


def halobox_call(api, n, N, hires):
    """The integrated branch (WS_HB_TABLES, the accumulation grids and the staging slots it shares with
    PerturbedField) and the extrema helper (WS_HB_PART)."""
    spec = halobox_spec(n, N, hires, make_tables())
    ics = halobox_ics(n, N, hires, seed=n + N)
    key = "hires_density" if hires else "lowres_density"

    def call():
        out = api.halobox_grids(spec, ics, with_whalo=True)
        out["min"], out["max"] = api.grid_minmax(ics[key])
        return out

    return call


@pytest.mark.parametrize("pt", [(16, 32, True), (80, 160, False)])
def test_perturb_and_ionize(api, pt):
    check_pair(perturb_call(api, *pt), ionize_ts_call(api, 64))


@pytest.mark.parametrize("n", [8, 40])
def test_brightness_and_halobox(api, n):
    check_pair(brightness_call(api, n), halobox_call(api, 16, 32, False))


@pytest.mark.parametrize("hb,pt", [((16, 32, False), (32, 64, False)), ((32, 64, True), (16, 32, True))])
def test_halobox_and_perturb(api, hb, pt):
    check_pair(halobox_call(api, *hb), perturb_call(api, *pt))


def test_halo_props_and_fused_recombination(api, gpu_lib, tmp_path):
    """test_halo_props stages ten host arrays; eight of its slots lie under the evaluated-window tables, the
    sharded TsBox exchange, WS_SFR_WORK2 and WS_R_DEV.  The ionize call's spectra are far larger than the
    catalogue's arrays; the property rows are larger than the ionize call's table of radii."""
    from test_gpu_abi import Session

    lib = gpu_lib
    n, nh, z = 16, 600, 11.0
    ses = Session(lib, tmp_path, HII_DIM=n, DIM=2 * n, USE_TS_FLUCT=True, USE_MINI_HALOS=True, Z_HEAT_MAX=35.0,
                  V_CB_MODEL=2, SOURCE_MODEL=2, HALO_SCALING_RELATIONS_MEDIAN=False)
    cat = random_catalogue(nh, ses.so.BOX_LEN * 0.9999, seed=21)
    cat["coords"] = np.abs(cat["coords"]) % np.float32(ses.so.BOX_LEN * 0.9999)
    rng = np.random.default_rng(4)
    vcb = (rng.random((n, n, n)) * 40).astype(np.float32)
    j21 = (10 ** rng.uniform(-3, 1, (n, n, n))).astype(np.float32)
    g12 = (10 ** rng.uniform(-2, 0, (n, n, n))).astype(np.float32)
    zre = np.where(rng.random((n, n, n)) < 0.5, rng.uniform(11.5, 16, (n, n, n)), -1.0).astype(np.float32)
    ptr = _bind_test_halo_props(lib)
    arrs = [cat[k] for k in ("masses", "coords", "star_rng", "sfr_rng", "xray_rng")]

    def halo_props():
        out = np.full((nh, 12), -7.0, np.float32)
        st = lib.test_halo_props(z, ptr(vcb), ptr(j21), ptr(zre), ptr(g12), nh, *[ptr(a) for a in arrs], ptr(out))
        assert st == 0, lib.c21cm_last_error()
        assert np.isfinite(out).all() and (out[:, 1] > 0).any()
        return {"props": out}

    check_pair(halo_props, ionize_fused_recomb_call(api, 128, 256))
