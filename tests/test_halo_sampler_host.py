"""The halo sampler's host side (csrc/host/halo_sampler_tables.c; no GPU needed): the exported condition
integrals and the inverse-CDF table against scipy quadrature / root finding of the exported conditional
mass function, the out-of-range markers, and the DexM radius ladder against a numpy walk.

Bounds.  Direct integrals and table NODES: rtol 1e-3, the reference's own quadrature tolerance
(IntegratedNdM_QAG, hmf.c:617).  Between nodes the tables are linear interpolants of curved functions; the
error was measured on the midpoints this test visits (every twelfth node interval inside the tested range;
DESIGN 4.13: cells 3.9e-4 PS / 3.2e-4 ST, descendants 7.3e-4 PS / 7.6e-4 ST, the larger of N and M) and the
assertion is twice the largest of those, BETWEEN_NODES_RTOL.  Inverse table: |d ln M| <= 1e-4 on nodes, the reference's root
tolerance (rf_tol_abs, interp_tables.c:676).
"""

import ctypes as C
import math

import numpy as np
import pytest
from scipy import integrate, optimize

from halo_sampler_reference import Condition

Z, Z_DESC = 7.0, 8.0 / 1.02 - 1.0
F99 = float(np.float32(0.99))
BETWEEN_NODES_RTOL = 2 * 7.6e-4
f64, dp = C.c_double, C.POINTER(C.c_double)


def ptr(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def host(pkg):
    lib = pkg.load()
    for name, args in (("dicke", [f64]), ("sigma_z0", [f64]), ("c21_sigma_fast", [f64]), ("c21_MtoR", [f64]),
                       ("c21_RtoM", [f64]), ("get_delta_crit", [C.c_int, f64, f64]),
                       ("conditional_hmf", [f64, f64, f64, f64, C.c_int]), ("expected_nhalo", [f64])):
        getattr(lib, name).restype = f64
        getattr(lib, name).argtypes = args
    lib.get_condition_integrals.restype = lib.get_halo_chmf_interval.restype = None
    lib.get_halomass_at_probability.restype = None
    lib.get_condition_integrals.argtypes = [f64, f64, C.c_int, dp, dp, dp]
    lib.get_halo_chmf_interval.argtypes = [f64, f64, C.c_int, dp, C.c_int, dp, dp, dp]
    lib.get_halomass_at_probability.argtypes = [f64, f64, C.c_int, dp, dp, dp]
    lib.c21cm_dexm_is_empty.argtypes = [f64]
    lib.c21cm_sampler_setup.argtypes = [f64, f64, C.c_ulonglong, C.c_void_p]
    return lib


def broadcast(lib, S, hmf=1, hii=32, box=128.0, **sim):
    keep = dict(so=S.default_simulation_options(HII_DIM=hii, DIM=2 * hii, BOX_LEN=box, SAMPLER_MIN_MASS=5e8, **sim),
                mo=S.default_matter_options(HMF=hmf, SOURCE_MODEL=4), cp=S.default_cosmo_params(),
                ap=S.default_astro_params(), ao=S.default_astro_options(), ct=S.default_cosmo_tables())
    lib.Broadcast_struct_global_all(*[C.byref(keep[k]) for k in ("so", "mo", "cp", "ap", "ao", "ct")])
    lib.init_ps()
    lib._keep_sampler_host = keep
    return keep


def spec_of(pkg, lib, z_desc):
    spec = pkg.structs.SampleHalosSpec()
    assert lib.c21cm_sampler_setup(Z, z_desc, 0, C.byref(spec)) == 0
    return spec


CELLS = np.array([-0.9, -0.5, 0.0, 1.0, 1.4])
MASSES = np.array([1e9, 1e10, 1e11, 1e12, 1e13])


@pytest.mark.parametrize("hmf", [0, 1])
@pytest.mark.parametrize("z_desc", [-1.0, Z_DESC])
def test_condition_integrals_against_quadrature(pkg, host, hmf, z_desc):
    broadcast(host, pkg.structs, hmf)
    spec = spec_of(pkg, host, z_desc)
    conds = MASSES if z_desc > 0 else CELLS
    lnM_min, lnM_max = math.log(spec.m_min), math.log(spec.m_max_tables)
    # get_halo_chmf_interval: direct quadrature over four mass intervals per condition
    lo = np.log(np.array([5e8, 3e9, 2e10, 5e8]))
    hi = np.log(np.array([3e9, 2e10, 1e16, 1e16]))
    out = np.zeros(conds.size * lo.size)
    host.get_halo_chmf_interval(Z, z_desc, conds.size, ptr(conds.copy()), lo.size, ptr(lo), ptr(hi), ptr(out))
    for i, v in enumerate(conds):
        c = Condition(host, spec, hmf, float(v))
        for j in range(lo.size):
            want = c.integral(lo[j], hi[j]) * c.M
            assert out[i * lo.size + j] == pytest.approx(want, rel=1e-3, abs=1e-12), (v, j)
    # the interpolated expected N, M: on the table's own nodes, and between them
    nodes = spec.x_min + spec.x_width * np.arange(spec.n_cond)
    span = np.log(conds) if z_desc > 0 else conds
    inside = nodes[(nodes >= span.min()) & (nodes <= span.max())]
    on = inside[:: max(1, inside.size // 6)]
    between = 0.5 * (inside[:-1] + inside[1:])[:: max(1, inside.size // 12)]
    worst = 0.0
    for xs, rtol in ((on, 1e-3), (between, BETWEEN_NODES_RTOL)):
        values = np.exp(xs) if z_desc > 0 else xs.copy()
        n, m = np.zeros(xs.size), np.zeros(xs.size)
        host.get_condition_integrals(Z, z_desc, xs.size, ptr(values), ptr(n), ptr(m))
        for k, v in enumerate(values):
            c = Condition(host, spec, hmf, float(v))
            want_n, want_m = c.integral(lnM_min, lnM_max) * c.M, c.integral(lnM_min, lnM_max, True) * c.M
            if rtol > 1e-3:
                worst = max(worst, abs(n[k] / want_n - 1), abs(m[k] / want_m - 1))
            assert n[k] == pytest.approx(want_n, rel=rtol), (v, "N")
            assert m[k] == pytest.approx(want_m, rel=rtol), (v, "M")
    print(f"hmf {hmf} z_desc {z_desc:.3f}: largest between-node error {worst:.2e}")


@pytest.mark.parametrize("hmf", [0, 1])
@pytest.mark.parametrize("z_desc", [-1.0, Z_DESC])
def test_inverse_table_against_root_finding(pkg, host, hmf, z_desc):
    broadcast(host, pkg.structs, hmf)
    spec = spec_of(pkg, host, z_desc)
    lnM_min = math.log(spec.m_min)
    rows = [5, 40, 90, 150, 190] if z_desc < 0 else [10, 40, 80, 120, 160]
    cols = [0, 20, 80, 160, 240, 320, 380, 396, 398]
    xs = spec.x_min + spec.x_width * np.array(rows)
    values = np.exp(xs) if z_desc > 0 else xs.copy()
    for v in values:
        c = Condition(host, spec, hmf, float(v))
        norm = c.integral(lnM_min, c.lnM)
        lnp = spec.p_min + spec.p_width * np.array(cols)
        out = np.zeros(len(cols))
        host.get_halomass_at_probability(Z, z_desc, len(cols), ptr(np.full(len(cols), v)), ptr(np.exp(lnp)), ptr(out))
        for k, target in enumerate(lnp):
            g = lambda x: math.log(max(c.integral(x, c.lnM), 1e-300) / norm) - target  # noqa: E731
            root = optimize.brentq(g, lnM_min, c.lnM - 1e-9, xtol=1e-6, rtol=1e-12)
            assert abs(math.log(out[k]) - root) <= 1e-4, (v, cols[k], math.log(out[k]), root)


def test_out_of_range_markers(pkg, host):
    broadcast(host, pkg.structs, 1)
    spec = spec_of(pkg, host, -1.0)
    top = F99 * host.get_delta_crit(1, spec.sigma_cell, spec.growth_out)
    conds = np.array([0.0, -1.5, top * 1.01, 0.0, 0.0, 0.5])
    probs = np.array([0.5, 0.5, 0.5, -0.1, 1.5, 1.0])
    out, n, m = np.zeros(6), np.zeros(6), np.zeros(6)
    host.get_halomass_at_probability(Z, -1.0, 6, ptr(conds), ptr(probs), ptr(out))
    assert list(out[1:5]) == [-1, -1, -1, -1] and out[0] > 0
    assert out[5] == pytest.approx(spec.m_min, rel=1e-12)  # p = 1: the sampling minimum
    host.get_condition_integrals(Z, -1.0, 6, ptr(conds), ptr(n), ptr(m))
    assert n[1] == -1 and n[2] == -1 and n[0] > 0 and m[0] > 0
    masses = np.array([1e10, 4e8, 2e16])
    out = np.zeros(3)
    host.get_halomass_at_probability(Z, Z_DESC, 3, ptr(masses), ptr(np.full(3, 0.3)), ptr(out))
    assert out[0] > 0 and out[1] == -1 and out[2] == -1
    # probabilities below exp(MIN_LOGPROB) are read at the table's edge
    tiny = np.zeros(2)
    host.get_halomass_at_probability(Z, Z_DESC, 2, ptr(np.full(2, 1e10)), ptr(np.array([0.0, 1e-9])), ptr(tiny))
    assert tiny[0] == tiny[1] > 0


def test_expected_nhalo_against_quadrature(pkg, host):
    """Nhalo_General over [SAMPLER_MIN_MASS, M_cell] times the box mass, against the sum over all cells at the
    mean density of the conditional integral in the limit of a large cell: checked instead against the
    unconditional limit of the conditional mass function (delta = 0, sigma_cond = 0), PS."""
    keep = broadcast(host, pkg.structs, 0)
    spec = spec_of(pkg, host, -1.0)
    D = host.dicke(Z)
    f = lambda x: host.conditional_hmf(D, x, 0.0, 0.0, 0)  # noqa: E731
    want = integrate.quad(f, math.log(5e8), math.log(spec.m_cell), epsrel=1e-8, limit=400)[0]
    box_mass = spec.m_cell * keep["so"].HII_DIM ** 3
    assert host.expected_nhalo(Z) == pytest.approx(want * box_mass, rel=1e-3)


@pytest.mark.parametrize("hii,box", [(32, 128.0), (64, 96.0)])
def test_dexm_ladder_against_a_numpy_walk(pkg, host, hii, box):
    """HaloCatalog.c:156-200 restated with the reference's float variables"""
    keep = broadcast(host, pkg.structs, 1, hii=hii, box=box)
    so = keep["so"]
    f32 = np.float32
    l_factor = 0.620350491
    for z in (6.0, 8.0, 10.0, 12.0, 16.0):
        growth = f32(host.dicke(z))
        m_min = f32(host.c21_RtoM(l_factor * so.BOX_LEN / so.HII_DIM))
        delta_r = f32(l_factor * 2.0 * so.BOX_LEN / so.DIM)
        R = f32(host.c21_MtoR(float(m_min) * 1.01))
        while R < l_factor * so.BOX_LEN:
            R = f32(float(R) * so.DELTA_R_FACTOR)
        empty = True
        while R > 0.5 * float(delta_r) and host.c21_RtoM(float(R)) >= float(m_min):
            M = f32(host.c21_RtoM(float(R)))
            sig, dl = host.sigma_z0(float(M)), 1.686 / float(growth)
            dcrit = f32(float(growth) * (math.sqrt(0.73) * dl * (1.0 + 0.15 * (sig * sig / (0.73 * dl * dl)) ** 0.05)))
            if not sig * float(growth) * 7.0 < float(dcrit):
                empty = False
                break
            R = f32(float(R) / so.DELTA_R_FACTOR)
        assert bool(host.c21cm_dexm_is_empty(z)) == empty, z
    assert not host.c21cm_dexm_is_empty(6.0) and host.c21cm_dexm_is_empty(16.0)


def test_unsupported_options_are_value_errors(pkg, host):
    S = pkg.structs
    host.c21hip_get_error.restype = C.c_char_p
    spec = S.SampleHalosSpec()
    for change, text in ((dict(SAMPLE_METHOD=2), "PARTITION"), (dict(SAMPLE_METHOD=3), "BINARY-SPLIT"),
                         (dict(HMF=2), "HMF"), (dict(USE_INTERPOLATION_TABLES=1), "USE_INTERPOLATION_TABLES")):
        keep = broadcast(host, S, 1)
        for k, v in change.items():
            setattr(keep["mo"], k, v)
        assert host.c21cm_sampler_setup(Z, Z_DESC, 0, C.byref(spec)) == 3
        assert text in host.c21hip_get_error().decode()
    broadcast(host, S, 1)
    assert host.c21cm_sampler_setup(Z, Z + 1.0, 0, C.byref(spec)) == 3
    assert "above the progenitor redshift" in host.c21hip_get_error().decode()


def test_dexm_ladder_answers_at_once_for_parameters_that_describe_no_box(pkg, host):
    """sigma_z0's adaptive quadrature does not return for a mass that is not finite; the ladder must not hand
    it one.  Parameters from which such a mass would follow (a box length whose top-hat mass overflows a
    float, non-finite values, a step factor next to 1) answer "not empty" without integrating anything."""
    S = pkg.structs
    for change in (dict(BOX_LEN=1e30), dict(BOX_LEN=float("inf")), dict(BOX_LEN=float("nan")),
                   dict(DELTA_R_FACTOR=1.0 + 1e-9), dict(DELTA_R_FACTOR=float("nan"))):
        keep = broadcast(host, S, 1)
        for k, v in change.items():
            setattr(keep["so"], k, v)
        assert host.c21cm_dexm_is_empty(11.0) == 0, change
    keep = broadcast(host, S, 1)
    keep["cp"].OMm = float("nan")
    assert host.c21cm_dexm_is_empty(11.0) == 0
    # expected_nhalo integrates between masses from the same globals: NaN at once where they are not finite
    assert math.isnan(host.expected_nhalo(11.0))
    for change in (dict(BOX_LEN=float("inf")), dict(SAMPLER_MIN_MASS=float("inf")), dict(SAMPLER_MIN_MASS=0.0)):
        keep = broadcast(host, S, 1)
        for k, v in change.items():
            setattr(keep["so"], k, v)
        assert math.isnan(host.expected_nhalo(11.0)), change
    broadcast(host, S, 1)
    assert host.expected_nhalo(11.0) > 0


def test_tables_of_a_coarse_redshift_ladder(pkg, host):
    """the snapshots of a run with ZPRIME_STEP_FACTOR = 1.15 from z = 11 upwards, cells first, then
    descendants with steps of dz ~ 1.8 instead of 0.16: every table entry finite, expected N and M within
    [0, 1] of the condition, the inverse CDF falling from 1 towards M_min / M_cond along ln p"""
    broadcast(host, pkg.structs, 1)
    z, z_below = 11.0, -1.0
    for _ in range(5):
        spec = pkg.structs.SampleHalosSpec()
        assert host.c21cm_sampler_setup(z, z_below, 0, C.byref(spec)) == 0
        nx, ny = spec.n_cond, spec.n_prob
        t = np.ctypeslib.as_array(spec.tables, shape=(nx * (3 + ny),))
        assert np.isfinite(t).all()
        x = spec.x_min + spec.x_width * np.arange(nx)
        m_cond = np.exp(x) if z_below > 0 else np.full(nx, spec.m_cell)
        assert (t[:nx] >= 0).all() and (t[nx:2 * nx] >= 0).all() and (t[nx:2 * nx] <= 1 + 1e-9).all()
        inv = t[3 * nx:].reshape(nx, ny)
        assert (inv >= 0).all() and (inv <= 1 + 1e-9).all()
        rows = m_cond > 2 * spec.m_min  # conditions that can hold a sampled halo at all
        assert (np.diff(inv[rows][:, 1:], axis=1) <= 1e-12).all()
        z_below, z = z, (1 + z) * 1.15 - 1
