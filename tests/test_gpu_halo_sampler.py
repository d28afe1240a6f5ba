"""The halo sampler on the device (SOURCE_MODEL = CHMF-SAMPLER; reference: Stochasticity.c:663-1113,
HaloCatalog.c:38-54), through the grid-level entry and ComputeHaloCatalog.

Comparator: tests/halo_sampler_reference.py, a numpy restatement that makes the same indexed draws.  Both
sides do the same fp64 operations in the same order (the library is built without fused multiply-adds), so
every count, mass, coordinate and deviate is expected bit-equal; log / pow / sin / cos of the two maths
libraries may differ in the last fp64 bit, which can cross a float32 rounding boundary or flip a comparison
once in ~2^29 values, hence the allowance of max(1, 1e-4 n_cond) differing conditions.  Thread path, wave
path and a repeated call must agree byte for byte: nothing but integer sums and indexed draws decides.

The statistical bounds are derived in the tests that use them.
"""

import ctypes as C
import importlib

import numpy as np
import pytest

import halo_sampler_reference as R

pytestmark = pytest.mark.gpu
S = importlib.import_module("21cmfast_amd.structs")
BackendError = importlib.import_module("21cmfast_amd._lib").BackendError

Z, Z_DESC = 7.0, 8.0 / 1.02 - 1.0
FIELDS = ("halo_masses", "halo_coords", "star_rng", "sfr_rng", "xray_rng")


@pytest.fixture()
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def broadcast(lib, hii=16, box=64.0, **matter):
    """globals of a 4 Mpc-cell box; kept alive on the library object"""
    keep = dict(so=S.default_simulation_options(HII_DIM=hii, DIM=4 * hii, BOX_LEN=box, SAMPLER_MIN_MASS=5e8),
                mo=S.default_matter_options(**matter), cp=S.default_cosmo_params(), ap=S.default_astro_params(),
                ao=S.default_astro_options(), ct=S.default_cosmo_tables())
    lib.Broadcast_struct_global_all(*[C.byref(keep[k]) for k in ("so", "mo", "cp", "ap", "ao", "ct")])
    lib.init_ps()
    lib._keep_sampler = keep
    return keep


def descendants(masses, box, seed, far=False):
    rng = np.random.default_rng(seed)
    n = masses.size
    coords = (rng.random((n, 3)) * box).astype(np.float32)
    coords[:3] = [[0.0, 0.01, box - 0.01], [box - 1e-3, 0.0, 0.5 * box], [0.02, box - 0.02, 0.0]]  # next to the faces
    if far:  # far outside the box on either side: progenitors still land inside
        coords[3:5] = [[-7.3 * box, 9.6 * box, -0.2 * box], [41.0 * box, -55.5 * box, 1.5 * box]]
    return dict(halo_masses=masses.astype(np.float32), halo_coords=coords,
                star_rng=rng.standard_normal(n).astype(np.float32),
                sfr_rng=rng.standard_normal(n).astype(np.float32),
                xray_rng=rng.standard_normal(n).astype(np.float32))


def run(api, spec, n_cond, rows, **inputs):
    out = S.empty_halo_catalog(rows)
    api.sample_halos(spec, out, **inputs)
    n = out.n_halos
    cat = {f: out.arrays[f] for f in FIELDS}
    for f in FIELDS:  # condense_sparse_halolist: zeros beyond n_halos
        assert not cat[f][n:].any(), f
    cat = {f: cat[f][:n].copy() for f in FIELDS}
    cat["counts"] = api.sample_halos_counts(n_cond).astype(np.int64)
    assert cat["counts"].sum() == n
    return cat


def differing_conditions(got, ref):
    """conditions whose count or any halo differs (bitwise)"""
    same = got["counts"] == ref["counts"]
    bad = int((~same).sum())
    cg, cr = got["counts"], ref["counts"]
    og, orr = np.cumsum(cg) - cg, np.cumsum(cr) - cr
    cond = np.repeat(np.flatnonzero(same), cg[same])
    within = np.arange(cond.size) - np.repeat(np.cumsum(cg[same]) - cg[same], cg[same])
    rg, rr = og[cond] + within, orr[cond] + within
    row_bad = np.zeros(cond.size, bool)
    for f in FIELDS:
        a, b = got[f][rg].view(np.uint32), ref[f][rr].view(np.uint32)
        row_bad |= (a != b).reshape(cond.size, -1).any(axis=1)
    return bad + np.unique(cond[row_bad]).size


def same_bytes(a, b):
    return all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in FIELDS) and \
        np.array_equal(a["counts"], b["counts"])


@pytest.mark.parametrize("hmf,method", [(1, 0), (1, 1), (0, 0)])
def test_progenitors_draw_for_draw(gpu_lib, api, hmf, method):
    """2048 descendants: 1e9 ... 1e13 log-spaced, 32 copies of 1e13 (hundreds of draws each), masses beyond
    the 7 sigma truncation (one progenitor of the expected mass), masses below SAMPLER_MIN_MASS but above the
    sampling minimum (no halo)."""
    broadcast(gpu_lib, HMF=hmf, SAMPLE_METHOD=method)
    spec = api.sampler_spec(Z, Z_DESC, seed=12345)
    # number-limited sampling has no rare-halo shortcut: 5e15 Msun would expect more halos than the cap
    top = [1e14, 1e15, 3e14, 5e14] if method else [1e14, 1e15, 5e15, 9.9e15]
    masses = np.concatenate([np.logspace(9, 13, 2008), np.full(32, 1e13), [3e8, 4.9e8, 2e14, 6e14], top])
    assert masses.size == 2048
    desc = descendants(masses, spec.box_len, 7, far=True)
    ref = R.Sampler(spec)
    c = ref.setup(desc["halo_masses"])
    expected = ref.catalogue(desc)
    kinds = set(np.unique(c["kind"]))
    assert (R.K_NUMBER if method else R.K_MASS) in kinds
    if not method:
        assert R.K_SINGLE in kinds, "no descendant took the rare-halo shortcut"
        assert (ref.words["removed"] == R.DROP_LAST).any() and ((ref.words["removed"] & ~R.DROP_LAST) > 1).any()
    assert ref.words["drawn"].max() > 128  # more than two rounds of a wave
    rows = int(expected["counts"].sum()) + 100
    got = run(api, spec, 2048, rows, desc=desc)
    n_bad = differing_conditions(got, expected)
    print(f"hmf {hmf} method {method}: {got['counts'].sum()} halos, {n_bad} conditions differ")
    assert got["halo_coords"].min() >= 0 and got["halo_coords"].max() < np.float32(spec.box_len)
    assert n_bad <= max(1, int(1e-4 * 2048))
    for path in (1, 2):  # every condition on the thread path, on the wave path
        spec.path = path
        assert same_bytes(run(api, spec, 2048, rows, desc=desc), got), path
    spec.path = 0
    assert same_bytes(run(api, spec, 2048, rows, desc=desc), got)


@pytest.mark.parametrize("hmf,method,with_extras", [(1, 0, False), (0, 1, True)])
def test_grid_draw_for_draw(gpu_lib, api, hmf, method, with_extras):
    """16^3 cells from delta = -1.2 to above delta_c (cells are always number-limited, so both sample
    methods must give this); with_extras: a catalogue of large halos in front and an overlap box."""
    broadcast(gpu_lib, HMF=hmf, SAMPLE_METHOD=method)
    spec = api.sampler_spec(Z, -1.0, seed=99)
    n = 16 ** 3
    delta = np.linspace(-1.2, 1.9, n)
    np.random.default_rng(3).shuffle(delta)
    density = (delta / spec.growth_out).astype(np.float32).reshape(16, 16, 16)
    overlap = large = None
    if with_extras:
        overlap = np.random.default_rng(4).choice([0.0, 0.25, 1.0], n).astype(np.float32).reshape(16, 16, 16)
        large = descendants(np.array([3e12, 4e12, 5e12]), spec.box_len, 5)
    ref = R.Sampler(spec)
    c = ref.setup(density, overlap)
    assert {R.K_NONE, R.K_SINGLE, R.K_NUMBER} <= set(np.unique(c["kind"]))
    expected = ref.catalogue()
    rows = int(expected["counts"].sum()) + 64
    got = run(api, spec, n, rows, density=density, overlap=overlap)
    n_bad = differing_conditions(got, expected)
    print(f"grid hmf {hmf}: {got['counts'].sum()} halos, {n_bad} conditions differ")
    assert n_bad <= max(1, int(1e-4 * n))
    # placement: every halo in its own cell, +-0.5 cell around the index, wrapped into the box
    cell = spec.box_len / 16
    cond = np.repeat(np.arange(n), got["counts"])
    idx = np.stack([cond // 256, (cond // 16) % 16, cond % 16], axis=1)
    off = got["halo_coords"].astype(np.float64) / cell - idx
    off -= 16 * np.rint(off / 16)
    assert np.abs(off).max() <= 0.5 + 1e-5
    assert got["halo_coords"].min() >= 0 and got["halo_coords"].max() < np.float32(spec.box_len)
    for path in (1, 2):
        spec.path = path
        assert same_bytes(run(api, spec, n, rows, density=density, overlap=overlap), got), path
    spec.path = 0
    if with_extras:  # the large halos come first, untouched; the sampled ones follow unchanged
        out = S.empty_halo_catalog(rows + 3)
        api.sample_halos(spec, out, density=density, overlap=overlap, large=large)
        assert out.n_halos == got["counts"].sum() + 3
        for f in FIELDS:
            assert np.array_equal(out.arrays[f][:3], large[f].reshape(out.arrays[f][:3].shape)), f
            assert np.array_equal(out.arrays[f][3:out.n_halos], got[f]), f


def test_poisson_counts_from_first_principles(gpu_lib, api):
    """15000 cells at delta = 0, everything drawn is stored (the storage cut lowered to the sampling
    minimum), so the counts are the Poisson numbers themselves: mean lambda with standard error
    sqrt(lambda / n), variance / mean = 1 with standard error sqrt(2 / n); five of each."""
    broadcast(gpu_lib, SAMPLE_METHOD=1)
    spec = api.sampler_spec(Z, -1.0, seed=2024)
    spec.hii_dim, spec.hii_dim_z = 25, 24
    spec.sampler_min_mass = 0.0
    n = 25 * 25 * 24
    assert n == 15000
    density = np.zeros((25, 25, 24), np.float32)
    ref = R.Sampler(spec)
    lam = float(ref.setup(density)["exp_N"][0])
    assert lam > 20  # several pieces of the mean per cell
    got = run(api, spec, n, int(1.2 * lam * n), density=density)
    counts = got["counts"].astype(np.float64)
    print(f"lambda {lam:.4f} mean {counts.mean():.4f} variance/mean {counts.var(ddof=1) / counts.mean():.4f}")
    assert abs(counts.mean() - lam) <= 5 * np.sqrt(lam / n)
    assert abs(counts.var(ddof=1) / counts.mean() - 1) <= 5 * np.sqrt(2 / n)


def test_progenitor_placement_and_correlations(gpu_lib, api):
    """60000 descendants of 1e11 Msun: progenitors within R(M_desc) - R(M_prog) of the descendant modulo the
    box; each deviate correlates with its descendant's by exp(-dz / CORR_*) within 5 / sqrt(n) and has unit
    variance within 5 sqrt(2 / n) (a conditioned bivariate normal: standard errors (1 - rho^2) / sqrt(n) and
    sqrt(2 / n))."""
    keep = broadcast(gpu_lib)
    spec = api.sampler_spec(Z, Z_DESC, seed=77)
    n_desc = 60000
    desc = descendants(np.full(n_desc, 1e11), spec.box_len, 11)
    got = run(api, spec, n_desc, 12 * n_desc, desc=desc)
    n = int(got["counts"].sum())
    assert n >= 100000
    parent = np.repeat(np.arange(n_desc), got["counts"])
    box = spec.box_len
    d = got["halo_coords"].astype(np.float64) - desc["halo_coords"][parent].astype(np.float64)
    d -= box * np.rint(d / box)
    radius = lambda m: np.cbrt(m.astype(np.float64) / spec.rtom_unit)  # noqa: E731
    slack = radius(desc["halo_masses"][parent]) - radius(got["halo_masses"])
    assert (np.sqrt((d * d).sum(axis=1)) <= slack + 1e-4).all()  # float32 coordinates of a 64 Mpc box
    assert got["halo_coords"].min() >= 0 and got["halo_coords"].max() < np.float32(box)
    dz = Z - Z_DESC
    for f, corr in (("star_rng", keep["so"].CORR_STAR), ("sfr_rng", keep["so"].CORR_SFR),
                    ("xray_rng", keep["so"].CORR_LX)):
        x, y = desc[f][parent].astype(np.float64), got[f].astype(np.float64)
        rho = np.corrcoef(x, y)[0, 1]
        print(f"{f}: rho {rho:.4f} expected {np.exp(-dz / corr):.4f} variance {y.var():.4f} n {n}")
        assert abs(rho - np.exp(-dz / corr)) <= 5 / np.sqrt(n)
        assert abs(y.var() - 1) <= 5 * np.sqrt(2 / n)


def test_cap_and_bad_conditions_are_errors(gpu_lib, api):
    """a condition that needs more draws than the cap, and a descendant outside the tables, are ValueErrors
    naming the condition; nothing is truncated"""
    broadcast(gpu_lib)
    spec = api.sampler_spec(Z, Z_DESC, seed=1)
    desc = descendants(np.array([1e10, 1e10, 1e13, 1e10]), spec.box_len, 2)
    spec.max_halo_cell = 4
    with pytest.raises(BackendError, match="too many halos in condition 2"):
        api.sample_halos(spec, S.empty_halo_catalog(1000), desc=desc)
    spec.max_halo_cell = 0
    desc["halo_masses"][1] = 1e8
    with pytest.raises(BackendError, match="condition 1 of 4 lies outside the tables"):
        api.sample_halos(spec, S.empty_halo_catalog(1000), desc=desc)


# ---------------------------------------------------------------- the boundary
def compute_halo_catalog(lib, z_desc, z, ics, seed, desc, out):
    lib.ComputeHaloCatalog.restype = C.c_int
    lib.ComputeHaloCatalog.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p]
    return lib.ComputeHaloCatalog(z_desc, z, C.byref(ics) if ics is not None else None, seed,
                                  C.byref(desc) if desc is not None else None, C.byref(out))


def error_text(lib):
    lib.c21hip_get_error.restype = C.c_char_p
    return lib.c21hip_get_error().decode()


def test_boundary(gpu_lib, api):
    import torch

    lib = gpu_lib
    broadcast(lib, SOURCE_MODEL=4)
    masses = np.logspace(9.5, 12.5, 500)
    desc = descendants(masses, 64.0, 21)
    desc_s = api._catalog_of(desc)
    out = S.empty_halo_catalog(20000)
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, desc_s, out) == 0, error_text(lib)
    n = out.n_halos
    assert 500 < n < 20000
    for f in FIELDS:
        assert not out.arrays[f][n:].any()
    # the same catalogue from device arrays
    desc_t = {f: torch.from_numpy(desc[f]).cuda() for f in FIELDS}
    out_t = S.empty_halo_catalog(20000, device="cuda")
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, api._catalog_of(desc_t), out_t) == 0, error_text(lib)
    assert out_t.n_halos == n
    for f in FIELDS:
        assert np.array_equal(out_t.arrays[f].cpu().numpy(), out.arrays[f]), f
    # one row short: ValueError, nothing written
    short = S.empty_halo_catalog(n - 1)
    for f in FIELDS:
        short.arrays[f][...] = -7.25
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, desc_s, short) == 3
    assert "HALO_CATALOG_MEM_FACTOR" in error_text(lib) and f"{n} halos" in error_text(lib)
    for f in FIELDS:
        assert (short.arrays[f] == np.float32(-7.25)).all(), f
    # no descendants
    empty = S.HaloCatalogStruct(n_halos=0, buffer_size=0)
    out.n_halos = 99
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, empty, out) == 0 and out.n_halos == 0
    # refusals
    assert compute_halo_catalog(lib, Z + 1, Z, None, 5, desc_s, out) == 3
    assert "above the progenitor redshift" in error_text(lib)
    broadcast(lib, SOURCE_MODEL=4, SAMPLE_METHOD=2)
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, desc_s, out) == 3
    assert "PARTITION" in error_text(lib)
    broadcast(lib, SOURCE_MODEL=3)
    assert compute_halo_catalog(lib, Z_DESC, Z, None, 5, desc_s, out) == 3
    assert "DexM halo finder" in error_text(lib)
    # cells: allowed where the DexM ladder finds nothing, refused with the finder's name elsewhere
    lib.c21cm_dexm_is_empty.argtypes = [C.c_double]
    broadcast(lib, SOURCE_MODEL=4)
    ics = S.InitialConditionsStruct()
    density = (np.random.default_rng(8).standard_normal((16, 16, 16)) * 2.0).astype(np.float32)
    ics.lowres_density = density.ctypes.data_as(S.c_float_p)
    assert not lib.c21cm_dexm_is_empty(Z)
    assert compute_halo_catalog(lib, -1.0, Z, ics, 5, None, out) == 3
    assert "DexM halo finder" in error_text(lib)
    z_hi = 14.0
    assert lib.c21cm_dexm_is_empty(z_hi)
    big = S.empty_halo_catalog(400000)
    assert compute_halo_catalog(lib, -1.0, z_hi, ics, 5, None, big) == 0, error_text(lib)
    spec = api.sampler_spec(z_hi, -1.0, seed=5)
    direct = run(api, spec, 16 ** 3, 400000, density=density)
    assert big.n_halos == direct["counts"].sum() > 0
    for f in FIELDS:
        assert np.array_equal(big.arrays[f][:big.n_halos], direct[f]), f


@pytest.mark.parametrize("hmf", [0, 1])
@pytest.mark.parametrize("cond_type", ["cat", "grid"])
def test_known_answer_statistics(gpu_lib, api, hmf, cond_type):
    """The reference's own known-answer test (its tests/test_halo_sampler.py:33-142) with its numbers, through
    single_test_sample: 15000 copies of one condition (five overdensities, five descendant masses),
    SAMPLER_MIN_MASS = 5e8, z = 7; mean count per condition against out_n_exp at rtol 0.1 / atol 1, mean mass
    against out_m_exp at rtol 0.1 / atol SAMPLER_MIN_MASS (both expectations held to quadrature first), the mass
    function in 10-per-dex bins up to 1e14 against get_halo_chmf_interval at rtol 0.5 / atol two halos.  The box
    is the reference test's (HII_DIM = 50, BOX_LEN = 100: 2 Mpc cells); all twenty cases are held to it."""
    lib = gpu_lib
    f64, dp = C.c_double, C.POINTER(C.c_double)
    for name, args in (("c21_sigma_fast", [f64]), ("get_delta_crit", [C.c_int, f64, f64]),
                       ("conditional_hmf", [f64, f64, f64, f64, C.c_int])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = f64, args
    lib.get_halo_chmf_interval.restype = None
    lib.get_halo_chmf_interval.argtypes = [f64, f64, C.c_int, dp, C.c_int, dp, dp, dp]
    broadcast(lib, hii=50, box=100.0, HMF=hmf)  # the box of the reference's test: 2 Mpc cells
    from_cat = cond_type == "cat"
    z_desc = Z_DESC if from_cat else -1.0
    n_cond, min_mass = 15000, 5e8
    edges = np.linspace(np.log10(min_mass), 14.0, int(10 * (14.0 - np.log10(min_mass)))) * np.log(10)
    lo, hi = edges[:-1].copy(), edges[1:].copy()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.single_test_sample.restype = C.c_int
    lib.single_test_sample.argtypes = [C.c_ulonglong, C.c_int, fp, fp, f64, f64, ip, ip, dp, dp, dp, fp, fp]
    crd = (np.random.default_rng(17).random((n_cond, 3)) * 100.0).astype(np.float32)
    for k, value in enumerate([1e9, 1e10, 1e11, 1e12, 1e13] if from_cat else [-0.9, -0.5, 0.0, 1.0, 1.4]):
        conditions = np.full(n_cond, value, np.float32)
        value = float(conditions[0])
        n_tot, n_cell = np.zeros(1, np.int32), np.zeros(n_cond, np.int32)
        n_exp, m_cell, m_exp = np.zeros(n_cond), np.zeros(n_cond), np.zeros(n_cond)
        masses, coords = np.zeros(500 * n_cond, np.float32), np.zeros((500 * n_cond, 3), np.float32)
        st = lib.single_test_sample(1000 + k, n_cond, conditions.ctypes.data_as(fp), crd.ctypes.data_as(fp), Z, z_desc,
                                    n_tot.ctypes.data_as(ip), n_cell.ctypes.data_as(ip), n_exp.ctypes.data_as(dp),
                                    m_cell.ctypes.data_as(dp), m_exp.ctypes.data_as(dp), masses.ctypes.data_as(fp),
                                    coords.ctypes.data_as(fp))
        assert st == 0, error_text(lib)
        n = int(n_tot[0])
        assert n == n_cell.sum() and (n_exp == n_exp[0]).all() and (m_exp == m_exp[0]).all()
        masses, coords = masses[:n], coords[:n]
        np.testing.assert_allclose(m_cell.sum(), masses.astype(np.float64).sum(), rtol=1e-12)
        # the expectations above SAMPLER_MIN_MASS against scipy quadrature of the exported mass function
        spec = api.sampler_spec(Z, z_desc, seed=1000 + k)
        c = R.Condition(lib, spec, hmf, value)
        np.testing.assert_allclose(n_exp[0], c.integral(np.log(min_mass), np.log(1e16)) * c.M, rtol=1e-3)
        np.testing.assert_allclose(m_exp[0], c.integral(np.log(min_mass), np.log(1e16), True) * c.M, rtol=1e-3)
        if not from_cat:  # every halo in the cell of its condition's position
            idx = np.repeat(np.trunc(crd.astype(np.float64) / 100.0 * 50), n_cell, axis=0)
            off = coords.astype(np.float64) / (100.0 / 50) - idx
            off -= 50 * np.rint(off / 50)
            assert np.abs(off).max() <= 0.5 + 1e-5
        binned = np.zeros(lo.size)
        lib.get_halo_chmf_interval(Z, z_desc, 1, np.array([value]).ctypes.data_as(dp), lo.size,
                                   lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), binned.ctypes.data_as(dp))
        hist, _ = np.histogram(np.log(masses.astype(np.float64)), edges)
        worst = np.max(np.abs(hist - binned * n_cond) - 0.5 * binned * n_cond)
        print(f"hmf {hmf} {cond_type} {value:g}: N {n_cell.mean():.4f} / {n_exp[0]:.4f}, M {m_cell.mean():.4e} / "
              f"{m_exp[0]:.4e}, largest |hist - expected| - rtol * expected over the bins {worst:.2f} halos")
        np.testing.assert_allclose(n_cell.mean(), n_exp[0], rtol=0.1, atol=1)
        np.testing.assert_allclose(m_cell.mean(), m_exp[0], rtol=0.1, atol=min_mass)
        np.testing.assert_allclose(hist, binned * n_cond, rtol=0.5, atol=2)  # halos per bin, all conditions
