"""The DexM halo finder on the device (reference: HaloCatalog.c:38-456), through the grid-level entry
c21cm_find_halos_grids, ComputeHaloCatalog and the drivers.

Comparator: tests/dexm_reference.py, the reference's serial raster-order greedy restated in numpy.  The
selection is integer and float32 arithmetic that both sides do in the same order, so masses, coordinates,
n_halos and the in_halo box are compared byte for byte, at every path (0 rounds + tail, 1 serial workgroup,
2 rounds only) and on a repeated call.

Filtered fields are compared with a float64 numpy filter.  The bound is four times the largest error of the
existing c21cm_filter_grid against the same float64 filter on the same input and radii, computed in the test:
both run the same float32 transforms, and the finder adds one multiply by the growth factor.  The catalogue
of a full run is compared with the restatement run on the RETURNED float32 fields: thresholding float32
transforms against a float64 filter is ill-posed for cells next to the threshold.
"""

import ctypes as C
import importlib

import numpy as np
import pytest

import dexm_reference as D

pytestmark = pytest.mark.gpu
S = importlib.import_module("21cmfast_amd.structs")
BackendError = importlib.import_module("21cmfast_amd._lib").BackendError

FIELDS = ("halo_masses", "halo_coords", "star_rng", "sfr_rng", "xray_rng")
RTOM = 1.0e10  # any positive unit: the masses below are RTOM R^3, so MtoR gives the radius back


@pytest.fixture()
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def make_spec(dim, dim_z, box_len, R, crit, r_overlap=1.0, optimize=0, minmass=0.0, mode=1, path=0, seed=11,
              hii=0, hii_z=0, halo_filter=0, growth=1.0, redshift=8.0):
    spec = S.FindHalosSpec()
    spec.dim, spec.dim_z, spec.hii_dim, spec.hii_dim_z = dim, dim_z, hii, hii_z
    spec.halo_filter, spec.n_R, spec.optimize, spec.filtered_mode, spec.path = halo_filter, len(R), optimize, mode, path
    spec.seed, spec.redshift = seed, redshift
    spec.box_len, spec.box_len_z = box_len, box_len * dim_z / dim
    spec.growth, spec.r_overlap, spec.optimize_minmass, spec.rtom_unit = growth, r_overlap, minmass, RTOM
    R = np.asarray(R, np.float32)
    for r in range(len(R)):
        spec.R[r] = R[r]
        spec.mass[r] = np.float32(RTOM * float(R[r]) ** 3)
        spec.delta_crit[r] = np.float32(crit[r])
    return spec


def spec_arrays(spec):
    n = spec.n_R
    return (np.array(spec.R[:n], np.float32), np.array(spec.mass[:n], np.float32),
            np.array(spec.delta_crit[:n], np.float32))


def reference_of(spec, filtered):
    f = D.Finder(spec.dim, spec.dim_z, spec.box_len, spec.r_overlap, spec.optimize, spec.optimize_minmass, spec.rtom_unit)
    R, mass, crit = spec_arrays(spec)
    in_halo, rung_of, per_rung, over = f.run(filtered, R, mass, crit)
    cat = f.catalogue(rung_of, mass, spec.seed, spec.redshift)
    return dict(in_halo=in_halo, per_rung=per_rung, over=over, cat=cat)


def run(api, spec, filtered=None, density=None, rows=None, device=False, overlap_shape=None):
    n = spec.dim * spec.dim * spec.dim_z
    rows = n if rows is None else rows
    if device:
        import torch

        dev = "cuda:0"
        out = S.empty_halo_catalog(rows, device=dev)
        in_halo = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        overlap = torch.full(overlap_shape, -3.0, dtype=torch.float32, device=dev) if overlap_shape else None
        filtered = torch.from_numpy(filtered).to(dev) if filtered is not None else None
        density = torch.from_numpy(density).to(dev) if density is not None else None
    else:
        out = S.empty_halo_catalog(rows)
        in_halo = np.full(n, 7, np.uint8)
        overlap = np.full(overlap_shape, -3.0, np.float32) if overlap_shape else None
    api.find_halos(spec, density, out, filtered=filtered, in_halo=in_halo, overlap=overlap)
    rep = api.find_halos_report()
    host = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
    k = out.n_halos
    cat = {f: host(out.arrays[f]) for f in FIELDS}
    for f in FIELDS:
        assert not cat[f][k:].any(), f  # zeros beyond n_halos
    return dict(n=k, cat={f: cat[f][:k].copy() for f in FIELDS}, in_halo=host(in_halo).copy(), rep=rep,
                overlap=None if overlap is None else host(overlap).copy(),
                filtered=None if filtered is None else host(filtered))


def assert_selection_equal(got, ref, what):
    assert got["n"] == ref["cat"]["halo_masses"].size, what
    assert np.array_equal(got["in_halo"], ref["in_halo"]), what
    for f in ("halo_masses", "halo_coords"):
        assert np.array_equal(got["cat"][f].view(np.uint32), ref["cat"][f].view(np.uint32)), (what, f)
    n_R = got["rep"].n_R
    assert list(got["rep"].accepted[:n_R]) == ref["per_rung"], what


def same_bytes(a, b):
    return a["n"] == b["n"] and np.array_equal(a["in_halo"], b["in_halo"]) and all(
        np.array_equal(a["cat"][f].view(np.uint32), b["cat"][f].view(np.uint32)) for f in FIELDS)


def check_all_paths(api, spec, filtered, ref, what):
    """paths 0, 1, 2, each twice: the restatement's bytes, and identical bytes among all six runs"""
    first, reports = None, {}
    for path in (0, 1, 2):
        spec.path = path
        for again in (0, 1):
            got = run(api, spec, filtered=filtered)
            assert_selection_equal(got, ref, (what, path, again))
            first = first or got
            assert same_bytes(got, first), (what, path, again)
            reports[path] = got["rep"]
    spec.path = 0
    return first, reports


def smooth_field(shape, scale, seed):
    """white noise smoothed with a Gaussian of `scale` cells, unit variance, float64"""
    rng = np.random.default_rng(seed)
    k = [np.fft.fftfreq(n) * 2.0 * np.pi for n in shape[:2]] + [np.fft.rfftfreq(shape[2]) * 2.0 * np.pi]
    ksq = k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2 + k[2][None, None, :] ** 2
    a = np.fft.irfftn(np.fft.rfftn(rng.standard_normal(shape)) * np.exp(-0.5 * ksq * scale * scale), s=shape,
                      axes=(0, 1, 2))
    return a / a.std()


def ladder_fields(shape, r_idx, seed):
    """one field per rung: the same white noise smoothed at half the rung's radius"""
    return np.stack([smooth_field(shape, 0.5 * r, seed) for r in r_idx]).astype(np.float32).reshape(len(r_idx), -1)


CELL = 2.0  # Mpc
R_IDX_LADDER = 6.0 / 1.1 ** np.arange(24)  # 6 ... 0.67 cells


@pytest.fixture(scope="module")
def gaussian_case():
    """(a): per box the fields, the spec's numbers and the serial restatement, computed once"""
    cases = {}
    for shape in ((32, 32, 32), (32, 32, 48)):
        filtered = ladder_fields(shape, R_IDX_LADDER, 5)
        spec = make_spec(shape[0], shape[2], CELL * shape[0], R_IDX_LADDER * CELL, [1.5] * 24)
        cases[shape] = (filtered, reference_of(spec, filtered))
    return cases


@pytest.mark.parametrize("shape", [(32, 32, 32), (32, 32, 48)])
def test_selection_gaussian_ladder(api, gaussian_case, shape):
    """(a) 24 rungs from 6 to 0.67 cells, one threshold of 1.5 sigma: thousands of candidates and hundreds of
    halos on the small rungs, chains of candidates that block each other over several rounds"""
    filtered, ref = gaussian_case[shape]
    spec = make_spec(shape[0], shape[2], CELL * shape[0], R_IDX_LADDER * CELL, [1.5] * 24)
    assert max(ref["over"]) > 1500 and max(ref["per_rung"]) > 100 and ref["in_halo"].any()
    got, reports = check_all_paths(api, spec, filtered, ref, "gaussian")
    rep = reports[2]
    print("rounds per rung:", list(rep.rounds[:24]), "candidates:", list(rep.candidates[:24]), "accepted:",
          list(rep.accepted[:24]))
    assert max(rep.rounds[:24]) > 1  # some rung needed more than one round: order mattered
    assert all(reports[1].tail[r] == (reports[1].candidates[r] > 0) for r in range(24))
    assert not any(reports[2].tail[:24])


@pytest.mark.parametrize("shape", [(32, 32, 32), (32, 32, 48)])
def test_selection_every_cell_a_candidate(api, shape):
    """(b) one rung of 1.5 cells with every cell over the threshold: the longest chains, each accepted halo
    waits for the decisions before it in raster order; path 0 must reach the round cap and finish in the
    serial tail"""
    n = shape[0] * shape[1] * shape[2]
    filtered = np.ones((1, n), np.float32)
    spec = make_spec(shape[0], shape[2], CELL * shape[0], [1.5 * CELL], [0.5])
    ref = reference_of(spec, filtered)
    assert ref["over"] == [n] and ref["per_rung"][0] > 100
    got, reports = check_all_paths(api, spec, filtered, ref, "every cell")
    assert reports[0].candidates[0] == n and reports[0].tail[0] == 1
    assert reports[0].rounds[0] == 64  # C21CM_DEXM_ROUND_CAP: every round decides at least the earliest candidate
    assert reports[2].tail[0] == 0 and reports[2].rounds[0] > 64
    print("rounds without the cap:", reports[2].rounds[0], "halos:", got["n"])


@pytest.mark.parametrize("r_overlap", [0.0, 1.0, 2.0])
def test_selection_overlap_factor(api, r_overlap):
    """(c) DEXM_R_OVERLAP 0 (the own cell alone is tested), 1 and 2"""
    shape = (32, 32, 32)
    r_idx = R_IDX_LADDER[::3]
    filtered = ladder_fields(shape, r_idx, 9)
    spec = make_spec(32, 32, CELL * 32, r_idx * CELL, [1.5] * len(r_idx), r_overlap=r_overlap)
    ref = reference_of(spec, filtered)
    assert sum(ref["per_rung"]) > 50
    check_all_paths(api, spec, filtered, ref, f"overlap {r_overlap}")


def test_selection_sphere_wraps_past_itself(api):
    """(d) 16^3, one rung of 0.6 * dim cells: the sphere and the overlap range cover the box more than once"""
    shape = (16, 16, 16)
    filtered = ladder_fields(shape, [2.0], 3)
    spec = make_spec(16, 16, CELL * 16, [0.6 * 16 * CELL], [2.2])
    ref = reference_of(spec, filtered)
    assert ref["over"][0] > 10 and ref["per_rung"][0] >= 1 and not ref["in_halo"].all()
    check_all_paths(api, spec, filtered, ref, "wrap")


def test_selection_dexm_optimize(api):
    """(e) DEXM_OPTIMIZE with DEXM_OPTIMIZE_MINMASS in the middle of the ladder: the upper rungs test and paint
    `forbidden`, rebuilt per rung from the halos found so far; the lower rungs test in_halo"""
    shape = (32, 32, 32)
    r_idx = R_IDX_LADDER[4::2]
    filtered = ladder_fields(shape, r_idx, 13)
    R = (r_idx * CELL).astype(np.float32)
    minmass = RTOM * float(R[len(R) // 2]) ** 3 * 0.999  # rungs 0 ... n/2 are above it
    spec = make_spec(32, 32, CELL * 32, R, [1.5] * len(R), optimize=1, minmass=minmass)
    ref = reference_of(spec, filtered)
    upper = sum(ref["per_rung"][:len(R) // 2 + 1])
    assert upper > 5 and sum(ref["per_rung"]) - upper > 20
    plain = reference_of(make_spec(32, 32, CELL * 32, R, [1.5] * len(R)), filtered)
    assert plain["per_rung"] != ref["per_rung"]  # the branch changes the catalogue
    check_all_paths(api, spec, filtered, ref, "optimize")


# ---------------------------------------------------------------- the full path
def density_field(n, seed):
    """a field with power on the scales of the ladder: white noise smoothed at one cell, plus a long mode"""
    a = smooth_field((n, n, n), 1.0, seed)
    x = np.arange(n) * 2.0 * np.pi / n
    return (a + 0.5 * np.sin(x)[:, None, None] * np.cos(2 * x)[None, None, :]).astype(np.float32)


@pytest.fixture(scope="module")
def full_case():
    cache = {}

    def get(api, n, halo_filter):
        key = (n, halo_filter)
        if key not in cache:
            density = density_field(n, 21 + n)
            box_len, growth = CELL * n, 0.2
            R = (np.array([5.0, 3.7, 2.6, 1.9, 1.3, 0.9]) * CELL).astype(np.float32)
            exact = D.filtered_f64(density, box_len, box_len, halo_filter, R, growth)
            # the yardstick: the existing filter entry against the same float64 filter
            yard = max(np.abs(api.filter_grid(density, box_len, halo_filter, float(r)).astype(np.float64) * growth - e).max()
                       for r, e in zip(R, exact))
            crit = [1.9 * e.std() for e in exact]
            cache[key] = (density, R, exact, yard, crit, box_len, growth)
        return cache[key]
    return get


@pytest.mark.parametrize("halo_filter", [0, 1, 2])
@pytest.mark.parametrize("n", [64, 48])
def test_full_path(api, gpu_lib, full_case, n, halo_filter):
    """transforms (64^3: the native split layout, 48^3: rocFFT), thresholds, selection, catalogue"""
    assert bool(gpu_lib.c21hip_fft_is_native(n, n, n)) == (n == 64)
    density, R, exact, yard, crit, box_len, growth = full_case(api, n, halo_filter)
    spec = make_spec(n, n, box_len, R, crit, mode=2, halo_filter=halo_filter, growth=growth)
    filtered = np.zeros((len(R), n ** 3), np.float32)
    got = run(api, spec, filtered=filtered, density=density)
    err = np.abs(filtered.astype(np.float64) - exact.reshape(len(R), -1)).max()
    print(f"n {n} filter {halo_filter}: |filtered - float64| max {err:.3e}, c21cm_filter_grid's {yard:.3e}, "
          f"halos {got['n']}, candidates {list(got['rep'].candidates[:len(R)])}")
    assert err <= 4.0 * yard
    ref = reference_of(spec, filtered)
    assert sum(ref["per_rung"]) > 20 and np.count_nonzero(ref["per_rung"]) >= 3
    assert_selection_equal(got, ref, "full")
    # the same from device arrays, and from the returned fields through filtered_mode 1
    dev = run(api, spec, filtered=np.zeros_like(filtered), density=density, device=True)
    assert same_bytes(dev, got) and np.array_equal(dev["filtered"], filtered)
    spec.filtered_mode = 1
    assert same_bytes(run(api, spec, filtered=filtered), got)


@pytest.mark.parametrize("n,hii", [(64, 64), (64, 32), (48, 16)])
def test_overlap_box(api, full_case, n, hii):
    """HII_DIM = DIM (no smoothing), DIM / 2 and DIM / 3 against the float64 restatement on the returned mask.
    Bound: four times the error of c21cm_filter_grid smoothing the same 0 / 1 mask at the same radius against
    the same float64 filter (where the grids are equal nothing is filtered and that error is zero: then the
    rounding of the two float32 transforms themselves, see below)."""
    density, R, exact, yard, crit, box_len, growth = full_case(api, n, 0)
    spec = make_spec(n, n, box_len, R, crit, mode=0, growth=growth, hii=hii, hii_z=hii)
    got = run(api, spec, density=density, overlap_shape=(hii, hii, hii))
    mask = got["in_halo"].reshape(n, n, n)
    assert 0.01 < mask.mean() < 0.9
    want = D.overlap_f64(mask, box_len, box_len, hii, hii)
    if n != hii:
        R_lo = np.float32(D.L_FACTOR * box_len / hii)
        smooth = api.filter_grid(mask.astype(np.float32), box_len, 0, float(R_lo)).astype(np.float64)
        exact_smooth = np.fft.irfftn(D.WR.filtered_spectrum(mask.astype(np.float64), box_len, box_len, 0, float(R_lo)),
                                     s=mask.shape, axes=(0, 1, 2))
        bound = 4.0 * np.abs(smooth - exact_smooth).max()
    else:  # two float32 transforms of N points: log2(N) butterfly stages each, one rounding of values <= 1 per stage
        bound = 2 * np.log2(float(n) ** 3) * np.finfo(np.float32).eps
    err = np.abs(got["overlap"].astype(np.float64) - want).max()
    print(f"n {n} hii {hii}: overlap error {err:.3e}, bound {bound:.3e}, mean {got['overlap'].mean():.4f}")
    assert got["overlap"].min() >= 0.0 and got["overlap"].max() <= 1.0
    assert err <= bound
    assert abs(got["overlap"].mean() - mask.mean()) < 0.05
    dev = run(api, spec, density=density, overlap_shape=(hii, hii, hii), device=True)
    assert np.array_equal(dev["overlap"], got["overlap"]) and same_bytes(dev, got)


def test_deviates(api):
    """one Philox block per halo, purpose 8, counter the hi-res cell: equal to the numpy restatement (cos, sin
    and log of two maths libraries may differ in the last float64 bit, which moves a float32 by at most one
    unit in the last place), and standard normal: over n halos the mean within 5 / sqrt(n) and the variance
    within 5 sqrt(2 / n) of 1, the sampling errors of n independent normals"""
    shape = (32, 32, 32)
    n = 32 ** 3
    filtered = np.ones((1, n), np.float32)
    # a radius below one cell and no overlap test: every cell becomes a halo
    spec = make_spec(32, 32, CELL * 32, [0.6 * CELL], [0.5], r_overlap=0.0, seed=2 ** 40 + 17, redshift=9.25)
    ref = reference_of(spec, filtered)
    got = run(api, spec, filtered=filtered)
    assert got["n"] == n >= 2000
    assert_selection_equal(got, ref, "all cells")
    for f in ("star_rng", "sfr_rng", "xray_rng"):
        g, w = got["cat"][f], ref["cat"][f]
        assert np.abs(g - w).max() <= np.spacing(np.abs(w).max()), f
        assert np.mean(g != w) < 1e-3, f
        assert abs(g.mean()) < 5.0 / np.sqrt(n), f
        assert abs(g.astype(np.float64).var() - 1.0) < 5.0 * np.sqrt(2.0 / n), f
    c = np.corrcoef([got["cat"][f] for f in ("star_rng", "sfr_rng", "xray_rng")])
    assert np.abs(c - np.eye(3)).max() < 5.0 / np.sqrt(n)
    other = run(api, make_spec(32, 32, CELL * 32, [0.6 * CELL], [0.5], r_overlap=0.0, seed=2 ** 40 + 18, redshift=9.25),
                filtered=filtered)
    assert not np.array_equal(other["cat"]["star_rng"], got["cat"]["star_rng"])


def test_refusals(api):
    n = 16 ** 3
    filtered = np.ones((1, n), np.float32)
    spec = make_spec(16, 16, 32.0, [0.6 * CELL], [0.5], r_overlap=0.0)
    with pytest.raises(ValueError, match="filtered"):
        api.find_halos(spec, None, S.empty_halo_catalog(n), filtered=filtered[:, :-1].copy())
    spec.filtered_mode = 0
    with pytest.raises(BackendError, match="hires_density"):
        api.find_halos(spec, None, S.empty_halo_catalog(n))
    spec.filtered_mode, spec.path = 1, 3
    with pytest.raises(BackendError, match="path"):
        api.find_halos(spec, None, S.empty_halo_catalog(n), filtered=filtered)


# ---------------------------------------------------------------- ComputeHaloCatalog
Z_ABI = 7.0


def broadcast(lib, source, hii=16, dim=64, box=64.0, **matter):
    keep = dict(so=S.default_simulation_options(HII_DIM=hii, DIM=dim, BOX_LEN=box, SAMPLER_MIN_MASS=5e8),
                mo=S.default_matter_options(SOURCE_MODEL=source, **matter), cp=S.default_cosmo_params(),
                ap=S.default_astro_params(), ao=S.default_astro_options(), ct=S.default_cosmo_tables())
    lib.Broadcast_struct_global_all(*[C.byref(keep[k]) for k in ("so", "mo", "cp", "ap", "ao", "ct")])
    lib.init_ps()
    lib._keep_dexm = keep
    return keep


def compute_halo_catalog(lib, z_desc, z, ics, seed, desc, out):
    lib.ComputeHaloCatalog.restype = C.c_int
    lib.ComputeHaloCatalog.argtypes = [C.c_float, C.c_float, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_void_p]
    return lib.ComputeHaloCatalog(z_desc, z, C.byref(ics) if ics is not None else None, seed,
                                  C.byref(desc) if desc is not None else None, C.byref(out))


def error_text(lib):
    lib.c21hip_get_error.restype = C.c_char_p
    return lib.c21hip_get_error().decode()


def abi_fields(seed=4):
    """a z = 0 hi-res field strong enough for DexM halos at z = 7, and any low-res field"""
    hires = (density_field(64, seed) * 6.0).astype(np.float32)
    lowres = (np.random.default_rng(8).standard_normal((16, 16, 16)) * 2.0).astype(np.float32)
    return hires, lowres


def ics_of(hires, lowres, device=None):
    ics = S.InitialConditionsStruct()
    if device:
        import torch

        keep = [torch.from_numpy(a).to(device) for a in (hires, lowres)]
        ics.hires_density = C.cast(keep[0].data_ptr(), S.c_float_p)
        ics.lowres_density = C.cast(keep[1].data_ptr(), S.c_float_p)
    else:
        keep = [hires, lowres]
        ics.hires_density = hires.ctypes.data_as(S.c_float_p)
        ics.lowres_density = lowres.ctypes.data_as(S.c_float_p)
    ics._keep = keep
    return ics


def rows_of(cat, device=False):
    n = cat.n_halos
    return {f: (cat.arrays[f].cpu().numpy() if device else cat.arrays[f])[:n].copy() for f in FIELDS}


def same_rows(a, b):
    return all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)) for f in FIELDS)


def test_abi_dexm_esf(gpu_lib, api):
    """SOURCE_MODEL = DEXM-ESF: ComputeHaloCatalog is the ladder plus the grid entry, byte for byte; numpy and
    device arrays agree; one row short is a ValueError with nothing written"""
    lib = gpu_lib
    broadcast(lib, 3, HALO_FILTER=0)
    hires, lowres = abi_fields()
    spec = api.dexm_spec(Z_ABI, seed=5)
    assert spec.n_R > 0 and spec.hii_dim == 0 and spec.dim == 64
    direct = S.empty_halo_catalog(200000)
    api.find_halos(spec, hires, direct)
    n = direct.n_halos
    rep = api.find_halos_report()
    assert n == sum(rep.accepted[:rep.n_R]) > 50 and np.count_nonzero(rep.accepted[:rep.n_R]) >= 3
    out = S.empty_halo_catalog(200000)
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres), 5, None, out) == 0, error_text(lib)
    assert out.n_halos == n and same_rows(rows_of(out), rows_of(direct))
    out_d = S.empty_halo_catalog(200000, device="cuda:0")
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres, "cuda:0"), 5, None, out_d) == 0, error_text(lib)
    assert out_d.n_halos == n and same_rows(rows_of(out_d, True), rows_of(direct))
    short = S.empty_halo_catalog(n - 1)
    for f in FIELDS:
        short.arrays[f][...] = -7.25
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres), 5, None, short) == 3
    assert "HALO_CATALOG_MEM_FACTOR" in error_text(lib) and f"{n} halos" in error_text(lib)
    for f in FIELDS:
        assert (short.arrays[f] == np.float32(-7.25)).all(), f
    # without the hi-res field the refusal names the finder
    assert compute_halo_catalog(lib, -1.0, Z_ABI, None, 5, None, out) == 3 and "DexM halo finder" in error_text(lib)


def test_abi_chmf_sampler_with_dexm_halos(gpu_lib, api):
    """SOURCE_MODEL = CHMF-SAMPLER at a redshift whose ladder is not empty: the finder into a catalogue of
    large halos, the overlap box, then the sampler with both -- the same bytes as the three grid-level calls"""
    lib = gpu_lib
    broadcast(lib, 4)
    hires, lowres = abi_fields()
    lib.c21cm_dexm_is_empty.argtypes = [C.c_double]
    assert not lib.c21cm_dexm_is_empty(Z_ABI)
    spec = api.dexm_spec(Z_ABI, seed=5)
    assert spec.n_R > 0 and (spec.hii_dim, spec.hii_dim_z) == (16, 16)
    found = S.empty_halo_catalog(200000)
    overlap = np.zeros((16, 16, 16), np.float32)
    api.find_halos(spec, hires, found, overlap=overlap)
    n_large = found.n_halos
    assert n_large > 5 and overlap.max() > 0.0
    large = {f: found.arrays[f][:n_large] for f in FIELDS}
    direct = S.empty_halo_catalog(400000)
    api.sample_halos(api.sampler_spec(Z_ABI, -1.0, seed=5), direct, density=lowres, overlap=overlap, large=large)
    n = direct.n_halos
    assert n > n_large
    out = S.empty_halo_catalog(400000)
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres), 5, None, out) == 0, error_text(lib)
    assert out.n_halos == n and same_rows(rows_of(out), rows_of(direct))
    assert same_rows({f: out.arrays[f][:n_large] for f in FIELDS}, large)  # the large halos come first
    out_d = S.empty_halo_catalog(400000, device="cuda:0")
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres, "cuda:0"), 5, None, out_d) == 0, error_text(lib)
    assert out_d.n_halos == n and same_rows(rows_of(out_d, True), rows_of(direct))
    short = S.empty_halo_catalog(n - 1)
    for f in FIELDS:
        short.arrays[f][...] = -7.25
    assert compute_halo_catalog(lib, -1.0, Z_ABI, ics_of(hires, lowres), 5, None, short) == 3
    assert "HALO_CATALOG_MEM_FACTOR" in error_text(lib) and f"{n} halos" in error_text(lib)
    for f in FIELDS:
        assert (short.arrays[f] == np.float32(-7.25)).all(), f
    # the low-res field alone: refused with the finder's name; an empty ladder needs no hi-res field
    only_low = S.InitialConditionsStruct()
    only_low.lowres_density = lowres.ctypes.data_as(S.c_float_p)
    assert compute_halo_catalog(lib, -1.0, Z_ABI, only_low, 5, None, out) == 3 and "DexM halo finder" in error_text(lib)
    assert lib.c21cm_dexm_is_empty(14.0)
    assert compute_halo_catalog(lib, -1.0, 14.0, only_low, 5, None, out) == 0, error_text(lib)


# ---------------------------------------------------------------- the drivers
def driver_case(monkeypatch):
    """HII_DIM 32 / DIM 64 with 1.5 Mpc low-res cells at z = 6, where the mass function expects about 60 halos
    above the cell mass of 1.3e11 Msun; three snapshots"""
    from pathlib import Path

    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    drivers = importlib.import_module("21cmfast_amd.drivers")
    data = Path(__file__).parent / "golden" / "reference" / "_data"
    common = dict(HII_DIM=32, DIM=64, BOX_LEN=48.0, N_THREADS=8, ZPRIME_STEP_FACTOR=1.15, Z_HEAT_MAX=8.0,
                  USE_LYA_HEATING=False, USE_TS_FLUCT=True, R_BUBBLE_MAX=20.0, PERTURB_ON_HIGH_RES=False)
    inputs = drivers.Inputs(random_seed=5, SOURCE_MODEL=4, SAMPLER_MIN_MASS=1e10, **common)
    all_z, nodes = drivers.required_redshifts(inputs, [6.0])
    assert len(all_z) == 3
    return drivers, data, inputs, all_z, nodes


def test_run_coeval_samples_its_own_catalogues(gpu_lib, api, monkeypatch):
    """halo_catalogs="sample" is evolve_halos followed by the usual loop, bit for bit; the lowest snapshot has
    DexM halos; halo_catalogs=None still raises"""
    drivers, data, inputs, all_z, nodes = driver_case(monkeypatch)
    z = 6.0
    keep = ("neutral_fraction", "n_ion", "halo_sfr", "brightness_temp")
    sampled = drivers.run_coeval(inputs, [z], data_path=data, device="cuda", lib=gpu_lib, keep=keep,
                                 halo_catalogs="sample")
    ics = sampled["initial_conditions"]
    cats = drivers.evolve_halos(inputs, all_z, ics, nodes=nodes, lib=gpu_lib, device="cuda", data_path=data)
    assert sorted(cats) == sorted(all_z) and all(c.n_halos > 0 for c in cats.values())
    lowest = drivers.determine_halo_catalog(inputs, min(all_z), ics, lib=gpu_lib, device="cuda", data_path=data)
    rep = api.find_halos_report()  # of the finder call just made: the snapshot without descendants
    print("DexM halos per rung at z =", min(all_z), list(rep.accepted[:rep.n_R]), "rounds", list(rep.rounds[:rep.n_R]))
    assert rep.n_R > 0 and cats[min(all_z)].n_halos == lowest.n_halos > rep.n_halos > 0  # DexM halos, then sampled ones
    listed = drivers.run_coeval(inputs, [z], data_path=data, device="cuda", lib=gpu_lib, keep=keep,
                                halo_catalogs=cats.__getitem__)
    for k in keep:
        a, b = sampled[z][k].cpu().numpy(), listed[z][k].cpu().numpy()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert sampled[z]["n_ion"].sum() > 0
    one = drivers.determine_halo_catalog(inputs, max(all_z), ics, descendant_halos=cats[sorted(all_z)[1]], lib=gpu_lib,
                                         device="cuda", data_path=data)
    assert one.n_halos == cats[max(all_z)].n_halos
    with pytest.raises(NotImplementedError, match="halo_catalogs"):
        drivers.run_coeval(inputs, [z], data_path=data, device="cuda", lib=gpu_lib)
    with pytest.raises(ValueError, match="sample"):
        drivers.run_coeval(inputs, [z], data_path=data, device="cuda", lib=gpu_lib, halo_catalogs="find")


def test_run_lightcone_samples_its_own_catalogues(gpu_lib, api, monkeypatch):
    """a lightcone over the same three redshifts, where every node is the descendant of the next one up:
    halo_catalogs="sample" against the catalogues of evolve_halos on the same initial conditions, bit for bit"""
    drivers, data, inputs, all_z, _ = driver_case(monkeypatch)
    lc_nodes = sorted(all_z, reverse=True)
    lc = drivers.RectilinearLightconer.between_redshifts(lc_nodes[-1] + 0.1, lc_nodes[0] - 0.1, 48.0 / 32,
                                                         quantities=("brightness_temp", "neutral_fraction"))
    drivers._initialise(gpu_lib, inputs, data)
    so, mo = inputs.simulation_options, inputs.matter_options
    ics = api.new_ics_arrays(S.IcsSpec(dim=so.DIM, dim_z=so.DIM, hii_dim=so.HII_DIM, hii_dim_z=so.HII_DIM,
                                       perturb_algorithm=mo.PERTURB_ALGORITHM,
                                       perturb_on_high_res=int(mo.PERTURB_ON_HIGH_RES)), device="cuda")
    icss = api.ics_struct(ics)
    assert gpu_lib.ComputeInitialConditions(inputs.random_seed, C.byref(icss)) == 0, error_text(gpu_lib)
    chain = drivers.evolve_halos(inputs, lc_nodes, ics, lib=gpu_lib, device="cuda", data_path=data)
    assert all(chain[zz].n_halos > 0 for zz in lc_nodes)
    cones = [drivers.run_lightcone(inputs, lc, lc_nodes, data_path=data, device="cuda", lib=gpu_lib, halo_catalogs=h)
             for h in ("sample", chain.__getitem__)]
    for k in ("brightness_temp", "neutral_fraction"):
        a, b = (c["lightcones"][k].cpu().numpy() for c in cones)
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
