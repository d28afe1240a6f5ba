"""ComputePerturbedHaloCatalog on the device: the catalogue moved to its Eulerian positions and converted
to galaxy properties (reference: PerturbedHaloCatalog.c:25-149, HaloBox.c:781-880), through the
grid-level entry, the ABI entry and the drivers.

Comparators: tests/halo_perturb_reference.py (numpy fp64, written from the reference's C) for the
coordinates and the turnover lookup, and the exported test_halo_props -- pinned to the reference's
known-answer test by tests/test_gpu_halobox_catalogue.py -- for the scaling relations.

Tolerances.
* Coordinates: both sides do the same fp64 operations (the library is built without fused
  multiply-adds), so float32 of the restatement, at most 1 float32 ulp; 0 against the box length only
  where the fp64 value is within one fp64 ulp of a face.
* Properties against the restatement: the kernel evaluates the power laws as exp(index * ln x) on shared
  logarithms, numpy as pow(): both are a few fp64 roundings of arguments below ~50 (|M_turn / M|,
  |ln M|), i.e. <= 50 * 2^-52 * O(10) ~ 1e-13 relative, far below the float32 store; two fp64 values
  that close round to the same float or to neighbours: PROP_RTOL = 2 float32 ulp = 2 * 2^-23.
* Properties against test_halo_props: see HALO_PROPS_RTOL below.
"""

import ctypes as C
import importlib

import numpy as np
import pytest

import halo_perturb_reference as R
from halo_catalogue_helpers import halo_consts

pytestmark = pytest.mark.gpu
S = importlib.import_module("21cmfast_amd.structs")
D = importlib.import_module("21cmfast_amd.drivers")

PROP_RTOL = 2 * 2.0 ** -23
# Against test_halo_props.  Without mini-halos both kernels call the same device function on the same
# fp64 inputs, so the floats should be bit-identical; the tolerance is the smallest step there is, 1 float32
# ulp.  With mini-halos test_halo_props takes the turnover masses of the halo's cell in fp64 while the
# catalogue reads 10^(CIC of the FLOAT log10 grids): on uniform feedback grids the two turnover masses
# differ by the float rounding of log10 M_turn, d = ln(10) |log10 M_turn| 2^-24 (1.4e-6 at 1e10 Msun).
# M* carries exp(-M_turn / M), so its relative change is d M_turn / M per population; the SFR adds the
# change of its scatter, sigma_sfr_idx / ln(10) (|r| + sigma) d' < 0.3 d' for |r| < 5, L_X a power < 1 of
# the metallicity term on top: below 3 d (1 + (M_turn,a + M_turn,m) / M) for every array, plus the two
# float stores.  The bound is evaluated per halo from the turnover masses test_halo_props reports.
HALO_PROPS_RTOL_NOMINI = 2.0 ** -23


def mini_bound(masses, mturn_a, mturn_m):
    d = np.log(10.0) * np.maximum(np.abs(np.log10(mturn_a)), np.abs(np.log10(mturn_m))) * 2.0 ** -24
    return 2.0 ** -22 + 3.0 * d * (1.0 + (mturn_a + mturn_m) / masses)


PROPS = ("halo_masses", "stellar_masses", "sfr", "ion_emissivity", "xray_emissivity", "fesc_sfr",
         "stellar_mini", "sfr_mini")
SENTINEL = np.float32(-7.25)


@pytest.fixture()
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def geometry(hii, dim, ncf, hires):
    hii_z, dim_z = int(ncf * hii), int(ncf * dim)
    box = 1.25 * dim  # > DIM Mpc: coordinate * HII_DIM / DIM reaches the last cell, where the CIC read wraps
    vel_dim = (dim, dim, dim_z) if hires else (hii, hii, hii_z)
    return dict(hii=hii, dim=dim, hii_z=hii_z, dim_z=dim_z, box=box, box_z=box * ncf, vel_dim=vel_dim,
                hires=hires)


VDF, VDF2 = 0.0712, -0.0031  # D - D_i and the 2LPT analogue at z ~ 8


def make_case(g, n, lpt2, seed, cut=True):
    """Seeded velocity grids and catalogue with the edge cases: halos at 0, just below the box length
    on each axis, on the boundaries between nearest cells and between cells, halos carried across either
    face (once by more than a box length), masses set to 0."""
    rng = np.random.default_rng(seed)
    box3 = np.array([g["box"], g["box"], g["box_z"]])
    pre = "hires_" if g["hires"] else "lowres_"
    ics = {pre + k: (rng.standard_normal(g["vel_dim"]) * 12.0).astype(np.float32) for k in ("vx", "vy", "vz")}
    if lpt2:
        ics.update({pre + k + "_2LPT": (rng.standard_normal(g["vel_dim"]) * 30.0).astype(np.float32)
                    for k in ("vx", "vy", "vz")})
    coords = (rng.random((n, 3)) * box3).astype(np.float32)
    masses = (10.0 ** rng.uniform(8.0, 13.0, n)).astype(np.float32)
    cell = g["box"] / g["vel_dim"][0]
    below = [np.nextafter(np.float32(b), np.float32(0)) for b in box3]
    special = [[0, 0, 0], [below[0], 1.0, 2.0], [1.0, below[1], 2.0], [1.0, 2.0, below[2]],
               [2.5 * cell, 3.5 * cell, 0.5 * cell], [3 * cell, 4 * cell, 1 * cell],
               [0.01, 5.0, 5.0], [5.0, below[1], 5.0], [5.0, 5.0, 0.02], [below[0], below[1], below[2]],
               [7.0, 7.0, 7.0]]
    k = min(n, len(special))
    coords[:k] = np.array(special[:k], np.float32)
    if cut and n > 20:
        masses[rng.random(n) < 0.05] = 0.0
        masses[[0, 6]] = 0.0  # cut halos get coordinates too
    # displacements across the faces: set the velocity of those halos' cells
    idx = lambda p: tuple(int(np.trunc(np.float64(p[a]) * g["vel_dim"][0] / g["box"] + 0.5)) % g["vel_dim"][a]
                          for a in range(3))  # noqa: E731
    push = {6: (0, -3.0), 7: (1, +2.0), 8: (2, -(box3[2] + 4.0)), 9: (0, +1.0), 10: (1, 2 * box3[1] + 3.0)}
    for j, (axis, shift) in push.items():
        if j < n:
            ics[pre + "v" + "xyz"[axis]][idx(coords[j])] = np.float32(shift / VDF)
    cat = dict(masses=masses, coords=coords, star_rng=rng.standard_normal(n).astype(np.float32),
               sfr_rng=rng.standard_normal(n).astype(np.float32),
               xray_rng=rng.standard_normal(n).astype(np.float32))
    return ics, cat


def spec_of(g, lpt2):
    return S.PerturbHalosSpec(dim=g["dim"], dim_z=g["dim_z"], hii_dim=g["hii"], hii_dim_z=g["hii_z"],
                              box_len=g["box"], box_len_z=g["box_z"], perturb_on_high_res=int(g["hires"]),
                              lpt2=int(lpt2), velocity_displacement_factor=VDF,
                              velocity_displacement_factor_2lpt=VDF2)


def out_struct(n_rows, fields, fill=SENTINEL):
    """A PerturbedHaloCatalog over numpy arrays filled with a sentinel; only ``fields`` are non-NULL."""
    out = S.PerturbedHaloCatalogStruct(n_halos=12345, buffer_size=n_rows)
    out.arrays = {}
    for f in fields:
        a = np.full((n_rows, 3) if f == "halo_coords" else (n_rows,), fill, np.float32)
        out.arrays[f] = a
        setattr(out, f, a.ctypes.data_as(S.c_float_p))
    return out


def reference(g, ics, cat, lpt2, consts, mta=None, mtm=None):
    pre = "hires_" if g["hires"] else "lowres_"
    vel = [ics[pre + k] for k in ("vx", "vy", "vz")]
    vel2 = [ics[pre + k + "_2LPT"] for k in ("vx", "vy", "vz")] if lpt2 else None
    return R.perturbed_halo_catalog(cat, vel, vel2, g["vel_dim"], (g["box"], g["box"], g["box_z"]), VDF, VDF2,
                                    consts, g["hii"], g["dim"], mta, mtm)


def check_coords(got, ref, box3):
    """<= 1 float32 ulp at the value; 0 against the box length only within one fp64 ulp of a face.
    Returns the fraction of bit-identical coordinates."""
    want, p64 = ref["halo_coords"], ref["pos64"]
    assert got.shape == want.shape
    box = np.broadcast_to(np.asarray(box3, np.float64), p64.shape)
    face = ((got == 0) & (want == box.astype(np.float32))) | ((want == 0) & (got == box.astype(np.float32)))
    near = (np.abs(p64 - box) <= np.spacing(box)) | (np.abs(p64) <= np.spacing(box))
    assert not (face & ~near).any()
    ulp = np.spacing(np.abs(want).astype(np.float32))
    bad = ~face & ~(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])
    assert (got >= 0).all() and (got <= box.astype(np.float32)).all()
    return float(np.mean(got == want))


GRIDS = [(12, 36, 1.0), (12, 36, 1.5), (16, 32, 1.0), (16, 32, 1.5)]


@pytest.mark.parametrize("hii,dim,ncf", GRIDS)
@pytest.mark.parametrize("hires", [False, True])
@pytest.mark.parametrize("lpt2", [False, True])
def test_coordinates_match_the_fp64_restatement(api, hii, dim, ncf, hires, lpt2):
    g = geometry(hii, dim, ncf, hires)
    n = 4099
    ics, cat = make_case(g, n, lpt2, seed=hii + 7 * hires + 3 * lpt2)
    consts = halo_consts(use_xray=0)
    hc = S.halo_catalog(cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
    out = out_struct(n, ("halo_coords", "halo_masses", "stellar_masses", "sfr", "ion_emissivity"))
    api.perturb_halos_grids(spec_of(g, lpt2), consts, ics, hc, out)
    assert out.n_halos == n
    ref = reference(g, ics, cat, lpt2, consts)
    box3 = (g["box"], g["box"], g["box_z"])
    same = check_coords(out.arrays["halo_coords"], ref, box3)
    print(f"bit-identical coordinates: {same:.6f} ({hii}/{dim} x{ncf} hires={hires} 2lpt={lpt2})")
    # the case really crosses both faces, once by more than a box length, and cuts halos
    moved = ref["halo_coords"][:11].astype(np.float64) - cat["coords"][:11].astype(np.float64)
    assert moved[6, 0] > 0.5 * box3[0] and moved[7, 1] < -0.5 * box3[1]  # wrapped across the lower / upper face
    pre = "hires_" if hires else "lowres_"
    cell8 = tuple(int(np.trunc(cat["coords"][8, a] * g["vel_dim"][0] / g["box"] + 0.5)) % g["vel_dim"][a] for a in range(3))
    assert abs(float(ics[pre + "vz"][cell8]) * VDF) > box3[2]
    assert (cat["masses"] == 0).sum() > 100 and cat["masses"][0] == 0
    live = ref["live"]
    assert (out.arrays["halo_masses"][~live] == SENTINEL).all()  # cut halos: coordinates only
    np.testing.assert_array_equal(out.arrays["halo_masses"][live], cat["masses"][live])


@pytest.mark.parametrize("n,rows", [(0, 0), (0, 5), (1, 1), (63, 63), (63, 100), (4099, 4099)])
def test_halo_counts_and_buffer_size(api, n, rows):
    g = geometry(16, 32, 1.0, False)
    ics, cat = make_case(g, max(n, 1), True, seed=n + 1, cut=False)
    cat = {k: v[:n] for k, v in cat.items()}
    consts = halo_consts(use_xray=1)
    hc = S.halo_catalog(cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
    fields = ("halo_coords", "halo_masses", "stellar_masses", "sfr", "ion_emissivity", "xray_emissivity")
    out = out_struct(max(rows, 1), fields)
    out.buffer_size = rows
    api.perturb_halos_grids(spec_of(g, True), consts, ics, hc, out)
    assert out.n_halos == n
    for f in fields:  # nothing beyond row n is touched
        assert (out.arrays[f][n:] == SENTINEL).all(), f
    if n:
        ref = reference(g, ics, cat, True, consts)
        check_coords(out.arrays["halo_coords"][:n], ref, (g["box"], g["box"], g["box_z"]))
        np.testing.assert_allclose(out.arrays["sfr"][:n], ref["sfr"], rtol=PROP_RTOL)
        np.testing.assert_allclose(out.arrays["xray_emissivity"][:n], ref["xray_emissivity"], rtol=PROP_RTOL)


def turnover_grids(g, kind, seed):
    rng = np.random.default_rng(seed)
    shape = (g["hii"], g["hii"], g["hii_z"])
    if kind == "smooth":
        x, y, z = np.meshgrid(*[np.arange(s) / s for s in shape], indexing="ij")
        a = 8.7 + 0.4 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0.2 * np.sin(4 * np.pi * z)
        m = 6.5 + 0.8 * np.cos(2 * np.pi * (x + y)) + 0.3 * np.sin(2 * np.pi * z)
    else:  # rough: independent cells over the whole table range
        a, m = rng.uniform(8.0, 10.0, shape), rng.uniform(5.0, 9.5, shape)
    return a.astype(np.float32), m.astype(np.float32)


@pytest.mark.parametrize("hii,dim,ncf,hires,lpt2", [(12, 36, 1.5, False, True), (16, 32, 1.0, True, False),
                                                     (16, 32, 1.5, False, False)])
@pytest.mark.parametrize("mini,kind", [(0, None), (1, "smooth"), (1, "rough")])
@pytest.mark.parametrize("xray,recomb", [(1, 1), (0, 0)])
def test_properties_match_the_restatement(api, hii, dim, ncf, hires, lpt2, mini, kind, xray, recomb):
    """The numpy anchor: turnover lookup (CIC read of the log10 grids at coordinate * HII_DIM / DIM,
    wrapping in the last cell of each axis) and the relations; cut halos keep a sentinel; arrays that the
    options switch off are untouched (given) or NULL (not given)."""
    import torch

    g = geometry(hii, dim, ncf, hires)
    n = 4099
    ics, cat = make_case(g, n, lpt2, seed=50 + hii + mini)
    consts = halo_consts(z=9.0, use_xray=xray, use_mini_halos=mini, scaling_median=int(recomb == 0))
    mta, mtm = turnover_grids(g, kind, 3) if mini else (None, None)
    hc = S.halo_catalog(cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
    # with recomb: every array given (the switched-off ones must stay untouched); without: they are NULL
    fields = ("halo_coords",) + PROPS if recomb else (
        ("halo_coords", "halo_masses", "stellar_masses", "sfr", "ion_emissivity")
        + (("xray_emissivity",) if xray else ()) + (("stellar_mini", "sfr_mini") if mini else ()))
    out = out_struct(n, fields)
    api.perturb_halos_grids(spec_of(g, lpt2), consts, ics, hc, out, mta, mtm)
    ref = reference(g, ics, cat, lpt2, consts, mta, mtm)
    live = ref["live"]
    check_coords(out.arrays["halo_coords"], ref, (g["box"], g["box"], g["box_z"]))
    written = ["halo_masses", "stellar_masses", "sfr", "ion_emissivity"] + (["xray_emissivity"] if xray else []) \
        + (["fesc_sfr"] if recomb else []) + (["stellar_mini", "sfr_mini"] if mini else [])
    for f in fields[1:]:
        a = out.arrays[f]
        if f not in written:
            assert (a == SENTINEL).all(), f  # switched off: untouched
            continue
        assert (a[~live] == SENTINEL).all(), f
        want = ref[f]
        # values below float32's normal range are stored as denormals or 0: absolute slack of one denormal step
        np.testing.assert_allclose(a[live], want, rtol=PROP_RTOL, atol=1.5e-45, err_msg=f)
        assert np.isfinite(a[live]).all() and (want > 0).any(), f
    if mini:  # the lookup reaches the last cell of every axis, where the CIC read wraps
        hp = ref["halo_coords"][live].astype(np.float64) * (hii / dim)
        for a, size in enumerate((g["hii"], g["hii"], g["hii_z"])):
            assert ((np.floor(hp[:, a]) % size) == size - 1).sum() > 10, a
        assert np.ptp(np.log10(ref["mturn"][1])) > (0.5 if kind == "smooth" else 2.0)
    # device-resident inputs and outputs: the same numbers
    t = lambda a: None if a is None else torch.from_numpy(a).cuda()  # noqa: E731
    dp = lambda x: C.cast(x.data_ptr(), S.c_float_p)  # noqa: E731
    dcat = {k: t(v) for k, v in cat.items()}
    hcd = S.HaloCatalogStruct(n_halos=n, buffer_size=n, halo_masses=dp(dcat["masses"]),
                              halo_coords=dp(dcat["coords"]), star_rng=dp(dcat["star_rng"]),
                              sfr_rng=dp(dcat["sfr_rng"]), xray_rng=dp(dcat["xray_rng"]))
    dout = {f: torch.full(out.arrays[f].shape, float(SENTINEL), device="cuda") for f in fields}
    outd = S.PerturbedHaloCatalogStruct(n_halos=0, buffer_size=n, **{f: dp(v) for f, v in dout.items()})
    api.perturb_halos_grids(spec_of(g, lpt2), consts, {k: t(v) for k, v in ics.items()}, hcd, outd, t(mta), t(mtm))
    torch.cuda.synchronize()
    for f in fields:
        np.testing.assert_array_equal(dout[f].cpu().numpy(), out.arrays[f], err_msg=f)


# ---- the ABI entry ------------------------------------------------------------------------------------
def bind(lib):
    lib.ComputePerturbedHaloCatalog.restype = C.c_int
    lib.ComputePerturbedHaloCatalog.argtypes = [C.c_float] + [C.c_void_p] * 5
    lib.c21cm_last_error.restype = C.c_char_p


def session_case(ses, n, seed, hires=False):
    so = ses.so
    g = dict(hii=so.HII_DIM, dim=so.DIM, hii_z=so.HII_DIM, dim_z=so.DIM, box=float(so.BOX_LEN),
             box_z=float(so.BOX_LEN), hires=hires,
             vel_dim=(so.DIM,) * 3 if hires else (so.HII_DIM,) * 3)
    ics, cat = make_case(g, n, True, seed)
    ics["lowres_vcb"] = np.full((so.HII_DIM,) * 3, 25.0, np.float32)
    return g, ics, cat


def call_abi(lib, z, ics, cat, out, prev_ts=None, prev_ion=None):
    from test_gpu_abi import fptr

    hc = cat if isinstance(cat, S.HaloCatalogStruct) else S.halo_catalog(
        cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
    icss = S.InitialConditionsStruct(**{k: fptr(v) for k, v in ics.items()})
    return lib.ComputePerturbedHaloCatalog(z, C.byref(icss), C.byref(prev_ts) if prev_ts else None,
                                           C.byref(prev_ion) if prev_ion else None, C.byref(hc), C.byref(out))


@pytest.mark.parametrize("mini,recomb,ts,z_heat_max", [
    (False, 0, True, 35.0), (False, 2, False, 35.0), (True, 2, True, 35.0), (True, 0, True, 5.0)])
def test_entry_point_against_test_halo_props(gpu_lib, tmp_path, mini, recomb, ts, z_heat_max):
    """The relations anchor: the arrays of ComputePerturbedHaloCatalog against the columns of
    test_halo_props (HaloBox.c:746-760: mass, M*, SFR, L_X, n_ion, f_esc-weighted SFR, M*_mini, SFR_mini)
    fed with the perturbed coordinates times HII_DIM / DIM.  With mini-halos the feedback grids are
    uniform, so that the cell's turnover masses and the CIC read of the grids describe the same number.
    Also: numpy and device inputs give the same arrays; switched-off arrays stay untouched."""
    import torch
    from test_gpu_abi import Session, fptr
    from test_gpu_halobox_catalogue import _bind_test_halo_props

    lib = gpu_lib
    n_grid, n = 16, 4099
    ses = Session(lib, tmp_path, HII_DIM=n_grid, DIM=32, SOURCE_MODEL=4, USE_TS_FLUCT=ts, RECOMB_MODEL=recomb,
                  USE_MINI_HALOS=mini, Z_HEAT_MAX=z_heat_max, V_CB_MODEL=3, PERTURB_ON_HIGH_RES=False)
    bind(lib)
    z = 11.0
    below = z < z_heat_max
    g, ics, cat = session_case(ses, n, seed=77)
    shape = (n_grid,) * 3
    j21, g12, zre = (np.full(shape, v, np.float32) for v in (0.3, 0.2, 13.0))
    pts = S.TsBoxStruct(J_21_LW=fptr(j21))
    pion = S.IonizedBoxStruct(ionisation_rate_G12=fptr(g12), z_reion=fptr(zre))
    out = out_struct(n, ("halo_coords",) + PROPS)
    st = call_abi(lib, z, ics, cat, out, pts if mini else None, pion if mini else None)
    assert st == 0, lib.c21cm_last_error()
    assert out.n_halos == n
    live = cat["masses"] != 0
    ptr = _bind_test_halo_props(lib)
    props = np.full((n, 12), SENTINEL, np.float32)
    scaled = (out.arrays["halo_coords"].astype(np.float64) * (n_grid / 32.0)).astype(np.float32)
    st = lib.test_halo_props(z, None, ptr(j21) if mini and below else None, ptr(zre) if mini and below else None,
                             ptr(g12) if mini and below else None, n, ptr(cat["masses"]), ptr(scaled),
                             ptr(cat["star_rng"]), ptr(cat["sfr_rng"]), ptr(cat["xray_rng"]), ptr(props))
    assert st == 0, lib.c21cm_last_error()
    cols = dict(halo_masses=0, stellar_masses=1, sfr=2, xray_emissivity=3, ion_emissivity=4, fesc_sfr=5,
                stellar_mini=6, sfr_mini=7)
    on = dict(xray_emissivity=ts, fesc_sfr=recomb != 0, stellar_mini=mini, sfr_mini=mini)
    m64 = cat["masses"][live].astype(np.float64)
    bound = (mini_bound(m64, props[live, 8].astype(np.float64), props[live, 9].astype(np.float64)) if mini
             else np.full(m64.shape, HALO_PROPS_RTOL_NOMINI))
    worst, worst_of_bound = 0.0, 0.0
    for f, col in cols.items():
        a = out.arrays[f]
        if not on.get(f, True):
            assert (a == SENTINEL).all(), f  # switched off: untouched
            continue
        assert (a[~live] == SENTINEL).all(), f
        want = props[live, col].astype(np.float64)
        err = np.abs(a[live].astype(np.float64) - want)
        big = want > 1e-30  # below: denormal floats, compared absolutely
        worst = max(worst, float((err[big] / want[big]).max(initial=0.0)))
        worst_of_bound = max(worst_of_bound, float((err[big] / (want[big] * bound[big])).max(initial=0.0)))
        bad = err > bound * want + 1.5e-45
        assert not bad.any(), (f, int(bad.sum()), a[live][bad][:4], want[bad][:4])
        assert (want > 0).any(), f
    print(f"worst relative difference from test_halo_props: {worst:.3e}, {worst_of_bound:.3f} of the bound "
          f"(mini={mini} below={below})")
    if mini and below:  # the reionisation feedback is on: the turnovers are not the no-feedback constants
        assert props[live, 10].min() > 1.0
    # device inputs: the same arrays
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dp = lambda x: C.cast(x.data_ptr(), S.c_float_p)  # noqa: E731
    dev = {k: t(v) for k, v in {**ics, **cat, "j21": j21, "g12": g12, "zre": zre}.items()}
    hcd = S.HaloCatalogStruct(n_halos=n, buffer_size=n, halo_masses=dp(dev["masses"]), halo_coords=dp(dev["coords"]),
                              star_rng=dp(dev["star_rng"]), sfr_rng=dp(dev["sfr_rng"]), xray_rng=dp(dev["xray_rng"]))
    icsd = S.InitialConditionsStruct(**{k: dp(dev[k]) for k in ics})
    dout = {f: torch.full(out.arrays[f].shape, float(SENTINEL), device="cuda") for f in out.arrays}
    outd = S.PerturbedHaloCatalogStruct(n_halos=0, buffer_size=n, **{f: dp(v) for f, v in dout.items()})
    ptsd = S.TsBoxStruct(J_21_LW=dp(dev["j21"]))
    piond = S.IonizedBoxStruct(ionisation_rate_G12=dp(dev["g12"]), z_reion=dp(dev["zre"]))
    st = lib.ComputePerturbedHaloCatalog(z, C.byref(icsd), C.byref(ptsd) if mini else None,
                                         C.byref(piond) if mini else None, C.byref(hcd), C.byref(outd))
    assert st == 0, lib.c21cm_last_error()
    torch.cuda.synchronize()
    for f in out.arrays:
        np.testing.assert_array_equal(dout[f].cpu().numpy(), out.arrays[f], err_msg=f)


def test_entry_point_agrees_with_the_grid_level_entry(gpu_lib, api, tmp_path):
    """ComputePerturbedHaloCatalog == c21cm_perturb_halos_grids fed with the library's own growth
    factors (floats upstream: the displacement factors are differences of floats) and constants."""
    from test_gpu_abi import Session
    from test_gpu_halobox_catalogue import _consts_from_library

    lib = gpu_lib
    n = 4099
    ses = Session(lib, tmp_path, HII_DIM=16, DIM=32, SOURCE_MODEL=3, USE_TS_FLUCT=True, RECOMB_MODEL=1,
                  PERTURB_ON_HIGH_RES=True)
    bind(lib)
    z = 8.5
    g, ics, cat = session_case(ses, n, seed=5, hires=True)
    out = out_struct(n, ("halo_coords",) + PROPS)
    assert call_abi(lib, z, ics, cat, out) == 0, lib.c21cm_last_error()
    f32 = np.float32
    D_z, D_i = f32(lib.dicke(float(f32(z)))), f32(lib.dicke(float(ses.so.INITIAL_REDSHIFT)))
    d2 = lambda d: f32(-(3.0 / 7.0) * np.float64(d) * np.float64(d))  # noqa: E731
    spec = spec_of(g, True)
    spec.velocity_displacement_factor = float(f32(D_z - D_i))
    spec.velocity_displacement_factor_2lpt = float(f32(d2(D_z) - d2(D_i)))
    _, consts = _consts_from_library(lib, ses, float(f32(z)))
    # OMb / OMm is a quotient of two floats upstream (scaling_relations.c:346) and in the library
    consts.baryon_ratio = float(f32(ses.cp.OMb) / f32(ses.cp.OMm))
    hc = S.halo_catalog(cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
    out2 = out_struct(n, ("halo_coords",) + PROPS)
    api.perturb_halos_grids(spec, consts, ics, hc, out2)
    for f in out.arrays:
        np.testing.assert_array_equal(out2.arrays[f], out.arrays[f], err_msg=f)
    assert (out.arrays["stellar_mini"] == SENTINEL).all() and (out.arrays["fesc_sfr"][cat["masses"] != 0] > 0).all()
    assert np.abs(out.arrays["halo_coords"] - cat["coords"]).max() > 1.0  # the halos did move


def test_refusals_return_value_error_and_leave_the_device_usable(gpu_lib, tmp_path):
    from test_gpu_abi import Session, fptr

    lib = gpu_lib
    bind(lib)
    n, z = 63, 11.0
    all_fields = ("halo_coords",) + PROPS

    def refused(ses, *, cat_edit=None, drop=None, rows=n, prev=False, match=""):
        g, ics, cat = session_case(ses, n, seed=2)
        hc = S.halo_catalog(cat["masses"], cat["coords"], cat["star_rng"], cat["sfr_rng"], cat["xray_rng"])
        if cat_edit:
            setattr(hc, cat_edit, None)
        out = out_struct(n, tuple(f for f in all_fields if f != drop))
        out.buffer_size = rows
        shape = (ses.so.HII_DIM,) * 3
        keep = [np.full(shape, v, np.float32) for v in (0.3, 0.2, 13.0)]
        pts = S.TsBoxStruct(J_21_LW=fptr(keep[0]))
        pion = S.IonizedBoxStruct(ionisation_rate_G12=fptr(keep[1]), z_reion=fptr(keep[2]))
        st = call_abi(lib, z, ics, hc, out, pts if prev else None, pion if prev else None)
        msg = (lib.c21cm_last_error() or b"").decode()
        if match is None:
            assert st == 0, msg
            return out
        assert st == 3 and match in msg, (st, msg)
        assert (out.arrays["halo_coords"] == SENTINEL).all()  # nothing was launched
        return out

    base = dict(HII_DIM=16, DIM=32, USE_TS_FLUCT=True, RECOMB_MODEL=2, V_CB_MODEL=3, PERTURB_ON_HIGH_RES=False)
    ses = Session(lib, tmp_path, SOURCE_MODEL=4, **base)
    refused(ses, cat_edit="star_rng", match="deviates")          # a NULL required input array
    refused(ses, drop="sfr", match="sfr")                        # a NULL required output array
    refused(ses, drop="xray_emissivity", match="USE_TS_FLUCT")   # an output array the options ask for
    refused(ses, rows=n - 1, match="buffer_size")                # buffer_size < n_halos
    ses = Session(lib, tmp_path, SOURCE_MODEL=4, USE_MINI_HALOS=True, Z_HEAT_MAX=35.0, **base)
    refused(ses, prev=False, match="previous")                   # previous boxes missing where they are needed
    refused(ses, prev=True, match=None)
    ses = Session(lib, tmp_path, SOURCE_MODEL=4, USE_MINI_HALOS=True, **{**base, "PERTURB_ON_HIGH_RES": True})
    refused(ses, prev=True, match="PERTURB_ON_HIGH_RES")
    ses = Session(lib, tmp_path, SOURCE_MODEL=2, **base)
    refused(ses, match="SOURCE_MODEL")
    ses = Session(lib, tmp_path, SOURCE_MODEL=4, PHOTON_CONS_TYPE=1, **base)
    refused(ses, match="PHOTON_CONS_TYPE")
    # one good call afterwards: the device is usable and the result is right
    ses = Session(lib, tmp_path, SOURCE_MODEL=4, **base)
    out = refused(ses, match=None)
    assert out.n_halos == n and np.isfinite(out.arrays["sfr"]).all() and (out.arrays["sfr"] > 0).any()
    assert (out.arrays["halo_coords"] >= 0).all() and (out.arrays["halo_coords"] <= np.float32(ses.so.BOX_LEN)).all()


# ---- drivers ------------------------------------------------------------------------------------------
def test_drivers_keep_perturbed_halos(gpu_lib, monkeypatch):
    """perturb_halo_catalog on an HII_DIM = 16 run; run_coeval(..., keep_perturbed_halos=True) returns the
    catalogue of a direct call; the default flag leaves the result keys of a run as they were."""
    from pathlib import Path

    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    data = Path(__file__).parent / "golden" / "reference" / "_data"
    common = dict(HII_DIM=16, DIM=32, BOX_LEN=32.0, N_THREADS=2, USE_TS_FLUCT=False, RECOMB_MODEL=0,
                  R_BUBBLE_MAX=10.0, PERTURB_ON_HIGH_RES=False, SOURCE_MODEL=4, SAMPLER_MIN_MASS=1e10)
    rng = np.random.default_rng(8)
    nh, z = 300, 9.0
    m0, xyz = 10.0 ** rng.uniform(10.5, 12, nh), rng.random((nh, 3)) * 32.0
    m0[::17] = 0.0
    dev = [rng.standard_normal(nh) for _ in range(3)]
    catalogue = lambda zz: S.halo_catalog(m0, xyz, *dev)  # noqa: E731
    inputs = lambda: D.Inputs(random_seed=5, **common)  # noqa: E731
    plain = D.run_coeval(inputs(), [z], data_path=data, device="cuda", lib=gpu_lib, halo_catalogs=catalogue)
    zz = float(np.float32(z))
    assert set(plain) == {zz, "history", "initial_conditions"}
    assert set(plain[zz]) == {"density", "velocity_z", "neutral_fraction", "z_reion", "brightness_temp",
                              "mean_f_coll", "Q_HI"}  # the keys of this run before the flag existed
    kept = D.run_coeval(inputs(), [z], data_path=data, device="cuda", lib=gpu_lib, halo_catalogs=catalogue,
                        keep_perturbed_halos=True)
    assert set(kept[zz]) == set(plain[zz]) | {"perturbed_halos"}
    for k in ("density", "neutral_fraction", "brightness_temp"):
        assert bool((kept[zz][k] == plain[zz][k]).all()), k
    moved = kept[zz]["perturbed_halos"]
    assert moved.n_halos == nh and moved.xray_emissivity is None and moved.stellar_mini is None
    direct = D.perturb_halo_catalog(inputs(), z, kept["initial_conditions"], catalogue(z), data_path=data,
                                    device=None, lib=gpu_lib)
    assert direct.n_halos == nh and set(direct.fields()) == set(moved.fields())
    for k, v in direct.fields().items():
        np.testing.assert_array_equal(moved.fields()[k].cpu().numpy(), v, err_msg=k)
    live = m0 != 0
    assert (direct.sfr[live] > 0).all() and (direct.sfr[~live] == 0).all()
    assert np.abs(direct.halo_coords - xyz.astype(np.float32)).max() > 0.05
    assert (direct.halo_coords >= 0).all() and (direct.halo_coords <= 32.0).all()
