"""GPU parity: ComputeInitialConditions grid algorithm vs the CPU oracle.

Both sides share the Philox + Box-Muller mode sampler (the reference's GSL streams are
unpinned, see oracle/oracle_ics.c), so sampled fields agree to float round-off; the
`density_is_input` path is RNG-free.  Tolerance: atol = 3e-5 * max|field| (15 chained
float32 FFTs and sweeps), the reference's own round-trip test uses atol 1e-5 on O(1) fields.
"""

import importlib

import numpy as np
import pytest

from cic_reference import cic_last_path, density_error, oracle_threads
from test_oracle_ics import LOWRES_FIELDS, ics_spec
from test_oracle_perturb import perturb_spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def compare(got, ref, names=None):
    for k in names or ref.keys():
        a = got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy()
        assert np.isfinite(ref[k]).all(), k  # (assert_allclose passes where both sides are NaN)
        scale = np.abs(ref[k]).max()
        np.testing.assert_allclose(a, ref[k], atol=3e-5 * scale + 1e-12, rtol=1e-4, err_msg=k)


@pytest.mark.parametrize("dim,hii_dim,device", [(24, 8, None), (32, 16, "cuda"), (64, 32, "cuda"),
                                                (128, 64, "cuda"), (20, 10, None),
                                                (192, 64, "cuda")])  # DIM = 3 HII_DIM, native 192
def test_sampled_ics_match_oracle(api, oracle, dim, hii_dim, device):
    spec = ics_spec(dim, hii_dim, box_len=3.0 * hii_dim, seed=99)
    ref = oracle.ics_grids(spec)
    got = api.ics_grids(spec, device=device)
    compare(got, ref)


@pytest.mark.parametrize("opts", [dict(algorithm=1), dict(hires=1), dict(hires=1, algorithm=1)])
def test_option_branches(api, oracle, opts):
    spec = ics_spec(32, 16, box_len=48.0, seed=5, **opts)
    compare(api.ics_grids(spec), oracle.ics_grids(spec))


@pytest.mark.parametrize("dim,hii_dim,device,opts", [
    (256, 64, "cuda", {}),                      # fold by 4
    (128, 64, None, dict(hires=1)),             # hi-res velocities, folded low-res density
    (128, 64, "cuda", dict(algorithm=1)),       # Zel'dovich only
    (128, 64, None, dict(hires=1, algorithm=1)),
    (64, 64, "cuda", {}),                       # DIM == HII_DIM: no filter, no fold
    (192, 64, "cuda", {}),                      # the reference's default DIM = 3 HII_DIM: fold by 3
    (384, 128, None, dict(hires=1)),
])
def test_split_layout_pipeline_matches_oracle(api, oracle, dim, hii_dim, device, opts):
    """The split-layout pipeline (native transform sizes): spectra in the split layout, dense
    stores from pass Z, low-resolution outputs from the folded spectrum."""
    spec = ics_spec(dim, hii_dim, box_len=1.5 * dim, seed=31, **opts)
    compare(api.ics_grids(spec, device=device), oracle.ics_grids(spec))


def test_split_and_padded_pipelines_agree(api, monkeypatch):
    """C21CM_ICS=padded selects the padded-layout pipeline (full-size transforms + gathers);
    folding is an exact identity, so the two agree to transform round-off."""
    spec = ics_spec(128, 64, box_len=192.0, seed=77)
    a = api.ics_grids(spec, device="cuda")
    monkeypatch.setenv("C21CM_ICS", "padded")
    b = api.ics_grids(spec, device="cuda")
    for k in a:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        np.testing.assert_allclose(x, y, atol=2e-5 * np.abs(y).max(), rtol=1e-4, err_msg=k)
    assert not all(np.array_equal(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in LOWRES_FIELDS)


def test_density_input_on_the_split_pipeline(api, oracle):
    dim, hii = 128, 64
    spec = ics_spec(dim, hii, box_len=192.0, seed=8)
    ic = api.ics_grids(spec)
    spec2 = ics_spec(dim, hii, box_len=192.0, density_is_input=1)
    start = api.new_ics_arrays(spec2)
    start["hires_density"][...] = ic["hires_density"]
    ic2 = api.ics_grids(spec2, start)
    for name in LOWRES_FIELDS:
        scale = max(1.0, np.abs(ic[name]).max())
        np.testing.assert_allclose(ic[name], ic2[name], atol=1e-5 * scale, rtol=0.0, err_msg=name)
    ref = oracle.new_ics_arrays(spec2)
    ref["hires_density"][...] = ic["hires_density"]
    compare(ic2, oracle.ics_grids(spec2, ref), LOWRES_FIELDS)


def test_roundtrip_from_own_density_on_device(api, oracle):
    """Reference test tests/test_initial_conditions.py:153-167 on the HIP path."""
    dim, hii = 64, 32
    spec = ics_spec(dim, hii, box_len=96.0, seed=7)
    ic = api.ics_grids(spec)
    spec2 = ics_spec(dim, hii, box_len=96.0, density_is_input=1)
    start = api.new_ics_arrays(spec2)
    start["hires_density"][...] = ic["hires_density"]
    ic2 = api.ics_grids(spec2, start)
    assert np.all(ic2["hires_density"] == ic["hires_density"])
    for name in LOWRES_FIELDS:
        scale = max(1.0, np.abs(ic[name]).max())
        np.testing.assert_allclose(ic[name], ic2[name], atol=1e-5 * scale, rtol=0.0, err_msg=name)
    # and the input path agrees with the oracle run on the same density
    ref = oracle.new_ics_arrays(spec2)
    ref["hires_density"][...] = ic["hires_density"]
    compare(ic2, oracle.ics_grids(spec2, ref), LOWRES_FIELDS)


def test_full_size_properties(api):
    """Config 2 (HII_DIM=256, DIM=512): zero-mean fields, realisation independent of launch
    geometry (same seed twice -> identical bits), different seed -> different field."""
    import torch

    spec = ics_spec(512, 256, box_len=384.0, seed=12345)
    a = api.ics_grids(spec, device="cuda")
    b = api.ics_grids(spec, device="cuda")
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert abs(a[k].double().mean().item()) < 1e-5 * max(1.0, a[k].abs().max().item()), k
    c = api.ics_grids(ics_spec(512, 256, box_len=384.0, seed=54321), device="cuda")
    assert not torch.equal(a["hires_density"], c["hires_density"])
    # sigma of the low-res density is below the hi-res one (top-hat smoothing)
    assert a["lowres_density"].std() < a["hires_density"].std()


@pytest.mark.parametrize("dim,hii_dim,device", [(32, 16, None), (64, 32, "cuda"), (30, 10, None),
                                                (48, 48, "cuda")])
def test_relative_velocities_match_oracle(api, oracle, dim, hii_dim, device):
    """V_CB_MODEL = FLUCTS: lowres_vcb = sqrt(sum_a v_a^2) / V of the top-hat-filtered, subsampled
    relative velocity components (reference: InitialConditions.c:141-238)."""
    from test_oracle_ics import vcb_table

    S = importlib.import_module("21cmfast_amd.structs")
    L = 2.0 * hii_dim
    spec = ics_spec(dim, hii_dim, box_len=L, seed=12)
    h = vcb_table(dim, L)
    spec.vcb_by_m = h.ctypes.data_as(S.c_double_p)
    lo = (hii_dim,) * 3
    ref_arrays = oracle.new_ics_arrays(spec)
    ref_arrays["lowres_vcb"] = np.zeros(lo, np.float32)
    ref = oracle.ics_grids(spec, ref_arrays)
    got_arrays = api.new_ics_arrays(spec, device)
    if device:
        import torch

        got_arrays["lowres_vcb"] = torch.zeros(lo, dtype=torch.float32, device=device)
    else:
        got_arrays["lowres_vcb"] = np.zeros(lo, np.float32)
    got = api.ics_grids(spec, got_arrays)
    compare(got, ref)
    assert ref["lowres_vcb"].min() > 0


def test_relative_velocities_through_the_entry_point(gpu_lib, api, oracle, tmp_path):
    """ComputeInitialConditions with POWER_SPECTRUM = CLASS and V_CB_MODEL = FLUCTS: the tabulated
    transfer functions of CosmoTables feed P(k) and sqrt(P_vcb / P); checked against the oracle
    driven by the library's exported power_in_k / power_in_vcb."""
    import ctypes as C
    import math

    from test_gpu_abi import Session, fptr
    from test_host_scalars import class_like_tables

    S = importlib.import_module("21cmfast_amd.structs")
    lib = gpu_lib
    n, N, L = 16, 32, 48.0
    ses = Session(lib, tmp_path, HII_DIM=n, DIM=N, BOX_LEN=L)      # EH first: shapes the table
    k, T_d, T_v = class_like_tables(lib)
    ses.mo = S.default_matter_options(POWER_SPECTRUM=5, V_CB_MODEL=2)
    ses.ct = S.class_tables(k, T_d, T_v)
    lib.Broadcast_struct_global_all(C.byref(ses.so), C.byref(ses.mo), C.byref(ses.cp),
                                    C.byref(ses.ap), C.byref(ses.ao), C.byref(ses.ct))
    lib.init_ps()
    lib.power_in_vcb.restype = C.c_double
    lib.power_in_vcb.argtypes = [C.c_double]
    spec = S.IcsSpec(dim=N, dim_z=N, hii_dim=n, hii_dim_z=n, box_len=L, box_len_z=L,
                     perturb_algorithm=2)
    ics = api.new_ics_arrays(spec)
    ics["lowres_vcb"] = np.zeros((n, n, n), np.float32)
    st = lib.ComputeInitialConditions(2026, C.byref(api.ics_struct(ics)))
    assert st == 0, lib.c21cm_last_error()
    n_m = 3 * (N // 2) ** 2 + 1
    kk = 2 * math.pi / L * np.sqrt(np.arange(n_m, dtype=np.float64))
    pk = np.array([lib.power_in_k(x) for x in kk])
    h = np.zeros(n_m)
    h[1:] = [math.sqrt(lib.power_in_vcb(x) / lib.power_in_k(x)) * 2.99792458e5 / x for x in kk[1:]]
    vol = np.float32(np.float32(L) * np.float32(L)) * np.float32(1.0) * np.float32(L)
    ospec = S.IcsSpec(dim=N, dim_z=N, hii_dim=n, hii_dim_z=n, box_len=L, box_len_z=L,
                      volume=float(vol), perturb_algorithm=2, n_m=n_m,
                      pk_by_m=pk.ctypes.data_as(S.c_double_p), seed=2026, rng_stream=1,
                      rng_threads=1, vcb_by_m=h.ctypes.data_as(S.c_double_p))
    ref_arrays = oracle.new_ics_arrays(ospec)
    ref_arrays["lowres_vcb"] = np.zeros((n, n, n), np.float32)
    ref = oracle.ics_grids(ospec, ref_arrays)
    compare(ics, ref)
    assert 1.0 < ref["lowres_vcb"].mean() < 1e3   # km/s, tens for a CLASS-like table
    # without the array, or without CLASS, the request is refused
    del ics["lowres_vcb"]
    ics["hires_density"][...] = 0
    assert lib.ComputeInitialConditions(2026, C.byref(api.ics_struct(ics))) == 3
    del ses


@pytest.mark.parametrize("dim,hii,dim_z,hii_z", [(1024, 512, 128, 64), (1536, 512, 192, 64)])
def test_split_pipeline_on_x_blocked_spectra(api, oracle, monkeypatch, dim, hii, dim_z, hii_z):
    """DIM >= 1024: the main block of a split spectrum is stored x-blocked ([x / 8][y][x % 8][k_z]); the
    element-wise kernels of the split IC pipeline (k^2 division, top-hat, fold by 2 and by 3 -- the
    reference's default DIM = 3 HII_DIM at HII_DIM = 512) map memory lines to wavenumbers through
    split_layout.h.  On a thin 1024 x 1024 x 128 / 1536 x 1536 x 192 box with a given density the
    split pipeline agrees with the padded one (rocFFT, full-size transforms + gathers) to transform
    round-off, for every output, and with the oracle (density_is_input); the PerturbedField of its output
    (cell deposit, F = 2 / F = 3: the reference's default geometry) agrees with the oracle's.  (Thinner boxes
    would leave the split pipeline: 512 x 512 x 32 or x 16 output grids are not native transform sizes.)"""
    import torch

    L = 1.5 * hii
    spec = ics_spec(dim, hii, box_len=L, density_is_input=1)
    spec.dim_z, spec.hii_dim_z = dim_z, hii_z
    spec.box_len_z = L * dim_z / dim
    spec.volume = float(np.float32(L) * np.float32(L) * np.float32(spec.box_len_z))
    g = torch.Generator(device="cuda").manual_seed(dim)
    dens = torch.randn((dim, dim, dim_z), device="cuda", generator=g)
    # smooth it a little so that derivatives and the fold see structure on all scales
    dens = (dens + torch.roll(dens, 1, 0) + torch.roll(dens, 1, 1) + torch.roll(dens, 1, 2)).contiguous()
    out = {}
    for mode in ("split", "padded"):
        if mode == "padded":
            monkeypatch.setenv("C21CM_ICS", "padded")
        start = api.new_ics_arrays(spec, device="cuda")
        start["hires_density"].copy_(dens)
        out[mode] = {k: v.cpu().numpy() for k, v in api.ics_grids(spec, start, device="cuda").items()}
        del start
        torch.cuda.empty_cache()
    for k in LOWRES_FIELDS:
        x, y = out["split"][k], out["padded"][k]
        assert np.abs(y).max() > 0, k
        np.testing.assert_allclose(x, y, atol=3e-5 * np.abs(y).max(), rtol=1e-4, err_msg=k)
    # ... and the split pipeline meets the oracle, whose PerturbedField then meets the cell kernel's (F = 2, 3)
    monkeypatch.delenv("C21CM_ICS")
    lib = api.load()
    assert lib.c21hip_native_fft_supported(dim, dim, dim_z) and lib.c21hip_native_fft_supported(hii, hii, hii_z)
    oracle.set_threads(oracle_threads())
    ref_start = oracle.new_ics_arrays(spec)
    ref_start["hires_density"][...] = dens.cpu().numpy()
    del dens
    ref = oracle.ics_grids(spec, ref_start)
    compare(out["split"], ref, LOWRES_FIELDS)
    compare_perturbed(api, oracle, spec, out["split"])
    lib.c21cm_release_device_cache()


def compare_perturbed(api, oracle, spec, ics_host):
    """Both sides' PerturbedField (2LPT, 3D velocities) on the same ICs: the device ICs copied to the host.
    The library runs on the device and must take the cell deposit; density at 2e-6 max|delta|, rtol 0 (as
    tests/test_gpu_perturb.py; observed 2.4e-7 to 3.1e-7 at config 2 and on the x-blocked boxes), velocities
    at its 2e-5 max|v|, rtol 1e-4."""
    import torch

    pspec = perturb_spec(2, dim=spec.dim, dim_z=spec.dim_z, hii_dim=spec.hii_dim, hii_dim_z=spec.hii_dim_z,
                         box_len=spec.box_len, box_len_z=spec.box_len_z, growth_factor=0.127,
                         init_growth_factor=0.0042, dDdt_over_D=2e-17, keep_3d_velocities=1)
    ics_dev = {k: torch.from_numpy(v).cuda() for k, v in ics_host.items()}
    got = {k: v.cpu().numpy() for k, v in api.perturb_grids(pspec, ics_dev).items()}
    assert cic_last_path(api) == "cell"
    del ics_dev
    torch.cuda.empty_cache()
    ref = oracle.perturb_grids(pspec, ics_host)
    assert np.isfinite(ref["density"]).all() and ref["density"].std() > 0
    err = density_error(got["density"], ref["density"])
    print(f"\n[PerturbedField DIM {spec.dim} x {spec.dim} x {spec.dim_z}] max|ddelta|/max|delta| vs oracle: {err:.2e}")
    assert err <= 2e-6
    for k in ref:
        if k != "density":
            assert np.isfinite(ref[k]).all(), k
            scale = np.abs(ref[k]).max()
            np.testing.assert_allclose(got[k], ref[k], atol=2e-5 * scale + 1e-9, rtol=1e-4, err_msg=k)


@pytest.mark.parametrize("stream", ["gsl", "philox"])
def test_config2_full_size_vs_oracle(api, oracle, stream):
    """BASELINE config 2 at its own size (DIM 512, HII_DIM 256, 2LPT) against the oracle: the default
    reference-compatible GSL stream (rng_stream 1, N_THREADS 2) and Philox, the stream bench.py --mode icpf
    times.  Every output field at the module's 3e-5 max|field|; then the device ICs, copied to the host, go
    through both sides' PerturbedField (the cell deposit at F = 2)."""
    spec = ics_spec(512, 256, box_len=384.0, seed=12345)
    if stream == "gsl":
        spec.rng_stream, spec.rng_threads = 1, 2
    got = {k: v.cpu().numpy() for k, v in api.ics_grids(spec, device="cuda").items()}
    api.load().c21cm_release_device_cache()
    oracle.set_threads(oracle_threads())
    ref = oracle.ics_grids(spec)
    assert set(ref) == set(got)
    compare(got, ref)
    compare_perturbed(api, oracle, spec, got)
