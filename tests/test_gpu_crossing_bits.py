"""Crossing bits of the two-grid fused pass Z (fft_native.hip: zw_ionise_kernel<16, false, 16, false, true>,
ionize_kernels.hip: resolve_crossings_kernel) against the uint8 first-crossing mask they replace inside
the R loop (C21CM_CROSS_BITS=0).

Both paths evaluate the same barrier predicate on the same registers and keep the f_coll partial sums
where they were, so every output is compared with array_equal, no tolerance.  The switch is read once
per process: the mask path's outputs come from ONE child process (the `mask_path` fixture), which runs
this file as a script.

Boxes: the fused kernel needs 512-point z-lines.  32 x 32 x 512 is below the native transform's
shortest line (64), so that box takes the rocFFT route without a first-crossing grid -- it is kept as the
case where neither path may change anything; 64 x 64 x 512 is the smallest box whose loop launches the
fused kernel (asserted through the loop flags).  The x-blocked line mapping (logical_line) starts at
nx = 1024: it is covered at kernel level on a 1024 x 16 x 512 grid of random spectra (both pass-Z
kernels on the same inputs, walking the lines backwards and, in a second child process, forwards) and
end to end on a 1024 x 1024 x 512 box, where the single pass (crossing bits) must equal the world = 1
shard phases (mask) bit for bit.

Six radii: the loop holds two pairs of radii and one single radius (indices 5 + 4, 3 + 2, 1).  zeta = 1.1
lets 4 / 29 / 48 / 58 / 64 % of the cells of the 64 x 64 x 512 box cross by the five loop radii (CPU
oracle, cumulative) and 68.5 % in the end, 88 % with the x_e grid; the tests check the final fractions."""

import ctypes as C
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
W = importlib.import_module("21cmfast_amd.workloads")

BOXES = (32, 64)
ZETA = 1.1


def make_spec(n, **kw):
    """n x n x 512, six radii 0.93 ... 13.2 Mpc (factor 1.7 apart, so that each one matters)."""
    spec = W.ionize_spec(n, hii_dim_z=512, r_bubble_max=14.0, ion_eff_factor=ZETA, **kw)
    radii = W.radii_ladder(n, 1.5 * n, 14.0, delta_r_factor=1.7)
    assert len(radii) == 6
    spec.n_radii = len(radii)
    for i, R in enumerate(radii):
        spec.R[i] = R
    return spec


def inputs(n):
    density = W.density_field_numpy((n, n, 512), seed=77)
    return density, W.nion_from_density(density)


def xe_inputs(n):
    rng = np.random.default_rng(3)
    xe = (-0.05 + 0.6 * rng.random((n, n, 512)) ** 3).astype(np.float32)  # spans the clips at 0 and 0.999
    Tn = (8.0 + 4.0 * rng.random((n, n, 512))).astype(np.float32)
    return xe, Tn


def outputs(prefix, spec, buf, rep, flags):
    import torch

    torch.cuda.synchronize()
    out = {"neutral_fraction": buf.neutral_fraction.cpu().numpy(), "z_reion": buf.z_reion.cpu().numpy(),
           "kinetic_temperature": buf.kinetic_temperature.cpu().numpy(),
           "global_xH": np.float64(rep.global_xH),
           "f_coll_grid_mean": np.array(rep.f_coll_grid_mean[:spec.n_radii], np.float64),
           "loop_flags": np.int64(flags)}
    return {f"{prefix}__{k}": v for k, v in out.items()}


def run_two_grid(api, n):
    import torch

    spec = make_spec(n)
    density, n_ion = inputs(n)
    buf, _, rep = api.ionize_grids(spec, torch.from_numpy(density).cuda(), torch.from_numpy(n_ion).cuda())
    return outputs(f"two_grid_{n}", spec, buf, rep, api.ionize_last_loop_flags())


def run_xe(api, n=64):
    import torch

    spec = make_spec(n, use_ts_fluct=1)
    density, n_ion = inputs(n)
    xe, Tn = xe_inputs(n)
    buf, _, rep = api.ionize_grids(spec, torch.from_numpy(density).cuda(), torch.from_numpy(n_ion).cuda(),
                                   xe=torch.from_numpy(xe).cuda(), Tneutral=torch.from_numpy(Tn).cuda())
    return outputs("xe", spec, buf, rep, api.ionize_last_loop_flags())


def run_shard(api, n=64):
    import torch

    spec = make_spec(n)
    density, n_ion = inputs(n)
    d, s = torch.from_numpy(density).cuda(), torch.from_numpy(n_ion).cuda()
    fc = torch.zeros((n, n, 512), dtype=torch.uint8, device="cuda")
    api.ionize_shard_radii(spec, 0, 1, fc, d, s)
    buf, _, rep = api.ionize_shard_finish(spec, fc, d, s)
    out = outputs("shard", spec, buf, rep, api.ionize_last_loop_flags())
    out["shard__first_cross"] = fc.cpu().numpy()
    return out


def run_all(api):
    out = {}
    for n in BOXES:
        out.update(run_two_grid(api, n))
    out.update(run_xe(api))
    out.update(run_shard(api))
    return out


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


@pytest.fixture(scope="module")
def mask_path(tmp_path_factory):
    """Every case on the uint8 mask: one child process with C21CM_CROSS_BITS=0."""
    path = tmp_path_factory.mktemp("crossing_bits") / "mask_path.npz"
    env = dict(os.environ, C21CM_CROSS_BITS="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), str(path)]
    subprocess.run(cmd, check=True, env=env, cwd=str(ROOT), timeout=300)
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def bits_path(api, gpu_lib):
    """The same cases in this process: the default."""
    assert "C21CM_CROSS_BITS" not in os.environ
    assert gpu_lib.c21hip_z_cross_bits_supported(64, 64, 512) == 1
    return run_all(api)


FIELDS = ("neutral_fraction", "z_reion", "kinetic_temperature", "global_xH", "f_coll_grid_mean")


def assert_same(got, want, prefix):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f"{prefix}__{f}"], want[f"{prefix}__{f}"], err_msg=f"{prefix}__{f}")
    assert int(got[f"{prefix}__loop_flags"]) == int(want[f"{prefix}__loop_flags"])


@pytest.mark.parametrize("n", BOXES)
def test_bit_identity_with_the_mask_path(bits_path, mask_path, n):
    """neutral_fraction, z_reion, kinetic_temperature, global_xH and every f_coll_grid_mean: exactly equal."""
    prefix = f"two_grid_{n}"
    flags = int(bits_path[f"{prefix}__loop_flags"])
    if n >= 64:  # the fused loop, two radii per sweep: the crossing-bits kernel ran
        assert flags & 1 and flags & 32 and not flags & (2 | 4), flags
    else:  # below the native transform's shortest line: no fused loop, nothing to switch
        assert not flags & 1, flags
    ionised = float(np.mean(bits_path[f"{prefix}__neutral_fraction"] == 0))
    print(f"{prefix}: ionised fraction {ionised:.4f}, loop flags {flags}")
    assert 0.05 < ionised < 0.95, ionised
    assert np.all(bits_path[f"{prefix}__f_coll_grid_mean"][1:] > 0)
    assert_same(bits_path, mask_path, prefix)


def test_xe_route_untouched(bits_path, mask_path):
    """STARS + x_e at 64 x 64 x 512: the three-grid kernel keeps the mask whatever the switch says."""
    flags = int(bits_path["xe__loop_flags"])
    assert flags & 1 and flags & 4, flags
    assert 0.02 < float(np.mean(bits_path["xe__neutral_fraction"] == 0)) < 0.98
    assert_same(bits_path, mask_path, "xe")


def test_shard_phases_untouched(bits_path, mask_path):
    """shard_radii + shard_finish with world = 1: the exchange format is the mask, and equals the single
    pass's outcome on either path."""
    assert_same(bits_path, mask_path, "shard")
    np.testing.assert_array_equal(bits_path["shard__first_cross"], mask_path["shard__first_cross"])
    fc = bits_path["shard__first_cross"]
    assert set(np.unique(fc)) == {0, 1, 2, 3, 4, 5}  # every loop radius is some cell's first crossing
    for f in ("neutral_fraction", "z_reion", "global_xH"):
        np.testing.assert_array_equal(bits_path[f"shard__{f}"], bits_path[f"two_grid_64__{f}"])


# ---- the resolver on its own -----------------------------------------------------------------------
def cell_to_bit():
    """The bit order of the planes: cell z of a line sits in word (z / 2) % 16 at bit (z / 32) + 16 (z % 2)."""
    z = np.arange(512)
    return (z >> 1) & 15, (z >> 5) + 16 * (z & 1)


@pytest.mark.parametrize("r_hi,r_lo,nlines", [(39, 1, 200), (5, 1, 37), (70, 3, 200), (255, 250, 16)])
def test_resolver_against_numpy(gpu_lib, r_hi, r_lo, nlines):
    """Random planes with a known answer: the largest radius index in [r_lo, r_hi] whose bit is set, 0 where
    none is.  Line 0 is set in no plane, line 1 in the last visited plane only, line 2 in all planes; planes
    below r_lo hold ones and must not be read as crossings; 200 lines are 800 threads (three whole
    workgroups and a part of one), 37 lines a part of one; r_hi >= 64 takes the eight-slice instantiation.
    The bytes after the mask keep their pattern."""
    import torch

    rng = np.random.default_rng(r_hi * 1000 + nlines)
    planes = np.zeros((r_hi, nlines, 16), np.uint32)
    for r in range(r_lo, r_hi + 1):
        w = rng.integers(0, 2**32, (3, nlines, 16), dtype=np.uint64).astype(np.uint32)
        planes[r - 1] = w[0] & w[1] & w[2]  # an eighth of the bits set
    planes[: r_lo - 1] = 0xFFFFFFFF
    planes[r_lo - 1:, 0] = 0
    planes[r_lo - 1:, 1] = 0
    planes[r_lo - 1, 1] = 0xFFFFFFFF
    planes[r_lo - 1:, 2] = 0xFFFFFFFF
    word, bit = cell_to_bit()
    want = np.zeros((nlines, 512), np.uint8)
    for r in range(r_lo, r_hi + 1):  # ascending: the largest index wins
        hit = ((planes[r - 1][:, word] >> bit.astype(np.uint32)) & 1).astype(bool)
        want[hit] = r
    assert (want[0] == 0).all() and (want[1] == r_lo).all() and (want[2] == r_hi).all()
    if r_hi - r_lo > 3:
        assert len(np.unique(want[3:])) >= min(r_hi - r_lo, 20)

    d_planes = torch.from_numpy(planes.view(np.int32)).cuda()
    guard = 4096
    d_mask = torch.full((nlines * 512 + guard,), 0xAB, dtype=torch.uint8, device="cuda")
    gpu_lib.c21hip_resolve_crossings.restype = C.c_int
    gpu_lib.c21hip_resolve_crossings.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    st = gpu_lib.c21hip_resolve_crossings(d_planes.data_ptr(), r_hi, r_lo, d_mask.data_ptr(), nlines, None)
    assert st == 0
    torch.cuda.synchronize()
    got = d_mask.cpu().numpy()
    np.testing.assert_array_equal(got[: nlines * 512].reshape(nlines, 512), want)
    assert (got[nlines * 512:] == 0xAB).all()


# ---- the x-blocked line mapping (nx >= 1024) ------------------------------------------------------------
XB = (1024, 16, 512)  # the mapping depends on nx alone; 16384 lines = 1024 workgroups


class ZIoniseDesc(C.Structure):
    """c21hip_z_ionise_desc (c21hip.h); a mirror whose size differs from the library's is refused by the entry."""
    _fields_ = [("size", C.c_size_t), ("delta_work", C.c_void_p), ("stars_work", C.c_void_p),
                ("xe_work", C.c_void_p), ("nrec_work", C.c_void_p), ("nrec", C.c_void_p), ("rec0", C.c_double),
                ("recomb", C.c_int), ("g12", C.c_void_p), ("first_cross", C.c_void_p), ("cross_plane", C.c_void_p),
                ("partials", C.c_void_p), ("sum_out", C.c_void_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("r_index", C.c_int), ("rhocrit_omb", C.c_double), ("ion_eff", C.c_double),
                ("mass_dep_zeta", C.c_int), ("f_limit", C.c_double)]


def kernel_level_xblocked(lib):
    """Both two-grid pass-Z kernels on the same random spectra of a 1024 x 16 x 512 grid, three radii
    visited 3, 2, 1 with fresh emissivity spectra each: the mask kernel updates one uint8 mask, the bits
    kernel writes three planes that the resolver turns into a mask.  Returns both masks, both sets of
    workgroup partial sums and the words after the planes (a guard pattern)."""
    import torch

    nx, ny, nz = XB
    nlines, H = nx * ny, nz // 2
    lib.c21hip_split_floats.restype = C.c_size_t
    nf = lib.c21hip_split_floats(nx, ny, nz)
    assert nf == 2 * (nlines * H + nlines)
    lib.c21hip_z_ionise_partials.restype = C.c_int
    n_part = lib.c21hip_z_ionise_partials(nx, ny, nz)
    lib.c21hip_split_z_ionise.restype = C.c_int
    lib.c21hip_split_z_ionise.argtypes = [C.POINTER(ZIoniseDesc), C.c_void_p]
    lib.c21hip_resolve_crossings.restype = C.c_int
    lib.c21hip_resolve_crossings.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]

    g = torch.Generator(device="cuda")
    g.manual_seed(2024)
    # a z-line is the sum of its 256 coefficients' waves: amplitudes of 0.01 give cells of ~ +-0.3
    delta = 0.01 * torch.randn(nf, generator=g, device="cuda", dtype=torch.float32)
    delta[0:2 * nlines * H:2 * H] = 0.0  # DC of every line: delta_R averages to zero
    mask = torch.zeros(nlines * nz, dtype=torch.uint8, device="cuda")
    plane_words = nlines * nz // 32
    guard = 1024
    planes = torch.full((3 * plane_words + guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    part_m = torch.zeros((3, n_part), dtype=torch.float64, device="cuda")
    part_b = torch.zeros((3, n_part), dtype=torch.float64, device="cuda")
    for r in (3, 2, 1):
        stars = 0.01 * torch.randn(nf, generator=g, device="cuda", dtype=torch.float32)
        stars[0:2 * nlines * H:2 * H] = 1.0  # DC: the emissivity averages to the barrier of delta = 0
        common = dict(size=C.sizeof(ZIoniseDesc), delta_work=delta.data_ptr(), stars_work=stars.data_ptr(),
                      nx=nx, ny=ny, nz=nz, r_index=r, rhocrit_omb=1.0, ion_eff=1.2 - 0.1 * r, mass_dep_zeta=1,
                      f_limit=1e-9)  # zeta 0.9, 1.0, 1.1: about 41, 29, 17 % first crossings; sum_out NULL
        assert lib.c21hip_split_z_ionise(ZIoniseDesc(first_cross=mask.data_ptr(), partials=part_m[r - 1].data_ptr(),
                                                     **common), None) == 0
        plane = planes.data_ptr() + 4 * (r - 1) * plane_words
        assert lib.c21hip_split_z_ionise(ZIoniseDesc(cross_plane=plane, partials=part_b[r - 1].data_ptr(),
                                                     **common), None) == 0
        torch.cuda.synchronize()
    resolved = torch.full((nlines * nz,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.c21hip_resolve_crossings(planes.data_ptr(), 3, 1, resolved.data_ptr(), nlines, None) == 0
    torch.cuda.synchronize()
    return {"mask": mask.cpu().numpy(), "resolved": resolved.cpu().numpy(), "part_m": part_m.cpu().numpy(),
            "part_b": part_b.cpu().numpy(), "guard": planes[3 * plane_words:].cpu().numpy()}


def check_kernel_level_xblocked(out):
    share = [float(np.mean(out["mask"] == r)) for r in range(4)]
    print("x-blocked kernel level: share of cells by first crossing 0..3:", share)
    assert all(s > 0.05 for s in share), share  # every radius is the first crossing of many cells, some never cross
    np.testing.assert_array_equal(out["resolved"], out["mask"])
    np.testing.assert_array_equal(out["part_b"], out["part_m"])
    assert np.all(out["part_m"] > 0)
    assert (out["guard"] == 0x5A5A5A5A).all()


def test_xblocked_lines_kernel_level(gpu_lib):
    """lb = 3 (nx = 1024): planes indexed through logical_line() resolve to the mask kernel's mask, and
    the partial sums keep their places -- the lines walked backwards (the default)."""
    assert "C21CM_ZREV" not in os.environ
    assert gpu_lib.c21hip_z_cross_bits_supported(*XB) == 1
    check_kernel_level_xblocked(kernel_level_xblocked(gpu_lib))


def test_xblocked_lines_kernel_level_forwards():
    """The same with C21CM_ZREV=0 (the switch is read once per process: a child runs the check)."""
    env = dict(os.environ, C21CM_ZREV="0")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "--xblocked"]
    subprocess.run(cmd, check=True, env=env, cwd=str(ROOT), timeout=300)


def test_xblocked_box_single_pass_equals_shard_phases(api, gpu_lib):
    """1024 x 1024 x 512, four radii (one radius per sweep at this nx): the single pass runs the crossing-bits
    kernel under the x-blocked mapping, shard_radii + shard_finish with world = 1 stay on the mask; the two
    are bit for bit the same computation otherwise (test_gpu_ionize.py::test_shard_phases_equal_single_pass)."""
    import torch

    n, nz = 1024, 512
    assert gpu_lib.c21hip_z_cross_bits_supported(n, n, nz) == 1
    spec = W.ionize_spec(n, hii_dim_z=nz, r_bubble_max=11.0, ion_eff_factor=ZETA)
    radii = W.radii_ladder(n, 1.5 * n, 11.0, delta_r_factor=2.2)
    assert len(radii) == 4
    spec.n_radii = len(radii)
    for i, R in enumerate(radii):
        spec.R[i] = R
    density = W.density_field_torch(n, seed=5)[:, :, :nz].contiguous()
    torch.cuda.empty_cache()
    n_ion = W.nion_from_density(density)
    buf, _, rep = api.ionize_grids(spec, density, n_ion)
    flags = api.ionize_last_loop_flags()
    assert flags & 1 and not flags & (2 | 4), flags
    fc = torch.zeros((n, n, nz), dtype=torch.uint8, device="cuda")
    api.ionize_shard_radii(spec, 0, 1, fc, density, n_ion)
    buf2, _, rep2 = api.ionize_shard_finish(spec, fc, density, n_ion)
    torch.cuda.synchronize()
    ionised = float((buf.neutral_fraction == 0).float().mean())
    crossed = [float((fc == r).float().mean()) for r in range(4)]
    print(f"1024 x 1024 x 512: ionised fraction {ionised:.4f}, first crossings 0..3 {crossed}, loop flags {flags}")
    assert 0.05 < ionised < 0.95, ionised
    assert all(c > 0.01 for c in crossed), crossed
    assert torch.equal(buf.neutral_fraction, buf2.neutral_fraction)
    assert torch.equal(buf.z_reion, buf2.z_reion)
    assert torch.equal(buf.kinetic_temperature, buf2.kinetic_temperature)
    assert rep.global_xH == rep2.global_xH
    del buf, buf2, fc, density, n_ion
    torch.cuda.empty_cache()


if __name__ == "__main__":  # the children of `mask_path` and of the forwards x-blocked check
    pkg = importlib.import_module("21cmfast_amd")
    lib = pkg.load(require_gpu=True)
    if sys.argv[1] == "--xblocked":
        check_kernel_level_xblocked(kernel_level_xblocked(lib))
    else:
        np.savez(sys.argv[1], **run_all(importlib.import_module("21cmfast_amd.grid_api")))
