"""The x-blocked split layout of 512-point x-lines (fft_native.hip: split_xb_log2, C21CM_XBLOCK) against the plain
layout it replaces as the default.

The arithmetic of a line does not depend on where the line is stored, so the default library must reproduce
C21CM_XBLOCK=0 bit for bit in every output grid; only the f_coll partial sums are grouped differently (a partial
is the sum over 16 memory lines), so the per-radius f_coll means are held to rtol 1e-12.  global_xH is the mean of
an output grid and came out identical when the layouts were first compared (profiles/xblock_512_ab.txt): equality.

The switch is read once per process: the plain layout's results come from child processes that run this file as a
script.  A 512^3 grid is 0.5 GB, so a child does not send grids back: every grid is reduced on the device to three
wrapping 64-bit sums of its bit patterns (plain, and weighted by two position-dependent factors with coprime
periods), and the sums are compared.  A single differing bit changes the first sum; differences that cancel in
one sum would have to cancel under both weightings too.

Shape: the ionize driver takes nx = ny = hii_dim, so the smallest box with 512-point x-lines is 512 x 512 x 512
(512 x 64 x 512 cannot be requested).  Six radii (factor 1.7 up to 13.2 Mpc): the loop holds two pairs and one
single radius (indices 5 + 4, 3 + 2, 1), index 0 is the final sweep.  Inputs are drawn on the device from seeded
generators, which gives both processes the same fields.

The crossing-bit planes of the loop are indexed by memory line (c21hip_z_ionise_desc.cross_by_memory_line) and
c21hip_resolve_crossings_lines maps them back; the resolver has a case of its own at 512 x 64 x 512 lines, which
needs no driver: planes filled in memory-line order from one per-cell pattern for lb = 0 and lb = 4 must both
resolve to that pattern."""

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
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
W = importlib.import_module("21cmfast_amd.workloads")

N = 512
ZETA = 1.1
K_DEFAULT = 4  # blocks of 16 planes
GRIDS = ("neutral_fraction", "z_reion", "kinetic_temperature", "ionisation_rate_G12", "mean_free_path",
         "cumulative_recombinations")


def set_radii(spec, n, r_max, factor, count):
    radii = W.radii_ladder(n, 1.5 * n, r_max, delta_r_factor=factor)
    assert len(radii) == count, radii
    spec.n_radii = count
    for i, R in enumerate(radii):
        spec.R[i] = R
        spec.sigma_maxmass[i] = 2.4 * (R / 0.6) ** -0.62
    return spec


def six_radii(spec, n=N):
    return set_radii(spec, n, 14.0, 1.7, 6)


def digest(t):
    """Three wrapping int64 sums over the bit patterns of a device tensor (see the module docstring)."""
    import torch

    v = t.contiguous().view(-1).view(torch.int32 if t.element_size() != 1 else torch.uint8).to(torch.int64)
    i = torch.arange(v.numel(), device=v.device, dtype=torch.int64)
    out = [int(v.sum()), int((v * (i % 1000003 + 1)).sum()), int((v * (i % 999983 + 1)).sum())]
    return np.array(out, np.int64)


def fields(seed=77):
    import torch

    density = W.density_field_torch(N, seed=seed)
    n_ion = W.nion_from_density(density)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed + 1)

    def rnd():
        return torch.rand((N, N, N), generator=g, device="cuda", dtype=torch.float32)

    return density, n_ion, rnd


def collect(prefix, spec, buf, rep, flags, extra=None):
    import torch

    torch.cuda.synchronize()
    out = {f"{prefix}__global_xH": np.float64(rep.global_xH),
           f"{prefix}__f_coll_grid_mean": np.array(rep.f_coll_grid_mean[:spec.n_radii], np.float64),
           f"{prefix}__loop_flags": np.int64(flags),
           f"{prefix}__ionised": np.float64((buf.neutral_fraction == 0).float().mean().item())}
    for name in GRIDS:
        a = getattr(buf, name, None)
        if a is not None:
            out[f"{prefix}__grid__{name}"] = digest(a)
    for name, a in (extra or {}).items():
        out[f"{prefix}__grid__{name}"] = digest(a)
    return out


def case_stars(api):
    """two-grid STARS, the benchmark's loop (crossing bits unless C21CM_CROSS_BITS=0)"""
    density, n_ion, _ = fields()
    spec = six_radii(W.ionize_spec(N, r_bubble_max=14.0, ion_eff_factor=ZETA))
    buf, _, rep = api.ionize_grids(spec, density, n_ion)
    return collect("stars", spec, buf, rep, api.ionize_last_loop_flags())


def case_erfc(api):
    """closed-form ERFC: one grid, banded barrier"""
    density, _, _ = fields()
    spec = six_radii(W.ionize_spec(N, mode=W.FCOLL_ERFC, r_bubble_max=14.0))
    buf, _, rep = api.ionize_grids(spec, density, None)
    return collect("erfc", spec, buf, rep, api.ionize_last_loop_flags(), {"unnormalised_nion": buf.unnormalised_nion})


def case_xe(api):
    """STARS with the x_e grid of a spin-temperature run (three spectra in the fused pass Z)"""
    density, n_ion, rnd = fields()
    xe = -0.05 + 0.6 * rnd() ** 3  # spans the clips at 0 and 0.999
    Tn = 8.0 + 4.0 * rnd()
    spec = six_radii(W.ionize_spec(N, r_bubble_max=14.0, ion_eff_factor=ZETA, use_ts_fluct=1))
    buf, _, rep = api.ionize_grids(spec, density, n_ion, xe=xe, Tneutral=Tn)
    return collect("xe", spec, buf, rep, api.ionize_last_loop_flags())


def case_recomb(api):
    """the fused recombination loop (inhomogeneous model, CELL_RECOMB)"""
    import torch
    from recomb_helpers import recomb_spec

    density, n_ion, rnd = fields()
    whalo_sfr = (n_ion * (0.8 + 0.4 * rnd()) * 1e-9).contiguous()
    prev_nrec = 0.6 * rnd() ** 2
    prev_z = torch.where(rnd() < 0.1, 11.5, -1.0).to(torch.float32)
    spec = six_radii(recomb_spec(N, model=2, cell_recomb=1, r_bubble_max=14.0))
    buf, _, rep = api.ionize_grids(spec, density, n_ion, whalo_sfr=whalo_sfr, prev_nrec=prev_nrec,
                                   prev_z_reion=prev_z)
    return collect("recomb", spec, buf, rep, api.ionize_last_loop_flags())


def case_shard(api):
    """shard radii + finish and the slab finish, world = 1 (the exchange format is the uint8 mask)"""
    import torch

    density, n_ion, _ = fields()
    spec = six_radii(W.ionize_spec(N, r_bubble_max=14.0, ion_eff_factor=ZETA))
    fc = torch.zeros((N, N, N), dtype=torch.uint8, device="cuda")
    api.ionize_shard_radii(spec, 0, 1, fc, density, n_ion)
    flags = api.ionize_last_loop_flags()
    buf, _, rep = api.ionize_shard_finish(spec, fc, density, n_ion)
    out = collect("shard", spec, buf, rep, flags, {"first_cross": fc})
    del buf
    assert api.shard_slab_supported(spec)
    buf, _, rep = api.ionize_shard_finish_slab(spec, fc, 0, 1, density, n_ion, exchange=lambda st, status: status)
    out.update(collect("slab", spec, buf, rep, flags))
    return out


def case_1024(api):
    """1024 x 1024 x 512, four radii: blocks of 8 planes whatever C21CM_XBLOCK says"""
    import torch

    n = 1024
    spec = set_radii(W.ionize_spec(n, hii_dim_z=N, r_bubble_max=11.0, ion_eff_factor=ZETA), n, 11.0, 2.2, 4)
    density = W.density_field_torch(n, seed=5)[:, :, :N].contiguous()
    torch.cuda.empty_cache()
    n_ion = W.nion_from_density(density)
    buf, _, rep = api.ionize_grids(spec, density, n_ion)
    out = collect("n1024", spec, buf, rep, api.ionize_last_loop_flags())
    del buf, density, n_ion
    torch.cuda.empty_cache()
    api.load().c21cm_release_device_cache()
    return out


GROUPS = {"main": (case_stars, case_erfc, case_xe, case_recomb, case_shard, case_1024), "cb0": (case_stars,)}


def run_group(api, group):
    import torch

    lib = api.load()
    out = {"xb512": np.int64(lib.c21hip_split_xblock_log2(512)), "xb1024": np.int64(lib.c21hip_split_xblock_log2(1024)),
           "xb256": np.int64(lib.c21hip_split_xblock_log2(256)),
           "cross_bits": np.int64(lib.c21hip_z_cross_bits_supported(N, N, N))}
    for case in GROUPS[group]:
        out.update(case(api))
        torch.cuda.empty_cache()
    return out


def child(tmp_path_factory, group, **env_add):
    path = tmp_path_factory.mktemp("xblock_512") / f"{group}.npz"
    env = dict(os.environ, **env_add)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), str(path), group]
    subprocess.run(cmd, check=True, env=env, cwd=str(ROOT), timeout=600)
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


@pytest.fixture(scope="module")
def blocked(api):
    """Every case in this process: the default layout."""
    assert "C21CM_XBLOCK" not in os.environ and "C21CM_CROSS_BITS" not in os.environ
    return run_group(api, "main")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return child(tmp_path_factory, "main", C21CM_XBLOCK="0")


def assert_same(got, want, prefix):
    grids = sorted(k for k in want if k.startswith(f"{prefix}__grid__"))
    assert grids and grids == sorted(k for k in got if k.startswith(f"{prefix}__grid__"))
    for k in grids:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert int(got[f"{prefix}__loop_flags"]) == int(want[f"{prefix}__loop_flags"])
    assert float(got[f"{prefix}__global_xH"]) == float(want[f"{prefix}__global_xH"])
    a, b = got[f"{prefix}__f_coll_grid_mean"], want[f"{prefix}__f_coll_grid_mean"]
    print(f"{prefix}: ionised {float(got[prefix + '__ionised']):.4f}, loop flags {int(got[prefix + '__loop_flags'])}, "
          f"f_coll means max rel diff {float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))):.2e}")
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=0.0)
    assert 0.0 < float(got[f"{prefix}__ionised"]) < 1.0


def test_the_switch_decides_the_shift(blocked, plain):
    """512-point x-lines: blocks of 16 planes by default, plain with C21CM_XBLOCK=0; 1024 keeps 8, 256 stays plain."""
    assert (int(blocked["xb512"]), int(blocked["xb1024"]), int(blocked["xb256"])) == (K_DEFAULT, 3, 0)
    assert (int(plain["xb512"]), int(plain["xb1024"]), int(plain["xb256"])) == (0, 3, 0)


def test_two_grid_stars_crossing_bits(blocked, plain):
    flags = int(blocked["stars__loop_flags"])
    assert flags & 1 and flags & 32 and not flags & (2 | 4), flags  # the fused two-grid loop, two radii per sweep
    assert int(blocked["cross_bits"]) == 1 and int(plain["cross_bits"]) == 1
    assert 0.05 < float(blocked["stars__ionised"]) < 0.95
    assert_same(blocked, plain, "stars")


def test_two_grid_stars_on_the_mask(gpu_lib, tmp_path_factory):
    """The same with C21CM_CROSS_BITS=0: both layouts in child processes of their own."""
    b = child(tmp_path_factory, "cb0", C21CM_CROSS_BITS="0")
    p = child(tmp_path_factory, "cb0", C21CM_CROSS_BITS="0", C21CM_XBLOCK="0")
    assert int(b["xb512"]) == K_DEFAULT and int(p["xb512"]) == 0
    assert int(b["cross_bits"]) == 0 and int(p["cross_bits"]) == 0  # the uint8 mask is updated by every pass Z
    assert int(b["stars__loop_flags"]) & 1
    assert_same(b, p, "stars")


def test_closed_form_erfc(blocked, plain):
    assert_same(blocked, plain, "erfc")


def test_stars_with_an_xe_grid(blocked, plain):
    flags = int(blocked["xe__loop_flags"])
    assert flags & 1 and flags & 4, flags
    assert_same(blocked, plain, "xe")


def test_fused_recombination_loop(blocked, plain):
    assert int(blocked["recomb__loop_flags"]) & 2
    for name in ("ionisation_rate_G12", "mean_free_path", "cumulative_recombinations"):
        assert f"recomb__grid__{name}" in blocked
    assert_same(blocked, plain, "recomb")


def test_shard_phases_at_world_one(blocked, plain):
    assert "shard__grid__first_cross" in blocked
    assert_same(blocked, plain, "shard")
    assert_same(blocked, plain, "slab")
    for k in [k for k in blocked if k.startswith("slab__grid__")]:  # and both finishes equal the single pass
        np.testing.assert_array_equal(blocked[k], blocked[k.replace("slab__", "stars__")], err_msg=k)
        np.testing.assert_array_equal(blocked[k], blocked[k.replace("slab__", "shard__")], err_msg=k)


def test_resolver_maps_memory_lines_to_logical_lines(gpu_lib):
    """512 x 64 lines of 512 cells, radii 1..5.  Pattern: want[line, z] in 0..5 from a generator; the plane of
    radius r has the cell's bit set where want == r and, to exercise 'the largest index wins', at random where
    r < want.  The planes are laid out by memory line for lb = 0 (memory = logical) and lb = 4; both must resolve to
    `want`, and the bytes behind the mask keep their pattern.  A line count that is no whole number of blocks is
    refused."""
    import torch

    nx, ny, R = 512, 64, 5
    nlines = nx * ny
    rng = np.random.default_rng(2409)
    want = rng.integers(0, R + 1, (nlines, 512), dtype=np.uint8)
    want[0], want[1], want[-1] = 0, R, 1
    z = np.arange(512)
    word, bit = (z >> 1) & 15, ((z >> 5) + 16 * (z & 1)).astype(np.uint32)
    planes = np.zeros((R, nlines, 16), np.uint32)  # by logical line
    for r in range(1, R + 1):
        on = (want == r) | ((want > r) & (rng.random(want.shape) < 0.3))
        for b in range(16):
            cols = np.nonzero(word == b)[0]
            planes[r - 1, :, b] = np.bitwise_or.reduce(on[:, cols].astype(np.uint32) << bit[cols], axis=1)
    gpu_lib.c21hip_resolve_crossings_lines.restype = C.c_int
    gpu_lib.c21hip_resolve_crossings_lines.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int,
                                                       C.c_int, C.c_void_p]
    m = np.arange(nlines)
    masks = {}
    for lb in (0, K_DEFAULT):
        xb = 1 << lb
        blk, rem = m // (ny * xb), m % (ny * xb)
        logical = (blk * xb + rem % xb) * ny + rem // xb  # memory line m holds logical line x * ny + y
        assert np.array_equal(np.sort(logical), m)
        d_planes = torch.from_numpy(np.ascontiguousarray(planes[:, logical]).view(np.int32)).cuda()
        d_mask = torch.full((nlines * 512 + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
        assert gpu_lib.c21hip_resolve_crossings_lines(d_planes.data_ptr(), R, 1, d_mask.data_ptr(), nlines, ny, lb,
                                                      None) == 0
        torch.cuda.synchronize()
        got = d_mask.cpu().numpy()
        assert (got[nlines * 512:] == 0xAB).all()
        masks[lb] = got[: nlines * 512].reshape(nlines, 512)
        np.testing.assert_array_equal(masks[lb], want, err_msg=f"lb = {lb}")
    np.testing.assert_array_equal(masks[0], masks[K_DEFAULT])
    assert gpu_lib.c21hip_resolve_crossings_lines(d_planes.data_ptr(), R, 1, d_mask.data_ptr(), nlines - ny, ny,
                                                  K_DEFAULT, None) != 0


def test_1024_point_lines_ignore_the_switch(blocked, plain):
    """Both processes run blocks of 8 planes at nx = 1024: the switch does not reach these lines."""
    assert_same(blocked, plain, "n1024")


if __name__ == "__main__":
    api_ = importlib.import_module("21cmfast_amd.grid_api")
    importlib.import_module("21cmfast_amd").load(require_gpu=True)
    api_.load().c21hip_split_xblock_log2.restype = C.c_int
    np.savez(sys.argv[1], **run_group(api_, sys.argv[2]))
