"""What the Eulerian TABLE loops decide (FCOLL_TABLE_LINEAR, FCOLL_TABLE_EXP, with and without an x_e grid),
cell by cell, against mode (t) of the float64 restatement of tests/excursion_reference.py (pinned to the CPU
oracle and held to its caps by test_excursion_reference_host.py), on every route these loops have.

Per case and route the device gives the single pass (api.ionize_grids, device-resident) and the world = 1 shard
pair; excursion_reference.check_outputs holds them to what test_gpu_excursion_cells.py lists -- every decided
flag, every decided first-crossing radius, one of two candidates elsewhere, z_reion, x_HI on decided-neutral
cells, the per-radius means -- and to a first_cross grid without a marker (255).  All bounds come from the
reference side: t = 4 E32 (margin); means within 4 E32(mean), plus 2^-23 for the ln-tables (a one-sided
float-accuracy error in every exponential, which exp_f32acc's contract permits: derived, not measured); x_HI
within 4 x the float32 evaluation of the radius-0 expression.

Every variant asserts the route it means to test:
  * launch counts per kernel kind (c21hip_ktime_*): 0 pass X with streamed window tables, 7 / 8 pass X with
    evaluated windows for one / two radii, 11 the x_e grid's pass Z with a barrier, 13 the extrema-only pass Z,
    14 pass Z + table sweep + banded barrier;
  * the C21CM_EUL_BAND_DEBUG trace: "band fail=0" where banded sweeps ran and held, no band line where none
    ran, "band miss" (or a non-zero fail) under a forced miss;
  * bit 64 of the loop flags: the cell-scale radius and the post-loop ran as one sweep.
The switches are read with getenv per call, so monkeypatch.setenv in this process reaches them; the route
assertions would notice if one did not.

What no box here reaches: two radii per pass-X sweep and the four rotating k-space buffers that go with them.
The evaluated windows they need are built for x-lines of 128 points and more, and the fused table sweep for
512-point z-lines and more, so the smallest such box has 128 x 128 x 512 cells -- 8 M, a minute of host
restatement.  On the 64-point x-lines of these boxes pass X streams window tables, one radius per sweep (kind 0
runs, kinds 7 and 8 do not), and C21CM_EUL_PAIR=0 changes nothing; the variant is run and says so.

Each case prints one line EXCURSION.  The restatement of a case is computed once
per process (excursion_reference.restated_table)."""

import ctypes as C
import importlib
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import excursion_reference as X  # noqa: E402
from test_gpu_excursion_cells import device_outputs  # noqa: E402

pytestmark = pytest.mark.gpu

W = importlib.import_module("21cmfast_amd.workloads")
S = importlib.import_module("21cmfast_amd.structs")

KINDS = (0, 7, 8, 11, 13, 14)
SWITCHES = ("C21CM_EUL_TABLE_FUSED", "C21CM_EUL_BAND", "C21CM_EUL_PAIR", "C21CM_EUL_R0_FUSED",
            "C21CM_EUL_BAND_SHIFT", "C21CM_XE_MASK_FUSED")

# Default route of a case: (native passes?, kinds that must run, kinds that must not, band trace).  Band trace:
# "held" banded sweeps ran and every band held, "none" no banded sweep, "miss" a band missed and was recovered.
ROUTES = {
    # 64-point z-lines: no table sweep inside a pass Z; delta_R is stored, the banded sweep reads it
    # (fcoll_eulerian_band_kernel; the first radii and index 1 take fcoll_eulerian_kernel + eulerian_mask_kernel)
    "l-64": (True, (0,), (7, 8, 11, 13, 14), "held"),
    "e-64": (True, (0,), (7, 8, 11, 13, 14), "held"),
    "l-50": (False, (), KINDS, "none"),  # the library's transform route, one radius at a time, dense sweeps
    "e-64x512": (True, (0, 13, 14), (7, 8, 11), "held"),  # extrema-only pass Z, then pass Z + table + band
    "l-64x512": (True, (0, 13, 14), (7, 8, 11), "held"),
    "e-32x1024": (False, (), KINDS, "none"),  # 32 x 32 lines are not native: long lines on the transform route
    "e-64x1024": (True, (0, 13, 14), (7, 8, 11), "held"),  # 1024-point z-lines
    "ex-64x512": (True, (0, 11), (7, 8, 13, 14), "held"),  # the x_e grid's pass Z: table sweep + band
    "lx-64": (True, (0,), (7, 8, 11, 13, 14), "none"),  # x_e(R) stored, fcoll_eulerian_kernel + eulerian_mask_kernel
    "em-64x512": (True, (0, 13, 14), (7, 8, 11), "held"),
}
assert set(ROUTES) == set(X.TABLE_CASES)


@pytest.fixture(scope="module")
def api(gpu_lib):
    gpu_lib.c21hip_ktime_enable.restype = None
    gpu_lib.c21hip_ktime_enable.argtypes = [C.c_int]
    gpu_lib.c21hip_ktime_report.restype = C.c_int
    gpu_lib.c21hip_ktime_report.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    return importlib.import_module("21cmfast_amd.grid_api")


def run(api, gpu_lib, capfd, monkeypatch, name, switches=None):
    """The case on the device under `switches`: (outputs, launch count per kind, band trace, the case).  The band
    trace is "held", "none" or "miss", read from what C21CM_EUL_BAND_DEBUG prints."""
    spec, inp, ref, e = case = X.restated_table(W, name)
    X.install_table(spec, inp, S)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (switches or {}).items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("C21CM_EUL_BAND_DEBUG", "1")
    capfd.readouterr()
    gpu_lib.c21hip_ktime_enable(1)
    try:
        out = device_outputs(api, spec, inp)
        counts = {}
        for kind in KINDS:
            n = C.c_int(0)
            assert gpu_lib.c21hip_ktime_report(kind, None, C.byref(n)) == 0
            counts[kind] = n.value
    finally:
        gpu_lib.c21hip_ktime_enable(0)
        monkeypatch.delenv("C21CM_EUL_BAND_DEBUG")
    err = capfd.readouterr().err
    if re.search(r"band fail=[1-9]|band miss at r=", err):
        band = "miss"
    elif "band fail=0" in err:
        band = "held"
    else:
        assert "band " not in err, err[-2000:]
        band = "none"
    return out, counts, band, case


def check(name, case, out, counts, band, variant=""):
    spec, inp, ref, e = case
    fc = out["first_cross"]
    print(f"{name}{variant}: launches per kind {counts}, band trace {band}, loop flags {int(out['loop_flags'])}, "
          f"markers left {int((fc == 255).sum())}")
    assert not (fc == 255).any()
    fig = X.check_outputs(ref, out)
    print(X.excursion_line(name + variant, ref, e, fig))
    assert ref.flag_undecided_share <= X.FLAG_CAP and ref.radius_undecided_share <= X.RADIUS_CAP


def assert_route(counts, band, ran, not_ran, want_band):
    assert all(counts[k] > 0 for k in ran) and all(counts[k] == 0 for k in not_ran), (counts, ran, not_ran)
    assert band == want_band, (band, want_band)


@pytest.mark.parametrize("name", list(X.TABLE_CASES))
def test_every_decided_cell(api, gpu_lib, capfd, monkeypatch, name):
    native, ran, not_ran, want_band = ROUTES[name]
    out, counts, band, case = run(api, gpu_lib, capfd, monkeypatch, name)
    assert bool(gpu_lib.c21hip_fft_is_native(*case[1].density.shape)) == native
    check(name, case, out, counts, band)
    assert_route(counts, band, ran, not_ran, want_band)
    assert not int(out["loop_flags"]) & (1 | 2 | 4)  # no fused Lagrangian loop
    assert bool(int(out["loop_flags"]) & 64) == native  # the one-sweep finish of the Eulerian loops


@pytest.mark.parametrize("name", ["e-64x512", "ex-64x512"])
def test_sharded_radii_reduced_and_finished(api, gpu_lib, capfd, monkeypatch, name):
    """Worlds of 2 and 3 ranks: each rank's share of the ladder into its own first_cross grid, max-reduced,
    finished -- and the reduced grid and the finished box held to the accounting, not to the single pass."""
    import torch

    out, counts, band, case = run(api, gpu_lib, capfd, monkeypatch, name)
    spec, inp, ref, e = case
    density = torch.from_numpy(np.array(inp.density)).cuda()
    kw = {k: torch.from_numpy(np.array(v)).cuda() for k, v in inp.kwargs().items()}
    for world in (2, 3):
        reduced = torch.zeros(inp.density.shape, dtype=torch.uint8, device="cuda")
        for rank in range(world):
            fc = torch.zeros_like(reduced)
            api.ionize_shard_radii(spec, rank, world, fc, density, None, **kw)
            assert int((fc == 255).sum()) == 0  # no marker survives a shard phase
            reduced = torch.maximum(reduced, fc)
        buf, _, _ = api.ionize_shard_finish(spec, reduced.contiguous(), density, None, **kw)
        torch.cuda.synchronize()
        sharded = dict(out, first_cross=reduced.cpu().numpy(), shard_neutral_fraction=buf.neutral_fraction.cpu().numpy(),
                       shard_z_reion=buf.z_reion.cpu().numpy())
        check(name, case, sharded, counts, band, f" (world {world})")


#   switches -> (kinds that must run, kinds that must not, band trace, bit 64 of the loop flags)
E_VARIANTS = {
    "C21CM_EUL_TABLE_FUSED=0": ((0,), (7, 8, 11, 13, 14), "held", True),  # store pass + fcoll_eulerian_band_kernel
    "C21CM_EUL_BAND=0": ((0,), (7, 8, 11, 13, 14), "none", True),  # fcoll_eulerian_kernel + eulerian_mask_kernel
    "C21CM_EUL_PAIR=0": ((0, 13, 14), (7, 8, 11), "held", True),  # the default route on 64-point x-lines (above)
    "C21CM_EUL_R0_FUSED=0": ((0, 13, 14), (7, 8, 11), "held", False),  # the general kernels at the cell scale
    "C21CM_EUL_BAND_SHIFT=0.2": ((0, 13, 14), (7, 8, 11), "miss", True),  # rewind, dense rerun of the radius
}
EX_VARIANTS = {
    "C21CM_XE_MASK_FUSED=0": ((0,), (7, 8, 11, 13, 14), "none", True),  # x_e(R) stored: eulerian_mask_kernel
    "C21CM_EUL_BAND=0": ((0, 11), (7, 8, 13, 14), "none", True),  # c21hip_split_z_xe_mask on a dense f_coll grid
    "C21CM_EUL_BAND_SHIFT=0.2": ((0, 11), (7, 8, 13, 14), "miss", True),
}


def other_route(api, gpu_lib, capfd, monkeypatch, name, switch, want):
    ran, not_ran, want_band, r0_fused = want
    key, value = switch.split("=")
    out, counts, band, case = run(api, gpu_lib, capfd, monkeypatch, name, {key: value})
    check(name, case, out, counts, band, f" ({switch})")
    assert_route(counts, band, ran, not_ran, want_band)
    assert bool(int(out["loop_flags"]) & 64) == r0_fused


@pytest.mark.parametrize("switch", list(E_VARIANTS))
def test_other_routes_of_the_512_box(api, gpu_lib, capfd, monkeypatch, switch):
    """e-64x512 off its default route, each route held to the restatement itself (the banded-equals-dense tests
    of test_gpu_ionize.py compare the routes with one another)."""
    other_route(api, gpu_lib, capfd, monkeypatch, "e-64x512", switch, E_VARIANTS[switch])


@pytest.mark.parametrize("switch", list(EX_VARIANTS))
def test_other_routes_of_the_512_box_with_xe(api, gpu_lib, capfd, monkeypatch, switch):
    other_route(api, gpu_lib, capfd, monkeypatch, "ex-64x512", switch, EX_VARIANTS[switch])
