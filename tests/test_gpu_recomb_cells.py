"""What the radius loop decides WITH a recombination model, cell by cell, against the float64 restatement of
tests/recomb_excursion_reference.py (pinned to the CPU oracle and held to its caps by
test_excursion_reference_host.py).

Per case the device gives the single pass (api.ionize_grids, device-resident inputs) on each route listed in
ROUTES -- the fused recombination loop and, with C21CM_RECOMB_FUSED=0, the unfused sequence of the same box,
each against float64 instead of against each other -- and the world = 1 shard pair (the (first crossing,
Gamma_12) phases where api.shard_rc_supported, else the key phases), which must equal the single pass bit for
bit in all six output grids.  recomb_excursion_reference.check_recomb_outputs holds every route to:
  * mean_free_path is 0 or float(R[r]) exactly: that names the device's crossing index;
  * the decided crossing flag on EVERY flag-decided cell, the decided first-crossing radius on every
    radius-decided cell; elsewhere one of the two candidates (+t, -t) or, on the handful of cells where the
    reference finds one, a radius between the two whose float64 margin lies within t of the barrier too;
  * Gamma_12 == 0 exactly without a crossing; at a crossing within 4 x E32['gamma'] relative plus 4 x
    E32['gamma_abs'] of the largest Gamma_12, at the radius the device's own mean_free_path names;
  * z_reion == float(redshift), the previous z_reion where that is >= 0, or -1: exact;
  * x_HI == 0 on crossing cells; on decided non-crossing cells within 4 x the float32-vs-float64 deviation of
    the radius-0 expression (no rec term);
  * report.f_coll_grid_mean[r] within 4 x the float32 chain's largest relative deviation;
  * cumulative_recombinations within 1 float ulp of the float64 rate of the device's OWN Gamma_12 and x_HI
    (inhomogeneous), or within the span of the float neighbours of the two global means plus 1 ulp
    (homogeneous).
t = 4 E32; every E32 figure is measured on the reference side per case and printed.  No bound here is typed in
from a run of the device.

Each case and route prints one line RECOMB-EXCURSION.  A restatement is computed
once per process (recomb_excursion_reference.restated) and shared by the routes."""

import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import excursion_reference as X  # noqa: E402
import recomb_excursion_reference as RX  # noqa: E402

pytestmark = pytest.mark.gpu

SIX = ("neutral_fraction", "z_reion", "kinetic_temperature", "ionisation_rate_G12", "mean_free_path",
       "cumulative_recombinations")

# case -> (native passes?, fused recombination loop by default?).  Loop flags as in
# grid_api.ionize_last_loop_flags: 2 fused recombination loop, 4 third spectrum in the barrier kernel, 8 ...
# which is the filtered N_rec, 16 a fourth spectrum, 32 two radii per sweep.
ROUTES = {
    "r1": (True, True),    # c21hip_split_z_ionise with recomb: whalo_sfr as third spectrum, dense N_rec rows
    "r2": (True, True),    # ..._recomb_nrec
    "r3": (True, True),    # ..._recomb_xe, homogeneous
    "r4": (True, True),    # ..._recomb_xe_nrec: four spectra, 512-point z-lines
    "u-64": (True, False),   # 64-point z-lines: native passes, ionise_recomb_kernel on all five grids
    "u-50": (False, False),  # rocFFT
    "e-64": (True, False),   # Eulerian
}
assert set(ROUTES) == set(RX.CASES)
FUSED = [k for k, v in ROUTES.items() if v[1]]


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


@pytest.fixture(scope="module")
def on_device():
    """case -> (density, keyword inputs) as CUDA tensors, uploaded once."""
    import torch

    cache = {}

    def get(name):
        if name not in cache:
            inp = RX.restated(name).inp
            cache[name] = (torch.from_numpy(np.array(inp.density)).cuda(),
                           {k: torch.from_numpy(np.array(v)).cuda() for k, v in inp.kwargs().items()})
        return cache[name]

    return get


def single_pass(api, spec, density, kw):
    import torch

    buf, _, rep = api.ionize_grids(spec, density, **kw)
    flags = api.ionize_last_loop_flags()
    torch.cuda.synchronize()
    out = {k: getattr(buf, k).cpu().numpy() for k in RX.GRIDS}
    out["f_coll_grid_mean"] = np.array(rep.f_coll_grid_mean[:spec.n_radii], np.float64)
    return buf, out, flags


def check(name, route, out, flags):
    c = RX.restated(name)
    fig = RX.check_recomb_outputs(c.ref, out)
    print(RX.recomb_line(f"{name} ({route})", c.ref, c.e, fig) + f", loop flags {flags} (bits 8 / 32: "
          f"{int(bool(flags & 8))} / {int(bool(flags & 32))}), host {c.host_seconds:.0f} s")
    assert c.ref.flag_undecided_share <= X.FLAG_CAP and c.ref.radius_undecided_share <= X.RADIUS_CAP


@pytest.mark.parametrize("name", list(RX.CASES))
def test_every_decided_cell_default_route(api, gpu_lib, on_device, name):
    """The route a caller gets, and the world = 1 shard pair against it."""
    import torch

    c = RX.restated(name)
    spec, (density, kw) = c.spec, on_device(name)
    native, fused = ROUTES[name]
    assert bool(gpu_lib.c21hip_fft_is_native(*c.inp.density.shape)) == native
    buf, out, flags = single_pass(api, spec, density, kw)
    if fused:
        ts, cell = bool(spec.use_ts_fluct), bool(spec.cell_recomb)
        assert flags & 2, flags  # the fused recombination loop ran
        assert bool(flags & 4) == (ts or not cell) and bool(flags & 16) == (ts and not cell), flags
    else:
        assert flags & 3 == 0, flags
    check(name, "fused" if fused else "default", out, flags)
    # single pass == the world = 1 shard pair, bit for bit
    if api.shard_rc_supported(spec):
        fc = torch.empty(density.numel(), dtype=torch.uint8, device="cuda")
        g = torch.empty(density.numel(), dtype=torch.float32, device="cuda")
        api.ionize_shard_radii_rc(spec, 0, 1, fc, g, density, **kw)
        buf2, _, rep2 = api.ionize_shard_finish_rc(spec, fc, g, density, **kw)
        pair = "rc"
    else:
        keys = torch.zeros(density.shape, dtype=torch.int64, device="cuda")
        api.ionize_shard_radii_keys(spec, 0, 1, keys, density, **kw)
        buf2, _, rep2 = api.ionize_shard_finish_keys(spec, keys, density, **kw)
        pair = "keys"
    torch.cuda.synchronize()
    for grid in SIX:
        assert torch.equal(getattr(buf, grid), getattr(buf2, grid)), (name, pair, grid)
    print(f"{name}: single pass == world = 1 shard pair ({pair}) in all six grids")


@pytest.mark.parametrize("name", FUSED)
def test_every_decided_cell_unfused_sequence(api, on_device, monkeypatch, name):
    """The same boxes through the per-radius sequence (C21CM_RECOMB_FUSED=0, read per call), held to the same
    restatement."""
    spec, (density, kw) = RX.restated(name).spec, on_device(name)
    monkeypatch.setenv("C21CM_RECOMB_FUSED", "0")
    _, out, flags = single_pass(api, spec, density, kw)
    assert flags & 3 == 0, flags
    check(name, "C21CM_RECOMB_FUSED=0", out, flags)
