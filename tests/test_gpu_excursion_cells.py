"""What the excursion-set loop decides, cell by cell, against the float64 restatement of
tests/excursion_reference.py (pinned to the CPU oracle and held to its caps by
test_excursion_reference_host.py).

Per case the device gives the single pass (api.ionize_grids, device-resident) and the world = 1 shard pair
(api.ionize_shard_radii -> first_cross, api.ionize_shard_finish); excursion_reference.check_outputs holds
them to:
  * the decided flag on EVERY flag-decided cell (x_HI == 0; first_cross != 0 or the radius-0 outcome);
  * the decided first-crossing radius on every radius-decided cell, exactly;
  * one of the two candidates (+t, -t), never a third value, on the undecided cells;
  * single pass == shard pair, cell for cell (this carries the crossing-bit path into the radius check);
  * z_reion == redshift exactly where decided ionised, -1 where decided neutral;
  * x_HI on decided-neutral cells within 4 x the deviation of a float32 numpy evaluation of the radius-0
    expression from the float64 one.  Measured bounds (4 x): 5.6e-7 ... 5.8e-7 in modes (a) and (b) -- three
    float operations at x_HI ~ 1 -- and 4.9e-6 (64^3), see DESIGN.md Appendix C, in mode (c), whose
    erfc polynomial and exponential are a few dozen;
  * report.f_coll_grid_mean[r] within 4 x the float32 chain's largest relative deviation from the float64
    mean (bounds 2.9e-7 ... 7.4e-7).
t = 4 E32, E32 = the largest |m32 - m64| of the margin over cells and radii, reference side only.

Each case prints one line EXCURSION.  The restatement of a case is computed once
(module-scoped) and shared with the two child-process variants of the 64 x 64 x 512 box."""

import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import excursion_reference as X  # noqa: E402

pytestmark = pytest.mark.gpu

W = importlib.import_module("21cmfast_amd.workloads")
load = importlib.import_module("21cmfast_amd").load

# case -> (native passes?, loop flags that must be set, loop flags that must be clear); flags as in
# grid_api.ionize_last_loop_flags: 1 fused loop, 4 third spectrum (x_e) in the barrier kernel, 32 two radii
# per pass-X sweep
ROUTES = {
    "a-64": (True, 1 | 32, 2 | 4),       # 33 radii: pairs plus one lone radius
    "a-64x512": (True, 1 | 32, 2 | 4),   # the fused pass Z with crossing bits
    "a-64x256": (True, 1 | 32, 2 | 4),   # the other wave-level z length
    "a-50": (False, 0, 1),               # rocFFT route, odd factors: the per-radius driver path
    "a-192x64": (True, 1 | 32, 2 | 4),   # radix-3 x / y lines
    "a-128": (True, 1 | 32, 2 | 4),      # second trips of passes X / Y; windows evaluated from node tables
    "b-64x512": (True, 1 | 4 | 32, 2),   # three-grid fused pass Z
    "b-64": (True, 0, 1 | 2),            # 64-point z-lines have no three-grid pass Z: native passes, unfused loop
    "c-64": (True, 0, 1 | 2 | 4),        # erfc epilogue of pass Z, sharp-k window, mean fix (the Eulerian
    "c-64x512": (True, 0, 1 | 2 | 4),    # loops set no flag)
}
assert set(ROUTES) == set(X.CASES)


def device_outputs(api, spec, inp):
    """The single pass and the world = 1 shard pair on device-resident inputs, as numpy arrays."""
    import torch

    def dev(a):
        return None if a is None else torch.from_numpy(np.array(a)).cuda()

    density, n_ion = dev(inp.density), dev(inp.n_ion)
    kw = {k: dev(v) for k, v in inp.kwargs().items()}
    buf, _, rep = api.ionize_grids(spec, density, n_ion, **kw)
    flags = api.ionize_last_loop_flags()
    fc = torch.zeros(inp.density.shape, dtype=torch.uint8, device="cuda")
    api.ionize_shard_radii(spec, 0, 1, fc, density, n_ion, **kw)
    buf2, _, _ = api.ionize_shard_finish(spec, fc, density, n_ion, **kw)
    torch.cuda.synchronize()
    return {"neutral_fraction": buf.neutral_fraction.cpu().numpy(), "z_reion": buf.z_reion.cpu().numpy(),
            "first_cross": fc.cpu().numpy(), "shard_neutral_fraction": buf2.neutral_fraction.cpu().numpy(),
            "shard_z_reion": buf2.z_reion.cpu().numpy(),
            "f_coll_grid_mean": np.array(rep.f_coll_grid_mean[:spec.n_radii], np.float64),
            "loop_flags": np.int64(flags),
            # what the two process-wide switches of pass Z leave of the default route on this box
            "wave_pass_z": np.int64(load().c21hip_z_ionise_xe_supported(*inp.density.shape)),
            "cross_bits": np.int64(load().c21hip_z_cross_bits_supported(*inp.density.shape))}


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


@pytest.fixture(scope="module")
def restated():
    """case -> (spec, inputs, Restatement, e32 dict): the float64 host loop, once per case."""
    cache = {}

    def get(name):
        if name not in cache:
            spec, inp = X.make_case(W, *X.CASES[name])
            cache[name] = (spec, inp) + X.restate(spec, inp)
        return cache[name]

    return get


def check(name, ref, e, out, variant=""):
    fig = X.check_outputs(ref, out)
    print(X.excursion_line(name + variant, ref, e, fig) + f", loop flags {int(out['loop_flags'])}")
    assert ref.flag_undecided_share <= X.FLAG_CAP and ref.radius_undecided_share <= X.RADIUS_CAP


@pytest.mark.parametrize("name", list(X.CASES))
def test_every_decided_cell(api, gpu_lib, restated, name):
    spec, inp, ref, e = restated(name)
    native, flags_set, flags_clear = ROUTES[name]
    assert bool(gpu_lib.c21hip_fft_is_native(*inp.density.shape)) == native
    out = device_outputs(api, spec, inp)
    flags = int(out["loop_flags"])
    print(f"{name}: native passes {native}, loop flags {flags}")
    assert flags & flags_set == flags_set and not flags & flags_clear, flags
    check(name, ref, e, out)


@pytest.mark.parametrize("switch,value,wave_pass_z", [("C21CM_ZPASS", "tile", 0), ("C21CM_CROSS_BITS", "0", 1)])
def test_other_pass_z_routes_of_the_512_box(gpu_lib, restated, tmp_path, switch, value, wave_pass_z):
    """The 64 x 64 x 512 box through the tile version of pass Z, and on the uint8 mask instead of the
    crossing bits.  Both switches are read once per process: a child runs the device, this process checks --
    also that the child's library saw the switch: the wave-level pass Z is off under the first only, the
    crossing bits under both, and here neither is."""
    name = "a-64x512"
    assert switch not in os.environ
    path = tmp_path / "outputs.npz"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), name,
                                                                           str(path)]
    subprocess.run(cmd, check=True, env=dict(os.environ, **{switch: value}), cwd=str(ROOT), timeout=300)
    with np.load(path) as f:
        out = {k: f[k] for k in f.files}
    spec, inp, ref, e = restated(name)
    assert int(out["loop_flags"]) & 1
    assert (int(out["wave_pass_z"]), int(out["cross_bits"])) == (wave_pass_z, 0)
    assert gpu_lib.c21hip_z_ionise_xe_supported(64, 64, 512) == 1 and gpu_lib.c21hip_z_cross_bits_supported(64, 64, 512) == 1
    check(name, ref, e, out, f" ({switch}={value})")


if __name__ == "__main__":  # the child of test_other_pass_z_routes_of_the_512_box: <case> <npz path>
    importlib.import_module("21cmfast_amd").load(require_gpu=True)
    case_spec, case_inp = X.make_case(W, *X.CASES[sys.argv[1]])
    np.savez(sys.argv[2], **device_outputs(importlib.import_module("21cmfast_amd.grid_api"), case_spec, case_inp))
