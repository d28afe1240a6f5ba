"""The six per-cell shell sums of ComputeTsBox (SpinTemperatureBox.c:1541-1784), kernel by kernel,
against the CPU oracle's fp64 sums.

ts_kernels.hip holds three generations of the shell loop and three box-sum kernels; which one runs
depends on C21CM_TS_LOOP, on the parity / alignment of the arrays, on the source mode and on the number
of shells.  Every case here sets the environment, calls c21cm_ts_shell_sums and ASSERTS THE ROUTE the
launchers report (c21hip_ts_last_route), so that no case can silently test another kernel; then all six
rows are compared with the oracle's `acc` array over every cell (the special cells of ts_helpers.make
included).

Tolerance, per cell and sum, scaled by S = sum over shells of |addend| (oracle, abs_sums):
  * Lagrangian grids: both sides are fp64 arithmetic on the same float inputs, <= ~6 roundings per term
    and <= 128 accumulations, ~1.5e-14 in all  ->  |got - ref| <= 1e-12 S.
  * table modes (v1, v2, v3): the source term is a float upstream (del_fcoll_Rct), so the yardstick is
    the float resolution of that term  ->  |got - ref| <= 4 * 2^-23 S (4 float ulps; the factor is the
    convention of the pass-X window tests and covers the 2.5 ulp of the fp32 lookup chain plus the
    rounding flip against the oracle's own narrowing to float).
Where S = 0 (a cell no shell reaches, row 0 without X-ray heating) the sum must be exactly zero.
The largest measured error / bound per route family is tabulated in DESIGN.md (Appendix C2)."""

import functools
import importlib

import numpy as np
import pytest

import ts_helpers as H

pytestmark = pytest.mark.gpu
S = importlib.import_module("21cmfast_amd.structs")

TOL_GRIDS = 1e-12
TOL_TABLES = 4 * 2.0 ** -23

MODES = {"grids": dict(lagrangian=True), "sfrd": dict(lagrangian=False),
         "fcoll": dict(lagrangian=False, fcoll_tables=True)}
MODE_ID = {"grids": 0, "sfrd": 1, "fcoll": 2}
# (n, nz): n x n x nz cells
DIV4 = (12, 14)   # 2016 cells, divisible by 4
ODD = (11, 13)    # 1573 cells, odd
REM2 = (9, 14)    # 1134 cells, even, remainder 2
MAX_V3_SHELLS = 70  # 70 shells: 162680 of 163840 bytes of LDS; 71 would need 165004


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def expected_route(env, mode, ntot, n_step, aligned=True):
    """The kernel a case is meant to test, restated from the launchers' conditions."""
    m = MODE_ID[mode]
    cells = 2 if (ntot % 2 == 0 and aligned) else 1
    if env == "v1":
        loop = 1
    elif env == "v2" or m == 0 or cells == 1 or n_step > MAX_V3_SHELLS:
        loop = 2
    else:
        loop = 3
    if m == 0:
        box_sum = None
    elif ntot % 4 or not aligned:
        box_sum = "scalar"
    elif env == "v1":
        box_sum = "float4"
    else:
        box_sum = "sfrd_sum2"
    return {"loop": loop, "cells": cells, "mode": m, "box_sum": box_sum}


def kernel_names(route):
    """The instantiations of ts_kernels.hip a route launches."""
    loop, cells, m = route["loop"], route["cells"], route["mode"]
    names = {{1: f"ts_accumulate_kernel<{cells}>", 2: f"ts_accumulate2_kernel<{cells},{m}>",
              3: f"ts_accumulate3_kernel<{m}>"}[loop]}
    if route["box_sum"] == "scalar":
        names.add("sfrd_sum_kernel/scalar")
    elif route["box_sum"] == "float4":
        names.add("sfrd_sum_kernel/float4")
    elif route["box_sum"] == "sfrd_sum2":
        names.add(f"sfrd_sum2_kernel<{'true' if m == 1 else 'false'}>")
    return names


@functools.lru_cache(maxsize=3)
def workload(box, n_step, mode, xray_heating=True, lya_heating=True, skew=False):
    """(spec, inputs, oracle result with sums / abs_sums): computed once per workload and shared by the
    cases that differ only in the kernel they route to; nothing in it is modified afterwards."""
    oracle = importlib.import_module("oracle.oracle")
    n, nz = box
    spec, d = H.make(n=n, hii_dim_z=nz, n_step=n_step, xray_heating=xray_heating,
                     lya_heating=lya_heating, dark_shells=2 if n_step > 2 else 0, skew=skew,
                     **MODES[mode])
    ref = oracle.ts_shell_sums(spec, d["density"], d["previous"], d["source"], d["filtered_density"])
    return spec, d, ref


def on_device(x, offset=0):
    """A CUDA copy of a numpy array (or dict of arrays); offset = 1: a view that starts one float into
    its allocation, i.e. 4 bytes past a 16-byte boundary."""
    import torch

    if x is None:
        return None
    if isinstance(x, dict):
        return {k: on_device(v, offset) for k, v in x.items()}
    if not offset:
        return torch.from_numpy(x).cuda()
    buf = torch.empty(x.size + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
    return view


def run(api, monkeypatch, env, spec, d, offset=0):
    if env is None:
        monkeypatch.delenv("C21CM_TS_LOOP", raising=False)
    else:
        monkeypatch.setenv("C21CM_TS_LOOP", env)
    sums = api.ts_shell_sums(spec, on_device(d["density"], offset), on_device(d["previous"], offset),
                             on_device(d["source"], offset), on_device(d["filtered_density"], offset))
    return sums, api.ts_last_route()


def check(sums, ref, mode, label, rows=6):
    got = sums.cpu().numpy()
    assert np.isfinite(got[:rows]).all(), label
    assert np.isnan(got[rows:]).all(), label  # rows the loop does not own stay untouched
    tol = TOL_GRIDS if mode == "grids" else TOL_TABLES
    err = np.abs(got[:rows] - ref["sums"][:rows])
    bound = tol * ref["abs_sums"][:rows]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    worst = ratio.max(axis=1)
    print(f"TS-SUMS {label}: max error/bound per row {np.array2string(worst, precision=3)}")
    assert ref["abs_sums"][1].min() >= 0 and ref["abs_sums"][1].max() > 0
    for row in range(rows):
        cell = int(ratio[row].argmax())
        assert worst[row] <= 1.0, (f"{label}: row {row} cell {cell}: got {got[row, cell]!r}, oracle "
                                   f"{ref['sums'][row, cell]!r}, error / bound {worst[row]:.3g}")
    return got


# ---------------------------------------------------------------------------------- route matrix
MATRIX = [(env, mode, box) for box in (DIV4, ODD, REM2) for mode in MODES for env in (None, "v2", "v1")]


@pytest.mark.parametrize("env,mode,box", MATRIX, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_route_matrix(api, monkeypatch, env, mode, box):
    spec, d, ref = workload(box, 12, mode)
    ntot = box[0] * box[0] * box[1]
    sums, route = run(api, monkeypatch, env, spec, d)
    assert route == expected_route(env, mode, ntot, 12)
    check(sums, ref, mode, f"matrix {env} {mode} {ntot} {sorted(kernel_names(route))}")


def test_route_matrix_reaches_every_instantiation():
    """The matrix above (whose cases assert these routes on the device) names every shell-loop and
    box-sum instantiation of ts_kernels.hip at least once."""
    seen = set()
    for env, mode, box in MATRIX:
        seen |= kernel_names(expected_route(env, mode, box[0] * box[0] * box[1], 12))
    want = {f"ts_accumulate_kernel<{c}>" for c in (1, 2)}
    want |= {f"ts_accumulate2_kernel<{c},{m}>" for c in (1, 2) for m in (0, 1, 2)}
    want |= {"ts_accumulate3_kernel<1>", "ts_accumulate3_kernel<2>", "sfrd_sum_kernel/scalar",
             "sfrd_sum_kernel/float4", "sfrd_sum2_kernel<true>", "sfrd_sum2_kernel<false>"}
    assert seen == want


# ---------------------------------------------------------------------------------- skewed table ranges
SKEWED = [(env, mode, box, n_step) for n_step in (2, 12) for mode in ("sfrd", "fcoll")
          for env, box in ((None, DIV4), ("v2", DIV4), (None, ODD))]


@pytest.mark.parametrize("env,mode,box,n_step", SKEWED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_skewed_table_range(api, monkeypatch, env, mode, box, n_step):
    """Filtered densities of a real box are skewed: delta g from -0.9 to ~8, so the table's first knot sits
    40 - 85 bins from delta = 0 (off = 40 .. 85) while the dense cells, which carry most of the star formation, sit
    in bins 300 - 398.  The symmetric Gaussian workloads (off ~ 200, |off - idx| <= 200) cannot tell an
    fp32 bin weight that is exact only within off's binade from one that is exact everywhere; here
    off - idx reaches -358, and the tables move by up to 9 % per bin.  Two shells as well as twelve: with
    few shells a cell's error is that of single terms."""
    spec, d, ref = workload(box, n_step, mode, skew=True)
    ntot = box[0] * box[0] * box[1]
    g, fd = np.array(spec.zpp_growth[:n_step]), d["filtered_density"].reshape(n_step, -1)
    off = -np.array(spec.tab_min[:n_step]) / np.array(spec.tab_width[:n_step])
    top = ((fd * g[:, None] - np.array(spec.tab_min[:n_step])[:, None]) / np.array(spec.tab_width[:n_step])[:, None]) > 300
    # the premise of this case: off - idx leaves off's binade (off in 32 .. 128, idx beyond 300)
    assert 32 < off.min() and off.max() < 128 and top.mean() > 0.05
    lost = [abs(float(np.float32(o) - np.float32(398)) - (float(np.float32(o)) - 398)) for o in off]
    assert max(lost) > 7e-6  # ... where a float cannot hold it: >= 7e-6 bins lost in some shell
    sums, route = run(api, monkeypatch, env, spec, d)
    assert route == expected_route(env, mode, ntot, n_step)
    check(sums, ref, mode, f"skewed n_step={n_step} {env} {mode} {ntot} {sorted(kernel_names(route))}")


# ---------------------------------------------------------------------------------- shell-count edges
EDGES = [(mode, box, n_step) for box in (DIV4, ODD) for mode in MODES
         for n_step in ((1, 128) if mode == "grids" else (1, 2, 70, 71, 128))]


@pytest.mark.parametrize("mode,box,n_step", EDGES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_shell_count_edges(api, monkeypatch, mode, box, n_step):
    """n_step = 1: the prefetch never fires; 70: the last count v3 holds in LDS; 71: the first that
    falls back to v2; 128: C21CM_MAX_TS_RADII."""
    spec, d, ref = workload(box, n_step, mode)
    ntot = box[0] * box[0] * box[1]
    sums, route = run(api, monkeypatch, None, spec, d)
    assert route == expected_route(None, mode, ntot, n_step)
    if mode != "grids" and box == DIV4:
        assert route["loop"] == (3 if n_step <= 70 else 2)
    check(sums, ref, mode, f"edge n_step={n_step} {mode} {ntot} {sorted(kernel_names(route))}")


# ---------------------------------------------------------------------------------- second trips
# Launch caps (items): v3 256 x 1024 = 262144 (two cells each); the other shell loops 2048 x 256 = 524288
# (one or two cells each); sfrd_sum2 / sfrd_sum float4 512 x 256 = 131072 (four cells each); scalar box
# sum 131072 cells.
SECOND_TRIP = [
    # 82^3 = 551368 cells (divisible by 4).  v3: 275684 items, 2 trips (last: 13540 items, 228 in its
    # last workgroup); sfrd_sum2: 137842 items, 2 trips (last: 6770 items).
    (None, "sfrd", (82, 82)),
    (None, "fcoll", (82, 82)),
    # 81^3 = 531441 cells (odd): one cell per thread.  ts_accumulate2<1,*> / ts_accumulate<1>: 531441
    # items, 2 trips (last: 7153 items, 241 in its last workgroup); scalar box sum: 5 trips (last: 7153).
    (None, "grids", (81, 81)),
    (None, "sfrd", (81, 81)),
    (None, "fcoll", (81, 81)),
    ("v1", "sfrd", (81, 81)),
    # 102^3 = 1061208 cells (divisible by 4): two cells per thread, 530604 items, 2 trips (last: 6316
    # items, 172 in its last workgroup) for ts_accumulate2<2,*> and ts_accumulate<2>; sfrd_sum2 and the
    # float4 branch of sfrd_sum: 265302 items, 3 trips (last: 3158 items).
    (None, "grids", (102, 102)),
    ("v2", "sfrd", (102, 102)),
    ("v2", "fcoll", (102, 102)),
    ("v1", "fcoll", (102, 102)),
]


@pytest.mark.parametrize("env,mode,box", SECOND_TRIP, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_grid_stride_loops_take_a_second_partial_trip(api, monkeypatch, env, mode, box):
    spec, d, ref = workload(box, 4, mode)
    ntot = box[0] * box[0] * box[1]
    sums, route = run(api, monkeypatch, env, spec, d)
    assert route == expected_route(env, mode, ntot, 4)
    items = ntot // route["cells"]
    cap, group = (256 * 1024, 1024) if route["loop"] == 3 else (2048 * 256, 256)
    assert items > cap and items % cap and items % group  # a second, partial trip; a partial workgroup
    if route["box_sum"]:
        sum_items = ntot if route["box_sum"] == "scalar" else ntot // 4
        assert sum_items > 512 * 256 and sum_items % (512 * 256) and sum_items % 256
    check(sums, ref, mode, f"second-trip {env} {mode} {ntot} {sorted(kernel_names(route))}")


# ---------------------------------------------------------------------------------- misaligned arrays
@pytest.mark.parametrize("env,mode", [(None, "grids"), (None, "sfrd"), (None, "fcoll"), ("v1", "sfrd")])
def test_arrays_offset_by_one_float(api, monkeypatch, env, mode):
    """Device arrays that start 4 bytes past a 16-byte boundary, cell count divisible by 4: one cell per
    thread and the scalar box sum (no 8- or 16-byte load may touch them)."""
    spec, d, ref = workload(DIV4, 12, mode)
    ntot = DIV4[0] * DIV4[0] * DIV4[1]
    sums, route = run(api, monkeypatch, env, spec, d, offset=1)
    assert route == expected_route(env, mode, ntot, 12, aligned=False)
    assert route["cells"] == 1 and route["box_sum"] in (None, "scalar")
    got = check(sums, ref, mode, f"misaligned {env} {mode} {sorted(kernel_names(route))}")
    if mode == "grids":  # the same fp64 operations per cell, one or two cells per thread
        aligned, route2 = run(api, monkeypatch, env, spec, d)
        assert route2["cells"] == 2
        np.testing.assert_array_equal(got, aligned.cpu().numpy())


# ---------------------------------------------------------------------------------- switches
@pytest.mark.parametrize("env,mode", [(None, "grids"), (None, "sfrd"), ("v2", "fcoll"), ("v1", "sfrd")])
def test_switches(api, monkeypatch, env, mode):
    """use_xray_heating = 0 leaves row 0 at zero; use_lya_heating = 0 leaves rows 4 and 5 untouched."""
    ntot = DIV4[0] * DIV4[0] * DIV4[1]
    spec, d, ref = workload(DIV4, 12, mode, xray_heating=False)
    sums, route = run(api, monkeypatch, env, spec, d)
    assert route == expected_route(env, mode, ntot, 12)
    got = check(sums, ref, mode, f"no-xray-heating {env} {mode}")
    assert (got[0] == 0).all() and (got[1] > 0).any()
    spec, d, ref = workload(DIV4, 12, mode, lya_heating=False)
    sums, route = run(api, monkeypatch, env, spec, d)
    assert route == expected_route(env, mode, ntot, 12)
    check(sums, ref, mode, f"no-lya-heating {env} {mode}", rows=4)
