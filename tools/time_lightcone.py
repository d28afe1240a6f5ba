"""Time run_lightcone on the device and the lightcone kernels by themselves (GPU box only).

(1) For each HII_DIM and with / without USE_TS_FLUCT: a device-resident run_lightcone (E-INTEGRAL,
    BOX_LEN = 1.5 HII_DIM, DIM = 2 HII_DIM, nodes from Z_HEAT_MAX = 35 down to z_end, ZPRIME_STEP_FACTOR
    apart, the lightcone from the lowest node + 0.2 to the highest - 0.2 at the cell size, five
    fields) with the slab and dv/dr calls timed (host tables, launch and the synchronisation that
    ends each call included), their share of the run, the bytes the kernels move by contract
    (12 B per lightcone cell and field for the slabs, 12 / 16 B per cell for dv/dr) and the
    lightcone's footprint.
(2) The slab kernel alone at HII_DIM = 512 (5 fields, runs of 8 .. 256 slices, HII_D_PARA = 512)
    and the dv/dr kernel over a 512^2 x 1024 lightcone, timed with events over repeated launches.

(3) With --rsds: the runs of (1) with apply_rsds=True, the redshift-space shift of every lightcone
    timed as (1) times the slabs and its share of the run; then the RSD kernel alone over 256^2 and
    512^2 columns of 2000 and 4000 slices with 1 and 3 fields (4 sub-cells, not periodic), its
    contract (4 B of velocity + 8 B per field and cell) against the time of one call.

(4) With --angular ORDERS (e.g. 1,3): for each HII_DIM the run of (1) without USE_TS_FLUCT, with
    KEEP_3D_VELOCITIES and the fields density, neutral_fraction, brightness_temp (+ los_velocity for
    dv/dr), once rectilinear and once per order with a like_rectilinear AngularLightconer (n_pix =
    HII_DIM^2: the same output cells).  The assembly calls (slabs; angular sampling and the spline
    prefilter) are timed as (1) times the slabs, with the bytes of the taps the sampling reads (8 B per
    tap and component: both node boxes) plus 4 B per stored cell, the prefilter's 16 B per cell, pole and
    axis (two passes that read and write the line), and the HBM the kept coefficients take.

    python tools/time_lightcone.py [--sizes 256,512] [--z-end 6] [--step 1.02] [--rsds] [--angular 1,3]
                                   [--out FILE]
Run it under rocprofv3 --kernel-trace --stats for the kernel table.
"""
import argparse
import importlib
import json
import pathlib
import sys
import time

import numpy as np
import torch

root = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
pkg = importlib.import_module("21cmfast_amd")
DATA = root / "tests" / "golden" / "reference" / "_data"
FIELDS = ("density", "velocity_z", "neutral_fraction", "z_reion", "brightness_temp")

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="256,512")
ap.add_argument("--ts", default="0,1")
ap.add_argument("--z-end", type=float, default=6.0)
ap.add_argument("--step", type=float, default=1.02)
ap.add_argument("--skip-runs", action="store_true")
ap.add_argument("--rsds", action="store_true")
ap.add_argument("--angular", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lib = pkg.load(require_gpu=True)

if args.angular:  # ---- (4) rectilinear against angular assembly
    ANG_FIELDS = ("density", "neutral_fraction", "brightness_temp")
    tm = {"assembly_s": 0.0, "calls": 0, "tap_bytes": 0, "prefilter_s": 0.0, "prefilter_bytes": 0,
          "coef_boxes": 0}
    _ang, _pre, _sl = api.lightcone_angular, api.spline_prefilter, api.lightcone_slices

    def t_ang(lightcones, box_lo, box_hi, i0, distance, *a, order=1, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _ang(lightcones, box_lo, box_hi, i0, distance, *a, order=order, **kw)
        torch.cuda.synchronize()
        tm["assembly_s"] += time.perf_counter() - t0
        tm["calls"] += 1
        taps = (order + 1) ** 3
        comps = sum(len(v) if isinstance(v, tuple) else 1 for v in box_lo.values())
        n_pix = next(iter(lightcones.values())).shape[0]
        tm["tap_bytes"] += n_pix * len(distance) * (8 * taps * comps + 4 * len(lightcones))

    def t_pre(boxes, order, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = _pre(boxes, order, *a, **kw)
        torch.cuda.synchronize()
        tm["prefilter_s"] += time.perf_counter() - t0
        cells = next(iter(boxes.values())).numel()
        tm["prefilter_bytes"] += 16 * 3 * (1 if order == 3 else 2) * cells * len(boxes)
        tm["coef_boxes"] = len(boxes)
        return out

    def t_sl(lightcones, box_lo, box_hi, i0, plane, *a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _sl(lightcones, box_lo, box_hi, i0, plane, *a, **kw)
        torch.cuda.synchronize()
        tm["assembly_s"] += time.perf_counter() - t0
        tm["calls"] += 1
        first = next(iter(lightcones.values()))
        tm["tap_bytes"] += 12 * first.shape[0] * first.shape[1] * len(plane) * len(lightcones)

    api.lightcone_angular, api.spline_prefilter, api.lightcone_slices = t_ang, t_pre, t_sl
    res = {"runs": []}
    for n in (int(s) for s in args.sizes.split(",")):
        for kind in ["rectilinear"] + [f"angular_o{o}" for o in args.angular.split(",")]:
            for k in tm:
                tm[k] = 0
            inputs = D.Inputs(random_seed=12345, HII_DIM=n, DIM=2 * n, BOX_LEN=1.5 * n, SOURCE_MODEL=1,
                              USE_TS_FLUCT=False, USE_LYA_HEATING=False, HII_FILTER=0, USE_EXP_FILTER=False,
                              CELL_RECOMB=False, R_BUBBLE_MAX=30.0, ZPRIME_STEP_FACTOR=args.step,
                              Z_HEAT_MAX=35.0, N_THREADS=16, KEEP_3D_VELOCITIES=True)
            nodes = D.get_logspaced_redshifts(args.z_end, args.step, 35.0)
            z0, z1 = nodes[-1] + 0.2, nodes[0] - 0.2
            if kind == "rectilinear":
                lc = D.RectilinearLightconer.between_redshifts(z0, z1, 1.5, quantities=ANG_FIELDS)
            else:
                lc = D.AngularLightconer.like_rectilinear(inputs.simulation_options, z0, z1, quantities=ANG_FIELDS,
                                                          interpolation_order=int(kind[-1]))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = D.run_lightcone(inputs, lc, nodes, data_path=DATA, device="cuda", lib=lib)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            box_gb = n * n * n * 4 / 1e9
            row = {"hii_dim": n, "kind": kind, "n_nodes": len(nodes), "n_slices": len(lc.lc_distances),
                   "lightcone_fields": sorted(out["lightcones"]), "run_s": round(wall, 3),
                   "assembly_s": round(tm["assembly_s"], 4), "assembly_calls": tm["calls"],
                   "prefilter_s": round(tm["prefilter_s"], 4),
                   "share_of_run": round((tm["assembly_s"] + tm["prefilter_s"]) / wall, 5),
                   "assembly_GB": round(tm["tap_bytes"] / 1e9, 2),
                   "assembly_GBps_wall": round(tm["tap_bytes"] / max(tm["assembly_s"], 1e-12) / 1e9, 1),
                   "prefilter_GB": round(tm["prefilter_bytes"] / 1e9, 2),
                   "prefilter_GBps_wall": round(tm["prefilter_bytes"] / max(tm["prefilter_s"], 1e-12) / 1e9, 1),
                   # the coefficients of the current and the previous node of every box sampled
                   "coefficients_GB": round(2 * tm["coef_boxes"] * box_gb, 3),
                   "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3)}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
            del out
            torch.cuda.empty_cache()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0)

# ---- wrap the two lightcone calls of run_lightcone with wall-clock timers
acc = {"slab_s": 0.0, "slab_calls": 0, "slab_bytes": 0, "dvdr_s": 0.0, "dvdr_bytes": 0, "rsd_s": 0.0,
       "rsd_bytes": 0}
_slices, _dvdr, _rsd = api.lightcone_slices, api.lightcone_dvdr, api.rsd_shift


def timed_slices(lightcones, box_lo, box_hi, i0, plane, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _slices(lightcones, box_lo, box_hi, i0, plane, *a, **kw)
    torch.cuda.synchronize()
    acc["slab_s"] += time.perf_counter() - t0
    acc["slab_calls"] += 1
    first = next(iter(lightcones.values()))
    acc["slab_bytes"] += 12 * first.shape[0] * first.shape[1] * len(plane) * len(lightcones)


def timed_dvdr(bt, vel, hubble, dx, max_dvdr, tau_21=None, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _dvdr(bt, vel, hubble, dx, max_dvdr, tau_21=tau_21, **kw)
    torch.cuda.synchronize()
    acc["dvdr_s"] += time.perf_counter() - t0
    acc["dvdr_bytes"] += (16 if tau_21 is not None else 12) * bt.numel()


def timed_rsd(fields, vel, *a, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _rsd(fields, vel, *a, **kw)
    torch.cuda.synchronize()
    acc["rsd_s"] += time.perf_counter() - t0
    acc["rsd_bytes"] += (4 + 8 * len(fields)) * vel.numel()
    return out


api.lightcone_slices, api.lightcone_dvdr, api.rsd_shift = timed_slices, timed_dvdr, timed_rsd
res = {"runs": [], "kernels": {}}
if not args.skip_runs:
    for n in (int(s) for s in args.sizes.split(",")):
        for ts in (bool(int(t)) for t in args.ts.split(",")):
            for k in list(acc):
                acc[k] = 0
            inputs = D.Inputs(random_seed=12345, HII_DIM=n, DIM=2 * n, BOX_LEN=1.5 * n, SOURCE_MODEL=1,
                              USE_TS_FLUCT=ts, USE_LYA_HEATING=False, HII_FILTER=0, USE_EXP_FILTER=False,
                              CELL_RECOMB=False, R_BUBBLE_MAX=30.0, ZPRIME_STEP_FACTOR=args.step,
                              Z_HEAT_MAX=35.0, N_THREADS=16)
            nodes = D.get_logspaced_redshifts(args.z_end, args.step, 35.0)
            lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.2, nodes[0] - 0.2, 1.5, quantities=FIELDS)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = D.run_lightcone(inputs, lc, nodes, data_path=DATA, device="cuda", lib=lib, apply_rsds=args.rsds)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            n_lc = sum(v.numel() * 4 for v in out["lightcones"].values())
            row = {"hii_dim": n, "use_ts_fluct": ts, "n_nodes": len(nodes), "n_slices": len(lc.lc_distances),
                   "lightcone_fields": sorted(out["lightcones"]), "run_s": round(wall, 3),
                   "slab_s": round(acc["slab_s"], 4), "slab_calls": acc["slab_calls"],
                   "dvdr_s": round(acc["dvdr_s"], 4),
                   "share_of_run": round((acc["slab_s"] + acc["dvdr_s"]) / wall, 5),
                   "slab_contract_GB": round(acc["slab_bytes"] / 1e9, 3),
                   "slab_GBps_wall": round(acc["slab_bytes"] / max(acc["slab_s"], 1e-12) / 1e9, 1),
                   "dvdr_contract_GB": round(acc["dvdr_bytes"] / 1e9, 3),
                   "dvdr_GBps_wall": round(acc["dvdr_bytes"] / max(acc["dvdr_s"], 1e-12) / 1e9, 1),
                   "lightcone_GB": round(n_lc / 1e9, 3),
                   **({"rsd_s": round(acc["rsd_s"], 4), "rsd_share_of_run": round(acc["rsd_s"] / wall, 5),
                       "rsd_contract_GB": round(acc["rsd_bytes"] / 1e9, 3),
                       "rsd_GBps_wall": round(acc["rsd_bytes"] / max(acc["rsd_s"], 1e-12) / 1e9, 1)}
                      if args.rsds else {}),
                   "peak_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 3)}
            print(json.dumps(row), flush=True)
            res["runs"].append(row)
            del out
            torch.cuda.empty_cache()
api.lightcone_slices, api.lightcone_dvdr, api.rsd_shift = _slices, _dvdr, _rsd

if args.rsds:  # ---- the RSD kernel alone
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.Generator(device="cuda").manual_seed(2)
    for n in (256, 512):
        for n_s in (2000, 4000):
            vel = torch.randn((n, n, n_s), device="cuda", generator=g) * 1e-17
            scale = np.full(n_s, 2.0e17)  # ~2 pixels rms, as a lightcone at 1.5 Mpc cells
            for nf in (1, 3):
                fields = [torch.rand((n, n, n_s), device="cuda", generator=g) for _ in range(nf)]
                outs = [torch.empty_like(f) for f in fields]
                api.rsd_shift(fields, vel, scale, n_sub=4, out=outs)
                torch.cuda.synchronize()
                reps = 3
                ev0.record()
                for _ in range(reps):
                    api.rsd_shift(fields, vel, scale, n_sub=4, out=outs)
                ev1.record()
                torch.cuda.synchronize()
                ms = ev0.elapsed_time(ev1) / reps
                byt = (4 + 8 * nf) * n * n * n_s
                row = {"columns": n * n, "slices": n_s, "fields": nf, "ms_per_call": round(ms, 3),
                       "contract_MB": round(byt / 1e6, 1), "TBps_call": round(byt / ms / 1e9, 3)}
                print("rsd", json.dumps(row), flush=True)
                res["kernels"][f"rsd_{n}sq_{n_s}_f{nf}"] = row
                del fields, outs
            del vel
            torch.cuda.empty_cache()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0)

# ---- the kernels alone at 512
n, d_para, nf, reps = 512, 512, len(FIELDS), 10
g = torch.Generator(device="cuda").manual_seed(1)
lo = {k: torch.rand((n, n, d_para), device="cuda", generator=g) for k in FIELDS}
hi = {k: torch.rand((n, n, d_para), device="cuda", generator=g) for k in FIELDS}
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for run in (8, 32, 64, 128, 256):
    lcs = {k: torch.zeros((n, n, 2 * run), device="cuda") for k in FIELDS}
    plane = ((np.arange(run) + d_para - run // 2) % d_para).astype(np.int32)  # consecutive, wrapping
    w = np.linspace(0.1, 0.9, run)
    api.lightcone_slices(lcs, lo, hi, run // 2, plane, w, 1 - w, 1.0)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(reps):
        api.lightcone_slices(lcs, lo, hi, run // 2, plane, w, 1 - w, 1.0)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    byt = 12 * n * n * run * nf
    row = {"run_slices": run, "fields": nf, "ms_per_call": round(ms, 4), "contract_MB": round(byt / 1e6, 1),
           "TBps_call": round(byt / ms / 1e9, 3)}
    print(json.dumps(row), flush=True)
    res["kernels"][f"slab_run{run}"] = row
    del lcs
del lo, hi
torch.cuda.empty_cache()
n_s = 1024
bt = torch.rand((n, n, n_s), device="cuda", generator=g)
vel = (torch.rand((n, n, n_s), device="cuda", generator=g) - 0.5) * 1e-17
tau = torch.rand((n, n, n_s), device="cuda", generator=g) * 0.1
H = 2.2e-18 * np.ones(n_s)
for name, t in (("dvdr_taylor", None), ("dvdr_tau21", tau)):
    api.lightcone_dvdr(bt, vel, H, 1.5, 0.2, tau_21=t)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(reps):
        api.lightcone_dvdr(bt, vel, H, 1.5, 0.2, tau_21=t)
    ev1.record()
    torch.cuda.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    byt = (16 if t is not None else 12) * n * n * n_s
    row = {"cells": n * n * n_s, "ms_per_call": round(ms, 4), "contract_MB": round(byt / 1e6, 1),
           "TBps_call": round(byt / ms / 1e9, 3)}
    print(name, json.dumps(row), flush=True)
    res["kernels"][name] = row
if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
