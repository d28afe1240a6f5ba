#!/usr/bin/env python
"""Time the periodic dv/dr correction of a coeval box (grid_api.dvdr_periodic) on the MI355X.

Device arrays, both forms (Taylor, tau_21), on the transform path at 256^3 and 512^3 and on the direct
path at 200^3 and 300^3.  Per shape: warm-up calls, then `--rounds` windows of `--reps` calls between two
device events; the median window gives the time per call, the extremes its spread.  A call is the whole
library entry: the H(z) table upload, the one launch and the stream synchronise.  The byte contract is
12 B per cell (16 B with tau_21): what the launch must move, set beside the 6.2 TB/s a plain copy reaches
on this GPU (profiles/r05_copy_bench.txt).  Needs a GPU: there is no fallback.

    python tools/time_coeval_velocity.py --out profiles/coeval_velocity_timing.json
"""
import argparse
import importlib
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

COPY_TBPS = 6.2  # profiles/r05_copy_bench.txt

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--shapes", default="256:fft,512:fft,200:direct,300:direct")
args = ap.parse_args()

import torch  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_coeval_velocity.py needs an MI355X")
pkg = importlib.import_module("21cmfast_amd")
pkg.load(require_gpu=True)
api = importlib.import_module("21cmfast_amd.grid_api")

res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
       "copy_TBps": COPY_TBPS, "shapes": {}}
g = torch.Generator(device="cuda").manual_seed(1)
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for item in args.shapes.split(","):
    n, method = item.split(":")
    n = int(n)
    shape = (n, n, n)
    H = 2.2e-18 * np.ones(n)
    bt = torch.rand(shape, device="cuda", generator=g) * 20.0
    vel = (torch.rand(shape, device="cuda", generator=g) - 0.5) * 1e-18  # gradients of a few tenths of H
    tau = torch.rand(shape, device="cuda", generator=g) * 0.1
    out = torch.empty_like(bt)
    for name, t in (("taylor", None), ("tau21", tau)):
        for _ in range(3):
            api.dvdr_periodic(bt, vel, H, 1.5, 0.2, tau_21=t, method=method, out=out)
        torch.cuda.synchronize()
        windows = []
        for _ in range(args.rounds):
            ev0.record()
            for _ in range(args.reps):
                api.dvdr_periodic(bt, vel, H, 1.5, 0.2, tau_21=t, method=method, out=out)
            ev1.record()
            torch.cuda.synchronize()
            windows.append(ev0.elapsed_time(ev1) / args.reps)
        ms = float(np.median(windows))
        byt = (16 if t is not None else 12) * n ** 3
        row = {"n": n, "method": method, "form": name, "ms_per_call": round(ms, 4),
               "ms_min": round(min(windows), 4), "ms_max": round(max(windows), 4),
               "bytes_per_cell": 16 if t is not None else 12, "contract_MB": round(byt / 1e6, 1),
               "GBps_call": round(byt / ms / 1e6, 1), "share_of_copy": round(byt / ms / 1e9 / COPY_TBPS, 3)}
        print(json.dumps(row), flush=True)
        res["shapes"][f"{n}_{method}_{name}"] = row
    del bt, vel, tau, out
    torch.cuda.empty_cache()
if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
