"""Time the device bubble size distribution (21cmfast_amd.powerspec.get_bubble_sizes).

    python tools/time_bubble_sizes.py [--boxes 256 512] [--fractions 0.1 0.5 0.9] [--rays 1000000] [--reps 3]
                                      [--smooth 4] [--json out.json] [--trace kernel_trace.csv]

Per box size and selected fraction: a Gaussian field smoothed over --smooth cells (so that the selected phase comes in
regions several cells across, as an ionisation field does), thresholded at the quantile that selects the fraction;
one warm-up call and --reps timed ones of ``grid_api.bubble_sizes`` on a tensor already in HBM (CUDA events; every
repeat is listed).  The calls are made in a fixed order, so a kernel trace of the run
(``rocprofv3 --kernel-trace --output-format csv -- python tools/time_bubble_sizes.py ...``) splits into the same
cases: ``--trace`` reads such a CSV instead of running anything and prints the median time of each bubble kernel per
case.
"""

from __future__ import annotations

import argparse
import csv
import importlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
KERNELS = ("bubble_pack_kernel", "bubble_scan_kernel", "bubble_prefix_kernel", "bubble_walk_kernel")


def cases(args):
    return [(n, f) for n in args.boxes for f in args.fractions]


def read_trace(path, args):
    """median microseconds of each bubble kernel per case: every call launches the four kernels once, in order"""
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per_call = 1 + args.reps
    want = len(cases(args)) * per_call * len(KERNELS)
    if len(rows) != want:
        raise SystemExit(f"{path}: {len(rows)} bubble kernel dispatches, expected {want}")
    out = {}
    for c, (n, f) in enumerate(cases(args)):
        timed = rows[(c * per_call + 1) * len(KERNELS):(c + 1) * per_call * len(KERNELS)]  # less the warm-up call
        out[f"{n}^3 fraction {f}"] = {k: round(float(np.median([t for _, name, t in timed if name == k])), 2)
                                      for k in KERNELS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.5, 0.9])
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--smooth", type=float, default=4.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        res = {"kernel_us": read_trace(args.trace, args)}
    else:
        sys.path.insert(0, str(ROOT))
        import torch

        pkg = importlib.import_module("21cmfast_amd")
        pkg.load(require_gpu=True)
        api = importlib.import_module("21cmfast_amd.grid_api")
        PS = importlib.import_module("21cmfast_amd.powerspec")
        res = {"rays": args.rays, "device": torch.cuda.get_device_name(0), "calls": {}}
        for n in args.boxes:
            g = torch.Generator(device="cuda").manual_seed(n)
            white = torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float32)
            k = torch.fft.fftfreq(n, device="cuda") * (2.0 * np.pi)
            k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, : n // 2 + 1] ** 2
            field = torch.fft.irfftn(torch.fft.rfftn(white) * torch.exp(-0.5 * k2 * args.smooth**2), s=(n, n, n))
            field = (field / field.std()).contiguous()
            del white, k2
            L = (float(n),) * 3
            edges = PS.bubble_edges((n, n, n), L, 64, True, None)
            for frac in args.fractions:
                # the quantile of a subsample: torch.quantile does not take 512^3 values
                thr = float(torch.quantile(field.flatten()[:: max(1, field.numel() // 1_000_000)], frac))
                times, out = [], None
                for rep in range(1 + args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    out = api.bubble_sizes(field, (n, n, n), L, edges, threshold=thr, n_rays=args.rays, seed=1)
                    b.record()
                    b.synchronize()
                    if rep:
                        times.append(round(a.elapsed_time(b), 4))
                stats = [int(x) for x in out[1][0].cpu()]
                res["calls"][f"{n}^3 fraction {frac}"] = {
                    "threshold": thr, "filling_fraction": stats[0] / float(n) ** 3, "n_ended": stats[1],
                    "n_capped": stats[2], "call_ms": times, "call_ms_median": float(np.median(times))}
            del field
    text = json.dumps(res, indent=1)
    print(text)
    if args.json:
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
