"""Time the device friends-of-friends clusters (21cmfast_amd.powerspec.get_bubble_clusters).

    python tools/time_bubble_clusters.py [--boxes 256 512] [--fractions 0.1 0.3116 0.5 0.9] [--connectivity 6 26]
                                         [--smooth 4] [--reps 3] [--json out.json] [--trace kernel_trace.csv]

Per box size, selected fraction and connectivity: a Gaussian field smoothed over --smooth cells (0: white noise, whose
clusters percolate at 0.3116 with 6 neighbours), thresholded at the quantile that selects the fraction; one warm-up call
and --reps timed ones of ``grid_api.bubble_clusters`` on a tensor already in HBM, histograms and stats only (CUDA
events; every repeat is listed).  The calls are made in a fixed order, so a kernel trace of the run
(``rocprofv3 --kernel-trace --output-format csv -- python tools/time_bubble_clusters.py ...``) splits into the same
cases: ``--trace`` reads such a CSV instead of running anything and prints the median time of each kernel per case
(the scan and the prefix run twice per call, for the selection and for the roots; their two times are added).
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
# dispatches per call, in launch order
KERNELS = {"bubble_pack_kernel": 1, "bubble_scan_kernel": 2, "bubble_prefix_kernel": 2, "cluster_init_kernel": 1,
           "cluster_merge_kernel": 1, "cluster_count_kernel": 1, "cluster_roots_kernel": 1, "cluster_emit_kernel": 1,
           "cluster_finish_kernel": 1}
CONNECTIVITY = {6: 1, 18: 2, 26: 3}


def cases(args):
    return [(n, f, c) for n in args.boxes for f in args.fractions for c in args.connectivity]


def case_name(n, f, c):
    return f"{n}^3 fraction {f} connectivity {c}"


def read_trace(path, args):
    """median microseconds of each kernel per case: every call launches sum(KERNELS.values()) kernels, in order"""
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name:
                rows.append((int(r["Start_Timestamp"]), name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    per_call, calls = sum(KERNELS.values()), 1 + args.reps
    want = len(cases(args)) * calls * per_call
    if len(rows) != want:
        raise SystemExit(f"{path}: {len(rows)} cluster kernel dispatches, expected {want}")
    out = {}
    for i, (n, f, c) in enumerate(cases(args)):
        per_kernel = {k: [] for k in KERNELS}
        for rep in range(1, calls):  # less the warm-up call
            call = rows[(i * calls + rep) * per_call:(i * calls + rep + 1) * per_call]
            for k in KERNELS:
                per_kernel[k].append(sum(t for _, name, t in call if name == k))
        out[case_name(n, f, c)] = {k: round(float(np.median(v)), 2) for k, v in per_kernel.items()}
        out[case_name(n, f, c)]["all kernels"] = round(float(sum(np.median(v) for v in per_kernel.values())), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.3116, 0.5, 0.9])
    ap.add_argument("--connectivity", type=int, nargs="+", default=[6, 26], choices=sorted(CONNECTIVITY))
    ap.add_argument("--smooth", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
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
        res = {"smooth": args.smooth, "device": torch.cuda.get_device_name(0), "calls": {}}
        for n in args.boxes:
            g = torch.Generator(device="cuda").manual_seed(n)
            field = torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float32)
            if args.smooth > 0:
                k = torch.fft.fftfreq(n, device="cuda") * (2.0 * np.pi)
                k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, : n // 2 + 1] ** 2
                field = torch.fft.irfftn(torch.fft.rfftn(field) * torch.exp(-0.5 * k2 * args.smooth**2), s=(n, n, n))
                del k2
            field = (field / field.std()).contiguous()
            edges = PS.cluster_edges((n, n, n), 32, True)
            for frac in args.fractions:
                # the quantile of a subsample: torch.quantile does not take 512^3 values
                thr = float(torch.quantile(field.flatten()[:: max(1, field.numel() // 1_000_000)], frac))
                for c in args.connectivity:
                    times, out = [], None
                    for rep in range(1 + args.reps):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        out = api.bubble_clusters(field, (n, n, n), edges, threshold=thr, connectivity=CONNECTIVITY[c])
                        b.record()
                        b.synchronize()
                        if rep:
                            times.append(round(a.elapsed_time(b), 4))
                    stats = [int(x) for x in out[2][0].cpu()]
                    res["calls"][case_name(n, frac, c)] = {
                        "threshold": thr, "filling_fraction": stats[0] / float(n) ** 3, "n_clusters": stats[1],
                        "largest_fraction": stats[2] / max(stats[0], 1), "call_ms": times,
                        "call_ms_median": float(np.median(times))}
            del field
    text = json.dumps(res, indent=1)
    print(text)
    if args.json:
        Path(args.json).write_text(text + "\n")


if __name__ == "__main__":
    main()
