"""Time the device Minkowski functionals (21cmfast_amd.powerspec.get_minkowski_functionals).

    python tools/time_minkowski.py [--boxes 256 512] [--thresholds 1 32 255] [--fields gaussian two-valued]
                                   [--smooth 4] [--reps 3] [--step-timeout 120] [--json profiles/minkowski_timing.json]

Per box size, field and number of thresholds: one warm-up call and --reps timed ones of ``grid_api.minkowski`` on a
tensor already in HBM, all axes periodic, cells below the thresholds (CUDA events; every repeat is listed).  The
fields: a Gaussian one smoothed over --smooth cells with the thresholds of ``minkowski_thresholds``, and a two-valued
one (white noise cut at its median into 0 and 1, thresholds spaced inside (0, 1)), in which every lane of a wave adds
to one of two counters per element kind: the worst case for same-counter contention.  Each case runs in a child
process of its own under ``timeout``, so that one that hangs ends alone and the cases after a failure are not started.
Per case the file records the time, the bytes of one read of the field (4 N) and with them the fraction of the copy
rate (6.2 TB/s, profiles/r05_copy_bench.txt), and per box and field the ratio t(most thresholds) / t(fewest).
"""

from __future__ import annotations

import argparse
import importlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
COPY_RATE = 6.2e12  # bytes per second, profiles/r05_copy_bench.txt


def case_name(n, field, t):
    return f"{n}^3 {field} {t} thresholds"


def run_case(n, kind, n_thr, smooth, reps):
    sys.path.insert(0, str(ROOT))
    import torch

    pkg = importlib.import_module("21cmfast_amd")
    pkg.load(require_gpu=True)
    api = importlib.import_module("21cmfast_amd.grid_api")
    PS = importlib.import_module("21cmfast_amd.powerspec")
    g = torch.Generator(device="cuda").manual_seed(n)
    field = torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float32)
    if kind == "gaussian":
        if smooth > 0:
            k = torch.fft.fftfreq(n, device="cuda") * (2.0 * np.pi)
            k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, : n // 2 + 1] ** 2
            field = torch.fft.irfftn(torch.fft.rfftn(field) * torch.exp(-0.5 * k2 * smooth**2), s=(n, n, n))
            del k2
        field = (field / field.std()).contiguous()
        thresholds = PS.minkowski_thresholds(field, n_thr)
    else:
        field = (field > 0).to(torch.float32).contiguous()
        thresholds = np.linspace(0.0, 1.0, n_thr + 2)[1:-1]
    times, out = [], None
    for rep in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = api.minkowski(field, (n, n, n), thresholds)
        b.record()
        b.synchronize()
        if rep:
            times.append(round(a.elapsed_time(b), 4))
    mid = out[0, n_thr // 2].cpu().tolist()
    ms = float(np.median(times))
    nbytes = 4 * n**3
    return {"device": torch.cuda.get_device_name(0), "call_ms": times, "call_ms_median": ms, "field_bytes": nbytes,
            "fraction_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4), "middle_threshold_counts": mid,
            "euler_characteristic": mid[7] - sum(mid[4:7]) + sum(mid[1:4]) - mid[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--thresholds", type=int, nargs="+", default=[1, 32, 255])
    ap.add_argument("--fields", nargs="+", default=["gaussian", "two-valued"], choices=["gaussian", "two-valued"])
    ap.add_argument("--smooth", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds each case may take")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "minkowski_timing.json"))
    ap.add_argument("--case", nargs=3, default=None, metavar=("N", "FIELD", "THRESHOLDS"),
                    help="run this one case in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(int(args.case[0]), args.case[1], int(args.case[2]), args.smooth, args.reps)))
        return 0
    res = {"smooth": args.smooth, "copy_rate_bytes_per_s": COPY_RATE, "calls": {}, "ratio_most_to_fewest": {}}
    status = 0
    for n in args.boxes:
        for kind in args.fields:
            if status:
                break
            for t in args.thresholds:
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()),
                       "--smooth", str(args.smooth), "--reps", str(args.reps), "--case", str(n), kind, str(t)]
                done = subprocess.run(cmd, capture_output=True, text=True)
                if done.returncode:  # nothing more is started on the GPU after a failure
                    status = done.returncode
                    res["failed"] = {"case": case_name(n, kind, t), "returncode": status,
                                     "stderr": done.stderr[-2000:]}
                    break
                res["calls"][case_name(n, kind, t)] = json.loads(done.stdout.strip().splitlines()[-1])
            else:
                lo, hi = min(args.thresholds), max(args.thresholds)
                if lo != hi:
                    res["ratio_most_to_fewest"][f"{n}^3 {kind} {hi} / {lo}"] = round(
                        res["calls"][case_name(n, kind, hi)]["call_ms_median"]
                        / res["calls"][case_name(n, kind, lo)]["call_ms_median"], 3)
        if status:
            break
    text = json.dumps(res, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
