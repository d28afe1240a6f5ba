"""Time the device distance transform and granulometry (21cmfast_amd.grid_api.granulometry).

    python tools/time_granulometry.py [--boxes 256 512] [--radii 0 1 8 32] [--fields gaussian balls] [--smooth 4]
                                      [--reps 3] [--step-timeout 240] [--json profiles/granulometry_timing.json]

Per box size, field and number of radii: one warm-up call and --reps timed ones of ``grid_api.granulometry`` on a
tensor already in HBM, all axes periodic (CUDA events; every repeat is listed).  The fields: a Gaussian one smoothed
over --smooth cells and cut at its median, and a union of balls of radius 4 to 40 cells that fills about a third of the
box: its large D2 is the worst case for a walk whose reach is sqrt(max D2).  0 radii is the distance transform alone;
K radii are the distinct floor(r^2) of K radii log-spaced from 1 to 0.95 sqrt(max D2), so that every one of them is
launched (a radius at or above max D2 costs nothing), and 1 radius is the middle one of the 8.  Each case runs in a
child process of its own under ``timeout``, so that one that hangs ends alone and the cases after a failure are not
started.  Per case the file records the time, the compulsory bytes -- the field in (4 N) and the mask out, three
distance passes (mask in, 4 N out; 4 N in and out, twice), and per radius two passes of 4 N in and out and one of 4 N
in -- and with them the fraction of the copy rate (6.2 TB/s, profiles/r05_copy_bench.txt); per box and field the ratio
t(K radii) / (t(0) + K (t(1) - t(0))) for the largest K.
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


def case_name(n, field, k):
    return f"{n}^3 {field} {k} radii"


def model_bytes(n_cells, n_radii):
    mask = n_cells // 8
    return 4 * n_cells + mask + (mask + 4 * n_cells) + 2 * 8 * n_cells + n_radii * 20 * n_cells


def make_field(torch, n, kind, smooth):
    g = torch.Generator(device="cuda").manual_seed(n)
    if kind == "gaussian":
        field = torch.randn((n, n, n), generator=g, device="cuda", dtype=torch.float32)
        if smooth > 0:
            k = torch.fft.fftfreq(n, device="cuda") * (2.0 * np.pi)
            k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + k[None, None, : n // 2 + 1] ** 2
            field = torch.fft.irfftn(torch.fft.rfftn(field) * torch.exp(-0.5 * k2 * smooth**2), s=(n, n, n))
            del k2
        return (field / field.std()).contiguous(), float(field.median() / field.std())
    # balls: 1 outside, 0 inside, selected below 0.5
    field = torch.ones((n, n, n), device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(n)
    ax = torch.arange(n, device="cuda")
    n_balls = max(1, int(0.45 * n**3 / (4.0 / 3.0 * np.pi * 22.0**3 * 1.7)))
    for _ in range(n_balls):
        c, r = rng.integers(0, n, 3), rng.uniform(4.0, 40.0)
        d = [torch.minimum((ax - int(ci)).abs(), n - (ax - int(ci)).abs()) ** 2 for ci in c]
        lo = [torch.nonzero(di <= r * r).flatten() for di in d]
        sub = d[0][lo[0]][:, None, None] + d[1][lo[1]][None, :, None] + d[2][lo[2]][None, None, :] <= r * r
        ix, iy, iz = torch.meshgrid(lo[0], lo[1], lo[2], indexing="ij")
        field[ix[sub], iy[sub], iz[sub]] = 0.0
    return field.contiguous(), 0.5


def run_case(n, kind, n_radii, smooth, reps):
    sys.path.insert(0, str(ROOT))
    import torch

    pkg = importlib.import_module("21cmfast_amd")
    pkg.load(require_gpu=True)
    api = importlib.import_module("21cmfast_amd.grid_api")
    field, threshold = make_field(torch, n, kind, smooth)
    stats = api.granulometry(field, (n, n, n), [], threshold=threshold)[2]
    deepest = int(stats[0, 1])

    def spaced(k):
        r = np.geomspace(1.0, max(1.0, 0.95 * np.sqrt(deepest)), k)
        return np.unique(np.floor(r * r).astype(np.int64))

    radii2 = spaced(n_radii) if n_radii != 1 else spaced(8)[len(spaced(8)) // 2:][:1]
    radii2 = radii2[radii2 < deepest] if n_radii else np.zeros(0, np.int64)
    times, out = [], None
    for rep in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = api.granulometry(field, (n, n, n), radii2, threshold=threshold)
        b.record()
        b.synchronize()
        if rep:
            times.append(round(a.elapsed_time(b), 4))
    ms = float(np.median(times))
    nbytes = model_bytes(n**3, len(radii2))
    return {"device": torch.cuda.get_device_name(0), "call_ms": times, "call_ms_median": ms,
            "radii_launched": int(len(radii2)), "radii2": radii2.tolist(), "max_d2": deepest,
            "n_selected": int(out[2][0, 0]), "covered": out[0][0].cpu().tolist(), "eroded": out[1][0].cpu().tolist(),
            "model_bytes": nbytes, "fraction_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--radii", type=int, nargs="+", default=[0, 1, 8, 32])
    ap.add_argument("--fields", nargs="+", default=["gaussian", "balls"], choices=["gaussian", "balls"])
    ap.add_argument("--smooth", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each case may take")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "granulometry_timing.json"))
    ap.add_argument("--case", nargs=3, default=None, metavar=("N", "FIELD", "RADII"),
                    help="run this one case in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(int(args.case[0]), args.case[1], int(args.case[2]), args.smooth, args.reps)))
        return 0
    res = {"smooth": args.smooth, "copy_rate_bytes_per_s": COPY_RATE, "calls": {}, "ratio_to_sum_of_single_radii": {}}
    status = 0
    for n in args.boxes:
        for kind in args.fields:
            if status:
                break
            for k in args.radii:
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()),
                       "--smooth", str(args.smooth), "--reps", str(args.reps), "--case", str(n), kind, str(k)]
                done = subprocess.run(cmd, capture_output=True, text=True)
                if done.returncode:  # nothing more is started on the GPU after a failure
                    status = done.returncode
                    res["failed"] = {"case": case_name(n, kind, k), "returncode": status,
                                     "stderr": done.stderr[-2000:]}
                    break
                res["calls"][case_name(n, kind, k)] = json.loads(done.stdout.strip().splitlines()[-1])
            else:
                if 0 in args.radii and 1 in args.radii and max(args.radii) > 1:
                    t0 = res["calls"][case_name(n, kind, 0)]["call_ms_median"]
                    t1 = res["calls"][case_name(n, kind, 1)]["call_ms_median"]
                    most = res["calls"][case_name(n, kind, max(args.radii))]
                    res["ratio_to_sum_of_single_radii"][f"{n}^3 {kind} {most['radii_launched']} radii"] = round(
                        most["call_ms_median"] / (t0 + most["radii_launched"] * (t1 - t0)), 3)
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
