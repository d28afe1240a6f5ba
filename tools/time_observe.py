"""Time the telescope-resolution smoothing on the device (21cmfast_amd.grid_api.observe_smooth).

    python tools/time_observe.py [--shapes 256x256x2048 512x512x1024] [--baselines 2.0 0.5] [--reps 3]
                                 [--step-timeout 240] [--json profiles/observe_timing.json]

Lightcones of float32 cells of 1.5 Mpc whose slices run from z = 6 to z = 12, seen with a longest baseline of 2 km and
of 0.5 km, the channel matched to the beam (``los_ratio = 1``) and switched off.  Per case: one warm-up call and --reps
timed ones of ``grid_api.observe_smooth`` on a tensor already in HBM, with the widths and counts the helpers of
``21cmfast_amd.observe`` give (CUDA events; every repeat is listed).  Beside it, timed in the same way on the same
tensor, the plain torch formulation of the same operation that a user writes today: ``rfft2`` over the first two axes,
one Gaussian per slice in k (whose k = 0 mode removes the mean), ``irfft2``, and a boxcar from a cumulative sum along
the line of sight.  The two differ by the truncation of the beam at 4 sigma and by the rounding of the cumulative sum;
their largest difference is recorded.  Each case runs in a child process of its own under ``timeout``, so that one that
hangs ends alone, and the cases after a failure are not started.  Per case the file records the times, the largest lw,
the compulsory bytes -- 4 N read for the means and 8 N for every sweep that runs -- and with them the fraction of the
copy rate (6.2 TB/s, profiles/r05_copy_bench.txt).
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
CELL = 1.5  # Mpc
Z_RANGE = (6.0, 12.0)


def case_name(shape, baseline, channel):
    return f"{shape} {baseline:g} km channel {channel}"


def torch_formulation(torch, field, sigma, below, above):
    """what a user writes today: the beam in k space, the channel from a cumulative sum"""
    nx, ny, ns = field.shape
    kx = torch.fft.fftfreq(nx, device=field.device) * (2.0 * np.pi)
    ky = torch.fft.rfftfreq(ny, device=field.device) * (2.0 * np.pi)
    k2 = kx[:, None, None] ** 2 + ky[None, :, None] ** 2
    window = torch.exp(-0.5 * k2 * sigma[None, None, :] ** 2)
    window[0, 0, :] = 0.0  # the mean of every slice
    smooth = torch.fft.irfft2(torch.fft.rfft2(field, dim=(0, 1)) * window, s=(nx, ny), dim=(0, 1))
    if below is None:
        return smooth
    s = torch.arange(ns, device=field.device)
    lo, hi = torch.clamp(s - below, min=0), torch.clamp(s + above, max=ns - 1)
    total = torch.nn.functional.pad(torch.cumsum(smooth, dim=2), (1, 0))
    return (total[:, :, hi + 1] - total[:, :, lo]) / (hi - lo + 1).to(torch.float32)


def timed(torch, reps, call):
    times, out = [], None
    for rep in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        if rep:
            times.append(round(a.elapsed_time(b), 4))
    return times, out


def run_case(shape, baseline, channel, reps):
    sys.path.insert(0, str(ROOT))
    import torch

    pkg = importlib.import_module("21cmfast_amd")
    pkg.load(require_gpu=True)
    api = importlib.import_module("21cmfast_amd.grid_api")
    ob = importlib.import_module("21cmfast_amd.observe")
    nx, ny, ns = shape
    z = np.linspace(Z_RANGE[0], Z_RANGE[1], ns)
    fwhm = ob.beam_fwhm(z, baseline)
    sigma = fwhm / ob.FWHM_PER_SIGMA / CELL
    if channel == "matched":
        below, above = ob.los_windows(CELL * np.arange(ns), fwhm)
    else:
        below = above = np.zeros(ns, np.int32)
    g = torch.Generator(device="cuda").manual_seed(ns)
    field = torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * 20.0 - 10.0
    ours, (out, _) = timed(torch, reps, lambda: api.observe_smooth(field, sigma, below, above))
    t_sigma = torch.from_numpy(sigma).to(device="cuda", dtype=torch.float32)
    t_below = torch.from_numpy(below.astype(np.int64)).cuda() if channel == "matched" else None
    t_above = torch.from_numpy(above.astype(np.int64)).cuda() if channel == "matched" else None
    theirs, ref = timed(torch, reps, lambda: torch_formulation(torch, field, t_sigma, t_below, t_above))
    diff = float((out - ref).abs().max())
    del ref
    cells = nx * ny * ns
    sweeps = 2 + (channel == "matched")
    nbytes = 4 * cells + 8 * cells * sweeps
    ms, torch_ms = float(np.median(ours)), float(np.median(theirs))
    return {"device": torch.cuda.get_device_name(0), "call_ms": ours, "call_ms_median": ms, "torch_ms": theirs,
            "torch_ms_median": torch_ms, "torch_over_call": round(torch_ms / ms, 3),
            "sigma_cells": [round(float(sigma[0]), 3), round(float(sigma[-1]), 3)],
            "lw_max": int(max(int(4.0 * x + 0.5) for x in sigma)), "los_window_max": int((below + above).max()) + 1,
            "sweeps": sweeps, "model_bytes": nbytes,
            "fraction_of_copy_rate": round(nbytes / (ms * 1e-3) / COPY_RATE, 4),
            "max_abs_difference_to_torch": diff, "max_abs_field": float(field.abs().max())}


def parse_shape(text):
    shape = tuple(int(x) for x in text.split("x"))
    if len(shape) != 3:
        raise argparse.ArgumentTypeError("a shape is NXxNYxNS")
    return shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=parse_shape, nargs="+", default=[(256, 256, 2048), (512, 512, 1024)])
    ap.add_argument("--baselines", type=float, nargs="+", default=[2.0, 0.5])
    ap.add_argument("--channels", nargs="+", default=["matched", "off"], choices=["matched", "off"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each case may take")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "observe_timing.json"))
    ap.add_argument("--case", nargs=3, default=None, metavar=("SHAPE", "BASELINE", "CHANNEL"),
                    help="run this one case in this process and print its JSON (what the parent starts)")
    args = ap.parse_args()
    if args.case:
        print(json.dumps(run_case(parse_shape(args.case[0]), float(args.case[1]), args.case[2], args.reps)))
        return 0
    res = {"cell_mpc": CELL, "redshifts": list(Z_RANGE), "copy_rate_bytes_per_s": COPY_RATE, "calls": {}}
    status = 0
    for shape in args.shapes:
        text = "x".join(map(str, shape))
        for baseline in args.baselines:
            for channel in args.channels:
                if status:
                    break
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()),
                       "--reps", str(args.reps), "--case", text, str(baseline), channel]
                done = subprocess.run(cmd, capture_output=True, text=True)
                if done.returncode:  # nothing more is started on the GPU after a failure
                    status = done.returncode
                    res["failed"] = {"case": case_name(text, baseline, channel), "returncode": status,
                                     "stderr": done.stderr[-2000:]}
                    break
                case = json.loads(done.stdout.strip().splitlines()[-1])
                res["calls"][case_name(text, baseline, channel)] = case
                print(f"{case_name(text, baseline, channel)}: {case['call_ms_median']} ms, torch "
                      f"{case['torch_ms_median']} ms", file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
