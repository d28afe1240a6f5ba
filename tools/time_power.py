"""Time the device power spectrum (21cmfast_amd.powerspec) against the host path
users take today (copy to the host, fp64 numpy.fft.fftn, powerbox binning as oracle/powerbox_power.py).

    python tools/time_power.py [--box 512] [--lc 256 1536] [--reps 5] [--host] [--json out.json] [--root DIR]

Cases: a box of --box^3 cells (spherical bins) and a lightcone of --lc[0]^2 x --lc[1] slices in cubic
chunks (spherical and cylindrical).  Device times are whole calls on torch tensors already in HBM (median
of --reps after a warm-up, CUDA events); per-kernel times come from a run under
``rocprofv3 --kernel-trace --stats``.  --host adds the host path for the box and for one lightcone chunk
(device -> host copy included).  Where the package has them, the options beyond powerbox are timed on the box
one at a time (taper window, mu cut, per-bin variance; ``*_added_ms`` is the whole call less the default
call) and ``lightcone_moments`` on the lightcone.  ``*_all_ms`` lists every repeat, so the run-to-run spread
is on record.  --root times the package of another checkout (built there) with this tool, e.g. the parent
commit's for a before / after comparison."""

from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def device_ms(fn, reps, every=None):
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    if every is not None:
        every.extend(round(x, 4) for x in out)
    return float(np.median(out))


def host_s(field_dev, L):
    from oracle import powerbox_power as PB

    t0 = time.perf_counter()
    a = field_dev.cpu().numpy()
    PB.get_power(a, L)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, default=512)
    ap.add_argument("--lc", type=int, nargs=2, default=(256, 1536))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))

    import torch

    pkg = importlib.import_module("21cmfast_amd")
    pkg.load(require_gpu=True)
    PS = importlib.import_module("21cmfast_amd.powerspec")
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {}

    n = args.box
    box = torch.randn((n, n, n), device="cuda", generator=g)
    L = float(n) * 1.5
    every = []
    res["box"] = dict(shape=[n] * 3, call_ms=device_ms(lambda: PS.get_power(box, L), args.reps, every),
                      call_all_ms=every, half_spectrum_bytes=n * n * (n // 2 + 1) * 8)
    if hasattr(PS, "get_moments"):
        base = res["box"]["call_ms"]
        for name, kw in (("window", dict(window="blackmanharris")), ("cut", dict(mu_min=0.5)),
                         ("variance", dict(return_variance=True)),
                         ("all", dict(window="blackmanharris", mu_min=0.5, return_variance=True))):
            ms = device_ms(lambda: PS.get_power(box, L, **kw), args.reps)
            res["box"][f"{name}_call_ms"] = ms
            res["box"][f"{name}_added_ms"] = ms - base
        res["box"]["moments_call_ms"] = device_ms(lambda: PS.get_moments(box), args.reps)
    if args.host:
        res["box"]["host_numpy_s"] = host_s(box, L)
    del box
    torch.cuda.empty_cache()

    m, ns = args.lc
    lc = torch.randn((m, m, ns), device="cuda", generator=g)
    dx = 1.5
    sph = PS.lightcone_power_spectra(lc, dx)
    every = []
    res["lightcone"] = dict(shape=[m, m, ns], n_chunks=int(len(sph.chunk_starts)),
                            call_ms=device_ms(lambda: PS.lightcone_power_spectra(lc, dx), args.reps, every),
                            call_all_ms=every,
                            cylindrical_call_ms=device_ms(
                                lambda: PS.lightcone_power_spectra(lc, dx, cylindrical=True), args.reps))
    if hasattr(PS, "lightcone_moments"):
        res["lightcone"]["moments_call_ms"] = device_ms(lambda: PS.lightcone_moments(lc), args.reps)
        res["lightcone"]["moments_pdf64_call_ms"] = device_ms(
            lambda: PS.lightcone_moments(lc, bins=64, range=(-4.0, 4.0)), args.reps)
    if args.host:
        res["lightcone"]["host_numpy_s_one_chunk"] = host_s(lc[:, :, :m].contiguous(), (m * dx,) * 3)
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
