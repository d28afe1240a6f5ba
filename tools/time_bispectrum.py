"""Time the device bispectrum (21cmfast_amd.powerspec.get_bispectrum / lightcone_bispectra).

    python tools/time_bispectrum.py [--box 256] [--box-bins 12] [--lc 256 1536] [--lc-bins 8] [--reps 5] [--json out.json]

Cases: a box of --box^3 cells with --box-bins shells and every triangle that can close, and a lightcone of
--lc[0]^2 x --lc[1] slices in cubic chunks with --lc-bins shells.  Whole calls on torch tensors already in HBM:
  first_call_ms         the first call of the process with the geometry (wall clock): the rocFFT plans are made and
                        the triangle counts come from the fp64 indicator pass;
  new_geometry_call_ms  calls that alternate between two box lengths, so that each misses the one-entry cache of
                        counts while the plans are warm: the price of the indicator pass (median of --reps);
  cached_call_ms        calls with the geometry of the call before (median of --reps after a warm-up, CUDA events);
  entry_only_ms         ``grid_api.bispectrum`` alone, cached geometry: the call less the power spectrum that fills
                        ``power`` / ``k`` / ``n_modes``.
``*_all_ms`` lists every repeat, so the run-to-run spread is on record.  Per-kernel times come from a run of this tool
under ``rocprofv3 --kernel-trace --stats``."""

from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def device_ms(fn, reps, every=None, warm=True):
    import torch

    if warm:
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


def wall_ms(fn):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--box", type=int, default=256)
    ap.add_argument("--box-bins", type=int, default=12)
    ap.add_argument("--lc", type=int, nargs=2, default=(256, 1536))
    ap.add_argument("--lc-bins", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))

    import torch

    pkg = importlib.import_module("21cmfast_amd")
    pkg.load(require_gpu=True)
    PS = importlib.import_module("21cmfast_amd.powerspec")
    api = importlib.import_module("21cmfast_amd.grid_api")
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {}

    def skewed(shape):
        x = torch.randn(shape, device="cuda", generator=g)
        return x + 0.5 * x * x

    n, nb = args.box, args.box_bins
    box = skewed((n, n, n))
    L = float(n) * 1.5
    edges = PS.bispectrum_edges((n, n, n), L, nb)
    tri = PS.bispectrum_triangles(edges)
    first = wall_ms(lambda: PS.get_bispectrum(box, L, bins=nb))
    every, every_new = [], []
    cached = device_ms(lambda: PS.get_bispectrum(box, L, bins=nb), args.reps, every)
    flip = [0]

    def other_geometry():
        flip[0] ^= 1
        PS.get_bispectrum(box, L * (1.0 + 0.25 * flip[0]), bins=nb)

    new_geo = device_ms(other_geometry, args.reps, every_new)
    PS.get_bispectrum(box, L, bins=nb)
    entry = device_ms(lambda: api.bispectrum(box, (n, n, n), (L, L, L), edges, tri), args.reps)
    res["box"] = dict(shape=[n] * 3, n_bins=nb, n_triangles=int(len(tri)), first_call_ms=first,
                      new_geometry_call_ms=new_geo, new_geometry_call_all_ms=every_new, cached_call_ms=cached,
                      cached_call_all_ms=every, entry_only_ms=entry,
                      stack_bytes=nb * n * n * 2 * (n // 2 + 1) * 4)
    del box
    torch.cuda.empty_cache()

    m, ns = args.lc
    nb = args.lc_bins
    lc = skewed((m, m, ns))
    dx = 1.5
    first = wall_ms(lambda: PS.lightcone_bispectra(lc, dx, bins=nb))
    out = PS.lightcone_bispectra(lc, dx, bins=nb)
    every = []
    cached = device_ms(lambda: PS.lightcone_bispectra(lc, dx, bins=nb), args.reps, every)
    starts = out.chunk_starts
    e_np, t_np = out.edges.cpu().numpy(), out.triangles.cpu().numpy()
    entry = device_ms(lambda: api.bispectrum(lc, (m, m, m), (m * dx,) * 3, e_np, t_np, offsets=starts, row_pitch=ns),
                      args.reps)
    res["lightcone"] = dict(shape=[m, m, ns], n_chunks=int(len(starts)), n_bins=nb, n_triangles=int(len(t_np)),
                            first_call_ms=first, cached_call_ms=cached, cached_call_all_ms=every, entry_only_ms=entry,
                            stack_bytes=nb * m * m * 2 * (m // 2 + 1) * 4)
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
