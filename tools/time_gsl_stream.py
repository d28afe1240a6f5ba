#!/usr/bin/env python
"""The IC draw of the reference's random streams: host-staged (rng_stream = 1: acceptance loop on the host,
accepted pairs staged over PCIe, ln / sqrt on the device) against drawn on the device (rng_stream = 2).

Per point (DIM, N_THREADS) and per mode: the draw alone (deviates ready in a device buffer, timed with a host
clock around the call, which ends in a synchronise) and the whole c21cm_ics_grids call on device arrays.  One
warm-up, then --runs timed runs: median, minimum, maximum.  The two modes alternate run by run.  Every run
includes the selection of the per-thread seeds (seed_rng_threads on the host, the same for both modes).  For the device
draw also the time of one launch at the default pairs per launch (a draw of exactly that many pairs per stream).
The requirement recorded per point: the device draw's median is below the host-staged draw's minimum.

usage: time_gsl_stream.py [--dims 512,1024] [--threads 1,16] [--runs 5] [--out FILE.json] [--skip-whole]
A point already in FILE.json is replaced, the others are kept.
"""
import argparse
import ctypes as C
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

pkg = importlib.import_module("21cmfast_amd")
api = importlib.import_module("21cmfast_amd.grid_api")
S = importlib.import_module("21cmfast_amd.structs")

ap = argparse.ArgumentParser()
ap.add_argument("--dims", default="512,1024")
ap.add_argument("--threads", default="1,16")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--skip-whole", action="store_true")
args = ap.parse_args()

lib = pkg.load(require_gpu=True)
proto = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
lib.c21_gsl_mode_deviates_device.restype = C.c_int
lib.c21_gsl_mode_deviates_device.argtypes = proto + [C.c_void_p]
lib.c21_gsl_mode_deviates_ondevice.restype = C.c_int
lib.c21_gsl_mode_deviates_ondevice.argtypes = proto + [C.c_longlong, C.c_void_p]
lib.c21cm_gsl_default_pairs_per_launch.restype = C.c_longlong
SEED = 12345


def ics_spec(dim, hii_dim, box_len, seed):
    """a power-law P(k) = 30 k^-2 on the modes of the grid, 2LPT on the low-resolution grid"""
    import numpy as np

    n_m = 3 * (dim // 2) ** 2 + 1
    k = 2 * np.pi / box_len * np.sqrt(np.arange(n_m, dtype=np.float64))
    pk = np.zeros(n_m)
    pk[1:] = 30.0 * k[1:] ** -2.0
    vol = np.float32(np.float32(np.float32(box_len) * np.float32(box_len)) * np.float32(box_len))
    spec = S.IcsSpec(dim=dim, dim_z=dim, hii_dim=hii_dim, hii_dim_z=hii_dim, box_len=box_len, box_len_z=box_len,
                     volume=float(vol), perturb_algorithm=2, perturb_on_high_res=0, density_is_input=0, n_m=n_m,
                     pk_by_m=pk.ctypes.data_as(S.c_double_p), seed=seed)
    spec._pk = pk  # keep the table alive
    return spec


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, runs):
    """one warm-up of each, then `runs` rounds in which the modes take turns"""
    for fn in fns.values():
        fn()
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return {k: stats(v) for k, v in ms.items()}


def point(dim, n_threads):
    nzc = dim // 2 + 1
    buf = torch.empty(2 * dim * dim * nzc, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def staged():
        assert lib.c21_gsl_mode_deviates_device(SEED, n_threads, dim, dim, nzc, buf.data_ptr(), stream) == 0

    def device():
        assert lib.c21_gsl_mode_deviates_ondevice(SEED, n_threads, dim, dim, nzc, buf.data_ptr(), 0, stream) == 0

    res = {"dim": dim, "n_threads": n_threads, "deviates": 2 * dim * dim * nzc}
    res["draw"] = alternate({"rng_stream_1": staged, "rng_stream_2": device}, args.runs)
    del buf
    if not args.skip_whole:
        hii = dim // 2
        specs = {}
        for mode in (1, 2):
            s = ics_spec(dim, hii, box_len=1.5 * hii, seed=SEED)
            s.rng_stream, s.rng_threads = mode, n_threads
            specs[mode] = s
        ics = api.new_ics_arrays(specs[1], device="cuda")
        res["ics_call"] = alternate({f"rng_stream_{m}": (lambda m=m: api.ics_grids(specs[m], ics)) for m in (1, 2)},
                                    args.runs)
        del ics
    d = res["draw"]
    res["device_median_below_staged_min"] = d["rng_stream_2"]["median_ms"] < d["rng_stream_1"]["min_ms"]
    return res


def one_launch():
    """16 streams that owe exactly one and exactly two launches of the default length: the difference of the two
    draws is one launch (seed selection, uploads and the read-back of the flag are in both)"""
    per = lib.c21cm_gsl_default_pairs_per_launch()
    ny = 2048
    nzc = per // (2 * ny)
    assert 2 * ny * nzc == per
    buf = torch.empty(32 * per, dtype=torch.float64, device="cuda")
    lib.c21cm_gsl_stream_pairs.restype = C.c_int
    lib.c21cm_gsl_stream_pairs.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_longlong,
                                           C.c_long, C.c_void_p, C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def draw(rows_per_stream):
        st = lib.c21cm_gsl_stream_pairs(SEED, 16, 16 * rows_per_stream, ny, nzc, 1, 0, 0, buf.data_ptr(), stream)
        assert st == 0

    res = alternate({"one_launch_draw": lambda: draw(1), "two_launch_draw": lambda: draw(2)}, args.runs)
    res.update(pairs_per_launch=per, streams=16,
               launch_ms=res["two_launch_draw"]["median_ms"] - res["one_launch_draw"]["median_ms"])
    return res


out = {"device": torch.cuda.get_device_name(0), "points": [], "one_launch": one_launch()}
if args.out and Path(args.out).exists():
    out["points"] = json.loads(Path(args.out).read_text()).get("points", [])
for dim in (int(x) for x in args.dims.split(",")):
    for n_threads in (int(x) for x in args.threads.split(",")):
        p = point(dim, n_threads)
        out["points"] = [q for q in out["points"] if (q["dim"], q["n_threads"]) != (dim, n_threads)] + [p]
        print(json.dumps(p), flush=True)
        if args.out:
            Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps(out["one_launch"]))
