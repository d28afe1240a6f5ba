#!/usr/bin/env python
"""Time the DexM halo finder (c21cm_find_halos_grids) on initial conditions of this library.

For every (DIM, z): the whole call without any extra synchronisation (one warm-up, then the median and the
range of --repeats calls, host clock around a call that ends in a device synchronise), then once more with
C21CM_DEXM_TIMING=1, which drains the stream around every phase and reports the split into transforms,
compaction, decide rounds, paint and the serial workgroup, plus per rung the candidates, accepted halos,
rounds and whether the serial tail ran.  Beside it the host time of the sampler's table build at the same
redshift.  One JSON line per case; --out appends them to a file.

    python tools/time_dexm.py --dims 256 512 --redshifts 6 10 --out profiles/dexm_times.txt
"""

import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dims", type=int, nargs="+", default=[256])
    ap.add_argument("--redshifts", type=float, nargs="+", default=[6.0, 10.0])
    ap.add_argument("--hii-ratio", type=int, default=4, help="DIM / HII_DIM")
    ap.add_argument("--cell", type=float, default=1.5, help="low-resolution cell in Mpc")
    ap.add_argument("--path", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7, help="timed whole calls after one warm-up")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    pkg = importlib.import_module("21cmfast_amd")
    lib = pkg.load(require_gpu=True)
    S, D = pkg.structs, importlib.import_module("21cmfast_amd.drivers")
    api = importlib.import_module("21cmfast_amd.grid_api")
    check = importlib.import_module("21cmfast_amd._lib").check
    lines = []
    for dim in args.dims:
        hii = dim // args.hii_ratio
        inputs = D.Inputs(random_seed=args.seed, SOURCE_MODEL=4, HII_DIM=hii, DIM=dim, BOX_LEN=args.cell * hii)
        D._initialise(lib, inputs, None)
        so, mo = inputs.simulation_options, inputs.matter_options
        ispec = S.IcsSpec(dim=dim, dim_z=dim, hii_dim=hii, hii_dim_z=hii, perturb_algorithm=mo.PERTURB_ALGORITHM,
                          perturb_on_high_res=int(mo.PERTURB_ON_HIGH_RES))
        ics = api.new_ics_arrays(ispec, device="cuda")
        icss = api.ics_struct(ics)
        check(lib.ComputeInitialConditions(inputs.random_seed, C.byref(icss)), "ComputeInitialConditions")
        torch.cuda.synchronize()
        for z in args.redshifts:
            t0 = time.perf_counter()
            api.sampler_spec(z, -1.0, seed=args.seed)
            tables_s = time.perf_counter() - t0
            spec = api.dexm_spec(z, seed=args.seed)
            spec.path = args.path
            overlap = torch.zeros((hii, hii, hii), dtype=torch.float32, device="cuda")
            rows = max(int(1.2 * (lib_expected(lib, z) + 1)), 1000000)
            whole, split = [], 0.0
            for timing in ["0"] * (1 + args.repeats) + ["1"]:  # warm-up, the whole call `repeats` times, the split
                os.environ["C21CM_DEXM_TIMING"] = timing
                out = S.empty_halo_catalog(rows, device="cuda")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api.find_halos(spec, ics["hires_density"], out, overlap=overlap)
                torch.cuda.synchronize()
                if timing == "1":
                    split = time.perf_counter() - t0
                else:
                    whole.append(time.perf_counter() - t0)
            whole = sorted(whole[1:])
            os.environ["C21CM_DEXM_TIMING"] = "0"
            rep = api.find_halos_report()
            n = rep.n_R
            line = dict(dim=dim, hii_dim=hii, box_len=so.BOX_LEN, redshift=z, path=args.path, n_R=n,
                        n_halos=int(rep.n_halos), whole_call_ms_median=round(1e3 * whole[len(whole) // 2], 3),
                        whole_call_ms_min_max=[round(1e3 * whole[0], 3), round(1e3 * whole[-1], 3)], repeats=len(whole),
                        whole_call_with_phase_syncs_ms=round(1e3 * split, 3),
                        ms=dict(zip(("transforms", "compaction", "decide", "paint", "serial"), [round(v, 3) for v in rep.ms])),
                        candidates=list(rep.candidates[:n]), accepted=list(rep.accepted[:n]), rounds=list(rep.rounds[:n]),
                        tail=list(rep.tail[:n]), tail_rungs=int(sum(rep.tail[:n])), sampler_table_build_s=round(tables_s, 3))
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def lib_expected(lib, z):
    lib.expected_nhalo.restype = C.c_double
    lib.expected_nhalo.argtypes = [C.c_double]
    return lib.expected_nhalo(float(z))


if __name__ == "__main__":
    main()
