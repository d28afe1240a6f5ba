"""Time of the grid-level ComputePerturbedHaloCatalog call (c21cm_perturb_halos_grids, everything
resident on the device) next to two figures taken in the same process: the exported test_halo_props on
the same catalogue, and the bytes the kernel must move over the 6.2 TB/s a copy reaches
(profiles/r05_copy_bench.txt).  Diagnostic; GPU box only.

    PYTHONPATH=. python tools/time_perturb_halos.py [HII_DIM] [n_halos] [reps] [out.json]

Configurations: mini-halos off / on, PERTURB_ON_HIGH_RES off / on (DIM = 2 HII_DIM), 2LPT.  Every call
ends in a device synchronise; median, minimum and maximum of `reps` calls after 3 warm-up calls.
"""
import ctypes as C
import importlib
import json
import pathlib
import sys
import time

import numpy as np
import torch

root = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(root))
sys.path.insert(0, str(root / "tests"))
S = importlib.import_module("21cmfast_amd.structs")
D = importlib.import_module("21cmfast_amd.drivers")
api = importlib.import_module("21cmfast_amd.grid_api")
from halo_catalogue_helpers import halo_consts, random_catalogue  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n_halos = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 30
out_path = sys.argv[4] if len(sys.argv) > 4 else None
COPY_BW = 6.2e12
box = 1.5 * n
dp = lambda t: C.cast(t.data_ptr(), S.c_float_p)  # noqa: E731


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


lib = importlib.import_module("21cmfast_amd").load(require_gpu=True)
cat = random_catalogue(n_halos, box, seed=1)
cat["coords"] = np.abs(cat["coords"]) % np.float32(box * 0.9999)  # inside the box, as test_halo_props needs
dev = {k: torch.from_numpy(v).cuda() for k, v in cat.items()}
hc = S.HaloCatalogStruct(n_halos=n_halos, buffer_size=n_halos, halo_masses=dp(dev["masses"]),
                         halo_coords=dp(dev["coords"]), star_rng=dp(dev["star_rng"]), sfr_rng=dp(dev["sfr_rng"]),
                         xray_rng=dp(dev["xray_rng"]))
g = torch.Generator(device="cuda").manual_seed(5)
lo = (n, n, n)
mta = 8.7 + 0.5 * torch.rand(lo, device="cuda", generator=g)
mtm = 6.0 + 2.0 * torch.rand(lo, device="cuda", generator=g)
fields = ("halo_coords", "halo_masses", "stellar_masses", "sfr", "ion_emissivity", "xray_emissivity", "fesc_sfr",
          "stellar_mini", "sfr_mini")
res = {"hii_dim": n, "n_halos": n_halos, "reps": reps, "copy_bandwidth_B_per_s": COPY_BW, "runs": []}
for hires in (False, True):
    dim = 2 * n
    shape = (dim,) * 3 if hires else lo
    pre = "hires_" if hires else "lowres_"
    ics = {pre + k: torch.randn(shape, device="cuda", generator=g) * s
           for k, s in (("vx", 3.0), ("vy", 3.0), ("vz", 3.0), ("vx_2LPT", 1.0), ("vy_2LPT", 1.0), ("vz_2LPT", 1.0))}
    for mini in (0, 1):
        consts = halo_consts(z=9.0, use_mini_halos=mini, use_xray=1)
        spec = S.PerturbHalosSpec(dim=dim, dim_z=dim, hii_dim=n, hii_dim_z=n, box_len=box, box_len_z=box,
                                  perturb_on_high_res=int(hires), lpt2=1, velocity_displacement_factor=0.07,
                                  velocity_displacement_factor_2lpt=-0.003)
        use = [f for f in fields if mini or f not in ("stellar_mini", "sfr_mini")]
        arr = {f: torch.zeros((n_halos, 3) if f == "halo_coords" else (n_halos,), device="cuda") for f in use}
        out = S.PerturbedHaloCatalogStruct(n_halos=0, buffer_size=n_halos, **{f: dp(a) for f, a in arr.items()})
        t = timed(lambda: api.perturb_halos_grids(spec, consts, ics, hc, out, mta if mini else None,
                                                  mtm if mini else None))
        # the catalogue streams once (7 floats in, 3 + the property arrays out); every gather is at least its 4 bytes
        stream_bytes = 4 * n_halos * (7 + 3 + len(use) - 1)
        gather_bytes = 4 * n_halos * (6 + (16 if mini else 0))
        t.update(perturb_on_high_res=hires, mini_halos=mini, stream_bytes=stream_bytes, gather_bytes=gather_bytes,
                 bytes_over_copy_bandwidth_ms=round(1e3 * (stream_bytes + gather_bytes) / COPY_BW, 4),
                 checksum_sfr=float(arr["sfr"].double().sum()))
        res["runs"].append(t)
    del ics
    torch.cuda.empty_cache()

# test_halo_props on the same catalogue (the ABI entry: the constants come from the broadcast structs)
for mini in (False, True):
    inputs = D.Inputs(HII_DIM=n, DIM=2 * n, BOX_LEN=box, USE_TS_FLUCT=True, USE_MINI_HALOS=mini, V_CB_MODEL=3,
                      SOURCE_MODEL=4)
    i = inputs
    lib.Broadcast_struct_global_all(*(C.byref(x) for x in (i.simulation_options, i.matter_options, i.cosmo_params,
                                                           i.astro_params, i.astro_options, i.cosmo_tables)))
    lib.init_ps()
    lib.test_halo_props.restype = C.c_int
    lib.test_halo_props.argtypes = [C.c_double] + [S.c_float_p] * 4 + [C.c_ulonglong] + [S.c_float_p] * 6
    props = torch.zeros((n_halos, 12), device="cuda")
    grids = [torch.rand(lo, device="cuda", generator=g) for _ in range(3)]
    grids[1] = grids[1] * 5 + 10.0  # z_re above the redshift

    def call():
        st = lib.test_halo_props(9.0, None, dp(grids[0]) if mini else None, dp(grids[1]) if mini else None,
                                 dp(grids[2]) if mini else None, n_halos, dp(dev["masses"]), dp(dev["coords"]),
                                 dp(dev["star_rng"]), dp(dev["sfr_rng"]), dp(dev["xray_rng"]), dp(props))
        assert st == 0, lib.c21cm_last_error()

    t = timed(call)
    t.update(mini_halos=int(mini))
    res.setdefault("test_halo_props", []).append(t)
print(json.dumps(res))
if out_path:
    pathlib.Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out_path).write_text(json.dumps(res, indent=1) + "\n")
