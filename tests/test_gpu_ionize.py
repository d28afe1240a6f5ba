"""GPU parity: the ComputeIonizedBox grid algorithm on the MI355X vs the CPU oracle.

Tolerances (BASELINE.json north_star: "xH_box matching reference to rtol 1e-4"):
the barrier test is discontinuous, so parity is stated as
  * fraction of cells whose ionised/neutral flag differs  <= 2e-4, and
  * rtol 1e-4 (+ atol 1e-6) on xH over the cells whose flag agrees,
  * z_reion identical where flags agree, kinetic temperature rtol 1e-4,
  * per-radius f_coll grid means rtol 1e-5.
"""

import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = importlib.import_module("21cmfast_amd.workloads")


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


def compare(got, ref, spec, flag_tol=2e-4, flags=None):
    """`flags`: (got, ref) boolean arrays "the cell crossed a barrier"; default x_HI == 0 (with a
    recombination model a cell can also reach x_HI = 0 through the clamp of the partial
    ionisation without crossing, so those tests pass the first-crossing outputs instead)."""
    xg, xr = got["neutral_fraction"], ref["neutral_fraction"]
    ion_g, ion_r = (xg == 0, xr == 0) if flags is None else flags
    mismatch = np.mean(ion_g != ion_r)
    assert mismatch <= flag_tol, f"ionisation flag mismatch fraction {mismatch}"
    same = ion_g == ion_r
    # xH = 1 - f*zeta cancels near the barrier: float32-FFT round-off of ~1e-6 relative in f is
    # an ABSOLUTE ~1e-6 in xH, hence the atol next to the north-star rtol of 1e-4
    np.testing.assert_allclose(xg[same], xr[same], rtol=1e-4, atol=5e-6)
    np.testing.assert_array_equal(got["z_reion"][same], ref["z_reion"][same])
    if not spec.minimize_memory:
        # partial-ionisation T_k = T_HI*xH + T_re*(1-xH) is linear in xH with slope ~T_re, so
        # the xH tolerance (rtol 1e-4 at xH ~ 1) maps onto atol = 1e-4 * T_re
        np.testing.assert_allclose(got["kinetic_temperature"][same],
                                   ref["kinetic_temperature"][same], rtol=1e-4,
                                   atol=1e-4 * spec.T_re)
    n = spec.n_radii
    np.testing.assert_allclose(np.array(got["report"].f_coll_grid_mean[:n]),
                               np.array(ref["report"].f_coll_grid_mean[:n]), rtol=1e-5)
    assert got["report"].global_xH == pytest.approx(ref["report"].global_xH, rel=1e-4, abs=2e-4)
    return mismatch


def run_device(api, spec, density, n_ion=None, device_resident=False, **kw):
    if device_resident:
        import torch

        density_d = torch.from_numpy(density).cuda()
        n_ion_d = None if n_ion is None else torch.from_numpy(n_ion).cuda()
        kw_d = {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in kw.items()}
        buf, box, rep = api.ionize_grids(spec, density_d, n_ion_d, **kw_d)
        torch.cuda.synchronize()
        out = {k: getattr(buf, k).cpu().numpy() for k in
               ("neutral_fraction", "z_reion", "kinetic_temperature")
               if getattr(buf, k) is not None}
        if buf.unnormalised_nion is not None:
            out["unnormalised_nion"] = buf.unnormalised_nion.cpu().numpy()
    else:
        buf, box, rep = api.ionize_grids(spec, density, n_ion, **kw)
        out = {k: getattr(buf, k) for k in ("neutral_fraction", "z_reion", "kinetic_temperature")
               if getattr(buf, k) is not None}
        if buf.unnormalised_nion is not None:
            out["unnormalised_nion"] = buf.unnormalised_nion
    out["report"] = rep
    out["mean_f_coll"] = box.mean_f_coll
    return out


@pytest.mark.parametrize("n,device_resident", [(32, False), (64, True), (50, False), (35, True),
                                               (128, True), (192, True)])
def test_lagrangian_two_grid_parity(api, oracle, n, device_resident):
    """Config-3 semantics (G = 2: delta top-hat + n_ion exp-MFP) at oracle-sized boxes,
    including the odd sizes the reference's test-suite uses (35, 50)."""
    spec = W.ionize_spec(n, r_bubble_max=20.0)
    density = W.density_field_numpy(n, seed=12345)
    n_ion = W.nion_from_density(density)
    ref = oracle.ionize_grids(spec, density, n_ion)
    got = run_device(api, spec, density, n_ion, device_resident)
    compare(got, ref, spec)
    frac = np.mean(ref["neutral_fraction"] == 0)
    assert 0.05 < frac < 0.95, f"workload should exercise both branches (ionised {frac})"
    assert got["mean_f_coll"] == pytest.approx(ref["mean_f_coll"], rel=1e-5)


def test_long_lines_non_cubic_parity(api, oracle):
    """1024-point x/y lines (config-4 line length; unfused window path) on a thin non-cubic box
    1024 x 1024 x 64 so that the oracle still finishes in seconds."""
    oracle.set_threads(32)
    spec = W.ionize_spec(1024, hii_dim_z=64, r_bubble_max=2.6)
    assert spec.n_radii >= 8
    density = W.density_field_numpy((1024, 1024, 64), seed=31)
    n_ion = W.nion_from_density(density)
    ref = oracle.ionize_grids(spec, density, n_ion)
    got = run_device(api, spec, density, n_ion, device_resident=True)
    compare(got, ref, spec)
    oracle.set_threads(16)


@pytest.mark.parametrize("zpass", ["wave", "tile", "wave1024", "wave256"])
def test_512_point_z_lines_parity(api, oracle, zpass, monkeypatch):
    """The benchmark's z-line length (512 points: the wave-level fused pass Z, or the tile version
    with C21CM_ZPASS=tile) on a 64 x 64 x 512 box the oracle finishes in seconds; and the
    1024-point variant of the wave-level kernel on 64 x 64 x 1024."""
    import subprocess
    import sys

    if zpass == "tile":
        # the choice is cached per process: run the other variant in a child process
        code = ("import importlib, numpy as np, sys; sys.path.insert(0, 'tests');"
                "import test_gpu_ionize as t; api = importlib.import_module('21cmfast_amd.grid_api');"
                "oracle = importlib.import_module('oracle.oracle'); oracle.load();"
                "t.check_512_lines(api, oracle); print('OK-512')")
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                             env={**__import__("os").environ, "C21CM_ZPASS": "tile"})
        assert "OK-512" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        return
    check_512_lines(api, oracle, *{"wave1024": (64, 1024), "wave256": (64, 256)}.get(zpass, (64, 512)))


def check_512_lines(api, oracle, n=64, nz=512):
    oracle.set_threads(32)
    spec = W.ionize_spec(n, hii_dim_z=nz, r_bubble_max=12.0)
    assert spec.n_radii >= 10
    density = W.density_field_numpy((n, n, nz), seed=77)
    n_ion = W.nion_from_density(density)
    ref = oracle.ionize_grids(spec, density, n_ion)
    got = run_device(api, spec, density, n_ion, device_resident=True)
    compare(got, ref, spec)
    oracle.set_threads(16)
    assert 0.05 < (ref["neutral_fraction"] == 0).mean() < 0.95


_TABLE_CB = []  # ctypes callbacks must outlive the spec that points at them


def _install_table(spec):
    """A smooth exp-table callback (FCOLL_TABLE_EXP): ln f_coll(delta) per radius."""
    S = importlib.import_module("21cmfast_amd.structs")

    def table_fn(r_index, dmin, dmax, table, user):
        x = dmin + (dmax - dmin) / (S.NDELTA_TABLE - 1.0) * np.arange(S.NDELTA_TABLE)
        y = np.log(0.02 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index))
        for i in range(S.NDELTA_TABLE):
            table[i] = y[i]
        return 0

    cb = S.TABLE_FN(table_fn)
    _TABLE_CB.append(cb)
    spec.table_fn = cb


@pytest.mark.parametrize("mode", ["erfc", "table", "stars_ts", "stars_ts_prev"])
@pytest.mark.parametrize("nz", [256, 512, 1024])
def test_long_z_lines_plain_pass_parity(api, oracle, mode, nz):
    """The single-grid pass Z on 512- and 1024-point lines (wave-level kernel with the erfc,
    extrema and plain-store epilogues) on 64 x 64 x nz boxes."""
    n = 64
    oracle.set_threads(32)
    if mode.startswith("stars_ts"):  # x_e grid present: the three-grid fused pass Z
        prev = mode.endswith("prev")
        spec = W.ionize_spec(n, hii_dim_z=nz, r_bubble_max=8.0, use_ts_fluct=1,
                             first_snapshot=0 if prev else 1)
        density = W.density_field_numpy((n, n, nz), seed=5)
        n_ion = W.nion_from_density(density)
        rng = np.random.default_rng(3)
        # x_e spans the clips at 0 and 0.999 and is large enough to matter in the barrier
        xe = (-0.05 + 0.6 * rng.random((n, n, nz)) ** 3).astype(np.float32)
        xe[::7, ::5, ::3] = 1.2
        Tn = (8.0 + 4.0 * rng.random((n, n, nz))).astype(np.float32)
        kw = dict(xe=xe, Tneutral=Tn)
        if prev:
            kw["prev_z_reion"] = np.where(rng.random((n, n, nz)) < 0.3, 10.5, -1.0).astype(np.float32)
        ref = oracle.ionize_grids(spec, density, n_ion, **kw)
        got = run_device(api, spec, density, n_ion, device_resident=True, **kw)
        assert 0.02 < (ref["neutral_fraction"] == 0).mean() < 0.98
    else:
        fmode = W.FCOLL_ERFC if mode == "erfc" else W.FCOLL_TABLE_EXP
        spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=8.0)
        density = W.density_field_numpy((n, n, nz), seed=6)
        if mode == "table":
            _install_table(spec)
        ref = oracle.ionize_grids(spec, density, need_nion=True)
        got = run_device(api, spec, density, device_resident=True)
    compare(got, ref, spec)
    oracle.set_threads(16)


@pytest.mark.parametrize("mode", ["erfc", "table"])
@pytest.mark.parametrize("shape,device_resident", [((64, 64, 64), False), ((32, 32, 128), True)])
def test_eulerian_sources_with_xe_grid(api, oracle, mode, shape, device_resident):
    """Spin-temperature runs with Eulerian sources on the native passes: delta and x_e go through
    passes X / Y together, the barrier of the first-crossing mask reads f zeta > 1 - x_e(R) with the
    filtered x_e clipped to [0, 0.999]; the cell-scale radius and the post-loop take the partial
    ionisations and temperatures from the x_e / T_k boxes (IonisationBox.c:811-813,1118,1160-1200)."""
    n, nz = shape[0], shape[2]
    fmode = W.FCOLL_ERFC if mode == "erfc" else W.FCOLL_TABLE_EXP
    for first in (1, 0):
        spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=10.0, use_ts_fluct=1,
                             first_snapshot=first)
        if mode == "table":
            _install_table(spec)
        density = W.density_field_numpy(shape, seed=6)
        rng = np.random.default_rng(11)
        xe = (-0.05 + 0.7 * rng.random(shape) ** 2).astype(np.float32)  # spans both clips
        xe[::5, ::3, ::7] = 1.3
        Tn = (8.0 + 4.0 * rng.random(shape)).astype(np.float32)
        kw = dict(xe=xe, Tneutral=Tn)
        if not first:
            kw["prev_z_reion"] = np.where(rng.random(shape) < 0.25, 10.5, -1.0).astype(np.float32)
        ref = oracle.ionize_grids(spec, density, need_nion=True, **kw)
        got = run_device(api, spec, density, device_resident=device_resident, **kw)
        compare(got, ref, spec)
        assert 0.02 < (ref["neutral_fraction"] == 0).mean() < 0.98
        # the x_e grid matters: without it fewer cells cross
        spec0 = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=10.0, first_snapshot=first)
        if mode == "table":
            _install_table(spec0)
        kw0 = {k: v for k, v in kw.items() if k == "prev_z_reion"}
        ref0 = oracle.ionize_grids(spec0, density, need_nion=True, **kw0)
        assert (ref["neutral_fraction"] == 0).sum() > (ref0["neutral_fraction"] == 0).sum()


@pytest.mark.parametrize("n", [32, 50, 64])
def test_const_ion_eff_erfc_parity(api, oracle, n):
    """G = 1 variant: CONST-ION-EFF closed-form erfc, sharp-k filter, fix_mean."""
    spec = W.ionize_spec(n, mode=W.FCOLL_ERFC, r_bubble_max=20.0)
    density = W.density_field_numpy(n, seed=777)
    ref = oracle.ionize_grids(spec, density, need_nion=True)
    got = run_device(api, spec, density)
    compare(got, ref, spec)
    np.testing.assert_allclose(got["unnormalised_nion"], ref["unnormalised_nion"], rtol=1e-4,
                               atol=1e-9)


@pytest.mark.parametrize("mode", [W.FCOLL_TABLE_LINEAR, W.FCOLL_TABLE_EXP])
def test_table_modes_parity(api, oracle, pkg, mode):
    """Host-table modes: extrema on device -> host callback -> 400-bin table -> device lerp."""
    S = pkg.structs
    n = 32
    calls = []

    def table_fn(r_index, dmin, dmax, table, user):
        x = dmin + (dmax - dmin) / (S.NDELTA_TABLE - 1.0) * np.arange(S.NDELTA_TABLE)
        if mode == W.FCOLL_TABLE_LINEAR:
            y = 0.02 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index)
        else:
            y = np.log(0.02 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index))
        for i in range(S.NDELTA_TABLE):
            table[i] = y[i]
        calls.append((r_index, dmin, dmax))
        return 0

    cb = S.TABLE_FN(table_fn)
    spec = W.ionize_spec(n, mode=mode, r_bubble_max=12.0)
    spec.table_fn = cb
    density = W.density_field_numpy(n, seed=99)
    ref = oracle.ionize_grids(spec, density, need_nion=True)
    ref_calls = list(calls)
    calls.clear()
    got = run_device(api, spec, density)
    compare(got, ref, spec)
    assert [c[0] for c in calls] == [c[0] for c in ref_calls]
    np.testing.assert_allclose([c[1:] for c in calls], [c[1:] for c in ref_calls], atol=2e-5)


def test_ts_fluct_and_previous_snapshot(api, oracle):
    """x_e grid filtered alongside delta; z_reion inherited from a previous snapshot."""
    n = 32
    spec = W.ionize_spec(n, r_bubble_max=15.0, use_ts_fluct=1, first_snapshot=0)
    rng = np.random.default_rng(8)
    density = W.density_field_numpy(n, seed=4242)
    n_ion = W.nion_from_density(density)
    xe = (0.05 + 0.04 * rng.random((n, n, n))).astype(np.float32)
    Tn = (20 + 5 * rng.random((n, n, n))).astype(np.float32)
    prev_z = np.where(rng.random((n, n, n)) < 0.3, 10.5, -1.0).astype(np.float32)
    ref = oracle.ionize_grids(spec, density, n_ion, xe=xe, Tneutral=Tn, prev_z_reion=prev_z)
    got = run_device(api, spec, density, n_ion, xe=xe, Tneutral=Tn, prev_z_reion=prev_z)
    compare(got, ref, spec)
    assert np.any(got["z_reion"] == np.float32(10.5))


def test_edge_cases(api, oracle):
    n = 32
    density = W.density_field_numpy(n, seed=1)
    # (a) nothing ionises: xH stays at its partial value everywhere, z_reion = -1
    spec = W.ionize_spec(n, r_bubble_max=10.0)
    n_ion = W.nion_from_density(density, fbar=1e-6)
    got = run_device(api, spec, density, n_ion)
    ref = oracle.ionize_grids(spec, density, n_ion)
    compare(got, ref, spec, flag_tol=0)
    assert np.all(got["z_reion"] == -1) and got["neutral_fraction"].min() > 0.99
    # (b) everything ionises
    n_ion = W.nion_from_density(density, fbar=50.0)
    got = run_device(api, spec, density, n_ion)
    assert np.all(got["neutral_fraction"] == 0) and np.all(got["z_reion"] == np.float32(9.0))
    # (c) the radius loop stops early (M_min > RtoM(R)): no partial ionisation is assigned
    spec = W.ionize_spec(n, r_bubble_max=10.0, r_lowest=3)
    n_ion = W.nion_from_density(density)
    got = run_device(api, spec, density, n_ion)
    ref = oracle.ionize_grids(spec, density, n_ion)
    compare(got, ref, spec)
    assert set(np.unique(got["neutral_fraction"])) <= {0.0, 1.0}
    # (d) MINIMIZE_MEMORY: no temperature array at all
    spec = W.ionize_spec(n, r_bubble_max=10.0, minimize_memory=1)
    got = run_device(api, spec, density, n_ion)
    assert "kinetic_temperature" not in got
    # (e) unsupported option -> ValueError status, not a crash
    spec = W.ionize_spec(n, recomb_model=2)
    with pytest.raises(RuntimeError, match="status 3"):
        run_device(api, spec, density, n_ion)


def test_shard_phases_equal_single_pass(api):
    """R-loop sharding (world = 3 emulated on one GPU): max-reduced first_cross + finish
    must reproduce the single-pass result bit for bit."""
    import torch

    n = 48
    spec = W.ionize_spec(n, r_bubble_max=20.0)
    density = torch.from_numpy(W.density_field_numpy(n, seed=5)).cuda()
    n_ion = W.nion_from_density(density)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    world = 3
    masks = []
    for rank in range(world):
        fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
        api.ionize_shard_radii(spec, rank, world, fc, density, n_ion)
        masks.append(fc.clone())
    reduced = torch.stack(masks).max(dim=0).values.contiguous()
    buf2, box2, rep2 = api.ionize_shard_finish(spec, reduced, density, n_ion)
    torch.cuda.synchronize()
    assert torch.equal(buf.neutral_fraction, buf2.neutral_fraction)
    assert torch.equal(buf.z_reion, buf2.z_reion)
    assert torch.equal(buf.kinetic_temperature, buf2.kinetic_temperature)
    assert rep.global_xH == rep2.global_xH
    assert box.mean_f_coll == box2.mean_f_coll
    # world = 1: the only rank is the owner, so it transforms the emissivity for the cell-scale
    # step at the end of its shard phase and the finish step reuses it
    fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
    api.ionize_shard_radii(spec, 0, 1, fc, density, n_ion)
    buf3, box3, rep3 = api.ionize_shard_finish(spec, fc, density, n_ion)
    torch.cuda.synchronize()
    assert torch.equal(buf.neutral_fraction, buf3.neutral_fraction)
    assert torch.equal(buf.kinetic_temperature, buf3.kinetic_temperature)
    assert rep.global_xH == rep3.global_xH


@pytest.mark.parametrize("r_lowest", [2, 3])
def test_closed_form_shard_phases_with_a_radius_floor_equal_single_pass(api, r_lowest):
    """Closed-form Eulerian shards whose loop stops above the cell scale (r_lowest >= 2), world = 3: some
    rank's stride then ends on a radius whose successor lies between 1 and the floor.  No sweep is paired
    with, and no band is predicted for, a radius that does not run; the max-reduced first crossings and
    the finish must still be the single pass bit for bit (64-point lines: banded barrier and two radii
    per pass-X sweep are both in play)."""
    import torch

    n, world = 64, 3
    spec = W.ionize_spec(n, mode=W.FCOLL_ERFC, r_bubble_max=10.0, r_lowest=r_lowest)
    # the case in question: a rank whose last radius R has 1 <= R - world < r_lowest
    lasts = [[R for R in range(spec.n_radii - 1 - rank, 0, -world) if R >= r_lowest][-1] for rank in range(world)]
    assert any(1 <= R - world < r_lowest for R in lasts), lasts
    density = torch.from_numpy(W.density_field_numpy(n, seed=6)).cuda()
    buf, box, rep = api.ionize_grids(spec, density)
    assert 0.005 < float((buf.neutral_fraction == 0).float().mean()) < 0.98
    masks = []
    for rank in range(world):
        fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
        api.ionize_shard_radii(spec, rank, world, fc, density)
        masks.append(fc.clone())
    reduced = torch.stack(masks).max(dim=0).values.contiguous()
    buf2, box2, rep2 = api.ionize_shard_finish(spec, reduced, density)
    torch.cuda.synchronize()
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature"):
        assert torch.equal(getattr(buf, name), getattr(buf2, name)), name
    assert rep.global_xH == rep2.global_xH


def _emulated_slab_finish(api, spec, world, density, n_ion, **kw):
    """The sharded pass with the finish phase by cell slabs, the ranks of `world` run one after the
    other on the one GPU: every rank's shard phase, exchange 1 (packed first crossings by slab, through
    the library's pack / OR-unpack kernels), every rank's slab finish with exchange 2 done by copying
    the chunk sums between the ranks' calls.  Two rounds of finishes: the first collects every rank's
    chunk sums, the second hands every rank all of them (what the all-gather does).  Returns the box
    assembled from the ranks' slabs and every rank's report."""
    import torch

    ntot = density.numel()
    slabs = [api.shard_slab(spec, r, world) for r in range(world)]
    assert slabs[0]["cell_begin"] == 0 and slabs[-1]["cell_end"] == ntot
    for a, b in zip(slabs[:-1], slabs[1:]):
        assert a["cell_end"] == b["cell_begin"] and a["chunk_end"] == b["chunk_begin"]
        assert a["cell_end"] % 512 == 0
    packed = []
    for rank in range(world):
        fc = torch.zeros(density.shape, dtype=torch.uint8, device="cuda")
        api.ionize_shard_radii(spec, rank, world, fc, density, n_ion, want_report=False, **kw)
        packed.append(api.shard_pack_mask_bits(fc))
        del fc
    saved = {}
    bufs, reps = [None] * world, [None] * world
    for rnd in range(2):
        for rank in range(world):
            sl = slabs[rank]
            w0, w1 = sl["cell_begin"] // 32, (sl["cell_end"] + 31) // 32
            # only the slab's cells of first_cross are valid: everything else is poisoned
            fc = torch.full((ntot,), 7, dtype=torch.uint8, device="cuda")
            pieces = torch.stack([packed[q][w0:w1] for q in range(world)]).contiguous()
            if sl["cell_end"] > sl["cell_begin"]:
                api.shard_or_unpack_mask_bits(pieces, fc[sl["cell_begin"]:sl["cell_end"]])

            def exchange(st, local_status, rank=rank, rnd=rnd):
                assert local_status == 0 and st.rank == rank and st.world == world
                assert (st.chunk_begin, st.chunk_end) == (slabs[rank]["chunk_begin"], slabs[rank]["chunk_end"])
                stars = api.device_view(st.partials_stars, st.n_chunks, "f8")
                xh = api.device_view(st.partials_xh, st.n_chunks, "f8")
                if rnd == 0:
                    saved[rank] = (stars[st.chunk_begin:st.chunk_end].clone(),
                                   xh[st.chunk_begin:st.chunk_end].clone())
                    stars.zero_(), xh.zero_()  # nothing of this rank's own may survive by accident
                else:
                    stars.fill_(float("nan")), xh.fill_(float("nan"))
                    for q in range(world):
                        stars[slabs[q]["chunk_begin"]:slabs[q]["chunk_end"]] = saved[q][0]
                        xh[slabs[q]["chunk_begin"]:slabs[q]["chunk_end"]] = saved[q][1]
                return 0

            buf = api.IonizeBuffers(density, need_nion=spec.fcoll_mode != 0,
                                    minimize_memory=bool(spec.minimize_memory))
            buf.z_reion[...] = 123.0  # the sweep writes its slab only
            bufs[rank], _, reps[rank] = api.ionize_shard_finish_slab(
                spec, fc, rank, world, density, n_ion, buffers=buf, exchange=exchange, **kw)
            torch.cuda.synchronize()
            sl0, sl1 = sl["cell_begin"], sl["cell_end"]
            z = buf.z_reion.view(-1)
            assert bool((z[:sl0] == 123.0).all()) and bool((z[sl1:] == 123.0).all())
    box = {}
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature"):
        if getattr(bufs[0], name) is None:
            continue
        box[name] = torch.cat([getattr(bufs[r], name).view(-1)[slabs[r]["cell_begin"]:slabs[r]["cell_end"]]
                               for r in range(world)])
    if bufs[0].unnormalised_nion is not None:  # Eulerian models: the f_coll grid of index 0, whole on every rank
        box["unnormalised_nion"] = [b.unnormalised_nion.view(-1) for b in bufs]
    return box, reps


@pytest.mark.parametrize("n,world", [(64, 2), (64, 3), (64, 8), (128, 8), (64, 5)])
def test_slab_finish_equals_single_pass(api, n, world):
    """Round 5: the finish phase split by cell slabs (every rank sweeps the chunks of its slab from the
    combined first crossings of that slab; the chunk sums are all-gathered and reduced in the single
    pass' order on every rank) is BIT-identical to the single pass -- x_HI, z_reion, T_k, and global_xH
    / mean_f_coll on every rank (reference: IonisationBox.c:1031-1256 is per cell, :1531-1588 order
    independent)."""
    import torch

    spec = W.ionize_spec(n, r_bubble_max=20.0)
    assert api.shard_slab_supported(spec)
    density = torch.from_numpy(W.density_field_numpy(n, seed=11)).cuda()
    n_ion = W.nion_from_density(density)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    got, reps = _emulated_slab_finish(api, spec, world, density, n_ion)
    assert torch.equal(buf.neutral_fraction.view(-1), got["neutral_fraction"])
    assert torch.equal(buf.z_reion.view(-1), got["z_reion"])
    assert torch.equal(buf.kinetic_temperature.view(-1), got["kinetic_temperature"])
    assert 0.02 < rep.global_xH < 0.98
    for r in reps:
        assert r.global_xH == rep.global_xH
        assert r.mean_f_coll_out == rep.mean_f_coll_out
        assert list(r.f_coll_grid_mean)[:1] == list(rep.f_coll_grid_mean)[:1]


def test_slab_finish_with_xe_grid_and_previous_snapshot(api):
    """The slab finish of a spin-temperature run that is not the first snapshot: the x_e and T_k inputs
    and the previous z_reion are read per cell of the slab."""
    import torch

    n, world = 64, 3
    z_dim = 256  # the three-grid pass Z serves 256/512/1024-point z-lines
    spec = W.ionize_spec(n, r_bubble_max=12.0, hii_dim_z=z_dim, use_ts_fluct=1, first_snapshot=0)
    if not api.shard_slab_supported(spec):
        pytest.skip("no fused x_e path at this line length")
    g = torch.Generator(device="cpu").manual_seed(3)
    shape = (n, n, z_dim)
    density = torch.from_numpy(W.density_field_numpy(shape, seed=4)).cuda()
    n_ion = W.nion_from_density(density)
    xe = (0.05 * torch.rand(shape, generator=g)).float().cuda()
    Tn = (20.0 + 5.0 * torch.rand(shape, generator=g)).float().cuda()
    prev_z = torch.where(torch.rand(shape, generator=g) < 0.2, torch.tensor(11.5), torch.tensor(-1.0)).float().cuda()
    kw = dict(xe=xe, Tneutral=Tn, prev_z_reion=prev_z)
    buf, box, rep = api.ionize_grids(spec, density, n_ion, **kw)
    got, reps = _emulated_slab_finish(api, spec, world, density, n_ion, **kw)
    assert torch.equal(buf.neutral_fraction.view(-1), got["neutral_fraction"])
    assert torch.equal(buf.z_reion.view(-1), got["z_reion"])
    assert torch.equal(buf.kinetic_temperature.view(-1), got["kinetic_temperature"])
    assert all(r.global_xH == rep.global_xH for r in reps)


@pytest.mark.parametrize("mode,ts", [("erfc", 0), ("table", 0), ("erfc", 1), ("table", 1)])
def test_slab_finish_of_the_eulerian_models(api, mode, ts):
    """The Eulerian source models (closed form and table modes, with and without the x_e grid of a
    spin-temperature run) through the finish by cell slabs: every rank computes the cell-scale radius'
    f_coll grid and its box mean (replicated sweeps of one grid), the ONE sweep that applies mask + barrier +
    post-loop runs on the rank's slab.  Bit-identical to the single pass incl. global x_HI on every rank; the
    f_coll grid of index 0 (box->unnormalised_nion) is whole on every rank."""
    import torch

    n, nz, world = 64, 256, 3
    fmode = W.FCOLL_ERFC if mode == "erfc" else W.FCOLL_TABLE_EXP
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=10.0, use_ts_fluct=ts)
    if mode == "table":
        _install_table(spec)
    assert api.shard_slab_supported(spec)
    shape = (n, n, nz)
    density = torch.from_numpy(W.density_field_numpy(shape, seed=6)).cuda()
    kw = {}
    if ts:
        rng = np.random.default_rng(11)
        kw["xe"] = torch.from_numpy((-0.05 + 0.7 * rng.random(shape) ** 2).astype(np.float32)).cuda()
        kw["Tneutral"] = torch.from_numpy((8.0 + 4.0 * rng.random(shape)).astype(np.float32)).cuda()
    buf, box, rep = api.ionize_grids(spec, density, None, **kw)
    got, reps = _emulated_slab_finish(api, spec, world, density, None, **kw)
    assert 0.005 < float((buf.neutral_fraction == 0).float().mean()) < 0.98
    assert float((buf.neutral_fraction < 1).float().mean()) > 0.5  # partial ionisations at the cell scale
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature"):
        assert torch.equal(getattr(buf, name).view(-1), got[name]), name
    for r in range(world):
        assert torch.equal(buf.unnormalised_nion.view(-1), got["unnormalised_nion"][r])
        assert reps[r].global_xH == rep.global_xH


def test_c_level_slab_finish_on_one_rank_communicator(api):
    """c21cm_ionize_sharded on a one-rank RCCL communicator takes the slab path (pack, OR-unpack, slab
    finish, the agreement) and equals the single pass; C21CM_SHARD_FINISH=owner keeps the owner finish."""
    import os
    import torch

    n = 64
    spec = W.ionize_spec(n, r_bubble_max=20.0)
    density = torch.from_numpy(W.density_field_numpy(n, seed=11)).cuda()
    n_ion = W.nion_from_density(density)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    lib = api.load()
    api.shard_init_single()
    try:
        for bc in (False, True, None):
            b2, _, r2 = api.ionize_sharded(spec, density, n_ion, broadcast=bc)
            torch.cuda.synchronize()
            assert lib.c21cm_shard_last_finish_was_slab() == 1
            assert torch.equal(buf.neutral_fraction, b2.neutral_fraction)
            assert torch.equal(buf.z_reion, b2.z_reion)
            assert torch.equal(buf.kinetic_temperature, b2.kinetic_temperature)
            assert r2.global_xH == rep.global_xH
        os.environ["C21CM_SHARD_FINISH"] = "owner"
        b3, _, r3 = api.ionize_sharded(spec, density, n_ion)
        torch.cuda.synchronize()
        assert lib.c21cm_shard_last_finish_was_slab() == 0
        assert torch.equal(buf.neutral_fraction, b3.neutral_fraction) and r3.global_xH == rep.global_xH
        # host (numpy) arrays through the slab finish: staged, the slab copied back
        import numpy as np

        dn, nn = density.cpu().numpy(), n_ion.cpu().numpy()
        os.environ.pop("C21CM_SHARD_FINISH")
        b4, _, r4 = api.ionize_sharded(spec, dn, nn)
        assert lib.c21cm_shard_last_finish_was_slab() == 1
        np.testing.assert_array_equal(b4.neutral_fraction, buf.neutral_fraction.cpu().numpy())
        assert r4.global_xH == rep.global_xH
    finally:
        os.environ.pop("C21CM_SHARD_FINISH", None)
        api.shard_finalize()


@pytest.mark.parametrize("n,r_max", [(64, 20.0), (128, 17.0), (64, 9.0)])
def test_two_radii_per_sweep_equal_one(api, n, r_max, monkeypatch):
    """Pass X serves two radii per sweep (each spectrum tile read once, windowed and transformed
    twice; odd counts end on a single-radius step): same bits as one radius per sweep
    (C21CM_PAIR_RADII=0), single pass and sharded over 2 and 3 ranks (radius strides 2, 3)."""
    import torch

    spec = W.ionize_spec(n, r_bubble_max=r_max)
    density = torch.from_numpy(W.density_field_numpy(n, seed=77)).cuda()
    n_ion = W.nion_from_density(density)
    monkeypatch.setenv("C21CM_PAIR_RADII", "0")
    buf0, box0, rep0 = api.ionize_grids(spec, density, n_ion)
    monkeypatch.delenv("C21CM_PAIR_RADII")
    buf1, box1, rep1 = api.ionize_grids(spec, density, n_ion)
    torch.cuda.synchronize()
    assert 0.02 < float((buf0.neutral_fraction == 0).float().mean()) < 0.98
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature"):
        assert torch.equal(getattr(buf0, name), getattr(buf1, name)), name
    k = spec.n_radii
    assert list(rep0.f_coll_grid_mean[:k]) == list(rep1.f_coll_grid_mean[:k])
    assert rep0.global_xH == rep1.global_xH
    for world in (2, 3):
        masks = []
        for rank in range(world):
            fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
            api.ionize_shard_radii(spec, rank, world, fc, density, n_ion)
            masks.append(fc.clone())
        reduced = torch.stack(masks).max(dim=0).values.contiguous()
        buf2, _, rep2 = api.ionize_shard_finish(spec, reduced, density, n_ion)
        torch.cuda.synchronize()
        assert torch.equal(buf0.neutral_fraction, buf2.neutral_fraction), world
        assert torch.equal(buf0.kinetic_temperature, buf2.kinetic_temperature), world
        assert rep0.global_xH == rep2.global_xH


def test_two_radii_per_sweep_with_xe_grid(api, monkeypatch):
    """The same with the x_e grid of a spin-temperature run (three spectra per radius; the x_e
    spectrum rides a one-grid two-radius sweep on window a of both radii's tables)."""
    import torch

    n, nz = 64, 256
    spec = W.ionize_spec(n, hii_dim_z=nz, r_bubble_max=8.0, use_ts_fluct=1)
    rng = np.random.default_rng(11)
    density = torch.from_numpy(W.density_field_numpy((n, n, nz), seed=5)).cuda()
    n_ion = W.nion_from_density(density)
    xe = torch.from_numpy((-0.05 + 0.6 * rng.random((n, n, nz)) ** 3).astype(np.float32)).cuda()
    Tn = torch.from_numpy((8.0 + 4.0 * rng.random((n, n, nz))).astype(np.float32)).cuda()
    monkeypatch.setenv("C21CM_PAIR_RADII", "0")
    buf0, _, rep0 = api.ionize_grids(spec, density, n_ion, xe=xe, Tneutral=Tn)
    monkeypatch.delenv("C21CM_PAIR_RADII")
    buf1, _, rep1 = api.ionize_grids(spec, density, n_ion, xe=xe, Tneutral=Tn)
    torch.cuda.synchronize()
    assert 0.02 < float((buf0.neutral_fraction == 0).float().mean()) < 0.98
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature"):
        assert torch.equal(getattr(buf0, name), getattr(buf1, name)), name
    assert rep0.global_xH == rep1.global_xH


def test_full_size_properties(api):
    """Config-3 size (512^3, 40 radii): size-independent properties instead of the oracle.
    (1) run-to-run bit reproducibility (deterministic reductions),
    (2) global_xH equals mean(neutral_fraction),
    (3) monotonicity: scaling the emissivity up can only ionise more cells."""
    import torch

    n = 512
    spec = W.ionize_spec(n)
    assert spec.n_radii == 40
    density = W.density_field_torch(n)
    n_ion = W.nion_from_density(density)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    x1 = buf.neutral_fraction.clone()
    g1 = rep.global_xH
    assert g1 == pytest.approx(x1.double().mean().item(), rel=1e-6)
    assert 0.1 < g1 < 0.9
    buf.reset()
    buf, box, rep = api.ionize_grids(spec, density, n_ion, buffers=buf)
    assert torch.equal(x1, buf.neutral_fraction) and rep.global_xH == g1
    buf2, _, rep2 = api.ionize_grids(spec, density, n_ion * 1.5)
    assert bool(((buf2.neutral_fraction == 0) | (x1 != 0)).all())
    assert rep2.global_xH < g1


@pytest.mark.parametrize("mode", ["stars", "erfc"])
def test_config3_full_size_vs_oracle(api, oracle, mode):
    """BASELINE config 3 AT ITS OWN SIZE against the oracle: 512^3, 40 radii, the same
    density (and n_ion) realisation on both sides -- the fields are made on the GPU and copied to the host.
    Tolerances as everywhere (bench.parity_object): flag mismatch <= 2e-4, x_HI rtol 1e-4 / atol 5e-6 and z_reion
    equal on the agreeing cells, per-radius f_coll means rtol 1e-5, global x_HI to 2e-4.  G = 2 is the
    benchmark's Lagrangian model, G = 1 the closed-form erfc mode.  Reference: IonisationBox.c:773-1201."""
    import os
    import sys
    from pathlib import Path

    import torch

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    import bench

    n = 512
    fmode = W.FCOLL_STARS if mode == "stars" else W.FCOLL_ERFC
    spec = W.ionize_spec(n, mode=fmode)
    assert spec.n_radii == 40
    density = W.density_field_torch(n)
    n_ion = W.nion_from_density(density) if mode == "stars" else None
    buf, _, rep = api.ionize_grids(spec, density, n_ion)
    torch.cuda.synchronize()
    got = {"neutral_fraction": buf.neutral_fraction.cpu().numpy(), "z_reion": buf.z_reion.cpu().numpy(), "report": rep}
    oracle.set_threads(min(16, int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)))
    ref = oracle.ionize_grids(spec, density.cpu().numpy(), None if n_ion is None else n_ion.cpu().numpy(),
                              need_nion=mode != "stars")
    par = bench.parity_object(got, ref, spec.n_radii)
    assert 0.05 < par["ionised_fraction"] < 0.95, par
    assert par["pass"], par
    assert abs(par["d_global_xH"]) < 2e-4, par


def test_config4_1024_cubed_properties_and_sharding(api):
    """Config 4 (BASELINE.json: ComputeIonizedBox HII_DIM = 1024, R loop sharded): the whole
    1024^3 x 40-radii workload -- 1024-point line passes on the x-blocked split layout, the
    wave-level fused pass Z of 1024-point lines, 28 GB of workspace -- through size-independent
    properties: (1) global_xH equals mean(neutral_fraction), (2) run-to-run bit reproducibility,
    (3) the sharded path (two shard phases, uint8 max-reduce, finish phase; world = 2 emulated in
    one process, reference: IonisationBox.c:1531-1588 is order independent) is BIT-identical to
    the single pass (neutral fraction, z_reion, global x_HI)."""
    import torch

    n = 1024
    spec = W.ionize_spec(n)
    assert spec.n_radii == 40
    density = W.density_field_torch(n)
    n_ion = W.nion_from_density(density)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    x1 = buf.neutral_fraction.clone()
    z1 = buf.z_reion.clone()
    g1 = rep.global_xH
    assert g1 == pytest.approx(x1.double().mean().item(), rel=1e-6)
    assert 0.1 < g1 < 0.9
    buf.reset()
    buf, box, rep = api.ionize_grids(spec, density, n_ion, buffers=buf)
    assert torch.equal(x1, buf.neutral_fraction) and rep.global_xH == g1
    world = 2
    reduced = None
    for rank in range(world):
        fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
        api.ionize_shard_radii(spec, rank, world, fc, density, n_ion, want_report=False)
        reduced = fc if reduced is None else torch.maximum(reduced, fc)
        del fc
    buf.reset()
    buf, _, rep2 = api.ionize_shard_finish(spec, reduced, density, n_ion, buffers=buf)
    torch.cuda.synchronize()
    assert torch.equal(x1, buf.neutral_fraction)
    assert torch.equal(z1, buf.z_reion)
    assert rep2.global_xH == g1
    del reduced, buf, x1, z1, density, n_ion
    torch.cuda.empty_cache()
    api.load().c21cm_release_device_cache()  # 28 GB of workspace slots back to the pool


def test_bench_sharded_plumbing_on_one_rank():
    """bench.py --force-shard: the multi-GPU code path (shard phase without report, RCCL
    max-reduce of the uint8 mask, finish phase, x_HI broadcast) on a one-rank RCCL group; the
    result must equal the single-GPU path's."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    base = [sys.executable, str(root / "bench.py"), "--hii-dim", "128", "--steps", "2", "--warmup",
            "1", "--full", "--no-cpu-baseline", "--no-kernel-roofline", "--no-abi", "--config4-dim", "256"]
    outs = []
    for extra in ([], ["--force-shard"]):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == 1, p.stdout[-2000:]  # exactly one JSON line, no library banners
        outs.append(json.loads(lines[0]))
    single, shard = outs
    assert "sharded" in shard["config"]["parallelism"] and single["config"]["parallelism"] == "single GPU"
    assert shard["config"]["global_xH"] == single["config"]["global_xH"]
    assert 0.05 < single["config"]["global_xH"] < 0.95
    check_sharded_bench_objects(shard, world=1, config4_dim=256)
    assert "single_gpu_same_run" not in single and "config4" not in single


def check_sharded_bench_objects(line, world, config4_dim):
    """What a sharded bench line carries since round 4: the single-GPU time of
    the SAME run with the resulting speedup, and BASELINE config 4 (here a smaller box stands in for
    1024^3) sharded over the same ranks with its own same-run single-GPU time, per-rank phases and
    the same global x_HI sharded and unsharded."""
    same = line["single_gpu_same_run"]
    assert same["ms_per_step"] > 0 and line["speedup"] == pytest.approx(same["ms_per_step"] / line["ms_per_step"])
    c4 = line["config4"]
    assert c4["hii_dim"] == config4_dim and c4["n_gpus"] == world and c4["n_radii"] >= 30
    assert c4["ms_per_step"] > 0 and c4["single_gpu_same_run"]["ms_per_step"] > 0
    assert c4["speedup"] == pytest.approx(c4["single_gpu_same_run"]["ms_per_step"] / c4["ms_per_step"])
    assert c4["global_xH"] == c4["global_xH_single_gpu"] and 0.05 < c4["global_xH"] < 0.95
    if "shard_phases_ms_per_rank" in c4:  # the C-level exchange (RCCL)
        assert len(c4["shard_phases_ms_per_rank"]) == world and c4["rccl_comm_count"] == world


def test_bench_two_ranks_on_one_gpu():
    """The sharded path with world_size = 2 for real: two processes launched the way the driver
    launches them (torch.distributed.run), both on the one GPU of the box, exchanging the mask
    through gloo (RCCL refuses two ranks on one device).  Rank 1 owns radius 0 and finishes;
    the x_HI it broadcasts must equal the single-process result."""
    import json
    import socket
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    common = ["--hii-dim", "128", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
              "--no-kernel-roofline", "--no-abi", "--config4-dim", "256"]
    p = subprocess.run([sys.executable, str(root / "bench.py")] + common, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    single = json.loads(p.stdout.strip())
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                        str(port), str(root / "bench.py"), "--gpus", "2", "--backend", "gloo"]
                       + common, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    two = json.loads(lines[0])
    assert two["n_gpus"] == 2 and "sharded x2" in two["config"]["parallelism"]
    assert two["config"]["global_xH"] == single["config"]["global_xH"]
    check_sharded_bench_objects(two, world=2, config4_dim=256)


def test_bench_plain_line_is_the_headline_and_full_adds_the_rest():
    """A plain bench.py run carries the headline and nothing that takes runs of its own; --full adds the
    per-kernel roofline, the library-default allocation timing and the ABI timing (the CPU leg is left out here
    for time) around the same timed steps, with the same result."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    base = [sys.executable, str(root / "bench.py"), "--hii-dim", "128", "--steps", "2", "--warmup", "1"]
    env = dict(os.environ)
    env.pop("C21CM_WS_PLACE", None)
    lines = []
    for extra in ([], ["--full", "--no-cpu-baseline"]):
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        out = p.stdout.strip().splitlines()
        assert len(out) == 1, p.stdout[-2000:]
        lines.append(json.loads(out[0]))
    plain, full = lines
    for ln in lines:
        assert ln["metric"].startswith("IonizeBox cells/sec (128^3 HII_DIM, ")
        assert ln["unit"] == "cells/s" and ln["higher_is_better"] is True and ln["dtype"] == "f32"
        assert ln["steps"] == 2 and ln["warmup"] == 1 and ln["n_gpus"] == 1
        assert ln["value"] == pytest.approx(128.0 ** 3 / (ln["ms_per_step"] * 1e-3))
        assert ln["roofline"]["r_loop"]["ms"] > 0
    assert plain["config"]["global_xH"] == full["config"]["global_xH"]
    assert not {"default_allocation", "abi", "abi_ms", "h2d_d2h_ms", "cpu_baseline"} & set(plain)
    assert not [k for k in plain if k.startswith("parity_")]
    assert plain["roofline"]["kernel"] == "R loop (all kernels)" and "other_kernels" not in plain["roofline"]
    assert full["default_allocation"]["ms_per_step"] > 0 and "abi" in full
    assert full["roofline"]["other_kernels"] and "cpu_baseline" not in full


@pytest.mark.parametrize("mode,n,nz,device_resident", [
    ("stars", 64, None, True),     # native sizes: fused radii > 0, unfused cell-scale radius
    ("stars", 50, None, False),    # generic (rocFFT) per-radius sequence with the mask
    ("erfc", 64, 128, True),       # Eulerian mask path, non-cubic
    ("table", 48, None, False),
    ("stars_ts", 64, None, True),
])
def test_ionise_entire_sphere(api, oracle, mode, n, nz, device_resident):
    """AstroOptions.IONISE_ENTIRE_SPHERE: every cell that crosses the barrier at radius R flags
    the cells closer than R (strict, nearest periodic image) as ionised; z_reion stays with the
    centres (IonisationBox.c:1150-1158, bubble_helper_progs.c:262-418).  The spheres make the
    comparison with the oracle unforgiving -- a centre whose barrier test flips in the float32
    transform noise moves a whole sphere -- so the workloads keep a margin around the barrier."""
    fmode = {"stars": W.FCOLL_STARS, "stars_ts": W.FCOLL_STARS, "erfc": W.FCOLL_ERFC,
             "table": W.FCOLL_TABLE_EXP}[mode]
    kw = {}
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=12.0,
                         use_ts_fluct=int(mode == "stars_ts"))
    spec.ionise_entire_sphere = 1
    shape = (n, n, nz or n)
    density = W.density_field_numpy(shape, seed=21)
    n_ion = W.nion_from_density(density, fbar=0.7) if fmode == W.FCOLL_STARS else None
    if mode == "table":
        _install_table(spec)
    if fmode == W.FCOLL_ERFC:
        spec.mean_f_coll *= 0.6  # fewer crossings: spheres with room around them
    elif fmode == W.FCOLL_TABLE_EXP:
        spec.mean_f_coll *= 1.3
    if mode == "stars_ts":
        rng = np.random.default_rng(3)
        kw = dict(xe=(0.3 * rng.random(shape) ** 3).astype(np.float32),
                  Tneutral=(8.0 + 4.0 * rng.random(shape)).astype(np.float32))
    ref = oracle.ionize_grids(spec, density, n_ion, need_nion=fmode != W.FCOLL_STARS, **kw)
    got = run_device(api, spec, density, n_ion, device_resident=device_resident, **kw)
    ion_g, ion_r = got["neutral_fraction"] == 0, ref["neutral_fraction"] == 0
    assert 0.03 < ion_r.mean() < 0.97
    assert np.mean(ion_g != ion_r) <= 1e-3
    # the centres (cells that crossed themselves) carry z_reion; they agree like the plain method
    cen_g, cen_r = got["z_reion"] > 0, ref["z_reion"] > 0
    assert np.mean(cen_g != cen_r) <= 2e-4
    assert cen_r.sum() < ion_r.sum()  # spheres ionise more than their centres
    assert not (cen_r & ~ion_r).any() and not (cen_g & ~ion_g).any()
    same = ion_g == ion_r
    np.testing.assert_allclose(got["neutral_fraction"][same], ref["neutral_fraction"][same],
                               rtol=1e-4, atol=5e-6)
    # against the centre method: a superset of its ionised cells, identical centres
    spec.ionise_entire_sphere = 0
    plain = oracle.ionize_grids(spec, density, n_ion, need_nion=fmode != W.FCOLL_STARS, **kw)
    assert not ((plain["neutral_fraction"] == 0) & ~ion_r & (plain["z_reion"] > 0)).any()
    np.testing.assert_array_equal(plain["z_reion"] > 0, cen_r)


def test_ionise_entire_sphere_shape(api):
    """One crossing cell: the flagged cells are exactly |x - c|^2 < (R in cells)^2 over the nearest
    periodic images, with R formed in float as update_in_sphere does."""
    n, nz = 32, 48
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=W.FCOLL_ERFC, r_bubble_max=12.0)
    spec.ionise_entire_sphere = 1
    spec.hii_filter = 0
    # a single steep peak near a corner (wraps in all three axes) on an empty, underdense box
    density = np.full((n, n, nz), -0.9, np.float32)
    c = (1, n - 2, nz - 1)
    density[c] = 40.0
    spec.mean_f_coll = 1e-4
    spec.fix_mean = 0
    got = run_device(api, spec, density)
    ion = got["neutral_fraction"] == 0
    cen = np.argwhere(got["z_reion"] > 0)
    assert len(cen) >= 1 and ion.sum() > len(cen)
    # reconstruct: every centre's largest crossing radius is unknown, but the union must be a
    # union of strict lattice spheres around centres with radii from the ladder
    rsq = [float(np.float32(np.float32(np.float32(spec.R[r] / np.float32(spec.box_len)) * n)) ** 2)
           for r in range(spec.n_radii)]
    ii, jj, kk = np.meshgrid(np.arange(n), np.arange(n), np.arange(nz), indexing="ij")
    best = None
    for r in range(spec.n_radii - 1, -1, -1):  # the peak's own sphere: the largest radius that fits
        d2 = np.zeros((n, n, nz))
        for ax, (g, m, cc) in enumerate(((ii, n, c[0]), (jj, n, c[1]), (kk, nz, c[2]))):
            d = np.abs(g - cc)
            d2 += np.minimum(d, m - d) ** 2
        sphere = d2 < rsq[r]
        if not (sphere & ~ion).any():
            best = sphere
            break
    assert best is not None and best.sum() > 7
    # all flagged cells lie in the union of spheres around the centres: check the peak's sphere is
    # fully flagged and nothing beyond the largest ladder radius from any centre is
    far = np.ones((n, n, nz), bool)
    for cx, cy, cz in cen:
        d2 = np.zeros((n, n, nz))
        for g, m, cc in ((ii, n, cx), (jj, n, cy), (kk, nz, cz)):
            d = np.abs(g - cc)
            d2 += np.minimum(d, m - d) ** 2
        far &= d2 >= rsq[-1]
    assert not (ion & far).any()


def test_ionise_entire_sphere_refusals(api):
    from recomb_helpers import recomb_spec
    spec = recomb_spec(16, model=2)
    spec.ionise_entire_sphere = 1
    density = W.density_field_numpy(16, seed=1)
    with pytest.raises(RuntimeError, match="IONISE_ENTIRE_SPHERE"):
        api.ionize_grids(spec, density, W.nion_from_density(density),
                         prev_nrec=np.zeros_like(density), whalo_sfr=np.zeros_like(density),
                         prev_z_reion=np.zeros_like(density))


@pytest.mark.parametrize("n", [64, 48])
def test_ionise_entire_sphere_shard_phases_equal_single_pass(api, n):
    """The sphere method is a function of the first-crossing mask, so the sharded phases
    (world = 3 emulated) reproduce the single pass bit for bit with it, on the native and the
    generic transform sizes."""
    import torch

    spec = W.ionize_spec(n, r_bubble_max=12.0)
    spec.ionise_entire_sphere = 1
    density = torch.from_numpy(W.density_field_numpy(n, seed=21)).cuda()
    n_ion = W.nion_from_density(density, fbar=0.7)
    buf, box, rep = api.ionize_grids(spec, density, n_ion)
    world, masks = 3, []
    for rank in range(world):
        fc = torch.zeros((n, n, n), dtype=torch.uint8, device="cuda")
        api.ionize_shard_radii(spec, rank, world, fc, density, n_ion)
        masks.append(fc.clone())
    reduced = torch.stack(masks).max(dim=0).values.contiguous()
    buf2, box2, rep2 = api.ionize_shard_finish(spec, reduced, density, n_ion)
    torch.cuda.synchronize()
    assert torch.equal(buf.neutral_fraction, buf2.neutral_fraction)
    assert torch.equal(buf.z_reion, buf2.z_reion)
    assert torch.equal(buf.kinetic_temperature, buf2.kinetic_temperature)
    assert rep.global_xH == rep2.global_xH
    ion = (buf.neutral_fraction == 0).float().mean().item()
    assert 0.03 < ion < 0.97 and (buf.z_reion > 0).sum() < (buf.neutral_fraction == 0).sum()


def test_eulerian_table_model_with_xe_grid_fused_mask_pass(api, oracle, pkg, monkeypatch):
    """Config 5's IonizedBox (Eulerian f_coll table + the x_e grid of a spin-temperature run) at a
    size the wave-level pass Z serves: the x_e spectrum stays in k-space until the radius' f_coll
    mean is known and its pass Z applies the barrier itself (c21hip_split_z_xe_mask, round 3) --
    bit-identical to the path that stores x_e(R) and runs eulerian_mask_kernel
    (C21CM_XE_MASK_FUSED=0), and equal to the oracle like the other table tests."""
    import torch

    S = pkg.structs
    n = 256

    def table_fn(r_index, dmin, dmax, table, user):
        x = dmin + (dmax - dmin) / (S.NDELTA_TABLE - 1.0) * np.arange(S.NDELTA_TABLE)
        y = np.log(0.02 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index))
        for i in range(S.NDELTA_TABLE):
            table[i] = y[i]
        return 0

    cb = S.TABLE_FN(table_fn)
    spec = W.ionize_spec(n, mode=W.FCOLL_TABLE_EXP, r_bubble_max=20.0, use_ts_fluct=1)
    spec.hii_filter = 0
    spec.table_fn = cb
    rng = np.random.default_rng(11)
    density = W.density_field_numpy(n, seed=7)
    xe = (0.3 * rng.random((n, n, n))).astype(np.float32)
    Tn = (50 + 10 * rng.random((n, n, n))).astype(np.float32)
    d, x, t = (torch.from_numpy(a).cuda() for a in (density, xe, Tn))
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("C21CM_XE_MASK_FUSED", fused)
        buf, _, rep = api.ionize_grids(spec, d, None, xe=x, Tneutral=t)
        torch.cuda.synchronize()
        out[fused] = (buf.neutral_fraction.clone(), buf.z_reion.clone(), rep.global_xH)
    assert torch.equal(out["0"][0], out["1"][0]) and torch.equal(out["0"][1], out["1"][1])
    assert out["0"][2] == out["1"][2]
    assert 0.01 < float((out["1"][0] == 0).float().mean()) < 0.99
    ref = oracle.ionize_grids(spec, density, xe=xe, Tneutral=Tn, need_nion=True)
    got = out["1"][0].cpu().numpy()
    assert np.mean((got == 0) != (ref["neutral_fraction"] == 0)) <= 2e-4
    assert out["1"][2] == pytest.approx(ref["report"].global_xH, abs=2e-4)



@pytest.mark.parametrize("r_lowest", [0, 2])
def test_closed_form_loop_deferred_barrier_equals_separate_sweep(api, r_lowest, monkeypatch):
    """CONST-ION-EFF closed form on the wave-level pass Z: the barrier of a radius (which needs the box
    mean of its f_coll grid) rides the NEXT radius' pass Z on a second dense buffer instead of its own
    sweep.  Same statements on the same floats: every output -- the f_coll grid of the last radius
    included, whichever buffer it was computed in -- equals the separate-sweep sequence
    (the default; C21CM_EUL_DEFER=1 selects the deferred form) bit for bit, single pass and sharded over 2 ranks."""
    import torch

    n, nz = 64, 512
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=W.FCOLL_ERFC, r_bubble_max=9.0)
    spec.r_lowest = r_lowest
    density = torch.from_numpy(W.density_field_numpy((n, n, nz), seed=21)).cuda()
    buf0, _, rep0 = api.ionize_grids(spec, density)
    torch.cuda.synchronize()
    monkeypatch.setenv("C21CM_EUL_DEFER", "1")  # opt-in: measured slower than the separate sweep
    buf1, _, rep1 = api.ionize_grids(spec, density)
    torch.cuda.synchronize()
    assert 0.02 < float((buf0.neutral_fraction == 0).float().mean()) < 0.98
    for name in ("neutral_fraction", "z_reion", "kinetic_temperature", "unnormalised_nion"):
        assert torch.equal(getattr(buf0, name), getattr(buf1, name)), name
    k = spec.n_radii
    assert list(rep0.f_coll_grid_mean[:k]) == list(rep1.f_coll_grid_mean[:k])
    assert rep0.global_xH == rep1.global_xH
    if r_lowest == 0:
        world, masks = 2, []
        for rank in range(world):
            fc = torch.zeros((n, n, nz), dtype=torch.uint8, device="cuda")
            api.ionize_shard_radii(spec, rank, world, fc, density)
            masks.append(fc)
        reduced = torch.maximum(masks[0], masks[1]).contiguous()
        buf2, _, rep2 = api.ionize_shard_finish(spec, reduced, density)
        torch.cuda.synchronize()
        assert torch.equal(buf0.neutral_fraction, buf2.neutral_fraction)
        assert rep0.global_xH == rep2.global_xH


@pytest.mark.parametrize("fmode", [W.FCOLL_ERFC, W.FCOLL_TABLE_EXP, W.FCOLL_TABLE_LINEAR])
@pytest.mark.parametrize("r_lowest", [0, 2])
@pytest.mark.parametrize("mass_dep_zeta", [False, True])
def test_closed_form_loop_banded_barrier_equals_dense_sweeps(api, fmode, r_lowest, mass_dep_zeta, monkeypatch,
                                                             capfd):
    """CONST-ION-EFF closed form on the wave-level pass Z (the default): the barrier of a radius is decided
    INSIDE its own pass Z from a predicted band of the mean fix (monotone test: cells on which both ends
    agree are final, the others carry a marker until the exact mean is known).  Every output equals the
    dense-sweep sequence (C21CM_EUL_BAND=0: dense f_coll grid + eulerian_mask_kernel per radius) bit for
    bit, single pass and sharded over 2 and 3 ranks; a prediction that is off (test hook
    C21CM_EUL_BAND_SHIFT) is detected on the device, the grid is rewound to its state before that radius and the
    loop reruns from there on the dense sweeps."""
    import torch

    # fmode: the same for the loops whose f_coll comes from a per-radius table (E-INTEGRAL / CONST-ION-EFF
    # with interpolation tables): there the table sweep (fcoll_eulerian_band_kernel) decides the cells
    n, nz = 64, 512
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=9.0)
    spec.r_lowest = r_lowest
    if fmode != W.FCOLL_ERFC:
        S = importlib.import_module("21cmfast_amd.structs")

        def table_fn(r_index, dmin, dmax, table, user):
            x = dmin + (dmax - dmin) / (S.NDELTA_TABLE - 1.0) * np.arange(S.NDELTA_TABLE)
            y = 0.03 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index)
            if fmode == W.FCOLL_TABLE_EXP:
                y = np.log(y)
            for i in range(S.NDELTA_TABLE):
                table[i] = y[i]
            return 0

        cb = S.TABLE_FN(table_fn)
        _TABLE_CB.append(cb)
        spec.table_fn = cb
        spec.mean_f_coll *= 1.6  # (the mean fix rescales the table: this is what sets the ionised fraction)
    if mass_dep_zeta:
        spec.mass_dep_zeta = 1
        spec.f_limit_acg = 1e-4
    density = torch.from_numpy(W.density_field_numpy((n, n, nz), seed=21)).cuda()
    monkeypatch.setenv("C21CM_EUL_BAND", "0")
    buf0, _, rep0 = api.ionize_grids(spec, density)
    torch.cuda.synchronize()
    monkeypatch.delenv("C21CM_EUL_BAND")
    monkeypatch.setenv("C21CM_EUL_BAND_DEBUG", "1")
    buf1, _, rep1 = api.ionize_grids(spec, density)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert "band fail=0" in err, err  # the banded sweeps ran (a miss, if any, was recovered inside the loop)
    monkeypatch.delenv("C21CM_EUL_BAND_DEBUG")
    assert 0.02 < float((buf0.neutral_fraction == 0).float().mean()) < 0.98
    names = ["neutral_fraction", "z_reion", "kinetic_temperature"]
    if r_lowest > 0:
        names.append("unnormalised_nion")  # the last radius' dense grid (index 0 rewrites it otherwise)
    for name in names:
        assert torch.equal(getattr(buf0, name), getattr(buf1, name)), name
    k = spec.n_radii
    if fmode == W.FCOLL_ERFC:
        assert list(rep0.f_coll_grid_mean[:k]) == list(rep1.f_coll_grid_mean[:k])
    else:
        # round 6: the banded table sweep is the epilogue of a second pass Z of the radius' spectrum (no delta_R
        # round trip) -- the same f_coll values as the dense sweep reads them, added per line block instead of per
        # sweep block: the means agree to the last bits of a double
        np.testing.assert_allclose(rep0.f_coll_grid_mean[:k], rep1.f_coll_grid_mean[:k], rtol=1e-14, atol=0)
    assert rep0.global_xH == rep1.global_xH
    # a band that misses: detected, rerun on the dense sweeps, same box
    monkeypatch.setenv("C21CM_EUL_BAND_SHIFT", "0.2")
    monkeypatch.setenv("C21CM_EUL_BAND_DEBUG", "1")
    buf3, _, rep3 = api.ionize_grids(spec, density)
    torch.cuda.synchronize()
    import re

    # (the closed form learns of a miss at the end of the loop, the table loops while they run)
    assert re.search(r"band fail=[1-9]|band miss at r=", capfd.readouterr().err)
    monkeypatch.delenv("C21CM_EUL_BAND_SHIFT")
    monkeypatch.delenv("C21CM_EUL_BAND_DEBUG")
    for name in names:
        assert torch.equal(getattr(buf0, name), getattr(buf3, name)), name
    assert rep0.global_xH == rep3.global_xH
    if r_lowest == 0:
        for world in (2, 3):
            masks = []
            for rank in range(world):
                fc = torch.zeros((n, n, nz), dtype=torch.uint8, device="cuda")
                api.ionize_shard_radii(spec, rank, world, fc, density)
                masks.append(fc)
            reduced = masks[0]
            for m in masks[1:]:
                reduced = torch.maximum(reduced, m)
            assert int((reduced == 255).sum()) == 0  # no marker survives a shard phase
            buf2, _, rep2 = api.ionize_shard_finish(spec, reduced.contiguous(), density)
            torch.cuda.synchronize()
            assert torch.equal(buf0.neutral_fraction, buf2.neutral_fraction)
            assert rep0.global_xH == rep2.global_xH


@pytest.mark.parametrize("fmode", [W.FCOLL_TABLE_EXP, W.FCOLL_TABLE_LINEAR])
def test_table_loop_with_xe_grid_banded_barrier_equals_dense_sweeps(api, fmode, monkeypatch, capfd):
    """Eulerian table models WITH an x_e grid (spin-temperature runs: config 5's ComputeIonizedBox): the
    x_e grid's pass Z also does the radius' table sweep and decides the cells on a predicted band of the
    mean fix (the barrier f mf zeta > 1 - x_e is monotone in mf); undecided cells leave (f, x_e) for the
    next sweep.  No dense f_coll grid, no fcoll_eulerian_kernel.  Same first crossings as the dense
    sequence (C21CM_EUL_BAND=0) -- the f_coll sums are added in another order, so the means agree to the
    last bits of a double and a cell would have to sit within 1e-16 of its barrier to differ --, single pass
    and sharded over 2 and 3 ranks; a forced miss (C21CM_EUL_BAND_SHIFT) is detected and rerun."""
    import re

    import torch

    S = importlib.import_module("21cmfast_amd.structs")
    n, nz = 64, 512

    def table_fn(r_index, dmin, dmax, table, user):
        x = dmin + (dmax - dmin) / (S.NDELTA_TABLE - 1.0) * np.arange(S.NDELTA_TABLE)
        y = 0.03 * (1 + np.maximum(x, -0.999)) ** 1.5 / (1 + 0.05 * r_index)
        if fmode == W.FCOLL_TABLE_EXP:
            y = np.log(y)
        for i in range(S.NDELTA_TABLE):
            table[i] = y[i]
        return 0

    cb = S.TABLE_FN(table_fn)
    _TABLE_CB.append(cb)
    spec = W.ionize_spec(n, hii_dim_z=nz, mode=fmode, r_bubble_max=9.0, use_ts_fluct=1)
    spec.table_fn = cb
    spec.mean_f_coll *= 1.6
    rng = np.random.default_rng(5)
    density = torch.from_numpy(W.density_field_numpy((n, n, nz), seed=21)).cuda()
    xe = torch.from_numpy((0.3 * rng.random((n, n, nz)) ** 2).astype(np.float32)).cuda()
    Tn = torch.from_numpy((50 + 10 * rng.random((n, n, nz))).astype(np.float32)).cuda()
    kw = dict(xe=xe, Tneutral=Tn)
    monkeypatch.setenv("C21CM_EUL_BAND", "0")
    buf0, _, rep0 = api.ionize_grids(spec, density, None, **kw)
    torch.cuda.synchronize()
    monkeypatch.delenv("C21CM_EUL_BAND")
    monkeypatch.setenv("C21CM_EUL_BAND_DEBUG", "1")
    buf1, _, rep1 = api.ionize_grids(spec, density, None, **kw)
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert "band fail=0" in err, err  # the banded sweeps ran (a miss, if any, was recovered inside the loop)
    monkeypatch.delenv("C21CM_EUL_BAND_DEBUG")
    assert 0.02 < float((buf0.neutral_fraction == 0).float().mean()) < 0.98
    names = ["neutral_fraction", "z_reion", "kinetic_temperature"]
    for name in names:
        assert torch.equal(getattr(buf0, name), getattr(buf1, name)), name
    k = spec.n_radii
    np.testing.assert_allclose(np.array(rep1.f_coll_grid_mean[:k]), np.array(rep0.f_coll_grid_mean[:k]), rtol=1e-13)
    assert rep0.global_xH == rep1.global_xH
    monkeypatch.setenv("C21CM_EUL_BAND_SHIFT", "0.2")
    monkeypatch.setenv("C21CM_EUL_BAND_DEBUG", "1")
    buf3, _, rep3 = api.ionize_grids(spec, density, None, **kw)
    torch.cuda.synchronize()
    assert re.search(r"band fail=[1-9]|band miss at r=", capfd.readouterr().err)
    monkeypatch.delenv("C21CM_EUL_BAND_SHIFT")
    monkeypatch.delenv("C21CM_EUL_BAND_DEBUG")
    for name in names:
        assert torch.equal(getattr(buf0, name), getattr(buf3, name)), name
    for world in (2, 3):
        masks = []
        for rank in range(world):
            fc = torch.zeros((n, n, nz), dtype=torch.uint8, device="cuda")
            api.ionize_shard_radii(spec, rank, world, fc, density, None, **kw)
            masks.append(fc)
        reduced = masks[0]
        for m in masks[1:]:
            reduced = torch.maximum(reduced, m)
        assert int((reduced == 255).sum()) == 0  # no marker survives a shard phase
        buf2, _, rep2 = api.ionize_shard_finish(spec, reduced.contiguous(), density, None, **kw)
        torch.cuda.synchronize()
        assert torch.equal(buf0.neutral_fraction, buf2.neutral_fraction)
        assert rep0.global_xH == rep2.global_xH
