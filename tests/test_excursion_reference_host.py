"""tests/excursion_reference.py on the host: pinned to the CPU oracle, held to the caps on the share of
cells it leaves undecided, and shown to notice what test_gpu_ionize.compare lets through.  No GPU.

The three corruptions of test_accounting_bites_where_compare_does_not and the old compare():
  * 20 flipped flags at 64^3 (7.6e-5 of the cells) pass compare() -- asserted here;
  * a cleared z-line and a shifted 16 x 16 tile of the first-crossing grid never reach compare(): it takes
    no first-crossing grid, so it lets both through as well.

The table modes (mode (t)) have their own three tests below: the oracle pin with the callback's extrema, the
caps of every box of test_gpu_table_cells.py, and four single-cell or single-number corruptions of e-64x512.
"""

import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import excursion_reference as X

W = importlib.import_module("21cmfast_amd.workloads")


@pytest.fixture(scope="module")
def restated():
    """name or box -> (spec, inputs, Restatement, e32 dict): computed once, read only."""
    cache = {}

    def get(key):
        if key not in cache:
            spec, inp = X.make_case(W, *X.CASES.get(key, key))
            cache[key] = (spec, inp) + X.restate(spec, inp)
        return cache[key]

    return get


@pytest.mark.parametrize("n", [32, 35])
@pytest.mark.parametrize("mode", ["a", "b", "c"])
def test_pinned_to_the_oracle(oracle, restated, mode, n):
    """The oracle (float32 transforms, its own radix order, a transform round trip at radius 0) against the
    restatement: the same flag on every flag-decided cell, z_reion following it, and its per-radius means
    within FACTOR = 4 x the deviation measured with numpy's float32 chain.

    Why 4 x and not 1 x: the measured deviation is that of ONE float32 implementation.  Away from radius 0 a
    per-radius mean is the DC coefficient rounded to float, and which way it rounds is the implementation's
    summation order; at radius 0 the oracle's grid has been through a transform pair that the numpy chain
    does not make.  The oracle is a second float32 implementation exactly as the device is, and is granted
    the factor the device is granted.  Its largest deviation as a multiple of the
    measured one (printed as `oracle mean deviation`): (a) 1.25 at 32^3, 1.36 at 35^3; (b) 1.25, 1.36;
    (c) 2.00 (at radius 0), 0.75."""
    spec, inp, ref, e = restated((mode, n, n, 12.0, 4242))
    out = oracle.ionize_grids(spec, inp.density, inp.n_ion, need_nion=mode == "c", **inp.kwargs())
    flag = out["neutral_fraction"] == 0
    print(f"oracle pin {mode} {n}^3: E32 {e['margin']:.2e}, mean deviation {e['mean']:.2e}, flag-undecided "
          f"{ref.flag_undecided_share:.2e}, ionised {flag.mean():.3f}")
    assert 0.05 < flag.mean() < 0.95
    wrong = ref.flag_decided & (flag != ref.decided_flag)
    assert not wrong.any(), np.argwhere(wrong)[:5]
    np.testing.assert_array_equal(out["z_reion"][ref.flag_decided],
                                  np.where(ref.decided_flag, X.F32(spec.redshift), X.F32(-1))[ref.flag_decided])
    means = np.array(out["report"].f_coll_grid_mean[:spec.n_radii])
    dev = np.abs(means - ref.f_coll_grid_mean) / ref.f_coll_grid_mean
    print(f"oracle mean deviation {mode} {n}^3: {dev.max() / e['mean']:.2f} x the measured one, at radius "
          f"{int(np.argmax(dev))} (bound {X.FACTOR} x)")
    assert ref.mean_tol == X.FACTOR * e["mean"] and dev.max() <= ref.mean_tol, (dev.max(), ref.mean_tol)
    # the float32 chain's own outputs pass the accounting
    X.check_outputs(ref, e["outputs"])


@pytest.mark.parametrize("name", list(X.CASES))
def test_caps_hold(restated, name):
    """At t = 4 E32 the accounting leaves out no more than 1e-4 of the flags and 1e-3 of the radii, on every
    box of test_gpu_excursion_cells.py; and the float32 chain differs from the float64 one in no decided
    cell.  The caps are conditions on the box (seed, zeta, r_bubble_max), never adjusted to a result."""
    spec, inp, ref, e = restated(name)
    fig = X.check_outputs(ref, e["outputs"])
    print(X.excursion_line(name + " (float32 chain on the host)", ref, e, fig))
    assert ref.flag_undecided_share <= X.FLAG_CAP
    assert ref.radius_undecided_share <= X.RADIUS_CAP
    assert 0.02 < ref.decided_flag.mean() < 0.98  # both branches
    assert len(np.unique(ref.cross_hi)) > spec.n_radii // 2  # the crossings spread over the radii


def _corrupt(out, **changes):
    new = {k: v.copy() for k, v in out.items()}
    for k, (where, value) in changes.items():
        new[k][where] = value
        if "shard_" + k in new:
            new["shard_" + k][where] = value
    return new


def test_accounting_bites_where_compare_does_not(oracle, restated):
    compare = importlib.import_module("test_gpu_ionize").compare
    spec, inp, ref, e = restated("a-64")
    good = e["outputs"]
    X.check_outputs(ref, good)
    n_cells = ref.xhi.size

    # (1) 20 flag-decided ionised cells turned neutral, consistently in every output
    ion = np.flatnonzero((ref.flag_decided & ref.decided_flag & (ref.xhi > 0.01)).ravel())
    pick = np.unravel_index(ion[:: len(ion) // 20][:20], ref.xhi.shape)
    assert len(pick[0]) == 20 and 20 / n_cells < 1e-4
    flipped = _corrupt(good, neutral_fraction=(pick, ref.xhi[pick].astype(X.F32)), z_reion=(pick, X.F32(-1)),
                       first_cross=(pick, 0))
    with pytest.raises(AssertionError, match="decided cells with the wrong flag: 20 cells"):
        X.check_outputs(ref, flipped)
    # ... which the oracle comparison of test_gpu_ionize.py accepts: the oracle's outputs with the same flips
    want = oracle.ionize_grids(spec, inp.density, inp.n_ion)
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    got["neutral_fraction"][pick] = ref.xhi[pick]
    got["z_reion"][pick] = -1
    got["report"] = SimpleNamespace(f_coll_grid_mean=list(want["report"].f_coll_grid_mean),
                                    global_xH=float(got["neutral_fraction"].mean(dtype=np.float64)))
    assert compare(got, want, spec) == 20 / n_cells

    # (2) one whole z-line of the first-crossing grid cleared
    fc = good["first_cross"]
    x, y = np.unravel_index(np.argmax((fc > 0).sum(axis=2)), fc.shape[:2])
    assert (ref.radius_decided[x, y] & (fc[x, y] > 0)).sum() > 10
    cleared = _corrupt(good, first_cross=((x, y), 0))
    with pytest.raises(AssertionError, match="decided cells with the wrong first-crossing radius"):
        X.check_outputs(ref, cleared)

    # (3) the index shifted by one in one 16 x 16 tile of one plane
    tile = (slice(16, 32), slice(32, 48), 7)
    assert (fc[tile] > 0).sum() > 10
    shifted = _corrupt(good, first_cross=(tile, np.where(fc[tile] > 0, fc[tile] + 1, 0)))
    with pytest.raises(AssertionError, match="decided cells with the wrong first-crossing radius"):
        X.check_outputs(ref, shifted)


# ---- the table loops: mode (t) of tests/excursion_reference.py ------------------------------------------------

S = importlib.import_module("21cmfast_amd.structs")


def _oracle_run(oracle, spec, inp, calls=None):
    X.install_table(spec, inp, S, calls)
    return oracle.ionize_grids(spec, inp.density, need_nion=True, **inp.kwargs())


@pytest.mark.parametrize("n", [32, 35])
@pytest.mark.parametrize("with_xe", [False, True], ids=["", "xe"])
@pytest.mark.parametrize("fmode", [X.FCOLL_TABLE_LINEAR, X.FCOLL_TABLE_EXP], ids=["linear", "exp"])
def test_table_modes_pinned_to_the_oracle(oracle, fmode, with_xe, n):
    """test_pinned_to_the_oracle for the table modes, with and without an x_e grid: flags on every
    flag-decided cell, z_reion, the per-radius means within the bound of the restatement (radius 0 keeps the
    documented departure: the oracle's grid has been through a transform pair there) -- and what the oracle
    hands its table callback, (r_index, dmin, dmax), against the restatement's own extrema -/+ 0.001 at the
    atol of 2e-5 that test_gpu_ionize.py::test_table_modes_parity grants the device."""
    spec, inp, ref, e = X.restated_table(W, (fmode, n, n, 12.0, 4242, with_xe, False))
    calls = []
    out = _oracle_run(oracle, spec, inp, calls)
    flag = out["neutral_fraction"] == 0
    print(f"oracle pin table mode {fmode} x_e {with_xe} {n}^3: E32 {e['margin']:.2e}, mean deviation "
          f"{e['mean']:.2e}, flag-undecided {ref.flag_undecided_share:.2e}, ionised {flag.mean():.3f}")
    assert 0.05 < flag.mean() < 0.95
    wrong = ref.flag_decided & (flag != ref.decided_flag)
    assert not wrong.any(), np.argwhere(wrong)[:5]
    np.testing.assert_array_equal(out["z_reion"][ref.flag_decided],
                                  np.where(ref.decided_flag, X.F32(spec.redshift), X.F32(-1))[ref.flag_decided])
    means = np.array(out["report"].f_coll_grid_mean[:spec.n_radii])
    dev = np.abs(means - ref.f_coll_grid_mean) / ref.f_coll_grid_mean
    print(f"oracle mean deviation table mode {fmode} x_e {with_xe} {n}^3: {dev.max() / e['mean']:.2f} x the "
          f"measured one, at radius {int(np.argmax(dev))} (bound {ref.mean_tol / e['mean']:.2f} x)")
    assert ref.mean_tol == X.FACTOR * e["mean"] + (X.EXP_F32ACC if fmode == X.FCOLL_TABLE_EXP else 0.0)
    assert dev.max() <= ref.mean_tol, (dev.max(), ref.mean_tol)
    # the callback: every radius once, from the largest down, over the restatement's extrema
    assert [c[0] for c in calls] == list(range(spec.n_radii - 1, -1, -1))
    np.testing.assert_allclose([c[1:] for c in calls], [ref.table_range[c[0]] for c in calls], rtol=0, atol=2e-5)
    # the float32 chain's own outputs pass the accounting
    X.check_outputs(ref, e["outputs"])


@pytest.mark.parametrize("name", list(X.TABLE_CASES))
def test_table_caps_hold(name):
    """test_caps_hold on every box of test_gpu_table_cells.py; one TABLE-CAPS line per box (DESIGN.md,
    Appendix C.1-T).  The caps are those of the other modes, unchanged."""
    spec, inp, ref, e = X.restated_table(W, name)
    fig = X.check_outputs(ref, e["outputs"])
    print(X.table_caps_line(name, spec, ref, e))
    print(X.excursion_line(name + " (float32 chain on the host)", ref, e, fig))
    assert ref.flag_undecided_share <= X.FLAG_CAP
    assert ref.radius_undecided_share <= X.RADIUS_CAP
    assert 0.02 < ref.decided_flag.mean() < 0.98  # both flags occur
    assert len(np.unique(ref.cross_hi)) > spec.n_radii // 2  # the crossings spread over the radii


def test_table_accounting_bites_where_compare_does_not(oracle):
    """Four corruptions of the float32 chain's own outputs of e-64x512, each no larger than what a slip in the
    marker, pending or rewind bookkeeping of the banded sweeps would leave; each must raise, by name.  The
    first two pass test_gpu_ionize.compare against the oracle, the only outside reference these loops had:
    the gap this accounting closes, kept on record."""
    compare = importlib.import_module("test_gpu_ionize").compare
    spec, inp, ref, e = X.restated_table(W, "e-64x512")
    good = e["outputs"]
    X.check_outputs(ref, good)
    n_cells = ref.xhi.size
    want = _oracle_run(oracle, spec, inp)
    assert "first_cross" not in want  # compare() is handed no first-crossing grid

    def accepted(got):
        got = dict(got)
        got["report"] = SimpleNamespace(f_coll_grid_mean=list(want["report"].f_coll_grid_mean),
                                        global_xH=float(got["neutral_fraction"].mean(dtype=np.float64)))
        return compare(got, want, spec)

    # cells the banded sweeps defer: decided, crossing at a banded radius (index >= 2) with f mean_f_coll /
    # mean zeta within 0.5 % of its threshold 1 (the least half-width of a band); no x_e grid here, so that
    # is a margin below 0.005
    decided = ref.flag_decided & ref.radius_decided
    deferred = decided & (ref.cross_hi >= 3) & (ref.margin_at_cross < 0.005) & (ref.xhi > 0.01)
    assert (ref.margin_at_cross[deferred] > ref.t).all() and deferred.sum() > 100
    cells = np.argwhere(deferred)

    # (1) one of them turned neutral, consistently in every output
    one = tuple(cells[len(cells) // 2])
    assert want["neutral_fraction"][one] == 0
    flipped = _corrupt(good, neutral_fraction=(one, X.F32(ref.xhi[one])), z_reion=(one, X.F32(-1)),
                       first_cross=(one, 0))
    with pytest.raises(AssertionError, match="decided cells with the wrong flag: 1 cells"):
        X.check_outputs(ref, flipped)
    got = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    got["neutral_fraction"][one] = ref.xhi[one]
    got["z_reion"][one] = -1
    assert accepted(got) == 1 / n_cells

    # (2) the first crossing of another moved to the next smaller radius
    two = tuple(cells[len(cells) // 3])
    assert good["first_cross"][two] == ref.cross_hi[two] - 1 >= 2
    moved = _corrupt(good, first_cross=(two, good["first_cross"][two] - 1))
    with pytest.raises(AssertionError, match="decided cells with the wrong first-crossing radius: 1 cells"):
        X.check_outputs(ref, moved)
    assert accepted(dict(want, first_cross=moved["first_cross"])) == 0  # ... which compare() never reads

    # (3) a marker left behind
    marked = _corrupt(good, first_cross=(tuple(cells[len(cells) // 4]), 255))
    with pytest.raises(AssertionError, match=r"first_cross holds a marker \(255\): 1 cells"):
        X.check_outputs(ref, marked)

    # (4) one per-radius mean off by 1e-6 relative (compare() grants 1e-5)
    r = spec.n_radii // 2
    means = good["f_coll_grid_mean"].copy()
    means[r] *= 1 + 1e-6
    with pytest.raises(AssertionError, match=rf"f_coll_grid_mean\[{r}\]"):
        X.check_outputs(ref, dict(good, f_coll_grid_mean=means))


# ---- the recombination loop: tests/recomb_excursion_reference.py ---------------------------------------------

import recomb_excursion_reference as RX  # noqa: E402

#   variant: (recomb model, CELL_RECOMB, x_e grid, Lagrangian)
RECOMB_VARIANTS = {"cell": (2, 1, False, True), "filtered": (2, 0, False, True), "xe": (2, 1, True, True),
                   "homogeneous": (1, 1, False, True), "eulerian": (2, 0, False, False)}


@pytest.mark.parametrize("n", [32, 35])
@pytest.mark.parametrize("variant", list(RECOMB_VARIANTS))
def test_recomb_pinned_to_the_oracle(oracle, variant, n):
    """The oracle's own float32 outputs as the `device` of check_recomb_outputs: crossing flags and radii
    through its mean_free_path, Gamma_12 at the crossing, z_reion against the previous one, x_HI, the
    per-radius means and its N_rec recomputed from its own Gamma_12 and x_HI.

    The oracle sends radius 0 through a float32 transform pair; the float32 chain of this pin does so too, with
    the oracle's own transforms (recomb_excursion_reference.restate, round_trip0), and the x_HI bound is taken
    from that chain.  Multiples of the MEASURED deviations the oracle used (bound: FACTOR = 4), printed as
    `oracle used`: per-radius mean 1.25 (32^3, Lagrangian), 1.36 (35^3, Lagrangian), 1.00 / 1.34 (Eulerian);
    Gamma_12 0.26 ... 0.47 of the relative-plus-absolute pair; x_HI 1.00 (32^3; it IS that round trip) and 0.83
    (35^3) in the Lagrangian variants, 0.75 / 1.01 in the Eulerian one; N_rec 0 ulp."""
    model, cell, ts, lag = RECOMB_VARIANTS[variant]
    key = (n, n, model, cell, ts, lag, 10.0, 4242)
    c = RX.restated(key, lambda g: oracle.fft_c2r(oracle.fft_r2c(g) / X.F32(g.size), g.shape[2]))
    print(RX.caps_line(key, c))
    out = oracle.ionize_grids(c.spec, c.inp.density, need_nion=not lag, **c.inp.kwargs())
    out["f_coll_grid_mean"] = np.array(out["report"].f_coll_grid_mean[:c.spec.n_radii])
    assert 0.05 < (out["mean_free_path"] > 0).mean() < 0.95
    fig = RX.check_recomb_outputs(c.ref, out)
    print(f"oracle used {variant} {n}^3: mean {fig['mean_dev_over_bound'] * X.FACTOR:.2f} x the measured deviation, "
          f"Gamma_12 {fig['gamma_over_bound'] * X.FACTOR:.2f} x, x_HI {fig['xhi_dev'] / c.ref.xhi_tol * X.FACTOR:.2f} x, "
          f"N_rec {fig['nrec_ulp']} ulp (bound {X.FACTOR} x, 1 ulp)")
    print(RX.recomb_line(f"oracle {variant} {n}^3", c.ref, c.e, fig))
    RX.check_recomb_outputs(c.ref, c.e["outputs"])  # the float32 chain's own outputs pass as well


@pytest.mark.parametrize("name", list(RX.CASES))
def test_recomb_caps_hold(name):
    """Every box of test_gpu_recomb_cells.py: at t = 4 E32 the restatement alone leaves undecided no more than
    the caps of excursion_reference.py (unchanged: 1e-4 of the flags, 1e-3 of the radii), both branches are
    taken, the crossings spread over more than half the radii, and the float32 chain's own outputs pass the
    accounting.  Prints the caps table, one RECOMB-CAPS line per box."""
    c = RX.restated(name)
    fig = RX.check_recomb_outputs(c.ref, c.e["outputs"])
    print(RX.caps_line(name, c))
    print(RX.recomb_line(name + " (float32 chain on the host)", c.ref, c.e, fig))
    assert c.ref.flag_undecided_share <= X.FLAG_CAP
    assert c.ref.radius_undecided_share <= X.RADIUS_CAP
    assert 0.02 < c.ref.ionised_share < 0.98
    assert len(np.unique(c.ref.cross_hi)) - 1 > c.spec.n_radii // 2


def test_recomb_boxes_cover_both_radius_parities():
    parities = {RX.make_case(*v)[0].n_radii % 2 for v in RX.CASES.values()}
    assert parities == {0, 1}


def _accepted_by_the_oracle_comparison(got, ref, prev_nrec):
    """The comparison expressions of test_gpu_recomb.py::test_recombination_models_match_oracle for a box of
    more than 1e6 cells and model 2 (all but compare(), which reads none of the grids corrupted here)."""
    ion_g, ion_r = got["mean_free_path"] > 0, ref["mean_free_path"] > 0
    assert 0.03 < ion_r.mean() < 0.97 and ion_r.size > 10**6
    same = ion_g == ion_r
    same_R = same & (got["mean_free_path"] == ref["mean_free_path"])
    assert np.mean(~same_R & same) <= 2e-4
    same = same_R
    np.testing.assert_allclose(got["ionisation_rate_G12"][same], ref["ionisation_rate_G12"][same], rtol=2e-3,
                               atol=2e-6 * float(ref["ionisation_rate_G12"].max()))
    np.testing.assert_array_equal(got["mean_free_path"][same], ref["mean_free_path"][same])
    np.testing.assert_allclose(got["cumulative_recombinations"][same], ref["cumulative_recombinations"][same],
                               rtol=2e-4, atol=1e-7)
    assert (ref["cumulative_recombinations"] > prev_nrec).any()
    return True


def test_recomb_accounting_bites():
    """Four corruptions of the float32 chain's outputs of box r2 (128 x 128 x 256, 4.2 M cells); each must
    raise, by name.  The first two pass the comparison of test_recombination_models_match_oracle, which masks
    cells out before it compares and holds Gamma_12 to 2e-3: the gap this accounting closes, kept on record."""
    c = RX.restated("r2")
    ref, good = c.ref, c.e["outputs"]
    RX.check_recomb_outputs(ref, good)
    cross = RX.device_cross(good["mean_free_path"], ref.R32)

    def corrupted(**changes):
        new = dict(good)
        for k, (where, value) in changes.items():
            new[k] = good[k].copy()
            new[k][where] = value
        return new

    # a 16 x 16 x 1 tile with the most radius-decided crossings below the largest radius
    usable = ref.radius_decided & (cross > 0) & (cross < c.spec.n_radii)
    z = int(np.argmax(usable.sum(axis=(0, 1))))
    per_tile = usable[:, :, z].reshape(8, 16, 8, 16).sum(axis=(1, 3))
    tx, ty = np.unravel_index(np.argmax(per_tile), per_tile.shape)
    tile = (slice(16 * tx, 16 * tx + 16), slice(16 * ty, 16 * ty + 16), z)
    assert usable[tile].sum() > 50 and 256 / cross.size < 1e-4

    # (i) Gamma_12 x (1 + 1e-4) in the tile
    one = corrupted(ionisation_rate_G12=(tile, good["ionisation_rate_G12"][tile] * X.F32(1 + 1e-4)))
    with pytest.raises(AssertionError, match="Gamma_12 at the radius its mean free path names is off"):
        RX.check_recomb_outputs(ref, one)
    assert _accepted_by_the_oracle_comparison(one, good, c.inp.prev_nrec)

    # (ii) the mean free path moved to the next radius in the tile, Gamma_12 left as it is
    moved = np.where(usable[tile], ref.R32[np.minimum(cross[tile], c.spec.n_radii - 1)], good["mean_free_path"][tile])
    two = corrupted(mean_free_path=(tile, moved))
    with pytest.raises(AssertionError, match="decided cells with the wrong first-crossing radius"):
        RX.check_recomb_outputs(ref, two)
    assert _accepted_by_the_oracle_comparison(two, good, c.inp.prev_nrec)

    # (iii) one z-line of N_rec evaluated with table row z_ct + 1
    x, y = np.unravel_index(np.argmax((cross > 0).sum(axis=2)), cross.shape[:2])
    shifted = ref.rates.cells(good["ionisation_rate_G12"], good["neutral_fraction"], row_shift=1).astype(X.F32)
    assert (shifted[x, y] != good["cumulative_recombinations"][x, y]).sum() > 10
    three = corrupted(cumulative_recombinations=((x, y), shifted[x, y]))
    with pytest.raises(AssertionError, match="cumulative_recombinations more than 1 float ulp"):
        RX.check_recomb_outputs(ref, three)

    # (iv) z_reion set to the redshift on 20 crossing cells that held an earlier one
    held = np.flatnonzero(((cross > 0) & (c.inp.prev_z_reion >= 0)).ravel())
    pick = np.unravel_index(held[:: len(held) // 20][:20], cross.shape)
    assert len(pick[0]) == 20 and (c.inp.prev_z_reion[pick] != X.F32(c.spec.redshift)).all()
    four = corrupted(z_reion=(pick, X.F32(c.spec.redshift)))
    with pytest.raises(AssertionError, match="z_reion is not the previous z_reion on a crossing cell that held one: 20 cells"):
        RX.check_recomb_outputs(ref, four)


def test_rr_spline_restatement_matches_the_oracle(oracle):
    """The numpy rr_spline against oracle_splined_recombination_rate: rows, the floor and the ceiling of
    ln Gamma, knots, interior points."""
    import ctypes as C

    from recomb_helpers import synthetic_rr_tables

    lib = oracle.load()
    lib.oracle_splined_recombination_rate.restype = C.c_double
    lib.oracle_splined_recombination_rate.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double]
    y, c = synthetic_rr_tables()
    knots = RX.ln_gamma_knots()
    rng = np.random.default_rng(1)
    z = np.concatenate([rng.uniform(-1.0, 70.0, 300), [0.0, 0.1, 0.3, 59.8, 1e7]])
    g = np.concatenate([np.exp(rng.uniform(-12.0, 17.0, 300)), [0.0, np.exp(-10.0), np.exp(knots[-1]), 1e12, np.exp(knots[7])]])
    want = np.array([lib.oracle_splined_recombination_rate(y.ctypes.data, c.ctypes.data, zz, gg) for zz, gg in zip(z, g)])
    got = RX.rr_spline(y, c, z, g)
    assert (want == 0).sum() > 10 and (want > 0).sum() > 200
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
