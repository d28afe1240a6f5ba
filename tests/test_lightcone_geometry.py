"""The rectilinear lightconer's geometry (21cmfast_amd.drivers.RectilinearLightconer) on the CPU.

* Shape: the reference's 12 power_spectra fixtures were binned with powerbox over the lightcone of
  RectilinearLightconer.between_redshifts(node_z[-1] + 0.2, node_z[0] - 0.2, cell size)
  (reference: tests/produce_integration_test_data.py:292-325,395-426).  ``lightcone/k`` depends only on
  the lightcone's shape and extent, and one slice more or fewer moves it by more than a per cent, so
  reproducing it to 1e-12 pins the slice count.
* Tables: the per-slice plane indices and weights the host hands to the slab kernel, against a
  literal restatement of make_lightcone_slices / coeval_subselect / redshift_interpolation
  (tests/lightcone_reference.py)."""

import importlib

import numpy as np
import pytest

import lightcone_reference as LR
import refpin as RP

D = importlib.import_module("21cmfast_amd.drivers")
S = importlib.import_module("21cmfast_amd.structs")

# fixture -> evolution run (USE_TS_FLUCT or a recombination model: nodes from Z_HEAT_MAX = 35)
FIXTURES = {"simple": False, "no-mdz": False, "fixed_halogrids": False, "fftw_wisdom": False,
            "homo": True, "inhomo": True, "inhomo_ts": True, "minimize_mem": True,
            "multiple_scattering": True, "sampler_ts_ir_onethread": True, "ts": True, "ts_nomdz": True}


def lc_nodes(evolution):
    """get_node_z(18, lc=True) (produce_integration_test_data.py:292-325), ZPRIME_STEP_FACTOR 1.04."""
    return D.get_logspaced_redshifts(18.0, 1.04, 35.0 if evolution else 20.0)


def fixture_lightconer(evolution, quantities=("brightness_temp",)):
    z = lc_nodes(evolution)
    return D.RectilinearLightconer.between_redshifts(z[-1] + 0.2, z[0] - 0.2, RP.BOX_LEN / RP.HII_DIM,
                                                     quantities=quantities), z


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_lightconer_shape_reproduces_fixture_k(name):
    lc, nodes = fixture_lightconer(FIXTURES[name])
    so = S.default_simulation_options(HII_DIM=RP.HII_DIM, DIM=RP.DIM, BOX_LEN=RP.BOX_LEN)
    shape = lc.get_shape(so)
    assert shape == (RP.HII_DIM, RP.HII_DIM, 503 if FIXTURES[name] else 88)
    assert len(nodes) == (18 if FIXTURES[name] else 4)
    dims = lc.lightcone_dimensions(so)
    assert dims == (RP.BOX_LEN, RP.BOX_LEN, shape[2] * RP.BOX_LEN / RP.HII_DIM)
    field = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    f = RP.fixture("power_spectra", name)
    _, k = RP.get_power(field, dims)
    np.testing.assert_allclose(k, f["lightcone/k"], rtol=1e-12)
    # one slice fewer is a different lightcone
    _, k1 = RP.get_power(field[..., :-1], (dims[0], dims[1], dims[2] - RP.BOX_LEN / RP.HII_DIM))
    assert np.max(np.abs(k1 / f["lightcone/k"] - 1)) > 1e-2


def test_lightcone_redshifts_bracketed_by_nodes():
    lc, nodes = fixture_lightconer(True)
    z = lc.lc_redshifts
    assert np.all(np.diff(z) > 0)
    assert z[0] == pytest.approx(nodes[-1] + 0.2, abs=1e-9)
    # the inverse of the comoving distance to a few 1e-6 (linear interpolation on the 100-point grid)
    d = lc.cosmo.comoving_distance(z)
    np.testing.assert_allclose(d, lc.lc_distances, rtol=3e-6)


def check_tables(lc, nodes, cell, d_para):
    """slab_tables of every node pair against the literal restatement; returns the covered slices."""
    covered = np.zeros(len(lc.lc_distances), int)
    for z_hi, z_lo in zip(nodes[:-1], nodes[1:]):
        got = lc.slab_tables(z_lo, z_hi, cell, d_para)
        d_lo, d_hi = lc.cosmo.comoving_distance(z_lo), lc.cosmo.comoving_distance(z_hi)
        idx, plane, w_lo, w_hi, w_norm = LR.tables(lc.lc_distances, d_lo, d_hi, cell, lc.index_offset, d_para)
        if len(idx) == 0:
            assert got is None
            continue
        i0, p, a, b, nrm = got
        np.testing.assert_array_equal(np.arange(i0, i0 + len(p)), idx)
        np.testing.assert_array_equal(p, plane)
        assert p.dtype == np.int32 and p.min() >= 0 and p.max() < d_para
        np.testing.assert_array_equal(a, w_lo)
        np.testing.assert_array_equal(b, w_hi)
        assert nrm == w_norm
        # weights are distances to the other node: they sum to the node spacing
        np.testing.assert_allclose(a + b, nrm, rtol=1e-9)
        covered[idx] += 1
    return covered


@pytest.mark.parametrize("evolution", [False, True])
def test_slab_tables_match_literal_restatement(evolution):
    lc, nodes = fixture_lightconer(evolution)
    covered = check_tables(lc, nodes, RP.BOX_LEN / RP.HII_DIM, RP.HII_DIM)
    assert np.all(covered >= 1)  # every slice lies between two nodes


def test_slab_tables_wrap_across_d_para():
    """Runs longer than the node box: the plane index wraps and planes repeat."""
    lc, nodes = fixture_lightconer(False)
    d_para = 7
    check_tables(lc, nodes, RP.BOX_LEN / RP.HII_DIM, d_para)
    i0, plane, *_ = lc.slab_tables(nodes[-1], nodes[-2], RP.BOX_LEN / RP.HII_DIM, d_para)
    assert len(plane) > d_para
    assert np.all(np.diff(plane) % d_para == 1)  # consecutive slices, consecutive planes (mod d_para)
    assert plane[-1] == (lc.index_offset - (len(lc.lc_distances) - (i0 + len(plane) - 1))) % d_para


def test_slab_tables_non_cubic_and_offset():
    """NON_CUBIC_FACTOR = 1.2 (HII_D_PARA = 60) and a non-default index_offset."""
    so = S.default_simulation_options(HII_DIM=50, BOX_LEN=100.0, NON_CUBIC_FACTOR=1.2)
    d_para = int(so.NON_CUBIC_FACTOR * so.HII_DIM)
    assert d_para == 60
    nodes = lc_nodes(False)
    for offset in (None, 0, 13):
        lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.2, nodes[0] - 0.2, 2.0, index_offset=offset)
        check_tables(lc, nodes, 2.0, d_para)
    # the last slice of the lightcone sits on plane index_offset - 1
    lc = D.RectilinearLightconer.between_redshifts(nodes[-1] + 0.2, nodes[0] - 0.2, 2.0)
    _, plane, *_ = lc.slab_tables(nodes[1], nodes[0], 2.0, d_para)
    assert plane[-1] == (len(lc.lc_distances) - 1) % d_para


def test_slab_tables_node_boundary_tolerance():
    """A slice just below the lower node's distance belongs to the pair while it is within
    dcmin (1 - 1e-6) (make_lightcone_slices :199-203); further down it does not."""
    cosmo = D.RectilinearLightconer([1.0]).cosmo
    z_lo, z_hi, cell = 18.0, 18.72, 2.0
    d_lo, d_hi = cosmo.comoving_distance(z_lo), cosmo.comoving_distance(z_hi)
    inside, outside = d_lo * (1 - 0.5e-6), d_lo * (1 - 2e-6)
    lc = D.RectilinearLightconer(np.array([outside, inside, d_lo, d_lo + 1.0, d_hi - 0.5, d_hi]))
    i0, plane, w_lo, w_hi, w_norm = lc.slab_tables(z_lo, z_hi, cell, 50)
    assert (i0, len(plane)) == (1, 4)  # the slice at d_hi itself belongs to the next pair up
    idx, *_ = LR.tables(lc.lc_distances, d_lo, d_hi, cell, lc.index_offset, 50)
    np.testing.assert_array_equal(idx, [1, 2, 3, 4])
    assert w_hi[1] == 0.0 and w_lo[1] == pytest.approx(w_norm)  # exactly on the lower node
    assert lc.slab_tables(z_hi + 1.0, z_hi + 2.0, cell, 50) is None


def test_lightconer_validation():
    with pytest.raises(ValueError, match="non-negative"):
        D.RectilinearLightconer([-1.0, 2.0])
    with pytest.raises(ValueError, match="mean_max"):
        D.RectilinearLightconer([1.0], interp_kinds={"density": "nearest"})
    lc = D.RectilinearLightconer([1.0, 2.0, 3.0])
    assert lc.index_offset == 3 and lc.interp_kinds == {"z_reion": "mean_max"}
