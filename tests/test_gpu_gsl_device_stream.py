"""The reference's IC random streams drawn on the device (csrc/hip/gsl_stream_kernels.hip) against the host
restatement (csrc/host/gsl_stream.c), piece by piece and then through the IC entry points.

Everything up to the accepted pair is integer arithmetic and a handful of IEEE fp64 operations, so every
comparison here is exact: raw words, the compaction on synthetic words (against the numpy restatement of
tests/test_gsl_stream_host.py), the packed pairs of whole draws for several launch lengths, and the IC fields of
rng_stream = 2 against rng_stream = 1, which share the kernel that turns pairs into deviates.
"""

import importlib

import numpy as np
import pytest

import refpin as RP
from test_gsl_stream_host import KINDS, accept_pairs_numpy, wants, word_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api(gpu_lib):
    return importlib.import_module("21cmfast_amd.grid_api")


_host_pairs = {}


def host_pairs(api, n_threads, shape, seed=777):
    """the host's packed pairs, drawn once per case and left unchanged"""
    key = (seed, n_threads, tuple(shape))
    if key not in _host_pairs:
        ref = api.gsl_stream_pairs(seed, n_threads, shape)
        ref.setflags(write=False)
        _host_pairs[key] = ref
    return _host_pairs[key]


@pytest.mark.parametrize("kind", KINDS)
def test_raw_words_equal_the_host(api, kind):
    """50 000 words: 80 mt19937 blocks, three turns of the gfsr4 ring, 24 tiles of the jumping generators"""
    for seed in (0, 1, 12345, 2**32 + 7):
        host = api.gsl_raw_words(kind, seed, 50_000)
        dev = api.gsl_raw_words(kind, seed, 50_000, on_device=True)
        np.testing.assert_array_equal(dev, host, err_msg=f"seed {seed}")
    assert len(np.unique(host)) > 49_900


@pytest.mark.parametrize("kind", KINDS)
def test_accept_pairs_equal_the_numpy_restatement(api, kind):
    tile = api.gsl_tile_words(-1)
    assert tile > 0
    sets = word_sets(kind, tile)
    assert {"tile_edges", "tile_plus_one"} <= set(sets)
    for name, words in sets.items():
        for want in wants(words, kind):
            ref_pairs, ref_used = accept_pairs_numpy(kind, words, want)
            pairs, used = api.gsl_accept_pairs(kind, words, want, on_device=True)
            np.testing.assert_array_equal(pairs, ref_pairs, err_msg=f"{name} want={want}")
            assert used == ref_used, (name, want)


def test_accept_pairs_takes_device_words(api):
    import torch

    words = word_sets(0)["zeros"]
    d_words = torch.from_numpy(words.view(np.int32)).cuda()
    ref_pairs, ref_used = accept_pairs_numpy(0, words, 1000)
    for on_device in (False, True):
        pairs, used = api.gsl_accept_pairs(0, d_words, 1000, on_device=on_device)
        np.testing.assert_array_equal(pairs, ref_pairs)
        assert used == ref_used


SMALL = [(1, (12, 12, 12)), (2, (15, 15, 15)), (3, (10, 10, 10)), (5, (12, 8, 8)), (7, (16, 6, 6)),
         (15, (12, 8, 8))]  # the last: n_threads = nx + 3, streams without rows


@pytest.mark.parametrize("max_pairs", [0, 997])
@pytest.mark.parametrize("n_threads,shape", SMALL)
def test_stream_pairs_equal_the_host(api, n_threads, shape, max_pairs):
    ref = host_pairs(api, n_threads, shape)
    dev = api.gsl_stream_pairs(777, n_threads, shape, on_device=True, max_pairs_per_launch=max_pairs)
    np.testing.assert_array_equal(dev, ref)
    again = api.gsl_stream_pairs(777, n_threads, shape, on_device=True, max_pairs_per_launch=max_pairs)
    np.testing.assert_array_equal(again, ref)


@pytest.mark.parametrize("n_threads,n,max_pairs", [
    (5, 64, 0),        # about 54 k pairs per stream, the gfsr4 ring wrapped 8 times
    (1, 64, 0),        # one mt19937 stream of 270 k pairs
    (16, 256, 0),      # about 1 M pairs per stream
    (16, 256, 100_003),
])
def test_stream_pairs_equal_the_host_at_larger_sizes(api, n_threads, n, max_pairs):
    import torch

    shape = (n, n, n)
    ref = host_pairs(api, n_threads, shape, seed=12345)
    d_out = torch.zeros(ref.shape, dtype=torch.int64, device="cuda")
    for _ in range(2):  # a second call gives the same bits
        d_out.zero_()
        api.gsl_stream_pairs(12345, n_threads, shape, on_device=True, max_pairs_per_launch=max_pairs, out=d_out)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), ref)


@pytest.mark.parametrize("threads", [2, 5])
def test_ics_of_the_device_stream_equal_the_host_staged_path(api, threads):
    host = {k: np.array(v) for k, v in api.ics_grids(RP.ics_spec(2, 0, threads, rng_stream=1)).items()}
    dev = api.ics_grids(RP.ics_spec(2, 0, threads, rng_stream=2))
    assert set(dev) == set(host)
    for k in host:
        assert np.array_equal(dev[k], host[k]), k
        assert np.abs(host[k]).max() > 0, k


def test_entry_point_with_the_device_stream_equals_the_default(gpu_lib, api, monkeypatch):
    from test_gpu_reference_fixtures import run_abi

    monkeypatch.delenv("C21CM_IC_RNG", raising=False)
    ics0, dens0, vz0 = run_abi(gpu_lib, api, 10.0, 2)
    monkeypatch.setenv("C21CM_IC_RNG", "gsl-device")
    ics1, dens1, vz1 = run_abi(gpu_lib, api, 10.0, 2)
    for k in ics0:
        assert np.array_equal(ics1[k], ics0[k]), k
    assert np.array_equal(dens1, dens0) and np.array_equal(vz1, vz0)
    assert RP.check_perturb_fixture("simple", dens1, vz1) < 2e-6


def test_a_launch_that_reaches_its_tile_cap_fails_and_returns(api):
    """2016 pairs of one mt19937 stream need about nine tiles of 624 words: with a cap of one tile the launch
    saves what it has, raises the flag and the driver reports it."""
    BackendError = importlib.import_module("21cmfast_amd._lib").BackendError
    with pytest.raises(BackendError) as err:
        api.gsl_stream_pairs(777, 1, (12, 12, 12), on_device=True, tile_cap=1)
    assert err.value.code == 3 and "tile cap" in str(err.value)
    dev = api.gsl_stream_pairs(777, 1, (12, 12, 12), on_device=True)
    np.testing.assert_array_equal(dev, host_pairs(api, 1, (12, 12, 12)))
