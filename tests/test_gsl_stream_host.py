"""Host side of the reference's IC random streams, piece by piece (csrc/host/gsl_stream.c) -- CPU only.

The pieces are the ones the device draw (csrc/hip/gsl_stream_kernels.hip) is compared against bit for bit in
tests/test_gpu_gsl_device_stream.py: raw words, the polar method's compaction on caller-supplied words, the
packed accepted pairs of a whole draw, and the jump-ahead of cmrg / mrg / taus2 that gives every lane of the
device its start state.  Every comparison is exact.
"""

import ctypes as C
import importlib
import math

import numpy as np
import pytest

KINDS = (0, 1, 2, 3, 4)  # mt19937, gfsr4, cmrg, mrg, taus2
STATE_WORDS = {2: 6, 3: 5, 4: 3}


@pytest.fixture(scope="module")
def api(pkg):
    pkg.load()
    return importlib.import_module("21cmfast_amd.grid_api")


@pytest.fixture(scope="module")
def lib(pkg):
    lib = pkg.load()
    lib.c21_gsl_export_state.restype = C.c_int
    lib.c21_gsl_export_state.argtypes = [C.c_int, C.c_ulong, C.c_void_p]
    lib.c21_gsl_step.restype = C.c_uint
    lib.c21_gsl_step.argtypes = [C.c_int, C.c_void_p]
    lib.c21_gsl_jump.restype = C.c_int
    lib.c21_gsl_jump.argtypes = [C.c_int, C.c_void_p, C.c_ulonglong]
    lib.c21_gsl_mode_deviates.restype = C.c_int
    lib.c21_gsl_mode_deviates.argtypes = [C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


# ---- the numpy restatement of the compaction, shared with the GPU tests -----------------------------------
def accept_pairs_numpy(kind, words, want):
    """Drop zeros, reshape to pairs, the fp64 formula, mask.  Returns (pairs, words used)."""
    words = np.asarray(words, np.uint32)
    pos = np.flatnonzero(words)
    n_pairs = len(pos) // 2
    a = words[pos[0:2 * n_pairs:2]]
    c = words[pos[1:2 * n_pairs:2]]
    if kind in (2, 3):
        ua, uc = a / 2147483647.0, c / 2147483647.0
    else:
        ua, uc = a * (1.0 / 4294967296.0), c * (1.0 / 4294967296.0)
    x, y = 2 * ua - 1, 2 * uc - 1
    r2 = x * x + y * y
    keep = ~((r2 > 1.0) | (r2 == 0))
    pairs = (a.astype(np.uint64) | (c.astype(np.uint64) << np.uint64(32)))[keep]
    if len(pairs) >= want:
        if want == 0:
            return pairs[:0], 0
        last = np.flatnonzero(keep)[want - 1]  # the pair that completes the request
        return pairs[:want], int(pos[2 * last + 1]) + 1
    return pairs, len(words)


def word_sets(kind, tile=None):
    """Synthetic word sets of about 5000 words with the cases the compaction can get wrong.  With ``tile`` the
    zero words and rejected pairs sit on the edges of the device's tiles."""
    rng = np.random.default_rng(2026 + kind)
    top = 2147483646 if kind in (2, 3) else 2**32 - 1  # cmrg and mrg put out values below 2^31 - 1

    def base(n=5000):
        return rng.integers(1, top, n, dtype=np.uint64).astype(np.uint32)

    sets = {}
    w = base()
    w[[17, 400, 401, 402, 1999, 2000, 3500]] = 0  # single and consecutive zeros
    sets["zeros"] = w
    w = base()
    w[0] = w[-1] = 0  # a zero as the first and as the last word
    w[[100, 101]] = 0
    sets["zero_ends"] = w
    w = base(4999)
    w[[7, 8, 9]] = 0  # 4996 survivors ...
    w[2500] = 0  # ... 4995: the last one has no partner
    sets["odd_survivors"] = w
    if kind not in (2, 3):
        w = base()
        w[[10, 11]] = 0x80000000  # x = y = 0: r2 == 0 is rejected
        w[[2000, 2001, 2002]] = (0, 0x80000000, 0)
        w[2003] = 0x80000000
        sets["r2_zero"] = w
    if tile:
        w = base(2 * tile + 700)
        corner = 1 if kind in (2, 3) else 0xFFFFFFFF  # x = y = -1 (or +1): r2 = 2 is rejected
        for edge in (tile, 2 * tile):
            w[[edge - 3, edge - 1, edge, edge + 2]] = 0  # zeros on both sides of the edge: pairs straddle it
            w[[edge - 2, edge + 1]] = corner  # ... and the straddling pair is a rejected one
        w[tile - 8:tile - 4] = corner
        w[2 * tile + 3:2 * tile + 7] = 0
        sets["tile_edges"] = w
        w = base(tile + 1)  # the last tile holds one word
        w[tile - 1] = 0
        sets["tile_plus_one"] = w
    return sets


def wants(words, kind):
    """`want` in the middle of the input, on the last pair, and larger than the words yield"""
    total = len(accept_pairs_numpy(kind, words, 10**9)[0])
    return (1, total // 2, total - 1, total, total + 1, 10**6)


@pytest.mark.parametrize("kind", (2, 3, 4))
def test_jump_equals_single_steps(lib, kind):
    n_words = STATE_WORDS[kind]
    start = (C.c_uint * 6)()
    assert lib.c21_gsl_export_state(kind, 12345, start) == 0
    walked = (C.c_uint * 6)(*start)
    steps = 0
    for n in (1, 2, 623, 10_000, 1_000_003):
        while steps < n:
            lib.c21_gsl_step(kind, walked)
            steps += 1
        jumped = (C.c_uint * 6)(*start)
        assert lib.c21_gsl_jump(kind, jumped, n) == 0
        assert list(jumped)[:n_words] == list(walked)[:n_words], (kind, n)
    assert lib.c21_gsl_jump(0, start, 1) == 3  # mt19937 and gfsr4 do not jump


def test_raw_words_reproduce_gsl_self_test_values(api):
    for kind, seed, n, value in ((0, 4357, 1000, 1186927261), (2, 1, 10000, 719452880),
                                 (3, 1, 10000, 2064828650), (4, 1, 10000, 2733957125)):
        assert int(api.gsl_raw_words(kind, seed, n)[-1]) == value, kind
    # the exported state steps to the same words
    w = api.gsl_raw_words(1, 777, 40000)
    n = np.arange(9689, len(w))
    np.testing.assert_array_equal(w[n], w[n - 471] ^ w[n - 1586] ^ w[n - 6988] ^ w[n - 9689])


@pytest.mark.parametrize("kind", KINDS)
def test_accept_pairs_equals_numpy_restatement(api, kind):
    for name, words in word_sets(kind).items():
        for want in wants(words, kind):
            ref_pairs, ref_used = accept_pairs_numpy(kind, words, want)
            pairs, used = api.gsl_accept_pairs(kind, words, want)
            np.testing.assert_array_equal(pairs, ref_pairs, err_msg=f"{name} want={want}")
            assert used == ref_used, (name, want)
    pairs, used = api.gsl_accept_pairs(kind, np.zeros(0, np.uint32), 5)
    assert len(pairs) == 0 and used == 0


def test_accept_pairs_rejects_r2_zero(api):
    words = np.array([0x80000000, 0x80000000, 0x80000000, 0x40000000], np.uint32)
    pairs, used = api.gsl_accept_pairs(0, words, 5)
    assert list(pairs) == [0x80000000 | (0x40000000 << 32)] and used == 4


@pytest.mark.parametrize("n_threads,shape", [(5, (12, 8, 8)), (2, (15, 15, 15))])
def test_stream_pairs_give_the_host_deviates(api, lib, n_threads, shape):
    """The packed pairs through libm, element by element (the operations of next_ugaussian), are the deviates of
    c21_gsl_mode_deviates bit for bit."""
    nx, ny, nz = shape
    nzc = nz // 2 + 1
    pairs = api.gsl_stream_pairs(777, n_threads, shape)
    want = np.zeros((nx, ny, nzc, 2))
    assert lib.c21_gsl_mode_deviates(777, n_threads, nx, ny, nzc, want.ctypes.data) == 0
    q, rem = divmod(nx, n_threads)
    got = np.zeros_like(want)
    for t in range(n_threads):
        lo = t * q + min(t, rem)
        rows = q + (1 if t < rem else 0)
        scale = 1 / 2147483647.0 if t % 5 in (2, 3) else None
        flat = got[lo:lo + rows].reshape(-1)
        for i, p in enumerate(pairs[lo:lo + rows].reshape(-1).tolist()):
            a, c = p & 0xFFFFFFFF, p >> 32
            if scale is None:
                ua, uc = a * (1.0 / 4294967296.0), c * (1.0 / 4294967296.0)
            else:
                ua, uc = a / 2147483647.0, c / 2147483647.0
            x, y = 2 * ua - 1, 2 * uc - 1
            r2 = x * x + y * y
            flat[i] = y * math.sqrt(-2.0 * math.log(r2) / r2)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
