"""Pass X of the split-layout filter (line_pass_kernel<N, +1, FMODE>, fft_native.hip), every window mode,
mode by mode against a float64 filter -- through the exported C entries alone.

The chain is c21hip_split_r2c (1 / N folded in) -> the filter entry under test -> c21hip_split_z_c2r; the
test never looks into the split layout.  The comparison is in k-space, where a window error lives:

    G = rfftn(device output in float64),  ref = rfftn(a in float64) W(|k|)   (tests/window_reference.py)
    |G - ref| <= tol_k   for EVERY mode.

Shapes.  A pass-X launch has n_work = (ny/2+1) (nz/2/tile) + ny/tile work items for min(n_work, 256 per_cu)
persistent workgroups; the boxes below are the smallest whose n_work exceeds the workgroup count without
being a multiple of it, so that some workgroups take a second or third trip through the pipelined loop (next
tile's loads in flight during this tile's transform, column tiles rotated per trip) and others do not.
box_len = 1.5 nx, box_len_z = 0.8 box_len nz / nx: z cells differ from x cells, and y cells too (ny != nx
under x's box length), so a dk taken from the wrong axis shows.

Tolerance, from the reference side alone (never from the library's output):

    tol_k = 4 E32[class of k] + w env_k |A_k|

* E32: the error of the same chain in numpy's float32 transforms with the top-hat of radius R_E32, per shape:
  max over modes of |rfftn64(irfftn32(rfftn32(a) W32)) - ref|.  The input carries a mean of 0.5, i.e. a DC
  mode ~500 times the rms mode, and ANY float32 transform leaks that term's rounding (6e-8 x 0.5 N) into the
  modes that share a 1-D transform with it: measured with numpy, the error is 1.2e-5 .. 1.5e-4 rms|A| on the line
  (k_x, 0, 0), 4e-6 .. 1.7e-5 on the rest of the plane k_z = 0, and 6.5e-7 .. 8.3e-7 everywhere else (4.4e-7 for
  the same field without its mean).  One maximum over all modes would hand the line's figure to the other
  99.6 % of the modes, a hundred times what they need; so E32 is taken per class -- the line, the plane, the
  rest -- and each mode is held to its own class.  Every mode is thereby also within 4 max(E32).
* 4: the device differs from pocketfft in radix order, float twiddles formed by products and the r2c / c2r
  post-processing; 8 on the line (k_x, 0, 0), where the error is that of the DC term's partial sums (FACTOR_LINE).  (A window that leaves nothing but the mean and the first k_z has E32 measured with
  itself: the float roundings of nx ny identical lines add coherently, which the top-hat never shows; check().)
* w: the library's own bound on a window value, relative to the window's envelope env_k = min(1, 3 / (kR)^2)
  for the top-hat, 1 otherwise: 1.2e-7 for table entries (the double evaluation rounded to float: 2^-24, and
  the product with the float spectrum the same again), 1.5e-7 for the node tables
  (test_node_table_interpolation_accuracy), 5e-7 for the direct fp32 evaluation beyond them (DESIGN_HISTORY).

The route is asserted: c21hip_ktime_* counts the launches of each kernel kind around every call, and
c21hip_wev_covers tells FMODE 6 / 7 (node tables reach every kR) from 8 / 9 (direct evaluation beyond them).

Every case prints `PASSX ratio`: max over modes of |G - ref| / E32[class]; the largest per mode family are
recorded in DESIGN.md (Appendix C)."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

import window_reference as WR

pytestmark = pytest.mark.gpu

MFP = 37.66  # mfp_meandens of the excursion-set loop's emissivity window (ionize_driver.c: stars_filter = 3)
R_E32 = 5.0  # radius of the top-hat that measures E32 (3.3 cells)
W_TABLE, W_NODES, W_DIRECT = 1.2e-7, 1.5e-7, 5e-7
FACTOR = 4.0
# The nx modes of the line (k_x, 0, 0) take 8.  Their error is not the rounding of the mode (~1 rms) but of the
# partial sums of the DC term an implementation forms on the way, each up to N / 2 x 0.5 (ulp 0.06 .. 0.5), and
# which sums it forms is its radix order: the device's radix-8 Stockham passes leave k_x = nx / 2 as (even sum -
# odd sum), 0.084 = 0.7 ulp of the DC term at (64, 128, 256), where pocketfft's factorisation happens to show 0.018
# as the maximum over that line's 64 modes -- 4.7 E32.  The next largest on that line, over this file's 245
# comparisons, are 3.6 and 3.5.
FACTOR_LINE = 8.0
VALUE_ERROR = 3
# c21hip_ktime_report kinds: pass X with streamed tables, pass Y (and any windowless inverse pass), two-radius
# pass X with tables, pass X / two-radius pass X with evaluated windows, forward passes, anything else
K_TABLE, K_Y, K_PAIR_TABLE, K_EVAL, K_PAIR_EVAL, K_FWD, K_OTHER = 0, 1, 6, 7, 8, 9, 10


def x_shape(n):
    """The smallest box whose pass X over n-point lines takes uneven trips (module docstring)."""
    return (n, 128, 256) if n <= 256 else (n, 64, 256)


def tile_cols(n):
    return 8 if n == 1536 else 16


def pass_x_work(shape):
    nx, ny, nz = shape
    t = tile_cols(nx)
    return (ny // 2 + 1) * (nz // 2 // t) + ny // t


def assert_uneven_trips(shape):
    """n_work above the workgroup count and not a multiple of it (restated from launch_line_pass_mode)."""
    n_work = pass_x_work(shape)
    per_cu = 2 if shape[0] <= 256 else 1
    # (two-radius launches of short lines with long node tables are LDS-limited to one workgroup per CU)
    for groups in {256 * per_cu, 256}:
        assert n_work > groups and n_work % groups != 0, (shape, n_work, groups)


def geometry(shape):
    box_len = 1.5 * shape[0]
    return box_len, 0.8 * box_len * shape[2] / shape[0]


class Box:
    """Host side of one shape: inputs, their float64 spectra, |k|, E32 -- computed once, read only."""

    def __init__(self, shape):
        self.shape = shape
        self.box_len, self.box_len_z = geometry(shape)
        self.k = WR.k_magnitude(shape, self.box_len, self.box_len_z)
        self.k.setflags(write=False)
        self._grids, self.dev = {}, {}
        self.e32 = self.measure_e32(WR.window(0, self.k, R_E32))

    def grid(self, g):
        """(a, rfftn(a in float64)) of grid g: standard normal + 0.5 in float32, its own seed per grid."""
        if g not in self._grids:
            a = (np.random.default_rng([2026, g, *self.shape]).standard_normal(self.shape, np.float32)
                 + np.float32(0.5))
            A = np.fft.rfftn(a.astype(np.float64))
            a.setflags(write=False)
            A.setflags(write=False)
            self._grids[g] = (a, A)
        return self._grids[g]

    def measure_e32(self, W, g=0):
        """The error of numpy's float32 chain under window W, per class of modes: the line (k_x, 0, 0), the
        rest of the plane k_z = 0, everything else."""
        a, A = self.grid(g)
        A32 = np.fft.rfftn(a)
        if A32.dtype == np.complex64:
            f = np.fft.irfftn(A32 * W.astype(np.float32), s=self.shape, axes=(0, 1, 2))
        else:  # a numpy that widens: torch's float32 transforms on the CPU
            import torch

            t = torch.fft.rfftn(torch.from_numpy(np.array(a))) * torch.from_numpy(W.astype(np.float32))
            f = torch.fft.irfftn(t, s=self.shape).numpy()
        assert f.dtype == np.float32
        err = np.abs(np.fft.rfftn(f.astype(np.float64)) - A * W)
        line = err[:, 0, 0].max()
        err[:, 0, 0] = 0
        plane = err[:, :, 0].max()
        err[:, :, 0] = 0
        return {"line": line, "plane": plane, "rest": err.max()}

    def e32_of_modes(self, e32=None):
        e32 = e32 or self.e32
        e = np.full(self.k.shape, e32["rest"])
        e[:, :, 0] = e32["plane"]
        e[:, 0, 0] = e32["line"]
        return e

    def k_max(self):
        nx, ny, nz = self.shape
        return math.sqrt((math.pi * nx / self.box_len) ** 2 + (math.pi * ny / self.box_len) ** 2
                         + (math.pi * nz / self.box_len_z) ** 2)

    def radius(self, kR_max):
        return float(np.float32(kR_max / self.k_max()))

    def radius_direct(self):
        """A radius beyond the node tables of every launch: kR_max >= 1300 (int(4 x_max) + 3 > 4096)."""
        return float(np.float32(max(0.8 * self.box_len, 1300.0 / self.k_max())))

    def sharp_k_radius(self, R):
        """The radius at or just above R for which no mode sits within 1e-5 of the sharp-k edge."""
        for j in range(100):
            Rj = float(np.float32(R * (1 + 1e-3 * j)))
            kR = (self.k * Rj).astype(np.float32).astype(np.float64)
            if np.abs(0.413566994 * kR - 1).min() > 1e-5:
                return Rj
        raise AssertionError("no sharp-k radius clear of every mode")


@functools.lru_cache(maxsize=2)
def box_of(shape):
    return Box(shape)


class Win:
    """One window: (type, R, R_param, R_star) as filter_box takes them."""

    def __init__(self, ftype, R, R_param=0.0, R_star=0.0):
        self.ftype, self.R, self.R_param, self.R_star = ftype, R, R_param, R_star

    def at(self, R):
        return Win(self.ftype, R, self.R_param, self.R_star)

    def __repr__(self):
        return f"W{self.ftype}(R={self.R:.6g}, p={self.R_param:.6g}, s={self.R_star:.6g})"


NO_WINDOW = Win(2, 0.0)  # W = 1 on every mode: the Gaussian of radius 0


class Device:
    def __init__(self, lib):
        import torch

        self.lib, self.torch = lib, torch
        vp, i, d, f, lg = C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_long
        dims, lens = [i, i, i], [d, d]
        sig = {
            "c21hip_split_floats": (C.c_size_t, dims),
            "c21hip_split_r2c": (i, [vp, lg, vp, *dims, d, d, d, f, vp]),
            "c21hip_split_z_c2r": (i, [vp, vp, lg, *dims, vp]),
            "c21hip_split_filter_xy": (i, [vp, vp, *dims, *lens, i, f, f, i, vp]),
            "c21hip_split_filter_xy2": (i, [vp, vp, i, f, vp, vp, i, f, *dims, *lens, f, i, i, i, vp]),
            "c21hip_split_filter_shell": (i, [vp, vp, i, vp, vp, i, i, *dims, *lens, f, f, f, i, vp]),
            "c21hip_split_filter_xy2_pair": (i, [vp, vp, vp, i, f, vp, vp, vp, i, f, *dims, *lens, f, f, i, i, i,
                                                 vp]),
            "c21hip_split_filter_x_pair1": (i, [vp, vp, vp, i, *dims, *lens, f, f, i, vp]),
            "c21hip_split_filter_xy2_pair_eval": (i, [vp, vp, vp, i, vp, vp, vp, i, *dims, *lens, f, f, i, vp]),
            "c21hip_split_filter_xy_shared_pair": (i, [vp, vp, vp, i, *dims, *lens, f, f, i, i, i, vp]),
            "c21hip_split_filter_xy_single_pair": (i, [vp, vp, vp, i, f, *dims, *lens, f, f, i, vp]),
            "c21hip_split_filter_xy_shared": (i, [vp, vp, i, *dims, *lens, f, i, i, vp]),
            "c21hip_window_tables": (i, [i, i, f, i, f, *dims, *lens, f, vp]),
            "c21hip_wev_prepare": (i, [i, f, i, f, i, C.POINTER(f), i, *dims, *lens, i, C.POINTER(i), vp]),
            "c21hip_wev_release": (None, []),
            "c21hip_wev_covers": (i, []),
            "c21hip_ktime_enable": (None, [i]),
            "c21hip_ktime_report": (i, [i, C.POINTER(d), C.POINTER(i)]),
            "c21hip_get_error": (C.c_char_p, []),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    @property
    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def ok(self, status):
        assert status == 0, (status, self.lib.c21hip_get_error().decode())

    def split(self, shape):
        """A split-layout buffer full of NaN: whatever a pass leaves unwritten shows in every mode."""
        n = self.lib.c21hip_split_floats(*shape)
        return self.torch.full((n,), float("nan"), dtype=self.torch.float32, device="cuda")

    def spectrum(self, box, g):
        """The split spectrum of grid g on the device, 1 / N folded in (computed once per box)."""
        if g not in box.dev:
            a, _ = box.grid(g)
            real = self.torch.from_numpy(np.array(a)).cuda()
            out = self.split(box.shape)
            n_cells = float(np.prod(box.shape))
            self.ok(self.lib.c21hip_split_r2c(real.data_ptr(), box.shape[2], out.data_ptr(), *box.shape, 1.0, 1.0,
                                              0.0, 1.0 / n_cells, self.stream))
            self.torch.cuda.synchronize()
            assert bool(self.torch.isfinite(out).all())
            box.dev[g] = out
        return box.dev[g]

    def real(self, box, work):
        out = self.torch.full(box.shape, float("nan"), dtype=self.torch.float32, device="cuda")
        self.ok(self.lib.c21hip_split_z_c2r(work.data_ptr(), out.data_ptr(), box.shape[2], *box.shape, self.stream))
        self.torch.cuda.synchronize()
        return out.cpu().numpy()

    def launches(self, call, expect):
        """Run call() and hold the line-pass launches it made to `expect` {kind: count}: every pass-X kind
        not named must not have run, nor a forward pass."""
        self.lib.c21hip_ktime_enable(1)
        try:
            status = call()
            got = {}
            for kind in (K_TABLE, K_Y, K_PAIR_TABLE, K_EVAL, K_PAIR_EVAL, K_FWD, K_OTHER):
                total, count = C.c_double(), C.c_int()
                assert self.lib.c21hip_ktime_report(kind, C.byref(total), C.byref(count)) == 0
                got[kind] = count.value
        finally:
            self.lib.c21hip_ktime_enable(0)
        self.ok(status)
        want = {kind: expect.get(kind, 0) for kind in got}
        assert got == want, f"line-pass launches {got}, expected {want}"

    def prepare(self, box, wins, radii, pair, covers):
        """c21hip_wev_prepare for one or two windows; `covers`: the regime the case is built for, asserted
        on the CPU from wev_static_ok's cap restated here, and on the library through c21hip_wev_covers."""
        need, cap = wev_need(box, max(radii)), wev_cap(box.shape[0], pair, [w.ftype for w in wins])
        if covers:
            assert need <= min(cap, 4096), (need, cap)
        else:
            assert need > min(cap, 4096), (need, cap)
        wa, wb = wins[0], wins[-1]
        rad = (C.c_float * len(radii))(*radii)
        enabled = C.c_int(-1)
        self.ok(self.lib.c21hip_wev_prepare(wa.ftype, wa.R_param, wb.ftype, wb.R_param, len(wins), rad, len(radii),
                                            *box.shape, box.box_len, box.box_len_z, int(pair), C.byref(enabled),
                                            self.stream))
        assert enabled.value == 1
        assert self.lib.c21hip_wev_covers() == (1 if covers else 0)
        return W_NODES if covers else W_DIRECT


def wev_need(box, R_max):
    """Nodes (1/4 apart) that reach the largest kR of the set: c21hip_wev_prepare's count."""
    return int(box.k_max() * float(np.float32(R_max)) * (1.0 + 1e-6) * 4.0) + 3


def wev_cap(nx, pair, ftypes):
    """Nodes per table that fit in LDS beside the tiles (wev_static_ok): 158 KB less the tile(s) of 16 columns,
    the twiddles and the half twiddles of 1024-point lines, over 12 bytes a node and the tables of the largest
    launch (one top-hat table, one exp-MFP table per sweep member)."""
    two = pair and nx <= 512
    fixed = 8 * ((2 if two else 1) * nx * 16 + nx + (nx // 2 if nx >= 1024 else 0))
    worst = (1 if 0 in ftypes else 0) + sum(t == 3 for t in ftypes) * (2 if two else 1)
    return max(158 * 1024 - fixed, 0) // (12 * max(worst, 1))


@pytest.fixture(scope="module")
def dev(gpu_lib):
    d = Device(gpu_lib)
    yield d
    gpu_lib.c21hip_wev_release()
    gpu_lib.c21hip_ktime_enable(0)
    box_of.cache_clear()


@pytest.fixture(autouse=True)
def _release_window_set(dev):
    dev.lib.c21hip_wev_release()  # (a driver test before this module may have left its set active)
    yield
    dev.lib.c21hip_wev_release()


def check(dev, box, g, work, win, w, label):
    """Every mode of the device's filtered grid g within tol_k of the float64 filter; prints the ratio."""
    out = dev.real(box, work)
    assert np.isfinite(out).all(), f"{label}: non-finite cells"
    G = np.fft.rfftn(out.astype(np.float64))
    _, A = box.grid(g)
    W = WR.window(win.ftype, box.k, win.R, win.R_param, win.R_star)
    ref = A * W
    err = np.abs(G - ref)
    e32 = box.e32_of_modes()
    if not W[1:].any() and not W[0, 1:].any():
        # A window that passes only modes with k_x = k_y = 0 (sharp-k at the radii of the direct regime: the
        # mean and the first k_z) leaves the SAME z-line nx ny times.  Storing that line as float rounds all of
        # them identically, and along (0, 0, k_z) these roundings add coherently -- nx ny eps sqrt(nz) -- where
        # those of a field that differs from line to line add as a random walk, which is what the top-hat of
        # R_E32 measures.  The exact field rounded once to float is already 4.9 and 8.3 E32 off there at
        # (128, 128, 256), numpy's float32 chain 5.2 and 8.5, the device the same to three digits.  So for
        # such a window E32 is measured with the window itself.
        own = box.measure_e32(W, g)
        e32 = np.maximum(e32, box.e32_of_modes(own))
    if win.ftype == 0:
        kR = box.k * float(np.float32(win.R))
        env = np.minimum(1.0, 3.0 / np.maximum(kR, 1e-30) ** 2)
    else:
        env = 1.0
    allowed = w * env * np.abs(A)
    factor = np.full(err.shape, FACTOR)
    factor[:, 0, 0] = FACTOR_LINE
    tol = factor * e32 + allowed
    ratio = float((err / e32).max())
    worst = np.unravel_index(np.argmax(err - tol), err.shape)
    rms = rms_modes(A)
    over = (err - allowed) / e32
    print(f"PASSX ratio {ratio:7.3f}  beyond-window-bound {float(over.max()):7.3f} (line (k_x, 0, 0) "
          f"{float(over[:, 0, 0].max()):6.3f})  {label} "
          f"g{g} {win} w {w:.1e} shape {box.shape}  E32/rms|A| line {box.e32['line'] / rms:.2e} plane "
          f"{box.e32['plane'] / rms:.2e} rest {box.e32['rest'] / rms:.2e}")
    n_bad = int((err > tol).sum())
    assert n_bad == 0, (f"{label} g{g} {win}: {n_bad} modes beyond tol_k; worst {worst}: |G - ref| = {err[worst]:.4g}, "
                        f"tol = {tol[worst]:.4g}, |ref| = {abs(ref[worst]):.4g}, |A| = {abs(A[worst]):.4g}")


def rms_modes(A):
    """rms |A| over the modes other than DC."""
    return math.sqrt((np.sum(np.abs(A) ** 2) - abs(A[0, 0, 0]) ** 2) / A.size)


def ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------- FMODE 3, one grid
ALL_LENGTHS = [64, 128, 192, 256, 384, 512, 768, 1024, 1536]


def one_grid(dev, box, win, expect, w=W_TABLE, label="xy"):
    src, work = dev.spectrum(box, 0), dev.split(box.shape)
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy(src.data_ptr(), work.data_ptr(), *box.shape, box.box_len,
                                                        box.box_len_z, win.ftype, win.R, win.R_param, 1, dev.stream),
                 expect)
    check(dev, box, 0, work, win, w, label)


@pytest.mark.parametrize("n", ALL_LENGTHS)
def test_table_top_hat_every_length(dev, n):
    shape = (1536, 64, 256) if n == 1536 else x_shape(n)
    assert_uneven_trips(shape)
    one_grid(dev, box_of(shape), Win(0, 5.0), {K_TABLE: 1, K_Y: 1})


@pytest.mark.parametrize("n", ALL_LENGTHS)
def test_no_window_every_length(dev, n):
    """apply = 0: pass X is the windowless instantiation (FMODE 0, the kernel of pass Y) over the same uneven
    trips; the reference is the spectrum itself."""
    box = box_of((1536, 64, 256) if n == 1536 else x_shape(n))
    src, work = dev.spectrum(box, 0), dev.split(box.shape)
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy(src.data_ptr(), work.data_ptr(), *box.shape, box.box_len,
                                                        box.box_len_z, 0, 5.0, 0.0, 0, dev.stream), {K_Y: 2})
    check(dev, box, 0, work, NO_WINDOW, 0.0, "no window")


@pytest.mark.parametrize("ftype", [1, 2, 3])
@pytest.mark.parametrize("n", [192, 1024])
def test_table_sharp_k_gaussian_exp_mfp(dev, n, ftype):
    box = box_of(x_shape(n))
    win = {1: Win(1, box.sharp_k_radius(3.0)), 2: Win(2, 4.0), 3: Win(3, 7.5, MFP)}[ftype]
    if ftype == 1:
        assert 0.01 < WR.window(1, box.k, win.R).mean() < 0.99  # the edge is inside the grid
    one_grid(dev, box, win, {K_TABLE: 1, K_Y: 1})


@pytest.mark.parametrize("ftypes", [(4,), (5,), (4, 5), (5, 4)])
@pytest.mark.parametrize("n", [192, 1024])
def test_table_shells(dev, n, ftypes):
    """Windows 4 (spherical shell) and 5 (multiple scattering; kR crosses 30, where the series hands over to
    the asymptotic form) between R_inner and R_outer, one and two grids (c21hip_split_filter_shell)."""
    box = box_of(x_shape(n))
    R_in, R_out, R_star = 8.0, 11.0, 0.6
    assert box.k_max() * R_out > 30.0
    src = [dev.spectrum(box, g) for g in range(len(ftypes))]
    work = [dev.split(box.shape) for _ in ftypes]
    two = len(ftypes) == 2
    dev.launches(lambda: dev.lib.c21hip_split_filter_shell(
        src[0].data_ptr(), work[0].data_ptr(), ftypes[0], ptr(src[1]) if two else None,
        ptr(work[1]) if two else None, ftypes[-1], len(ftypes), *box.shape, box.box_len, box.box_len_z, R_in, R_out,
        R_star, 1, dev.stream), {K_TABLE: 1, K_Y: 1})
    for g, t in enumerate(ftypes):
        check(dev, box, g, work[g], Win(t, R_in, R_out, R_star), W_TABLE, "shell")


# ---------------------------------------------------------------- FMODE 3, two grids
def excursion_pair(R):
    """The excursion-set loop's windows (ionize_driver.c): HII_FILTER top-hat on the density, the exp-MFP
    window of mfp_meandens on the emissivity."""
    return [Win(0, R), Win(3, R, MFP)]


def xy2(dev, box, wins, src, work, slot, ready):
    a, b = wins
    return dev.lib.c21hip_split_filter_xy2(src[0].data_ptr(), work[0].data_ptr(), a.ftype, a.R_param,
                                           src[1].data_ptr(), work[1].data_ptr(), b.ftype, b.R_param, *box.shape,
                                           box.box_len, box.box_len_z, a.R, 1, slot, ready, dev.stream)


def window_tables(dev, box, wins, slot):
    a, b = wins
    dev.ok(dev.lib.c21hip_window_tables(slot, a.ftype, a.R_param, b.ftype, b.R_param, *box.shape, box.box_len,
                                        box.box_len_z, a.R, dev.stream))


@pytest.mark.parametrize("ready", [0, 1])
@pytest.mark.parametrize("n", [384, 512, 1024])
def test_table_two_grids(dev, n, ready):
    """c21hip_split_filter_xy2 building its tables, and with tables prebuilt by c21hip_window_tables into
    another slot -- which c21hip_split_filter_xy_shared then reuses for one grid under window a."""
    box = box_of(x_shape(n))
    wins = excursion_pair(6.5)
    src = [dev.spectrum(box, g) for g in (0, 1)]
    work = [dev.split(box.shape) for _ in (0, 1)]
    slot = 2 if ready else 0
    if ready:
        window_tables(dev, box, wins, slot)
    dev.launches(lambda: xy2(dev, box, wins, src, work, slot, ready), {K_TABLE: 1, K_Y: 1})
    for g in (0, 1):
        check(dev, box, g, work[g], wins[g], W_TABLE, f"xy2 ready={ready}")
    if ready:  # grid 1's spectrum under window a of the same tables
        shared = dev.split(box.shape)
        dev.launches(lambda: dev.lib.c21hip_split_filter_xy_shared(
            src[1].data_ptr(), shared.data_ptr(), wins[0].ftype, *box.shape, box.box_len, box.box_len_z, wins[0].R,
            1, slot, dev.stream), {K_TABLE: 1, K_Y: 1})
        check(dev, box, 1, shared, wins[0], W_TABLE, "xy_shared")


# ---------------------------------------------------------------- FMODE 5
def xy2_pair(dev, box, wins, R2, src, work, work2, phases):
    a, b = wins
    return dev.lib.c21hip_split_filter_xy2_pair(
        ptr(src[0]), work[0].data_ptr(), work2[0].data_ptr(), a.ftype, a.R_param, ptr(src[1]), work[1].data_ptr(),
        work2[1].data_ptr(), b.ftype, b.R_param, *box.shape, box.box_len, box.box_len_z, a.R, R2, 0, 1, phases,
        dev.stream)


@pytest.mark.parametrize("n", [64, 128, 192, 256, 384, 512])
def test_table_two_radii(dev, n):
    """Two radii out of one sweep, windows streamed from the tables of both (R2 ~ 3 R): both outputs of
    both grids; then one grid under window a of those tables (c21hip_split_filter_xy_shared_pair)."""
    shape = x_shape(n)
    assert_uneven_trips(shape)
    box = box_of(shape)
    R, R2 = 4.0, 12.5
    wins = excursion_pair(R)
    src = [dev.spectrum(box, g) for g in (0, 1)]
    work = [dev.split(box.shape) for _ in (0, 1)]
    work2 = [dev.split(box.shape) for _ in (0, 1)]
    dev.launches(lambda: xy2_pair(dev, box, wins, R2, src, work, work2, 15), {K_PAIR_TABLE: 1, K_Y: 2})
    for g in (0, 1):
        check(dev, box, g, work[g], wins[g], W_TABLE, "xy2_pair R")
        check(dev, box, g, work2[g], wins[g].at(R2), W_TABLE, "xy2_pair R2")
    # fresh tables in the other two slots' order, one grid (grid 1's spectrum) under window a
    window_tables(dev, box, wins, 0)
    window_tables(dev, box, [w.at(R2) for w in wins], 1)
    s1, s2 = dev.split(box.shape), dev.split(box.shape)
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy_shared_pair(
        src[1].data_ptr(), s1.data_ptr(), s2.data_ptr(), wins[0].ftype, *box.shape, box.box_len, box.box_len_z, R, R2,
        0, 1, 14, dev.stream), {K_PAIR_TABLE: 1, K_Y: 2})
    check(dev, box, 1, s1, wins[0], W_TABLE, "xy_shared_pair R")
    check(dev, box, 1, s2, wins[0].at(R2), W_TABLE, "xy_shared_pair R2")


def test_two_radii_refuse_1024_point_lines(dev):
    box = box_of(x_shape(1024))
    wins = excursion_pair(4.0)
    src = [dev.spectrum(box, 0)] * 2
    work = [dev.split(box.shape) for _ in range(4)]
    dev.lib.c21hip_ktime_enable(1)
    try:
        assert xy2_pair(dev, box, wins, 12.5, src, work[:2], work[2:], 15) == VALUE_ERROR
        for kind in (K_TABLE, K_Y, K_PAIR_TABLE, K_EVAL, K_PAIR_EVAL, K_OTHER):
            count = C.c_int()
            assert dev.lib.c21hip_ktime_report(kind, None, C.byref(count)) == 0 and count.value == 0
    finally:
        dev.lib.c21hip_ktime_enable(0)


# ---------------------------------------------------------------- FMODE 6 and 8
def eval_regime(box, covers):
    """(radius, exp-MFP mean free path): kR_max ~ 50 inside the node tables; beyond them R ~ 0.8 box_len or
    more (kR_max >= 1300 -- the window does not care that R exceeds the box), with a mean free path that keeps
    the exp-MFP window of order one (mfp / R = 0.6; the loop's 37.66 would leave 1e-4 of it)."""
    if covers:
        return box.radius(50.0), MFP
    R = box.radius_direct()
    return R, float(np.float32(0.6 * R))


@pytest.mark.parametrize("ftypes", [(0,), (1,), (3,), (0, 3), (1, 3)])
@pytest.mark.parametrize("covers", [True, False], ids=["nodes", "direct"])
@pytest.mark.parametrize("n", [128, 256, 512, 1024])
def test_evaluated_windows(dev, n, covers, ftypes):
    """FMODE 6 (node tables) / 8 (direct evaluation beyond them): one grid through c21hip_split_filter_xy,
    two through _xy2 -- and one grid under window b of the two-grid set."""
    shape = x_shape(n)
    assert_uneven_trips(shape)
    box = box_of(shape)
    R, mfp = eval_regime(box, covers)
    if 1 in ftypes:
        R = box.sharp_k_radius(R)
    wins = [Win(t, R, mfp if t == 3 else 0.0) for t in ftypes]
    w = dev.prepare(box, wins, [R], False, covers)
    if len(wins) == 1:
        one_grid(dev, box, wins[0], {K_EVAL: 1, K_Y: 1}, w, "xy eval")
        return
    src = [dev.spectrum(box, g) for g in (0, 1)]
    work = [dev.split(box.shape) for _ in (0, 1)]
    dev.launches(lambda: xy2(dev, box, wins, src, work, 0, 0), {K_EVAL: 1, K_Y: 1})
    for g in (0, 1):
        check(dev, box, g, work[g], wins[g], w, "xy2 eval")
    # grid 0's spectrum alone under window b (the whalo_sfr grid of a recombination run)
    alone = dev.split(box.shape)
    b = wins[1]
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy(src[0].data_ptr(), alone.data_ptr(), *box.shape, box.box_len,
                                                        box.box_len_z, b.ftype, b.R, b.R_param, 1, dev.stream),
                 {K_EVAL: 1, K_Y: 1})
    check(dev, box, 0, alone, b, w, "xy eval, window b")


# ---------------------------------------------------------------- FMODE 7 and 9
def pair_radii(box, covers, kR_max=None):
    if kR_max is not None:
        R2, mfp = box.radius(kR_max), MFP
    else:
        R2, mfp = eval_regime(box, covers)
    return float(np.float32(R2 / 3.0)), R2, mfp


def excursion_pair_eval(dev, box, R, R2, mfp, covers):
    """The two-grid two-radius sweep under evaluated windows, its phases split, and one grid under window b."""
    wins = [Win(0, R), Win(3, R, mfp)]
    w = dev.prepare(box, wins, [R, R2], True, covers)
    src = [dev.spectrum(box, g) for g in (0, 1)]
    work = [dev.split(box.shape) for _ in (0, 1)]
    work2 = [dev.split(box.shape) for _ in (0, 1)]
    dev.launches(lambda: xy2_pair(dev, box, wins, R2, src, work, work2, 14), {K_PAIR_EVAL: 1, K_Y: 2})
    # phases 2, 4, 8 in separate calls: the same bits (the calls without 2 need no source)
    p = [dev.split(box.shape) for _ in (0, 1)]
    p2 = [dev.split(box.shape) for _ in (0, 1)]
    dev.launches(lambda: xy2_pair(dev, box, wins, R2, src, p, p2, 2), {K_PAIR_EVAL: 1})
    dev.launches(lambda: xy2_pair(dev, box, wins, R2, [None, None], p, p2, 4), {K_Y: 1})
    dev.launches(lambda: xy2_pair(dev, box, wins, R2, [None, None], p, p2, 8), {K_Y: 1})
    for one, split in zip(work + work2, p + p2):
        assert dev.torch.equal(one, split), "phases 2, 4, 8 in separate calls differ from one call with 14"
    del p, p2
    for g in (0, 1):
        check(dev, box, g, work[g], wins[g], w, "xy2_pair eval R")
        check(dev, box, g, work2[g], wins[g].at(R2), w, "xy2_pair eval R2")
    b = wins[1]
    s1, s2 = dev.split(box.shape), dev.split(box.shape)
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy_single_pair(
        src[0].data_ptr(), s1.data_ptr(), s2.data_ptr(), b.ftype, b.R_param, *box.shape, box.box_len, box.box_len_z,
        R, R2, 14, dev.stream), {K_PAIR_EVAL: 1, K_Y: 2})
    check(dev, box, 0, s1, b, w, "xy_single_pair, window b, R")
    check(dev, box, 0, s2, b.at(R2), w, "xy_single_pair, window b, R2")


@pytest.mark.parametrize("covers", [True, False], ids=["nodes", "direct"])
@pytest.mark.parametrize("n", [128, 256, 512])
def test_evaluated_two_radii_excursion_pair(dev, n, covers):
    shape = x_shape(n)
    assert_uneven_trips(shape)
    box = box_of(shape)
    excursion_pair_eval(dev, box, *pair_radii(box, covers), covers)


@pytest.mark.parametrize("n", [128, 512])
def test_evaluated_two_radii_at_the_smallest_radii_of_the_loop(dev, n):
    """R = 0.9305 and 1.2385 Mpc (indices 0 and 3 of the loop's ladder on 1.5 Mpc cells), mfp / R = 40 and 30:
    filter_box forms exp(-R / mfp) from a float quotient, and what that rounding moves the term by is
    multiplied by 6 (mfp / R)^3 at k = 0 -- 2.8e-4 and 3.0e-4 of the window for these two radii, in a spike
    1 / 40 wide in kR that the lowest modes of the box sit in.  The node tables (1/4 apart) cannot carry it;
    the kernel adds it to the windows of those modes."""
    shape = x_shape(n)
    box = box_of(shape)
    R, R2 = float(np.float32(0.9305)), float(np.float32(0.9305 * 1.1 ** 3))
    assert ((box.k * R > 0) & (box.k * R < 0.05)).any()  # modes inside the spike
    excursion_pair_eval(dev, box, R, R2, MFP, True)


def test_evaluated_two_radii_512_between_the_caps(dev):
    """512-point lines, top-hat + exp-MFP, two radii: 739 nodes fit beside the two tiles, so a set that needs
    more than that -- but fewer than 4096 -- evaluates directly from kR = 184 on, where the windows are still
    1e-4 of their peak.  The regime of the 512^3 production box."""
    box = box_of(x_shape(512))
    R, R2, mfp = pair_radii(box, False, kR_max=400.0)
    assert wev_cap(512, True, [0, 3]) == 739 and 739 < wev_need(box, R2) < 4096
    excursion_pair_eval(dev, box, R, R2, mfp, False)


@pytest.mark.parametrize("covers", [True, False], ids=["nodes", "direct"])
@pytest.mark.parametrize("n", [128, 256, 512])
def test_evaluated_two_radii_eulerian_entries(dev, n, covers):
    """The Eulerian loops' entries: two grids under one sharp-k window (c21hip_split_filter_xy2_pair_eval) and one
    grid under the top-hat (c21hip_split_filter_x_pair1)."""
    box = box_of(x_shape(n))
    R, R2, _ = pair_radii(box, covers)
    # sharp-k: two radii, both clear of every mode
    Rs2 = box.sharp_k_radius(R2)
    Rs = box.sharp_k_radius(Rs2 / 3.0)
    wins = [Win(1, Rs), Win(1, Rs)]
    w = dev.prepare(box, wins, [Rs, Rs2], True, covers)
    src = [dev.spectrum(box, g) for g in (0, 1)]
    work = [dev.split(box.shape) for _ in (0, 1)]
    work2 = [dev.split(box.shape) for _ in (0, 1)]
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy2_pair_eval(
        src[0].data_ptr(), work[0].data_ptr(), work2[0].data_ptr(), 1, src[1].data_ptr(), work[1].data_ptr(),
        work2[1].data_ptr(), 1, *box.shape, box.box_len, box.box_len_z, Rs, Rs2, 14, dev.stream),
        {K_PAIR_EVAL: 1, K_Y: 2})
    for g in (0, 1):
        check(dev, box, g, work[g], wins[g], w, "xy2_pair_eval R")
        check(dev, box, g, work2[g], wins[g].at(Rs2), w, "xy2_pair_eval R2")
    del work, work2
    dev.lib.c21hip_wev_release()
    top = Win(0, R)
    w = dev.prepare(box, [top], [R, R2], True, covers)
    s1, s2 = dev.split(box.shape), dev.split(box.shape)
    dev.launches(lambda: dev.lib.c21hip_split_filter_x_pair1(
        src[0].data_ptr(), s1.data_ptr(), s2.data_ptr(), 0, *box.shape, box.box_len, box.box_len_z, R, R2, 14,
        dev.stream), {K_PAIR_EVAL: 1, K_Y: 2})
    check(dev, box, 0, s1, top, w, "x_pair1 R")
    check(dev, box, 0, s2, top.at(R2), w, "x_pair1 R2")


# ---------------------------------------------------------------- pass Y in the pipelined regime
@pytest.mark.parametrize("apply", [0, 1])
@pytest.mark.parametrize("n", [512, 768, 1024, 1536])
def test_pass_y_pipelined(dev, n, apply):
    """(64, n, 256): pass Y has 64 x 8 = 512 work items or more for 256 workgroups, so every workgroup takes
    at least a second trip; without a window (both inverse passes are FMODE 0) and under top-hat tables."""
    shape = (64, n, 256)
    assert shape[0] * (shape[2] // 2 // tile_cols(n)) >= 2 * 256
    box = box_of(shape)
    src, work = dev.spectrum(box, 0), dev.split(box.shape)
    win = Win(0, 5.0)
    dev.launches(lambda: dev.lib.c21hip_split_filter_xy(src.data_ptr(), work.data_ptr(), *box.shape, box.box_len,
                                                        box.box_len_z, win.ftype, win.R, 0.0, apply, dev.stream),
                 {K_TABLE: 1, K_Y: 1} if apply else {K_Y: 2})
    if apply:
        check(dev, box, 0, work, win, W_TABLE, "pass Y, top-hat tables")
    else:  # no window: the reference is the spectrum itself
        check(dev, box, 0, work, NO_WINDOW, 0.0, "pass Y, no window")
