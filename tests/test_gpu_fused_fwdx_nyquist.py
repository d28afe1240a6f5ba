"""Pass Y's epilogue over the Nyquist plane (fft_native.hip: line_pass_kernel, after `main_done`) against the
epilogue it replaces.

By default the epilogue deals one (tile, grid) pair per workgroup and moves the tile along y -- contiguous in
nyq[x][y] -- in 16-byte vectors, transposing on the LDS side; C21CM_YNYQ_SPLIT=0 restores two grids per workgroup
and 8-byte accesses at the column pitch.  That changes who transforms a tile and how it travels, never the tile's
contents or the arithmetic on it, so every comparison is array_equal against ONE child process that runs this file
as a script with the switch at 0 (it is read once per process).  c21hip_ynyq_split_enabled tells each process
which path it is on.

Shapes.  The native passes take lines of 64 points and more (c21hip_native_fft_supported), so:
  (64, 512, 256): 4 Nyquist tiles x 2 grids behind 512 main items (two trips of 256 workgroups);
  (64, 512, 64):  the smallest box with 512-point y-lines -- 128 main items, one trip, so that the 4 x 2 epilogue
                  tiles are most of the launch.
  (16, 512, 32) of the request is refused by the library (nx = 16 and nz = 32 are below the shortest native
  line); the refusal is asserted.
Covered: the forward pass Y of c21hip_split_r2c (one grid per launch), the inverse pass Y of two grids
(c21hip_split_filter_xy2) and of one (c21hip_split_filter_xy), and pass Z on what they leave.  The two grids hold
different data (their own seeds and means) and take different windows (top-hat, exp-MFP), so a swapped grid index
changes values.  Main block and Nyquist plane are compared separately.  The entries' main-block accesses are
16-byte vectors already and the plane follows the main block, so no entry allows an array offset of one float;
none is tested.

That pass Y computes the right transform on the default path is the business of test_gpu_pass_x_windows.py (every
mode against an fp64 filter)."""

import ctypes as C
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

Y_SHAPES = ((64, 512, 256), (64, 512, 64))
REFUSED = (16, 512, 32)
FILTERS = (0, 3)  # top-hat on grid 0, exp-MFP on grid 1: a.dual is set
MFP = 37.66
VALUE_ERROR = 3


def geometry(shape):
    box_len = 1.5 * shape[0]
    return box_len, 0.8 * box_len * shape[2] / shape[0]


class Dev:
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
            "c21hip_wev_release": (None, []),
            "c21hip_ynyq_split_enabled": (i, []),
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
        """A split-layout buffer full of NaN: whatever a pass leaves unwritten shows."""
        n = self.lib.c21hip_split_floats(*shape)
        return self.torch.full((n,), float("nan"), dtype=self.torch.float32, device="cuda")

    def real_input(self, shape, g):
        a = np.random.default_rng([411, g, *shape]).standard_normal(shape, np.float32) + np.float32(0.5 + g)
        return self.torch.from_numpy(a).cuda()

    def r2c(self, shape, real):
        out = self.split(shape)
        st = self.lib.c21hip_split_r2c(real.data_ptr(), shape[2], out.data_ptr(), *shape, 1.0, 1.0, 0.0,
                                       1.0 / float(np.prod(shape)), self.stream)
        return st, out

    def c2r(self, shape, work):
        out = self.torch.full(shape, float("nan"), dtype=self.torch.float32, device="cuda")
        self.ok(self.lib.c21hip_split_z_c2r(work.data_ptr(), out.data_ptr(), shape[2], *shape, self.stream))
        return out


def parts(out, name, shape, t):
    """A split spectrum as its main block and its Nyquist plane; anything else whole."""
    a = t.cpu().numpy()
    if a.ndim == 1:
        n_main = 2 * shape[0] * shape[1] * (shape[2] // 2)
        assert a.size == n_main + 2 * shape[0] * shape[1]
        assert np.isfinite(a).all(), f"{name}: modes left unwritten"
        out[f"{name}__main"], out[f"{name}__nyq"] = a[:n_main], a[n_main:]
    else:
        assert np.isfinite(a).all(), name
        out[name] = a


def tag(shape):
    return "x".join(str(n) for n in shape)


def run_pass_y(dev):
    """Forward pass Y (c21hip_split_r2c, one grid per call), the inverse pass Y of two grids (c21hip_split_filter_xy2)
    and of one (c21hip_split_filter_xy), then pass Z on each."""
    out = {}
    for shape in Y_SHAPES:
        box_len, box_len_z = geometry(shape)
        R = 0.05 * box_len
        spec = []
        for g in (0, 1):
            st, s = dev.r2c(shape, dev.real_input(shape, g))
            dev.ok(st)
            spec.append(s)
            parts(out, f"y_{tag(shape)}_spectrum{g}", shape, s)
        assert not dev.torch.equal(spec[0], spec[1])
        work = [dev.split(shape) for _ in (0, 1)]
        dev.ok(dev.lib.c21hip_split_filter_xy2(spec[0].data_ptr(), work[0].data_ptr(), FILTERS[0], 0.0,
                                               spec[1].data_ptr(), work[1].data_ptr(), FILTERS[1], MFP, *shape,
                                               box_len, box_len_z, R, 1, 0, 0, dev.stream))
        one = dev.split(shape)
        dev.ok(dev.lib.c21hip_split_filter_xy(spec[1].data_ptr(), one.data_ptr(), *shape, box_len, box_len_z,
                                              FILTERS[0], R, 0.0, 1, dev.stream))
        for g in (0, 1):
            parts(out, f"y_{tag(shape)}_work{g}", shape, work[g])
            parts(out, f"y_{tag(shape)}_real{g}", shape, dev.c2r(shape, work[g]))
        parts(out, f"y_{tag(shape)}_one_grid", shape, one)
        # the grids are told apart: grid 1's spectrum under grid 0's window differs from both two-grid outputs
        assert not dev.torch.equal(one, work[0]) and not dev.torch.equal(one, work[1])
    return out


SWITCH = "C21CM_YNYQ_SPLIT"


@pytest.fixture(scope="module")
def dev(gpu_lib):
    d = Dev(gpu_lib)
    gpu_lib.c21hip_wev_release()
    yield d
    gpu_lib.c21hip_wev_release()


@pytest.fixture(scope="module")
def both_paths(dev, tmp_path_factory):
    """(outputs of this process on the default path, outputs of one child with the switch at 0)."""
    assert SWITCH not in os.environ
    assert dev.lib.c21hip_ynyq_split_enabled() == 1
    here = run_pass_y(dev)
    path = tmp_path_factory.mktemp("ynyq_split") / "switch_off.npz"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), str(path)]
    subprocess.run(cmd, check=True, env=dict(os.environ, **{SWITCH: "0"}), cwd=str(ROOT), timeout=300)
    with np.load(path) as f:
        return here, {k: f[k] for k in f.files}


@pytest.mark.parametrize("shape", Y_SHAPES, ids=tag)
def test_bit_identity_with_the_switch_off(both_paths, shape):
    here, off = both_paths
    assert sorted(here) == sorted(off)
    names = [k for k in sorted(here) if k.startswith(f"y_{tag(shape)}_")]
    # 2 forward spectra, 2 two-grid work spectra, 1 one-grid work spectrum (main + Nyquist each), 2 real grids
    assert len(names) == 12, names
    for name in names:
        np.testing.assert_array_equal(here[name], off[name], err_msg=name)
    print(f"{tag(shape)}: {len(names)} arrays equal, {sum(here[k].size for k in names)} values")


def test_shape_below_the_native_lines_is_refused(dev):
    """(16, 512, 32) has lines shorter than 64 points: the entry refuses it before any launch, whatever the switch
    says."""
    shape = REFUSED
    real = dev.torch.zeros(shape, dtype=dev.torch.float32, device="cuda")
    out = dev.torch.zeros(2 * shape[0] * shape[1] * (shape[2] // 2 + 1), dtype=dev.torch.float32, device="cuda")
    st = dev.lib.c21hip_split_r2c(real.data_ptr(), shape[2], out.data_ptr(), *shape, 1.0, 1.0, 0.0, 1.0, dev.stream)
    assert st == VALUE_ERROR
    dev.torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


if __name__ == "__main__":  # the child of `both_paths`: the same cases with the switch at 0
    pkg = importlib.import_module("21cmfast_amd")
    lib = pkg.load(require_gpu=True)
    assert os.environ.get(SWITCH) == "0" and lib.c21hip_ynyq_split_enabled() == 0
    np.savez(sys.argv[1], **run_pass_y(Dev(lib)))
