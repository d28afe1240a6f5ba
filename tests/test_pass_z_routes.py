"""Which boxes each pass-Z route serves, as literal tables: the exported c21hip_z_*_supported predicates and
c21hip_z_ionise_partials (fft_native.hip: z_fused_select and the one-grid launchers' own conditions), and
c21cm_ionize_shard_rc_supported (ionize_driver.c: fused_rc_route, which ctx_setup shares).  The driver picks its
loop and sizes its workspaces by these answers, so a refactor of the launchers must not move one of them.

The tables were printed by a build of the commit before the predicates became calls of z_fused_select, under the
default environment (no C21CM_* switch set); they are not derived from the code under test.  No GPU needed: the
predicates are host arithmetic."""

import ctypes as C
import os

import pytest
from recomb_helpers import recomb_spec

NZ = (64, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048)
# (nx, ny).  The wave-level kernels take 16 lines per workgroup at 512 / 1024 points and 32 at 256 points
# (zw_lines_of), the 1024-point fused kernel 4: 32 lines serve all, 48 lines the 16-line kernels only, 20 lines
# the 4-line kernel only, 15 lines none.
SHAPES = ((8, 8), (64, 64), (1024, 16), (3, 5), (4, 8), (3, 16), (4, 5))
# predicate -> one string per NZ entry, one character per SHAPES entry
EXPECTED = {
    "c21hip_z_ionise_xe_supported":
        ('0000000', '0000000', '0000000', '1110100', '0000000', '1110110', '0000000', '1110110', '0000000', '0000000'),
    "c21hip_z_cross_bits_supported":
        ('0000000', '0000000', '0000000', '0000000', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_ionise_recomb_supported":
        ('0000000', '0000000', '0000000', '1110100', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_ionise_recomb_xe_supported":
        ('0000000', '0000000', '0000000', '1110100', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_ionise_recomb_xe_nrec_supported":
        ('0000000', '0000000', '0000000', '0000000', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_xe_mask_supported":
        ('0000000', '0000000', '0000000', '1110100', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_xe_fcoll_band_supported":
        ('0000000', '0000000', '0000000', '0000000', '0000000', '1110110', '0000000', '0000000', '0000000', '0000000'),
    "c21hip_z_fcoll_erfc_mask_supported":
        ('0000000', '0000000', '0000000', '0000000', '0000000', '1110110', '0000000', '1110110', '0000000', '0000000'),
    "c21hip_z_table_band_supported":
        ('0000000', '0000000', '0000000', '0000000', '0000000', '1110110', '0000000', '1110110', '0000000', '0000000'),
}
# c21hip_z_ionise_partials: one row per NZ entry, one column per SHAPES entry
PARTIALS = (
    (8, 512, 2048, 1, 4, 6, 2),
    (8, 512, 2048, 1, 4, 6, 2),
    (8, 512, 2048, 1, 4, 6, 2),
    (2, 128, 512, 1, 1, 6, 2),
    (8, 512, 2048, 1, 4, 6, 2),
    (4, 256, 1024, 1, 2, 3, 2),
    (8, 512, 2048, 1, 4, 6, 2),
    (16, 1024, 4096, 1, 8, 12, 5),
    (8, 512, 2048, 1, 4, 6, 2),
    (8, 512, 2048, 1, 4, 6, 2),
)
# (HII_DIM, z-line length) -> c21cm_ionize_shard_rc_supported for recombination model 0, 1, 2 (outermost) x
# cell_recomb 0, 1 x x_e grid 0, 1 (innermost)
ROUTES = {
    (128, 256): "000000111011",
    (128, 512): "000000111111",
    (128, 1024): "000000000000",
    (64, 64): "000000000000",
    (50, 50): "000000000000",
}


@pytest.fixture(scope="module")
def lib(pkg):
    switches = ("C21CM_ZPASS", "C21CM_CROSS_BITS", "C21CM_WINDOWS", "C21CM_R0_ROUNDTRIP", "C21CM_RECOMB_FUSED",
                "C21CM_RECOMB_FUSED_TS", "C21CM_RECOMB_FUSED_NREC")  # what the answers depend on
    assert not [k for k in switches if k in os.environ], "the tables hold under the default environment only"
    return pkg.load()


def test_pass_z_predicates_keep_their_table(lib):
    for name, want in EXPECTED.items():
        f = getattr(lib, name)
        f.restype = C.c_int
        got = tuple("".join(str(f(nx, ny, nz)) for nx, ny in SHAPES) for nz in NZ)
        assert got == want, name
    lib.c21hip_z_ionise_partials.restype = C.c_int
    got = tuple(tuple(lib.c21hip_z_ionise_partials(nx, ny, nz) for nx, ny in SHAPES) for nz in NZ)
    assert got == PARTIALS
    # what the issue that introduced this table observed
    at = lambda nz, shape: [EXPECTED[p][NZ.index(nz)][SHAPES.index(shape)] for p in EXPECTED]
    assert at(512, (64, 64)) == ["1"] * 9
    assert [p for p in EXPECTED if EXPECTED[p][NZ.index(1024)][1] == "1"] == [
        "c21hip_z_ionise_xe_supported", "c21hip_z_fcoll_erfc_mask_supported", "c21hip_z_table_band_supported"]
    assert all(at(nz, (3, 5)) == ["0"] * 9 for nz in NZ)
    assert all(at(nz, s) == ["0"] * 9 for nz in NZ if nz not in (256, 512, 1024) for s in SHAPES)


def test_ionise_entry_refuses_a_descriptor_of_another_size(lib):
    """c21hip_z_ionise_desc.size: a mirror of another layout is refused before any member is read (no launch)."""
    lib.c21hip_split_z_ionise.restype = C.c_int
    lib.c21hip_split_z_ionise.argtypes = [C.c_void_p, C.c_void_p]
    lib.c21hip_get_error.restype = C.c_char_p
    stale = (C.c_size_t * 32)()  # zeroed: every pointer NULL, should the entry read on
    for size in (0, 8, C.sizeof(stale)):
        stale[0] = size
        assert lib.c21hip_split_z_ionise(stale, None) == 3  # C21CM_VALUE_ERROR
        assert b"size" in lib.c21hip_get_error()
    assert lib.c21hip_split_z_ionise(None, None) == 3


def test_fused_recombination_route_keeps_its_table(lib):
    lib.c21cm_ionize_shard_rc_supported.restype = C.c_int
    for (n, nz), want in ROUTES.items():
        got = ""
        for model in (0, 1, 2):
            for cell_recomb in (0, 1):
                for ts in (0, 1):
                    spec = recomb_spec(n, model=model, cell_recomb=cell_recomb, hii_dim_z=nz, ts=ts)
                    got += str(lib.c21cm_ionize_shard_rc_supported(C.byref(spec)))
        assert got == want, (n, nz)
    assert lib.c21cm_ionize_shard_rc_supported(None) == 0
