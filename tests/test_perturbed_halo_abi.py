"""CPU checks of the PerturbedHaloCatalog boundary: the struct of include/c21cm_abi.h against the
reference's own layout (tests/golden/abi_layout.json), its ctypes mirror against gcc, and the exported
ComputePerturbedHaloCatalog / c21cm_perturb_halos_grids."""

import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "golden"))
import make_abi_layout as M  # noqa: E402

NAME = "PerturbedHaloCatalog"


def test_struct_matches_the_reference_layout_and_its_ctypes_mirror(pkg, tmp_path):
    doc = json.loads((ROOT / "tests" / "golden" / "abi_layout.json").read_text())
    ref = doc["structs"][NAME]
    fields = [f[0] for f in ref["fields"]]
    ours = dict(M.parse_structs((ROOT / "include" / "c21cm_abi.h").read_text()))
    assert NAME in ours, f"{NAME} is absent from include/c21cm_abi.h"
    assert ours[NAME] == fields  # same names, same order
    got = M.layout_of(["c21cm_abi.h"], [(NAME, fields)], include_dirs=[str(ROOT / "include")])
    assert got[NAME]["size"] == ref["size"]
    assert got[NAME]["fields"] == ref["fields"]  # offsets and sizes
    # the ctypes mirror, against what gcc lays out for the header
    cls = pkg.structs.PerturbedHaloCatalogStruct
    assert [f for f, _ in cls._fields_] == fields
    assert C.sizeof(cls) == ref["size"]
    for name, offset, size in ref["fields"]:
        assert getattr(cls, name).offset == offset and getattr(cls, name).size == size, name
    # ... and of the grid-level spec
    mirrors = {NAME: cls, "c21cm_perturb_halos_spec": pkg.structs.PerturbHalosSpec}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "c21cm_grid.h"', "int main(void){"]
    for name, mirror in mirrors.items():
        lines.append(f'printf("{name} size %zu\\n", sizeof({name}));')
        lines += [f'printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _ in mirror._fields_]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    for line in out.strip().splitlines():
        name, field, value = line.split()
        mirror = mirrors[name]
        assert (C.sizeof(mirror) if field == "size" else getattr(mirror, field).offset) == int(value), line


def test_entry_points_are_exported_with_the_reference_prototype(pkg):
    doc = json.loads((ROOT / "tests" / "golden" / "abi_layout.json").read_text())
    protos = M.parse_prototypes((ROOT / "include" / "c21cm_abi.h").read_text())
    assert protos.get("ComputePerturbedHaloCatalog") == 6 == doc["prototype_arg_counts"]["ComputePerturbedHaloCatalog"]
    lib = pkg.load()  # loads without a GPU
    assert hasattr(lib, "ComputePerturbedHaloCatalog") and hasattr(lib, "c21cm_perturb_halos_grids")
