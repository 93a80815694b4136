"""include/mythgpu.h is the one definition of the device interface's constants
(no GPU needed): mythril_amd.abi reads every one of them as the C preprocessor
does, and the Python modules that hand them on hold abi's values."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from mythril_amd import abi, lanes, native
from mythril_amd.smt import program

HEADER = Path(__file__).resolve().parent.parent / "include" / "mythgpu.h"


def test_c_compiler_agrees_with_the_parser(tmp_path):
    """A C program prints every name abi exposes; the preprocessor's values are abi's."""
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no host C compiler"
    names = list(abi.DEFINES) + list(abi.BV_ENUM)
    assert len(names) == len(set(names))
    src = tmp_path / "abi_print.c"
    src.write_text('#include <stdio.h>\n#include "mythgpu.h"\nint main(void) {\n'
                   + "".join(f'    printf("{n} %lld\\n", (long long)({n}));\n' for n in names)
                   + "    return 0;\n}\n")
    exe = tmp_path / "abi_print"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", f"-I{HEADER.parent}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {line.split()[0]: int(line.split()[1]) for line in out.splitlines()}
    assert got == {**abi.DEFINES, **abi.BV_ENUM}


def test_every_integer_define_is_exposed():
    """Counted by a regex of the test's own: an object-like `#define MG_*` (a name,
    then blanks, then its value; the function-like ones have a parenthesis there)."""
    found = [line.split()[1] for line in HEADER.read_text().splitlines()
             if line.startswith("#define MG_") and re.fullmatch(r"\w+", line.split()[1]) and len(line.split()) > 2]
    assert len(found) >= 100 and len(found) == len(set(found))
    assert found == list(abi.DEFINES)
    for name in found:
        assert type(getattr(abi, name)) is int and getattr(abi, name) == abi.DEFINES[name], name
    assert abi.MG_ABI_VERSION == 15


def test_unparsable_define_is_an_import_error():
    with pytest.raises(ImportError):
        abi.parse(HEADER.read_text() + "\n#define MG_BROKEN sizeof(int)\n")
    with pytest.raises(ImportError):
        abi.parse(HEADER.read_text() + "\n#define MG_BROKEN MG_NOT_DEFINED + 1\n")


def test_program_ops_are_the_headers_list():
    assert program.OPS == [host for _, host in abi.BV_OPS]
    assert len(program.OPS) == abi.MG_BV_NUM_OPS == 47
    assert [abi.BV_ENUM[f"MG_BV_{c}"] for c, _ in abi.BV_OPS] == list(range(47))
    assert program.OPCODE["copy"] == abi.MG_BV_COPY == 0 and program.OPCODE["rconcat"] == abi.MG_BV_RCONCAT == 46
    assert (program.REF_ACC, program.REF_SLOT, program.REF_VAR, program.REF_CONST) == (
        abi.MG_BV_REF_ACC, abi.MG_BV_REF_SLOT, abi.MG_BV_REF_VAR, abi.MG_BV_REF_CONST)
    assert (program.MAX_SLOTS, program.TILE_INSNS) == (abi.MG_BV_MAX_SLOTS, abi.MG_BV_TILE_INSNS) == (16, 2048)
    assert (program.TAB_PART_SHIFT, program.TAB_LO_SHIFT, program.TAB_INDEX_MASK) == (
        abi.MG_BV_TAB_PART_SHIFT, abi.MG_BV_TAB_LO_SHIFT, abi.MG_BV_TAB_INDEX_MASK)


def test_lanes_and_native_hand_on_abis_values():
    for name, value in {**abi.DEFINES, **abi.BV_ENUM}.items():
        assert getattr(lanes, name) is getattr(abi, name) and getattr(abi, name) == value, name
    errors = ["MG_OK"] + [n for n, v in abi.DEFINES.items() if v < 0]      # the MG_E* codes
    assert len(errors) == 7
    for name in errors:
        assert getattr(native, name) is getattr(abi, name), name
    assert native.INCLUDE / "mythgpu.h" == abi.HEADER == HEADER
