"""CPU-side checks of the budget entry points (kid_budget, kid_stock, kid_incr_mass): exported by the library and declared
in include/kid.h, kid_budget_out laid out the same in the header, in ctypes and in the generated Fortran include."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

from icebergs_amd import lib as L
from icebergs_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kid_budget", "kid_stock", "kid_incr_mass")


def test_symbols_are_exported_and_declared():
    L.build()
    lib = C.CDLL(L.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "kid.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in L.SYMBOLS
        assert "bind(C, name='%s')" % name in mod, name
    assert T.ENUMS["KID_STOCK_WATER"] != T.ENUMS["KID_STOCK_HEAT"]


def test_generated_fortran_types_are_current(tmp_path):
    """kid_types_gen.inc is what tools/gen_fortran_types.py makes of the header today, kid_budget_out included (the generator
    writes to a path of the test's: the committed file is only read)"""
    before = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_types_gen.inc")).read()
    fresh = tmp_path / "kid_types_gen.inc"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_fortran_types.py"), str(fresh)], check=True, capture_output=True)
    assert fresh.read_text() == before
    assert "type, bind(C) :: kid_budget_out" in before
    assert re.search(r"KID_STOCK_WATER = %d\b" % T.ENUMS["KID_STOCK_WATER"], before)
    assert re.search(r"KID_STOCK_HEAT = %d\b" % T.ENUMS["KID_STOCK_HEAT"], before)


def test_budget_out_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof of kid_budget_out as a C compiler sees the header, against the ctypes mirror"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    fields = [name for name, _ in T.BudgetOut._fields_]
    assert len(fields) == 12
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kid_types.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(kid_budget_out));\n'
                   + "".join('  printf("%s %%zu\\n", offsetof(kid_budget_out, %s));\n' % (f, f) for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(T.BudgetOut)
    for f in fields:
        assert int(out[f]) == getattr(T.BudgetOut, f).offset, f
    # no implicit padding: Fortran bind(C) types and stream I/O move components one by one
    assert C.sizeof(T.BudgetOut) == sum(C.sizeof(t) for _, t in T.BudgetOut._fields_)
