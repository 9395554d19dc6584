"""Bond tables through a row permutation, the parts that need no GPU.

* The rule (icebergs_amd/csrc/kid_rows_plan.hpp: bond_ref_moved, the BOND_FILL_* values, bond_refs_compose): tests/bond_rows_host.cpp
  enumerates it over the four kinds of partner, takes rings of bonded rows with empty to full lists at max_bonds 1, 4 and 6 through
  the identity, a reversal, a shuffle, a re-binning with dead rows and a compaction, and holds one table of eight rows against
  hand-written values -- under AddressSanitizer and UndefinedBehaviorSanitizer.  Host code with its own main; no HIP.
* The interface: kid_set_bonds_follow_rows and kid_bond_partner_rows are declared in include/kid.h, bound in icebergs_amd/lib.py with
  the argument types of the declaration, and have a bind(C) interface in the Fortran module."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_bond_rows_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "bond_rows_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "bond_rows_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"


def test_both_entries_are_declared_bound_and_in_the_fortran_module():
    from icebergs_amd import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kid.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kid_set_bonds_follow_rows\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int\s+on\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+kid_bond_partner_rows\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int32_t\s*\*\s*row\s*,\s*int32_t\s*\*\s*slot\s*,\s*int64_t\s+n\s*\)\s*;", hdr)
    assert "kid_set_bonds_follow_rows" in L.SYMBOLS and "kid_bond_partner_rows" in L.SYMBOLS
    L.build()
    lib = L.load()
    assert lib.kid_set_bonds_follow_rows.argtypes == [C.c_void_p, C.c_int] and lib.kid_set_bonds_follow_rows.restype is C.c_int
    assert lib.kid_bond_partner_rows.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]
    assert lib.kid_bond_partner_rows.restype is C.c_int
    # no handle: refused before anything is looked at (KID_EINVAL), as every entry point does
    assert lib.kid_set_bonds_follow_rows(None, 1) == -1
    assert lib.kid_bond_partner_rows(None, None, None, 0) == -1
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    public = set()
    for m in re.finditer(r"^\s*public ::(.*)$", mod, re.M):
        public |= {x.strip() for x in m.group(1).split(",")}
    for name in ("kid_set_bonds_follow_rows", "kid_bond_partner_rows"):
        assert re.search(r"bind\(C, name='%s'\)" % name, mod), name
        assert name in public, name
    from icebergs_amd.framework import Icebergs
    assert callable(Icebergs.set_bonds_follow_rows) and callable(Icebergs.bond_partner_rows)
