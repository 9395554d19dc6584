"""Growable capacity, the part that needs no GPU: the plan of kid_reserve (icebergs_amd/csrc/kid_reserve_plan.hpp: the next
capacity of the growth rule and the allocate-copy-swap-free sequence) runs on the host under the address and undefined-behaviour
sanitizers against an allocator that can be told to fail (tests/reserve_plan_host.cpp), and the three entry points are declared
through every host layer."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("kid_capacity", "kid_reserve", "kid_set_auto_reserve")


def test_reserve_plan_under_sanitizers(tmp_path):
    cxx = None
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            cxx = shutil.which(c)
            break
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "reserve_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "reserve_plan_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "reserve plan: all checks passed"


def test_plan_header_has_no_hip():
    """the plan is plain C++: the host program above is the proof that it compiles without a HIP header, this that nobody
    slips one in behind an #ifdef"""
    text = open(os.path.join(ROOT, "icebergs_amd", "csrc", "kid_reserve_plan.hpp")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip|__global__|__device__|hipMalloc|hipMemcpy", text)


def test_entry_points_are_declared_in_every_host_layer():
    from icebergs_amd import lib as L
    from icebergs_amd.decomposed import HipTile
    from icebergs_amd.framework import Icebergs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kid.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kid_capacity\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*rows\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+kid_reserve\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s+rows\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+kid_set_auto_reserve\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s+min_free\s*,\s*double\s+growth\s*,\s*int64_t\s+max_capacity\s*\)\s*;", hdr)
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    public = set()
    for m in re.finditer(r"^\s*public ::(.*)$", mod, re.M):
        public |= {x.strip() for x in m.group(1).split(",")}
    glue = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_icebergs_glue.F90")).read()
    for name in NAMES:
        assert name in L.SYMBOLS
        assert re.search(r"bind\(C,\s*name='%s'\)" % name, mod) and name in public
    for cls in (Icebergs, HipTile):
        assert isinstance(cls.capacity, property) and callable(cls.reserve) and callable(cls.set_auto_reserve)
    assert re.search(r"subroutine kid_glue_reserve\(g, rows\)", glue) and re.search(r"public ::[^!]*kid_glue_reserve", glue, re.S)
    assert "auto_reserve_growth" in glue and "auto_reserve_min_free" in glue
    assert "error stop 'kid_glue_unflatten: the population outgrew" not in glue      # it grows instead
    make = open(os.path.join(ROOT, "icebergs_amd", "fortran", "Makefile")).read()
    assert re.search(r"^kid_reserve_test:", make, re.M) and re.search(r"^all:.*\bkid_reserve_test\b", make, re.M)


def test_every_block_sized_by_the_capacity_is_in_the_inventory():
    """a block that a later change sizes by h->capacity must be listed in kid_reserve.inc (moved, reallocated or freed): the member
    names that csrc allocates with the capacity in the size are looked up in the list"""
    csrc = os.path.join(ROOT, "icebergs_amd", "csrc")
    inv = open(os.path.join(csrc, "kid_reserve.inc")).read()
    listed = set(re.findall(r"h->([A-Za-z_0-9.]+)", inv))
    sized = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".inc", ".hip", ".hpp")) or f == "kid_reserve.inc":
            continue
        text = open(os.path.join(csrc, f)).read()
        for line in text.splitlines():
            if "mem.dev(" not in line and "rp_mem.dev(" not in line:
                continue
            for member, size in re.findall(r"mem\.dev\(\s*(?:\*q|h->([A-Za-z_0-9.\[\]]+))\s*,\s*([^;]*?)\)\);", line):
                if re.search(r"\bcap\b|\bnb\b|h->capacity", size) and member:
                    sized.add(re.sub(r"\[[^\]]*\]", "", member))
    assert len(sized) >= 12, sorted(sized)
    missing = {m for m in sized if m not in listed}
    assert not missing, sorted(missing)
