"""Footloose calving among interacting bergs, the part that needs no GPU (tests/fl_interactive.py has the box and the composed
oracle step): the population shows what the GPU tests rely on, the fl_k = -1 guards of the oracle do what the composition
assumes, the guard is what makes the difference, the two decisions of the promotion pass (icebergs_amd/csrc/kid_fl_contact.hpp)
hold under sanitizers, and the entry point is declared through every host layer."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fl_interactive as FI
import halo_bergs as HB
from icebergs_amd import synthetic as S
from parity import TOL_TRAJ

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEARCHES = [pytest.param(False, id="3x3"), pytest.param(True, id="contact")]


@pytest.mark.parametrize("contact", SEARCHES)
def test_population_shows_what_it_must(contact):
    _, _, st, _, _ = FI.composed_run(contact)
    print("children %d promotions %d pairs %d held back at the end %d margin %.3e" %
          (st["children"], st["promotions"], st["pairs"], st["held_back"][-1], st["margin"]))
    assert st["children"] >= 100
    assert st["promotions"] >= 20
    assert st["pairs"] >= 100, "promoted children must go on to collide"
    assert min(st["held_back"]) >= 1, "at every step some child is held back at fl_k = -1"
    assert st["finite"]
    assert st["margin"] >= FI.MARGIN, "a promotion hangs on the last bits of r_dist / crit_dist"


def test_population_with_children_from_footloose_bits():
    """the other fl_style on the contact search: children are made from their parents' footloose bits (measured: 182 children,
    20 promotions, 157 held back at the end, margin 3.3e-4)"""
    _, _, st, _, _ = FI.composed_run(True, fl_bits=True)
    print("children %d promotions %d held back at the end %d margin %.3e" % (st["children"], st["promotions"], st["held_back"][-1], st["margin"]))
    assert st["children"] >= 100 and st["promotions"] >= 10 and min(st["held_back"]) >= 1
    assert st["finite"] and st["margin"] >= FI.MARGIN


def _evolve(grid, p, b):
    c = FI.Composed(grid, p, b)
    c.evolve()
    return b


def _subset(b, rows):
    q = S.empty_bergs(len(rows))
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            q[k][:] = v[rows]
    q["_n"] = len(rows)
    return q


@pytest.mark.parametrize("contact", SEARCHES)
def test_guards_do_what_the_composition_assumes(contact):
    """the evolve of the state before step 20: taking the fl_k = -1 children out changes nothing for anybody else, and each such
    child moves as it does alone in the box"""
    _, before, _, p, grid = FI.composed_run(contact)
    b0 = before[20]
    n = b0["_n"]
    live = b0["alive"][:n] != 0
    waiting = live & (b0["fl_k"][:n] == -1.0)
    assert waiting.sum() >= 10 and (live & ~waiting).sum() >= 100
    full = _evolve(grid, p, _subset(b0, np.nonzero(live)[0]))
    others = _evolve(grid, p, _subset(b0, np.nonzero(live & ~waiting)[0]))
    keep = np.nonzero(~waiting[live])[0]
    assert np.array_equal(full["id"][keep], others["id"])
    for f in HB.FIELDS + ("ine", "jne", "alive"):
        assert np.array_equal(full[f][keep], others[f]), f
    rows = np.nonzero(waiting)[0]
    at = {int(i): q for q, i in enumerate(full["id"])}
    for k in rows:
        alone = _evolve(grid, p, _subset(b0, np.array([k])))
        q = at[int(b0["id"][k])]
        for f in HB.FIELDS + ("ine", "jne", "alive"):
            assert alone[f][0] == full[f][q], (f, int(b0["id"][k]))


@pytest.mark.parametrize("contact", SEARCHES)
def test_the_guard_is_what_makes_the_difference(contact):
    """children relabelled interactive (fl_k = -2) at birth collide with their parents at once: another run"""
    snaps, _, _, _, _ = FI.composed_run(contact)
    relabelled, _, _, _, _ = FI.composed_run(contact, relabel=True)
    a, b = snaps[20][0], relabelled[20][0]
    la, lb = a["alive"][:a["_n"]] != 0, b["alive"][:b["_n"]] != 0
    ids, ia, ib = np.intersect1d(a["id"][:a["_n"]][la], b["id"][:b["_n"]][lb], return_indices=True)
    assert len(ids) >= 100
    ua, ub = a["uvel"][:a["_n"]][la][ia], b["uvel"][:b["_n"]][lb][ib]
    dev = float(np.abs(ua - ub).max() / np.abs(ua).max())
    print("uvel of the relabelled run deviates by %.3e" % dev)
    assert dev > TOL_TRAJ


def test_promotion_pass_on_a_hand_made_case():
    """three discs of 1 km radius in one cell and a fourth two cells away: the child next to its parent waits, the child alone
    is promoted, nobody else's fl_k is touched; a dead neighbour is nobody's partner"""
    p = FI.params(False)
    d = FI.grid()["desc"]
    b = S.empty_bergs(5)
    side = np.sqrt(np.pi) * 1000.0
    b["length"][:], b["width"][:] = side, side
    b["lon"][:] = [12000.0, 13500.0, 27000.0, 31000.0, 27500.0]
    b["lat"][:] = 12000.0
    b["ine"][:] = np.floor(b["lon"] / HB.RES).astype(np.int32) + 1
    b["jne"][:] = 3
    b["fl_k"][:] = [100.0, -1.0, -1.0, -2.0, 50.0]
    b["alive"][4] = 0
    assert FI.np_adjust(p, d, b, 5) == [2]
    assert list(b["fl_k"]) == [100.0, -1.0, -2.0, -2.0, 50.0]
    b["fl_k"][2], b["alive"][4] = -1.0, 1             # alive, 500 m away: the child waits
    assert FI.np_adjust(p, d, b, 5) == []


@pytest.mark.parametrize("contact", [False, True])
def test_latlon_state_takes_the_latlon_branch_with_a_margin(contact):
    """the box on a lat-lon patch (FI.latlon_state): np_adjust takes its grid_is_latlon branch, promotes some children and holds
    some back, no decision is closer to its threshold than MARGIN, and the other branch would decide differently"""
    g, p, b = FI.latlon_state(contact)
    n = len(b["lon"])
    assert g["desc"].grid_is_latlon == 1 and p.Rearth == 6.36e6 and np.abs(b["lat"]).min() > 69.0
    children = int((b["fl_k"] == -1.0).sum())
    margins, w = [], S.copy_bergs(b)
    rows = FI.np_adjust(p, g["desc"], w, n, margins)
    print("lat-lon %s: %d rows, %d children, %d promoted, smallest margin %.1e" % ("contact" if contact else "3x3", n, children, len(rows), min(margins)))
    assert 3 <= len(rows) <= children - 10 and min(margins) >= FI.MARGIN
    flat = S.cartesian_grid(HB.NI * HB.NTX, HB.NJ * HB.NTY, HB.RES)["desc"]     # the same cells, grid_is_latlon = 0: degrees taken for metres
    assert FI.np_adjust(p, flat, S.copy_bergs(b), n) != rows


def test_fl_contact_under_sanitizers(tmp_path):
    cxx = None
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            cxx = shutil.which(c)
            break
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "fl_contact_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "fl_contact_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"


def test_entry_point_is_declared_in_every_host_layer():
    from icebergs_amd import lib as L
    name = "kid_adjust_fl_berg_interactivity"
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kid.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*promoted\s*\)\s*;" % name, hdr)
    assert name in L.SYMBOLS
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    assert "bind(C, name='%s')" % name in mod
    public = set()
    for m in re.finditer(r"^\s*public ::(.*)$", mod, re.M):
        public |= {x.strip() for x in m.group(1).split(",")}
    assert name in public
    L.build()
    lib = L.load()
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.POINTER(C.c_int64)]
    from icebergs_amd.framework import Icebergs
    assert callable(Icebergs.adjust_fl_berg_interactivity)
