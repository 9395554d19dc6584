"""The rows of the berg SoA (icebergs_amd/csrc/kid_rows.inc): compaction as a permutation, and the state that depends on rows.

* kid_compact_bergs equals x[alive != 0], bit for bit, for every member: it goes through the one-launch gather of the re-binning,
  so sizes around the 256-thread workgroup and the 64-lane wave, none / all / first-and-last / every 7th / a run of 70 rows dead;
  members uploaded as NULL come back as zeros and at least one of them was left where it was (the skip rule had work to do).
* compaction right after a re-binning -- pending for the next plain hot build, or copied at once (KID_REBIN_EAGER) -- gives the
  rows that compaction of the downloaded and re-uploaded state gives, which are the live rows in cell order.
* with bond tables (indexed by row, and nothing moves them) compaction is refused and changes nothing.
* footloose children appended behind the dead tail of a re-binning survive the count that follows.

All on the 48 x 40 lat-lon box of tests/test_handle_memory_gpu.py under the plain namelist, but the footloose case (config 3 of the
golden run c3_new_bergs).  No case steps more than once."""
import ctypes as C
import os

import numpy as np
import pytest

from icebergs_amd import lib as L
from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from icebergs_amd.framework import Icebergs

pytestmark = pytest.mark.gpu

NF64 = T.ENUMS["KID_NB_F64"]
MEMBERS = list(T.BERG_F64_NAMES) + list(T.BERG_I32_NAMES) + ["id"]
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


def _box():
    grid = S.c2_forcing(S.latlon_grid(ni=48, nj=40, lon0=10.0, dlon=0.02, lat0=-60.0, dlat=0.02))
    p = S.default_params()
    p.dt = 1800.0
    return grid, p


@pytest.fixture(scope="module")
def box():
    """one handle for the compaction cases: every case uploads its own population"""
    grid, p = _box()
    ib = Icebergs(grid, p, capacity=max(SIZES))
    yield ib
    ib.close()


def _full_soa(n, alive):
    """every member distinct and non-zero per row; cells valid and inside"""
    b = S.empty_bergs(n)
    k = np.arange(n)
    for f, name in enumerate(T.BERG_F64_NAMES):
        b[name][:] = (f + 1) * 4096.0 + k + 0.5
    b["ine"][:] = 4 + (k * 7) % 41                # 4 .. 44
    b["jne"][:] = 4 + (k * 5) % 33                # 4 .. 36
    b["start_year"][:] = 1900 + k
    b["n_bonds"][:] = 1 + k % 5
    b["conglom_id"][:] = 7 + 3 * k
    b["alive"][:] = alive
    b["id"][:] = (np.int64(1) << 33) + 11 * k.astype(np.int64) + 1     # both halves of the id in use
    return b


PATTERNS = {
    "none-dead": (lambda n: np.ones(n, dtype=np.int32), lambda n: True),
    "all-dead": (lambda n: np.zeros(n, dtype=np.int32), lambda n: True),
    "first-and-last-dead": (lambda n: np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 0, 1).astype(np.int32), lambda n: n >= 2),
    "every-7th-dead": (lambda n: np.where(np.arange(n) % 7 == 6, 0, 1).astype(np.int32), lambda n: n >= 7),
    "run-of-70-dead": (lambda n: np.where((np.arange(n) >= n // 3) & (np.arange(n) < n // 3 + 70), 0, 1).astype(np.int32), lambda n: n > 70 + n // 3),
}
CASES = [(name, n) for name, (_, defined) in PATTERNS.items() for n in SIZES if defined(n)]


def _moved_fields(ib):
    """fp64 members the last row permutation moved (kid_perm_moved_fields, a hook for this test; not part of include/kid.h)"""
    fn = ib.lib.kid_perm_moved_fields
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_int64)], C.c_int
    c = C.c_int64(-1)
    assert fn(ib.h, C.byref(c)) == 0
    return c.value


def _assert_rows_equal(got, want, keep, label):
    for name in MEMBERS:
        assert got[name].dtype == want[name].dtype, (label, name)
        assert got[name].tobytes() == np.ascontiguousarray(want[name][keep]).tobytes(), (label, name)


@pytest.mark.parametrize("pattern,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_compaction_is_the_kept_rows_in_order(box, pattern, n):
    alive = PATTERNS[pattern][0](n)
    b = _full_soa(n, alive)
    keep = alive != 0
    kept = int(keep.sum())
    box.upload_bergs(b)
    box.compact()
    assert box.num_bergs() == (kept, kept)
    assert box.num_bergs() == (kept, kept)
    got = box.download_bergs()
    assert len(got["lon"]) == kept
    _assert_rows_equal(got, b, keep, (pattern, n))
    if kept:
        assert _moved_fields(box) == NF64          # nothing was zeros: every member moved


def test_members_uploaded_as_null_stay_zero_and_are_not_moved(box):
    n = 257
    alive = PATTERNS["every-7th-dead"][0](n)
    b = _full_soa(n, alive)
    # members no kernel of the plain namelist writes (so zeros stay zeros: the permutation may leave them), and some it does write
    skippable = ["halo_berg", "static_berg", "start_lon", "start_lat", "heat_density", "axn_fast", "rot"]
    written = ["uvel", "mass_of_bits"]
    s = box._soa(b)
    for name in skippable + written:
        s.f64[T.BERG_F64_NAMES.index(name)] = None
        b[name][:] = 0.0                            # NULL means zeros
    box._check(box.lib.kid_upload_bergs(box.h, C.byref(s)), "kid_upload_bergs")
    box.compact()
    keep = alive != 0
    assert box.num_bergs() == (int(keep.sum()),) * 2
    moved = _moved_fields(box)
    assert NF64 - len(skippable) - len(written) <= moved < NF64, "the skip rule had nothing to skip"
    got = box.download_bergs()
    _assert_rows_equal(got, b, keep, "null members")
    for name in skippable + written:
        assert not got[name].any(), name


def _scattered(n=300, seed=31):
    grid, p = _box()
    b = S.place_bergs(grid, n, seed, (4, 44), (4, 36))
    b["alive"][::9] = 0
    return grid, p, b


@pytest.mark.parametrize("eager", [False, True], ids=["pending", "eager"])
def test_compaction_after_a_rebinning(monkeypatch, eager):
    """KID_STABLE_RESORT: the order inside a cell is the upload's, so the rows can be compared as they are"""
    monkeypatch.setenv("KID_STABLE_RESORT", "1")
    if eager:
        monkeypatch.setenv("KID_REBIN_EAGER", "1")
    else:
        monkeypatch.delenv("KID_REBIN_EAGER", raising=False)
    grid, p, b = _scattered()
    d = grid["desc"]
    ib, other = Icebergs(grid, p, capacity=len(b["lon"])), Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(S.copy_bergs(b))
        ib.move_berg_between_cells()
        ib.compact()
        got = ib.download_bergs()
        # the same through a download and an upload between the two
        other.upload_bergs(S.copy_bergs(b))
        other.move_berg_between_cells()
        between = other.download_bergs()
        other.upload_bergs(between)
        other.compact()
        want = other.download_bergs()
        live = np.flatnonzero(b["alive"] != 0)
        assert len(got["lon"]) == len(want["lon"]) == len(live) < len(b["lon"])
        _assert_rows_equal(got, want, slice(None), "re-uploaded")
        # ... which are the live rows in cell order (j-major, i-minor), the upload's order inside a cell
        key = (b["ine"][live] - d.isd) + (b["jne"][live] - d.jsd) * (d.ied - d.isd + 1)
        _assert_rows_equal(got, b, live[np.argsort(key, kind="stable")], "cell order")
        # was that re-binning left pending?  This handle's next one is taken by the hot build exactly when it is not eager
        ib.move_berg_between_cells()
        ib.run(1)
        assert ib.rebin_fused_count() == (0 if eager else 1)
    finally:
        ib.close()
        other.close()


def test_compaction_is_refused_while_bond_tables_exist():
    grid, p = _box()
    b = S.place_bergs(grid, 4, 5, (4, 44), (4, 36))
    b["alive"][0] = 0                               # compaction would move rows 1 .. 3
    bd = S.empty_bonds(4, 2)
    bd["count"][1] = bd["count"][2] = 1
    bd["other_id"][1], bd["other_id"][2] = b["id"][2], b["id"][1]
    for name in T.BOND_F64_NAMES:
        bd[name][1], bd[name][2] = 0.25, -0.25
    ib = Icebergs(grid, p, capacity=8)
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(bd)
        with pytest.raises(L.KidError, match=r"rc=-5 .*bonds keep their rows"):
            ib.compact()
        assert ib.num_bergs() == (4, 3)
        got = ib.download_bergs()
        _assert_rows_equal(got, b, slice(None), "rows after the refusal")
        gd = ib.download_bonds(2)
        for name in ["count", "other_id", "broken"] + list(T.BOND_F64_NAMES):
            assert np.array_equal(gd[name], bd[name]), name
    finally:
        ib.close()


def _footloose_pass(rebin):
    """one step of config 3 up to the footloose pass, phase by phase (IB:5423-5453), then the count"""
    grid, p, b = S.config_c3(n=200, seed=3, fl_style="new_bergs")      # tests/golden/c3_new_bergs.npz is this configuration
    S.set_diag_all(p)
    n0 = b["_n"]
    dead = np.arange(5, n0, 9)
    b["alive"][dead] = 0
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        for call in ("kid_zero_accumulators", "kid_interp_gridded_fields_to_bergs", "kid_evolve_icebergs"):
            ib._check(getattr(ib.lib, call)(ib.h), call)
        if rebin:
            ib.move_berg_between_cells()                               # IB:5437: the dead go to the tail
        ib._check(ib.lib.kid_footloose_calving(ib.h), "kid_footloose_calving")   # IB:5453: children behind them
        slots, alive = ib.num_bergs()
        rows = ib.download_bergs()
        return n0, len(dead), slots, alive, rows
    finally:
        ib.close()


def test_footloose_children_behind_a_dead_tail_are_counted_and_kept():
    """The oracle's first step of this configuration appends 3 children (200 -> 203 rows); 22 of the 200 rows are dead here."""
    n0, ndead, slots_r, alive_r, rows_r = _footloose_pass(rebin=True)
    _, _, slots_p, alive_p, rows_p = _footloose_pass(rebin=False)
    assert ndead > 0, "the re-binning had no dead rows to sort to the tail"
    live_r, live_p = rows_r["alive"] != 0, rows_p["alive"] != 0
    assert slots_p > n0 and int(live_p.sum()) > n0 - ndead, "the pass appended no child"
    assert alive_r == int(live_r.sum()) and alive_p == int(live_p.sum())
    assert alive_r == alive_p == n0 - ndead + (slots_p - n0)
    assert np.array_equal(np.sort(rows_r["id"][live_r]), np.sort(rows_p["id"][live_p]))
