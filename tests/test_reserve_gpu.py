"""Growable capacity on the device (include/kid.h: kid_capacity, kid_reserve, kid_set_auto_reserve; csrc/kid_reserve.inc).

Every case runs handle A, created tight and grown, against handle B, created roomy and never grown, through the same inputs and
the same calls.  "Equal" is numpy.array_equal on every downloaded berg field and the ids -- by id where a re-binning, a pack
or an append leaves the row order to the order atomics arrive in, which no result depends on.  Planes are held to TOL_GRID of
tests/parity.py (atomics order their sums), and are equal to the bit where reproducible sums are on."""
import ctypes as C
import gc
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import framework as FW        # noqa: E402
from icebergs_amd import lib as L               # noqa: E402
from icebergs_amd import synthetic as S         # noqa: E402
from icebergs_amd import types as T             # noqa: E402
import halo_bergs as HB                         # noqa: E402
import parity as P                              # noqa: E402

pytestmark = pytest.mark.gpu

ROW_BYTES = 8 * T.ENUMS["KID_NB_F64"] + 4 * T.ENUMS["KID_NB_I32"] + 8      # one berg of the SoA
EMPTY = np.empty((0, 34))
KidError = L.KidError


def _mem():
    d = C.c_int64(-1)
    assert L.load().kid_memory_in_use(C.byref(d), None) == 0
    return d.value


def _destroy(ib):
    h, ib.h = ib.h, None
    FW._LIVE.discard(ib)
    assert L.load().kid_destroy(h) == 0, L.load().kid_last_error(None)


def _fields(b):
    return [k for k, v in b.items() if isinstance(v, np.ndarray)]


def _assert_same_rows(a, b, label):
    """row for row"""
    assert len(a["id"]) == len(b["id"]), (label, len(a["id"]), len(b["id"]))
    for k in _fields(a):
        assert np.array_equal(a[k], b[k], equal_nan=True), (label, k)


def _assert_same_bergs(a, b, label, live_only=True):
    """berg for berg, whatever rows they stand in (ids are unique)"""
    def by_id(x):
        rows = np.flatnonzero(x["alive"] != 0) if live_only else np.arange(len(x["id"]))
        assert len(np.unique(x["id"][rows])) == len(rows), label
        return rows[np.argsort(x["id"][rows], kind="stable")]
    ra, rb = by_id(a), by_id(b)
    assert len(ra) == len(rb) and len(ra) > 0, (label, len(ra), len(rb))
    for k in _fields(a):
        assert np.array_equal(a[k][ra], b[k][rb], equal_nan=True), (label, k)


def _assert_planes(a, b, label, exact=False):
    for name, x, y in (("acc", a[0], b[0]), ("out", a[1], b[1])):
        if exact:
            assert np.array_equal(x, y), (label, name)
            continue
        sc = P.acc_scales(y) if name == "acc" else np.array([np.max(np.abs(y[k])) for k in range(y.shape[0])])
        worst = max(P.acc_err(x, y, k, sc) for k in range(y.shape[0]))
        print(label, name, "worst deviation relative to the plane's scale %.3e" % worst)
        assert worst <= P.TOL_GRID, (label, name, worst)


# ---- 1. plain step -------------------------------------------------------------------------------------------------------------
N1, CAP1 = 2000, 5000
_C2 = {}


def _c2():
    if not _C2:
        _C2["case"] = S.config_c2(n=N1, seed=2)
    return _C2["case"]


def _plain_run(capacity, variant):
    """3 steps, [compaction], the reserve (a no-op on the roomy handle), 3 more steps with a re-binning among them.  One handle
    at a time, so that kid_memory_in_use -- a count over the process -- is this handle's figure."""
    grid, p, b = _c2()
    gc.collect()
    base = _mem()
    ib = FW.Icebergs(grid, p, capacity=capacity)
    try:
        if variant == "repro":
            ib.set_reproducible_sums(True)
        ib.upload_bergs(b)
        ib.set_resort_interval(0)
        ib.run(3)
        if variant == "compact":
            ib.compact()                         # the second set of arrays exists from here on
        ib.reserve(CAP1)
        mem_reserved = _mem() - base             # before anything can re-grow lazily
        cap = ib.capacity
        ib.set_resort_interval(2)
        ib.run(3)
        rebinned = ib.num_bergs()
        res = (ib.download_bergs(), tuple(x.copy() for x in ib.fetch()))
        mem_end = _mem() - base
    finally:
        _destroy(ib)
    assert _mem() == base, "kid_destroy left memory behind"
    return res, cap, mem_reserved, mem_end, rebinned


@pytest.mark.parametrize("variant", ["plain", "compact", "repro"])
def test_plain_step(variant):
    (ba, pa), cap_a, mem_a, end_a, n_a = _plain_run(N1, variant)
    (bb, pb), cap_b, mem_b, end_b, n_b = _plain_run(CAP1, variant)
    assert cap_a == CAP1 and cap_b == CAP1
    assert n_a == n_b and n_a[1] > 0
    _assert_same_bergs(ba, bb, variant)
    _assert_planes(pa, pb, variant, exact=(variant == "repro"))
    assert np.array_equal(pa[2], pb[2]) or variant != "repro"
    print(variant, "device bytes right after the reserve: grown", mem_a, "roomy", mem_b, "one SoA", CAP1 * ROW_BYTES, "; at the end", end_a, end_b)
    # a copy the reserve left behind would show here (scratch that waits for its next user leaves the grown handle below)
    assert mem_a < mem_b + CAP1 * ROW_BYTES, (mem_a, mem_b)
    assert end_a == end_b, (end_a, end_b)


# ---- 2. bonds ------------------------------------------------------------------------------------------------------------------
def test_bonds_keep_their_rows_and_tables():
    grid, p, b, bd = S.config_beam("cantilever")
    p = S.params_copy(p)
    p.dt, p.mts_sub_steps = 1.0, 20            # the test's own fast step (0.05 s), a short sub-step loop
    n, mb = len(b["lon"]), int(bd["max_bonds"])
    assert n == 90
    b0 = S.copy_bergs(b)
    b0["n_bonds"][:] = 0
    res = []
    for cap, grow in ((n, True), (4 * n, False)):
        ib = FW.Icebergs(grid, p, capacity=cap)
        try:
            ib.upload_bergs(b0)
            assert ib.initialize_bonds(from_radii=True) > 0
            ib.run(1)
            if grow:
                ib.reserve(4 * n)
            assert ib.capacity == 4 * n
            ib.run(1)
            res.append((ib.download_bergs(), ib.download_bonds(mb), ib.count_bonds()))
        finally:
            ib.close()
    (ba, ta, ca), (bb, tb, cb) = res
    _assert_same_rows(ba, bb, "beam")
    assert np.isfinite(ba["lon"]).all() and np.any(ba["lat"] != b["lat"])
    for k in ta:
        if k != "max_bonds":
            assert np.array_equal(ta[k], tb[k]), k
    assert ta["count"].sum() == 294 and np.abs(ta["length"]).max() > 0.0
    assert np.array_equal(ba["conglom_id"], bb["conglom_id"])
    assert ca == cb and ca[0] == 294 and ca[1] == 0


# ---- 3. interacting bergs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contact", [False, True])
def test_interacting_bergs_undivided(contact):
    whole, b = HB.population()
    p = HB.params(contact)
    n = len(b["lon"])
    res = []
    for cap, grow in ((n, True), (3 * n, False)):
        ib = FW.Icebergs(whole, p, capacity=cap)
        try:
            ib.upload_bergs(HB.trim(dict(b, _n=n)))
            ib.run(3)
            if grow:
                ib.reserve(3 * n)
            assert ib.capacity == 3 * n
            ib.run(3)
            res.append((ib.download_bergs(), tuple(x.copy() for x in ib.fetch())))
        finally:
            ib.close()
    _assert_same_rows(res[0][0], res[1][0], "contact box")
    _assert_planes(res[0][1], res[1][1], "contact box")


def _tiles_step(tiles, contact, between=None):
    """one step of the 2 x 2 tile set of tests/test_halo_bergs_gpu.py; `between` runs while the halo rows are resident"""
    import test_halo_bergs_gpu as HG

    def call(ib, name):
        ib._check(getattr(ib.lib, name)(ib.h), name)
    for ib in tiles.values():
        call(ib, "kid_zero_accumulators")
    HG._swap(tiles, lambda ib, axis, sides: ib.pack_halo_bergs_pair(axis, 0, sides), lambda ib, axis, lo, hi: ib.unpack_immigrants_pair(lo, hi))
    if between:
        between()
    for ib in tiles.values():
        if contact:
            ib.set_conglom_ids()
        call(ib, "kid_evolve_icebergs")
    HG._swap(tiles, lambda ib, axis, sides: ib.pack_emigrants_pair(axis), lambda ib, axis, lo, hi: ib.unpack_immigrants_pair(lo, hi))
    for ib in tiles.values():
        call(ib, "kid_thermodynamics")
        call(ib, "kid_calculate_mass_on_ocean")

    def pack_planes(ib, axis, sides):
        count = ib.halo_buffer_count(axis)
        return ib.pack_halo_pair(axis, out=tuple(np.empty(count) if s else None for s in sides))
    HG._swap(tiles, pack_planes, lambda ib, axis, lo, hi: ib.unpack_halo_pair(axis, lo if lo is not HG.EMPTY else None, hi if hi is not HG.EMPTY else None))
    for ib in tiles.values():
        call(ib, "kid_step_gather")


def test_tile_grows_while_halo_rows_are_resident():
    import test_halo_bergs_gpu as HG
    whole, b = HB.population()
    p = HB.params(True)
    res = []
    for grow in (True, False):
        tiles = {}
        try:
            for tx in range(HB.NTX):
                for ty in range(HB.NTY):
                    ib = FW.Icebergs(HB.tile_grid(tx, ty, whole), p, capacity=400)
                    ib.upload_bergs(HB.trim(HB.split_bergs(b, tx, ty, 400)))
                    tiles[(tx, ty)] = ib
            first = tiles[(0, 0)]

            def reserve():
                assert first.halo_berg_count() > 0
                before = first.download_bergs()
                first.reserve(900)
                assert first.capacity == 900 and first.halo_berg_count() > 0
                _assert_same_rows(before, first.download_bergs(), "tile (0, 0) across the reserve")
            _tiles_step(tiles, True)
            _tiles_step(tiles, True, reserve if grow else None)
            _tiles_step(tiles, True)
            for ib in tiles.values():
                assert ib.halo_berg_count() == 0 and ib.fetch()[2][T.ENUMS["KID_S_ERROR_COUNT"]] == 0.0
            res.append({k: (HG._live(ib.download_bergs()), ib.fetch()[1].copy()) for k, ib in tiles.items()})
        finally:
            for ib in tiles.values():
                ib.close()
    for k in res[0]:
        (ga, oa), (gb, ob) = res[0][k], res[1][k]
        ra, rb = np.argsort(ga["id"], kind="stable"), np.argsort(gb["id"], kind="stable")
        assert len(ra) == len(rb) and len(ra) > 0
        for f in ga:
            assert np.array_equal(ga[f][ra], gb[f][rb]), (k, f)
        sc = np.array([np.max(np.abs(ob[q])) for q in range(ob.shape[0])])
        assert max(P.acc_err(oa, ob, q, sc) for q in range(ob.shape[0])) <= P.TOL_GRID, k


# ---- 4. calving ----------------------------------------------------------------------------------------------------------------
def test_calving_grows_between_its_two_passes():
    import test_calving as TC
    grid, p, cp, b = TC._setup(n=100)
    calv, hflx = S.coupler_calving(grid, seed=1, frac=0.05, buckets=4.0)
    n = len(b["lon"])
    res = []
    for cap, auto in ((n, True), (20000, False)):
        ib = FW.Icebergs(grid, p, capacity=cap)           # the tight one has zero free rows
        try:
            ib.set_forcing(grid["forcing"])
            ib.set_calving_params(cp)
            ib.upload_bergs(b)
            if auto:
                ib.set_auto_reserve(0, 1.5)
            scal = ib.calving(calv, hflx)
            res.append((ib.download_bergs(), scal, ib.get_calving_state(), ib.capacity, ib.get_iceberg_counter()))
        finally:
            ib.close()
    (ba, sa, sta, cap_a, cnt_a), (bb, sb, stb, cap_b, cnt_b) = res
    born = len(bb["id"]) - n
    assert born > 200 and cap_b == 20000
    assert cap_a == max(n + born, int(np.ceil(n * 1.5)))            # the growth rule, need above capacity * growth
    _assert_same_rows({k: ba[k][:n] for k in _fields(ba)}, {k: bb[k][:n] for k in _fields(bb)}, "resident bergs")
    _assert_same_bergs(ba, bb, "calved bergs")
    assert np.array_equal(sa, sb) and np.array_equal(cnt_a, cnt_b)
    TC._compare_state(stb, sta, "calving state")
    # off: as ever
    ib = FW.Icebergs(grid, p, capacity=n)
    try:
        ib.set_forcing(grid["forcing"])
        ib.set_calving_params(cp)
        ib.upload_bergs(b)
        with pytest.raises(KidError, match=r"rc=-4 calving ran out of capacity: create the handle with room for new bergs$"):
            ib.calving(calv, hflx)
        assert ib.capacity == n
    finally:
        ib.close()


# ---- 5. footloose --------------------------------------------------------------------------------------------------------------
N5, STEPS5 = 2000, 5
_C3 = {}


def _c3():
    """config 3 small: 2000 parents whose fl_k starts within a foot of the threshold, so that children appear from the first step"""
    if not _C3:
        grid, p, b = S.config_c3(n=N5, seed=3, fl_style="new_bergs", capacity_factor=3)
        _C3["case"] = (grid, p, b)
    return _C3["case"]


def _fl_roomy(mode):
    if mode not in _C3:
        grid, p, b = _c3()
        ib = FW.Icebergs(grid, p, capacity=len(b["lon"]))
        try:
            ib.upload_bergs(b)
            slots = [ib.num_bergs()[0]]
            for _ in range(STEPS5):
                ib.run(1) if mode == "run_step" else ib.run_phases(1)
                slots.append(ib.num_bergs()[0])
            _C3[mode] = (ib.download_bergs(), np.diff(slots), ib.capacity)
        finally:
            ib.close()
    return _C3[mode]


@pytest.mark.parametrize("mode", ["run_step", "phases"])
def test_footloose_children_find_room(mode):
    grid, p, b = _c3()
    want, children, cap_b = _fl_roomy(mode)
    print(mode, "children per step", children)
    assert children[0] > 1 and children.sum() > 20 and cap_b == len(b["lon"])
    busiest = int(children.max())
    ib = FW.Icebergs(grid, p, capacity=N5)
    try:
        ib.upload_bergs(b)
        ib.set_auto_reserve(busiest, 1.0)                  # growth = 1: every step grows to exactly n + min_free
        for s in range(STEPS5):
            ib.run(1) if mode == "run_step" else ib.run_phases(1)
            assert ib.capacity == N5 + int(children[:s].sum()) + busiest
        got = ib.download_bergs()
    finally:
        ib.close()
    _assert_same_bergs(got, want, mode)
    assert len(got["id"]) == N5 + children.sum()


def test_footloose_overflow_names_the_attempt():
    grid, p, b = _c3()
    _, children, _ = _fl_roomy("run_step")
    ib = FW.Icebergs(grid, p, capacity=N5)
    try:
        ib.upload_bergs(b)
        ib.set_auto_reserve(1, 1.0)
        with pytest.raises(KidError, match=r"rc=-4 footloose calving ran out of capacity: create the handle with room for child bergs \(the launch tried to append (\d+) rows, 1 were free") as e:
            ib.run(1)
        assert int(re.search(r"tried to append (\d+) rows", str(e.value)).group(1)) == int(children[0])
        assert ib.capacity == N5 + 1
        got = ib.download_bergs()                           # the parents are still there
        assert len(got["id"]) == N5 + 1
        assert np.array_equal(got["id"][:N5], b["id"][:N5]) and np.all(got["alive"][:N5] == 1) and np.all(np.isfinite(got["lon"][:N5]))
    finally:
        ib.close()


# ---- 6. immigrants -------------------------------------------------------------------------------------------------------------
def _immigrants(count=300):
    """`count` records as the western tile of a 2 x 2 box packs them for its eastern neighbour"""
    import test_migration as TM
    g0 = TM._grid(0, 0, 2, 2)
    p = S.default_params()
    b = S.place_bergs(g0, count, 11, (3, TM.NI - 2), (3, TM.NJ - 2))
    rng = np.random.default_rng(12)
    edge = g0["static"]["lon"][S.HALO + 2, TM.NI + S.HALO - 1]
    b["ine"][:] = TM.NI + 1
    b["lon"][:] = edge + rng.uniform(0.1, 0.9, count) * TM.DL
    b["id"][:] = (np.int64(9) << 32) | (50000 + np.arange(count, dtype=np.int64))
    src = FW.Icebergs(g0, p, capacity=count)
    try:
        src.upload_bergs(b)
        recs = src.pack_emigrants(TM.E)
    finally:
        src.close()
    assert recs.shape == (count, 34)
    return TM, p, recs


def _full_east_tile(TM, p, n_own=60):
    """the eastern tile, full to the last row; its last berg has left through the east and waits, a dead row, to be packed"""
    g1 = TM._grid(1, 0, 2, 2)
    own = S.place_bergs(g1, n_own, 13, (3, TM.NI - 2), (3, TM.NJ - 2))
    own["ine"][-1] = TM.NI + 1
    own["alive"][-1] = 0
    ib = FW.Icebergs(g1, p, capacity=n_own)
    ib.upload_bergs(own)
    return ib, own


def test_immigrants_find_room_and_a_waiting_leaver_survives():
    TM, p, recs = _immigrants()
    ib, own = _full_east_tile(TM, p)
    n_own = len(own["id"])
    try:
        ib.set_auto_reserve(0, 1.5)
        ib.unpack_immigrants(recs)
        assert ib.capacity == n_own + len(recs)            # need above capacity * growth; the compaction found nothing to drop
        assert ib.num_bergs() == (n_own + len(recs), n_own - 1 + len(recs))
        got = ib.download_bergs()
        assert np.array_equal(np.sort(got["id"][n_own:]), np.sort(HB.record_ids(recs))) and np.all(got["alive"][n_own:] == 1)
        assert np.all(got["ine"][n_own:] == 1)
        for k in _fields(own):
            if k not in ("lon_old", "lat_old", "uvel_old", "vvel_old"):
                assert np.array_equal(got[k][:n_own], own[k]), k
        gone = ib.pack_emigrants(TM.E)                     # the leaver was carried through the compaction and the growth
        assert len(gone) == 1 and HB.record_ids(gone)[0] == own["id"][-1]
    finally:
        ib.close()


def test_immigrants_beyond_max_capacity_write_nothing():
    TM, p, recs = _immigrants()
    ib, own = _full_east_tile(TM, p)
    n_own = len(own["id"])
    try:
        ib.set_auto_reserve(0, 1.5, max_capacity=n_own + 100)
        before = ib.download_bergs()
        with pytest.raises(KidError, match=r"rc=-4 kid_unpack_immigrants: %d rows are needed.* %d; nothing was written" % (n_own + len(recs), n_own + 100)):
            ib.unpack_immigrants(recs)
        assert ib.capacity == n_own and ib.num_bergs() == (n_own, n_own - 1)
        _assert_same_rows(before, ib.download_bergs(), "after the refusal")
    finally:
        ib.close()


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------
def test_arguments():
    grid, p, b = S.config_c1()
    ib = FW.Icebergs(grid, p, capacity=64)
    try:
        ib.upload_bergs(b)
        mem = _mem()
        for rows in (64, 10, 0, -5):
            ib.reserve(rows)                               # no-ops
            assert ib.capacity == 64 and _mem() == mem
        for call in (lambda: ib.reserve((1 << 29) + 1), lambda: ib.set_auto_reserve(0, 0.5), lambda: ib.set_auto_reserve(0, 0.999),
                     lambda: ib.set_auto_reserve(-1, 1.5), lambda: ib.set_auto_reserve(0, 1.5, max_capacity=-1),
                     lambda: ib.set_auto_reserve(0, 1.5, max_capacity=(1 << 29) + 1)):
            with pytest.raises(KidError, match="rc=-1 "):
                call()
        assert ib.capacity == 64 and _mem() == mem
        ib.set_auto_reserve(0, 1.0)
        ib.set_auto_reserve(3, 2.0, max_capacity=1 << 29)
        ib.set_auto_reserve(0, 0.0)                        # off again
        big = S.empty_bergs(65)
        for k in _fields(b):
            big[k][:] = np.resize(b[k], 65)
        with pytest.raises(KidError, match=r"rc=-4 more bergs than capacity$"):
            ib.upload_bergs(big)
        ib.set_auto_reserve(0, 1.5)
        ib.upload_bergs(big)                               # kid_upload_bergs grows when host->n is above the capacity
        assert ib.capacity == 96 and ib.num_bergs()[0] == 65
        ib.reserve(97)
        assert ib.capacity == 97 and _mem() > mem
    finally:
        ib.close()
