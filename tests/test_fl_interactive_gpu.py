"""Footloose calving among interacting bergs on the device (csrc/kid_fl_interact.inc, kid_adjust_fl_berg_interactivity):
kid_run_step against the step composed from the oracle's phases (tests/fl_interactive.py) for both contact searches and both
interpolation orders, the phase entry points against the step, the control without the promotion pass, the call on its own
against its numpy restatement, capacity, and the refusals that stay."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import fl_interactive as FI               # noqa: E402
import halo_bergs as HB                   # noqa: E402
import parity as P                        # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, EUNSUPPORTED = -1, -4, -5
SEARCHES = [pytest.param(False, id="3x3"), pytest.param(True, id="contact")]
ALL_FIELDS = tuple(T.BERG_F64_NAMES) + tuple(T.BERG_I32_NAMES) + ("id",)


def _icebergs(grid, p, cap=FI.CAP):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)


def _loaded(contact, old_order=False, cap=FI.CAP, fl_bits=False):
    grid, b = FI.population(contact)
    p = FI.params(contact, old_order, fl_bits)
    ib = _icebergs(grid, p, cap)
    ib.upload_bergs(b)
    return ib, p


def _snapshot(ib):
    acc, out, scal = ib.fetch()
    return ib.download_bergs(), acc.copy(), out.copy(), scal.copy()


def _phase_step(ib, p, promote=True):
    """icebergs_run (IB:5423-5512) through the phase entry points; returns what kid_adjust_fl_berg_interactivity counted"""
    lib, h, ck = ib.lib, ib.h, ib._check
    ck(lib.kid_zero_accumulators(h), "kid_zero_accumulators")
    if not p.old_interp_flds_order:
        ck(lib.kid_interp_gridded_fields_to_bergs(h), "interp")                      # IB:5423
    ck(lib.kid_evolve_icebergs(h), "kid_evolve_icebergs")                            # IB:5433
    ck(lib.kid_footloose_calving(h), "kid_footloose_calving")                        # IB:5453
    if FI.is_contact(p):
        ib.set_conglom_ids()                                                         # IB:5470
    if not p.old_interp_flds_order:
        ck(lib.kid_interp_gridded_fields_to_bergs(h), "interp")                      # IB:5473
    count = ib.adjust_fl_berg_interactivity() if promote else 0                      # IB:5486
    ck(lib.kid_thermodynamics(h), "kid_thermodynamics")                              # IB:5505
    ck(lib.kid_create_gridded_icebergs_fields(h), "kid_create_gridded")              # IB:5512
    return count


def _phase_run(contact, steps, promote=True):
    ib, p = _loaded(contact)
    try:
        if contact:
            ib.set_conglom_ids()                                                     # the `Visited` block, IB:5415-5416
        counts = [_phase_step(ib, p, promote) for _ in range(steps)]
        return _snapshot(ib), counts, p
    finally:
        ib.close()


_NO_PROMOTION = {}


def _without_promotion(contact):
    """20 steps through the phase entry points without the promotion call, once per search"""
    if contact not in _NO_PROMOTION:
        _NO_PROMOTION[contact] = _phase_run(contact, 20, promote=False)
    return _NO_PROMOTION[contact]


def _same_fl_sets(ref_b, got_b, label):
    for name, want, got in zip(("live", "fl_k = -1", "fl_k = -2"), FI.fl_sets(ref_b), FI.fl_sets(got_b)):
        assert np.array_equal(want, got), "%s: the %s ids differ (%d against %d)" % (label, name, len(want), len(got))


# ---- the namelist is accepted ----
def test_combination_is_accepted():
    """footloose with interactive_icebergs_on was KID_EUNSUPPORTED (rc=-5) from kid_create"""
    for contact in (False, True):
        for old in (False, True):
            _icebergs(FI.grid(), FI.params(contact, old)).close()


# ---- parity ----
@pytest.mark.parametrize("contact,old_order,fl_bits", [pytest.param(False, False, False, id="3x3"), pytest.param(True, False, False, id="contact"),
                                                       pytest.param(False, True, False, id="3x3-old_interp_flds_order"),
                                                       pytest.param(True, False, True, id="contact-fl_bits")])
def test_run_step_against_the_composed_oracle(contact, old_order, fl_bits):
    """fl_bits: the other fl_style, where a child is made from its parent's footloose bits (and takes a share of their bergy bits)"""
    snaps, _, st, _, _ = FI.composed_run(contact, old_order, fl_bits=fl_bits)
    assert st["children"] >= 100 and st["promotions"] >= (10 if fl_bits else 20) and min(st["held_back"]) >= 1 and st["margin"] >= FI.MARGIN
    ib, p = _loaded(contact, old_order, fl_bits=fl_bits)
    try:
        done = 0
        for step in FI.CHECK_AT:
            ib.run(step - done)
            done = step
            got = _snapshot(ib)
            label = "%s%s%s step %d" % ("contact" if contact else "3x3", " old order" if old_order else "", " fl_bits" if fl_bits else "", step)
            _same_fl_sets(snaps[step][0], got[0], label)
            rep = P.compare(snaps[step], got, label, params=p)
            print("%s: trajectories %.2e sizes %.2e planes %.2e (%d live, %d at -1, %d at -2)" % (
                label, max(rep[f] for f in P.TRAJ_FIELDS), max(rep[f] for f in P.SIZE_FIELDS),
                max(v for k, v in rep.items() if k.startswith(("acc", "out"))), *(len(x) for x in FI.fl_sets(got[0]))))
    finally:
        ib.close()


# ---- the phase entry points ----
@pytest.mark.parametrize("contact", SEARCHES)
def test_phases_equal_the_step(contact):
    _, _, st, _, _ = FI.composed_run(contact)
    phases, counts, p = _phase_run(contact, 5)
    assert counts == [len(st["promoted_ids"][s]) for s in range(1, 6)], "kid_adjust_fl_berg_interactivity counts what the oracle promotes"
    ib, _ = _loaded(contact)
    try:
        ib.run(5)
        fused = _snapshot(ib)
    finally:
        ib.close()
    def by_id(b):          # (the children of one pass take their rows in the order their lanes got there)
        live = np.nonzero(b["alive"] != 0)[0]
        return live[np.argsort(b["id"][live])]
    ra, rb = by_id(fused[0]), by_id(phases[0])
    assert np.array_equal(fused[0]["id"][ra], phases[0]["id"][rb])
    for f in P.TRAJ_FIELDS + P.SIZE_FIELDS:
        assert P.rel_err(phases[0][f][rb], fused[0][f][ra]) <= 1e-12, f
    for k in range(fused[1].shape[0]):
        assert P.rel_err(phases[1][k], fused[1][k]) <= 1e-12, k
    for k in range(fused[2].shape[0]):
        assert P.rel_err(phases[2][k], fused[2][k]) <= 1e-12, k


@pytest.mark.parametrize("contact", SEARCHES)
def test_control_without_the_promotion_pass(contact):
    """the same phase sequence without the call: nobody is ever promoted, and the run is not the oracle's"""
    snaps, _, _, _, _ = FI.composed_run(contact)
    got, _, p = _without_promotion(contact)
    live, waiting, promoted = FI.fl_sets(got[0])
    assert len(waiting) >= 50 and len(promoted) == 0
    assert len(FI.fl_sets(snaps[20][0])[2]) >= 10
    with pytest.raises(AssertionError):
        P.compare(snaps[20], got, "control", params=p)


# ---- the call on its own ----
@pytest.mark.parametrize("contact", SEARCHES)
def test_the_call_on_its_own(contact):
    """a step-20 state in which nobody has been promoted yet, uploaded into a fresh handle: one call changes fl_k of exactly the
    rows the numpy pass changes and nothing else, a second call changes nothing, and with footloose = 0 nothing happens"""
    state = _without_promotion(contact)[0][0]
    n = len(state["lon"])
    grid, p = FI.grid(), FI.params(contact)
    want = S.copy_bergs(state)
    rows = FI.np_adjust(p, grid["desc"], want, n)
    assert len(rows) >= 10 and len(rows) < int((state["fl_k"] == -1.0).sum()), "some children are promoted, some keep waiting"
    ib = _icebergs(grid, p)
    try:
        ib.upload_bergs(state)
        assert ib.adjust_fl_berg_interactivity() == len(rows)
        got = ib.download_bergs()
        assert np.array_equal(np.nonzero(got["fl_k"] != state["fl_k"])[0], np.array(rows))
        for f in ALL_FIELDS:
            assert np.array_equal(got[f], want[f]), f
        assert ib.adjust_fl_berg_interactivity() == 0
        again = ib.download_bergs()
        for f in ALL_FIELDS:
            assert np.array_equal(again[f], got[f]), f
        # promoted = NULL: the same pass, nothing read back
        ib.upload_bergs(state)
        assert ib.lib.kid_adjust_fl_berg_interactivity(ib.h, None) == 0
        assert np.array_equal(ib.download_bergs()["fl_k"], want["fl_k"])
    finally:
        ib.close()
    q = FI.params(contact)
    q.footloose = 0
    ib = _icebergs(grid, q)
    try:
        ib.upload_bergs(state)
        assert ib.adjust_fl_berg_interactivity() == 0
        same = ib.download_bergs()
        for f in ALL_FIELDS:
            assert np.array_equal(same[f], state[f]), f
    finally:
        ib.close()


@pytest.mark.parametrize("contact", SEARCHES)
def test_the_call_on_a_latlon_grid(contact):
    """the box's discs on a lat-lon patch at 70 S (FI.latlon_state, single tile): the pass measures pairs in metres with cos of
    their mean latitude (IB:2816-2822) and promotes exactly the rows np_adjust's grid_is_latlon branch promotes -- no decision of
    which is closer to its threshold than MARGIN -- and changes nothing else"""
    grid, p, state = FI.latlon_state(contact)
    n = len(state["lon"])
    want, margins = S.copy_bergs(state), []
    rows = FI.np_adjust(p, grid["desc"], want, n, margins)
    assert grid["desc"].grid_is_latlon == 1 and min(margins) >= FI.MARGIN
    assert 3 <= len(rows) < int((state["fl_k"] == -1.0).sum()), "some children are promoted, some keep waiting"
    ib = _icebergs(grid, p, n)
    try:
        ib.upload_bergs(state)
        assert ib.adjust_fl_berg_interactivity() == len(rows)
        got = ib.download_bergs()
        assert np.array_equal(np.nonzero(got["fl_k"] != state["fl_k"])[0], np.array(rows))
        for f in ALL_FIELDS:
            assert np.array_equal(got[f], want[f]), f
        assert ib.adjust_fl_berg_interactivity() == 0
    finally:
        ib.close()


def test_refused_while_halo_rows_are_resident():
    """tile (0, 0) of the box holds copies of its east neighbour's bergs: KID_EINVAL by name, whatever the namelist says of footloose"""
    whole, b = HB.population()
    p = HB.params(False)
    west = _icebergs(HB.tile_grid(0, 0, whole), p, 400)
    east = _icebergs(HB.tile_grid(1, 0, whole), p, 400)
    try:
        west.upload_bergs(HB.trim(HB.split_bergs(b, 0, 0, 400)))
        east.upload_bergs(HB.trim(HB.split_bergs(b, 1, 0, 400)))
        _, to_west = east.pack_halo_bergs_pair(0, 0, (False, True))
        west.unpack_immigrants_pair(np.empty((0, 34)), to_west)
        assert west.halo_berg_count() == len(to_west) > 0
        n = C.c_int64(-1)
        for q in (p, FI.params(False, old_order=True)):
            west.set_params(q)
            assert west.lib.kid_adjust_fl_berg_interactivity(west.h, C.byref(n)) == EINVAL
            msg = west.lib.kid_last_error(west.h)
            assert b"kid_adjust_fl_berg_interactivity" in msg and b"halo rows" in msg, msg
            assert n.value == 0
    finally:
        west.close()
        east.close()


# ---- capacity ----
def test_capacity():
    """room for ten children where the first calving step makes more: KID_ECAPACITY with the footloose message, and the population
    the handle had is still there to download"""
    _, _, st, _, _ = FI.composed_run(False)
    from icebergs_amd.lib import KidError
    grid, b = FI.population(False)
    n = b["_n"]
    assert st["held_back"][0] > 10
    ib, p = _loaded(False, cap=n + 10)
    try:
        with pytest.raises(KidError, match="rc=-4 footloose calving ran out of capacity"):
            ib.run(1)
        got = ib.download_bergs()
        assert len(got["id"]) == n + 10
        assert np.array_equal(got["id"][:n], b["id"][:n]) and np.all(got["alive"][:n] == 1)
        assert np.all(np.isfinite(got["lon"][:n])) and np.all(got["fl_k"][:n] >= 0.0)
    finally:
        ib.close()


# ---- refusals that stay ----
def test_refusals_that_stay():
    from icebergs_amd.lib import KidError
    grid = FI.grid()
    p = FI.params(False)
    p.iceberg_bonds_on, p.max_bonds = 1, 4
    with pytest.raises(KidError, match="rc=-5 .*bonded footloose calving"):
        _icebergs(grid, p)
    p = FI.params(False)
    p.mts, p.mts_sub_steps, p.max_bonds = 1, 4, 4
    with pytest.raises(KidError, match="rc=-5 .*footloose together with mts"):
        _icebergs(grid, p)
    ib, p = _loaded(False)
    try:
        q = FI.params(False)
        q.iceberg_bonds_on, q.max_bonds = 1, 4
        assert ib.lib.kid_set_params(ib.h, C.byref(q)) == EUNSUPPORTED
        assert b"bonded footloose calving" in ib.lib.kid_last_error(ib.h)
        n_hi, n_lo = C.c_int64(), C.c_int64()
        a, c = np.full((64, 34), -7.0), np.full((64, 34), -7.0)
        dp = C.POINTER(C.c_double)
        assert ib.lib.kid_pack_halo_bergs_pair(ib.h, 0, 0, a.ctypes.data_as(dp), 64, C.byref(n_hi), c.ctypes.data_as(dp), 64, C.byref(n_lo)) == EUNSUPPORTED
        msg = ib.lib.kid_last_error(ib.h)
        assert b"footloose" in msg and b"kid_pack_halo_bergs_pair" in msg, msg
        assert np.all(a == -7.0) and np.all(c == -7.0)
    finally:
        ib.close()
