"""Interacting bergs under RK4 on the device (sts_ia_rk4_kernel, sts_ia_rk4_old_kernel of csrc/kid_mts.inc):
kid_run_step against the step composed from the oracle's phases around the checker (tests/rk_interactive.py) on the box for both
contact searches and both interpolation orders, on the bonded collision test and above 89 N; row counts around the block size with
dead, static and fl_k = -1 rows; the phase entry points against the step; the order of the rows; and the refusals that stay."""
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
import halo_bergs as HB                   # noqa: E402
import parity as P                        # noqa: E402
import rk_interactive as RK               # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -5
SEARCHES = [pytest.param(False, id="3x3"), pytest.param(True, id="contact")]
ALL_FIELDS = tuple(T.BERG_F64_NAMES) + tuple(T.BERG_I32_NAMES) + ("id",)
OLD_FIELDS = ("lon_old", "lat_old", "uvel_old", "vvel_old")


def _icebergs(grid, p, cap):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)


def _loaded(case):
    grid, p, b, bonds, _ = case
    ib = _icebergs(grid, p, max(len(b["lon"]), 1))
    ib.upload_bergs(b)
    if bonds is not None:
        ib.upload_bonds(bonds)
    return ib


def _snapshot(ib):
    acc, out, scal = ib.fetch()
    return ib.download_bergs(), acc.copy(), out.copy(), scal.copy()


ACCEL_FIELDS = ("axn", "ayn", "bxn", "byn")


def accel_tolerance(p, rb):
    """What holding positions and velocities to TOL_TRAJ leaves for an acceleration.  A pair force is spring_coef (crit_dist - r) plus,
    with critical_interaction_damping_on, 2 sqrt(spring_coef) times a velocity difference (IB:611-804): r is a difference of
    positions that agree to TOL_TRAJ max|lon|, the velocities agree to TOL_TRAJ max|uvel|, so ONE pair's acceleration agrees to
    TOL_TRAJ (spring_coef max|lon| + 2 sqrt(spring_coef) max|uvel|) and no better -- the reasoning of parity.mts_tolerances for the
    DEM springs.  Relative to the field's maximum, taken from the checker's state; never below TOL_TRAJ."""
    k = max(p.spring_coef, p.contact_spring_coef)
    damp = 2.0 * np.sqrt(k) if p.critical_interaction_damping_on else max(p.radial_damping_coef, p.tangental_damping_coef)
    live = rb["alive"] != 0
    amax = max(float(np.abs(rb[f][live]).max()) for f in ACCEL_FIELDS)
    absolute = P.TOL_TRAJ * (k * float(np.abs(rb["lon"][live]).max()) + damp * float(np.abs(rb["uvel"][live]).max()))
    return max(P.TOL_TRAJ, absolute / amax) if amax > 0.0 else P.TOL_TRAJ


def _compare(ref, got, label, p, accel_tol=None):
    """tests/parity.py::compare (1e-10 trajectories and sizes, 1e-9 planes; live ids, ine, jne, error_count and nspeeding_tickets
    identical), conglom_id identical, and the *_old members the second sweep writes held to the trajectories' tolerance.
    accel_tol: axn .. byn are held to it here, and compare sees the checker's values in their place."""
    rb, gb = ref[0], got[0]
    ra, ga = np.nonzero(rb["alive"] != 0)[0], np.nonzero(gb["alive"] != 0)[0]
    ra, ga = ra[np.argsort(rb["id"][ra], kind="stable")], ga[np.argsort(gb["id"][ga], kind="stable")]
    assert np.array_equal(rb["id"][ra], gb["id"][ga]), label + ": set of surviving bergs differs"
    for f in tuple(P.TRAJ_FIELDS) + OLD_FIELDS:                 # every figure before anything is asserted
        print("%s: %s %.3e" % (label, f, P.rel_err(gb[f][ga], rb[f][ra])))
    accel = {}
    if accel_tol is not None:
        gb = S.copy_bergs(gb)
        for f in ACCEL_FIELDS:
            accel[f] = P.rel_err(gb[f][ga], rb[f][ra])
            assert accel[f] <= accel_tol, "%s: %s rel err %.3e > %.3e" % (label, f, accel[f], accel_tol)
            gb[f][ga] = rb[f][ra]
        got = (gb,) + tuple(got[1:])
    rep = P.compare(ref, got, label, params=p)
    rep.update(accel)
    assert np.array_equal(rb["conglom_id"][ra], gb["conglom_id"][ga]), label + ": conglom_id differs"
    for f in OLD_FIELDS:
        rep[f] = P.rel_err(gb[f][ga], rb[f][ra])
        assert rep[f] <= P.TOL_TRAJ, "%s: %s rel err %.3e" % (label, f, rep[f])
    print("%s: trajectories %.2e old %.2e sizes %.2e planes %.2e (%d live)" % (
        label, max(rep[f] for f in P.TRAJ_FIELDS), max(rep[f] for f in OLD_FIELDS), max(rep[f] for f in P.SIZE_FIELDS),
        max(v for k, v in rep.items() if k.startswith(("acc", "out"))), len(ga)))
    return rep


# ---- the handle exists ----
def test_the_handle_exists_and_steps():
    """RK4 with interactive_icebergs_on was KID_EUNSUPPORTED (rc=-5) from kid_create"""
    for contact in (False, True):
        for old in (True, False):
            case = RK.box(contact, old_order=old)
            ib = _loaded(case)
            try:
                ib.run(1)
                got = ib.download_bergs()
                assert np.isfinite(got["uvel"]).all() and not np.array_equal(got["lon"], case[2]["lon"])
                assert np.array_equal(got["lon_old"], got["lon"]) and np.array_equal(got["uvel_old"], got["uvel"])
            finally:
                ib.close()
    grid, p, b, bonds, _ = RK.collision()
    _loaded((grid, p, b, bonds, 1)).close()


# ---- parity ----
@pytest.mark.parametrize("contact,old_order", [pytest.param(False, True, id="3x3"), pytest.param(True, True, id="contact"),
                                               pytest.param(False, False, id="3x3-stored_environment")])
def test_box_against_the_composed_checker(contact, old_order):
    snaps, st = RK.box_run(contact, old_order)
    assert st["pairs"] > 0 and st["cell_changes"] > 0 and st["finite"]
    case = RK.box(contact, old_order)
    ib = _loaded(case)
    try:
        done = 0
        for step in RK.CHECK_AT:
            ib.run(step - done)
            done = step
            _compare(snaps[step], _snapshot(ib), "box %s%s step %d" % ("contact" if contact else "3x3", "" if old_order else " stored environment", step), case[1])
    finally:
        ib.close()


def test_collision_against_the_composed_checker():
    """(b) after its COLLISION_STEPS steps: the conglomerates have met (tests/test_rk_interactive_cpu.py holds the step count).

    Positions, velocities, sizes and planes are held to the standing tolerances.  The accelerations are not: bxn came out at
    1.2e-10 of its maximum against TOL_TRAJ = 1e-10 (lon, lat, uvel, vvel inside it), after 550 steps of sixteen elements that sit
    at their bonds' rest length and, for 43 steps, in contact.  They are held to accel_tolerance() instead, 5.8e-8 here
    (spring_coef 1e-5 s-2, max|lon| 1.02e4 m, critical damping 6.3e-3 s-1, max|uvel| 0.22 m/s, max|bxn| 1.8e-4 m/s2): what a
    position and a velocity that agree to TOL_TRAJ leave for one pair's force."""
    snaps, st = RK.collision_run()
    assert st["contact_steps"][-1] >= 20 and st["finite"]
    case = RK.collision()
    ib = _loaded(case)
    try:
        ib.run(RK.COLLISION_STEPS)
        tol = accel_tolerance(case[1], snaps[RK.COLLISION_STEPS][0])
        print("collision: accelerations held to %.3e" % tol)
        assert P.TOL_TRAJ <= tol <= 1.0e-6
        _compare(snaps[RK.COLLISION_STEPS], _snapshot(ib), "collision step %d" % RK.COLLISION_STEPS, case[1], accel_tol=tol)
    finally:
        ib.close()


def test_polar_against_the_composed_checker():
    """(c): elements above 89 N step on the tangent plane, their partners below it do not"""
    snaps, st = RK.polar_run()
    assert st["tangent_steps"] > 0 and st["pairs"] > 0 and st["finite"]
    case = RK.polar()
    ib = _loaded(case)
    try:
        ib.run(RK.POLAR_STEPS)
        _compare(snaps[RK.POLAR_STEPS], _snapshot(ib), "polar step %d" % RK.POLAR_STEPS, case[1])
    finally:
        ib.close()


# ---- shapes ----
@pytest.mark.parametrize("n", RK.SHAPES)
def test_shapes(n):
    """n rows, one step: the live rows against the checker.  Dead rows come back bit for bit as uploaded.  A static row is melted and
    spread like any other (the thermodynamics rounds its mass its own way, within the sizes' tolerance), so after the STEP it is
    held bit for bit in what an evolve could write; after kid_evolve_icebergs ALONE, on a handle of its own, dead and static rows
    are as uploaded in every field.  The second sweep writes nothing to a static row: its *_old members, poisoned before the
    upload, are still the poison.  The row with fl_k = -1 keeps its fl_k and is stepped like the checker's."""
    grid, p, b, _, _ = RK.shapes(n)
    b = S.copy_bergs(b)
    static = np.nonzero(b["static_berg"] >= 0.5)[0]
    for f in OLD_FIELDS:
        b[f][static] = -12345.0
    c = RK.Composed(grid, p, S.copy_bergs(b))
    RK.checker().tko_set_traversal(0, 0)
    c.step()
    ib = _loaded((grid, p, b, None, 1))
    try:
        ib.run(1)
        got = _snapshot(ib)
    finally:
        ib.close()
    ib = _loaded((grid, p, b, None, 1))
    try:
        ib._check(ib.lib.kid_evolve_icebergs(ib.h), "kid_evolve_icebergs")
        evolved = ib.download_bergs()
    finally:
        ib.close()
    _compare(c.snapshot(), got, "shapes n=%d" % n, p)
    gb = got[0]
    dead = np.nonzero(b["alive"] == 0)[0]
    moved = tuple(P.TRAJ_FIELDS) + OLD_FIELDS + ("uvel_prev", "vvel_prev", "ine", "jne", "alive", "static_berg", "halo_berg", "fl_k", "id")
    for state in (gb, evolved):
        assert len(state["lon"]) == n and np.array_equal(state["id"], b["id"]), "the rows stay where they were uploaded"
        for f in OLD_FIELDS:
            assert np.all(state[f][static] == -12345.0), f
    for f in ALL_FIELDS:
        assert np.array_equal(gb[f][dead], b[f][dead]), "dead rows after the step: " + f
        assert np.array_equal(evolved[f][dead], b[f][dead]), "dead rows after the evolve: " + f
        assert np.array_equal(evolved[f][static], b[f][static]), "static row after the evolve: " + f
        if f in moved:
            assert np.array_equal(gb[f][static], b[f][static]), "static row after the step: " + f
    live = np.nonzero((b["alive"] != 0) & (b["static_berg"] < 0.5))[0]
    assert np.array_equal(evolved["lon_old"][live], evolved["lon"][live]) and np.array_equal(evolved["uvel_old"][live], evolved["uvel"][live])
    for f in ("lon", "lat", "uvel", "vvel", "bxn", "byn", "xi", "yj"):
        assert P.rel_err(evolved[f][live], c.b[f][live]) <= P.TOL_TRAJ, "after the evolve alone: " + f
    if n > 4:
        assert gb["fl_k"][4] == -1.0 and gb["alive"][4] == 1 and gb["lon"][4] != b["lon"][4]


# ---- the phase entry points ----
def _phase_run(case, steps):
    ib = _loaded(case)
    p = case[1]
    lib, h, ck = ib.lib, ib.h, ib._check
    try:
        if HB.is_contact(p):
            ib.set_conglom_ids()                                                     # the `Visited` block, IB:5415-5416
        for _ in range(steps):
            ck(lib.kid_zero_accumulators(h), "kid_zero_accumulators")
            if not p.old_interp_flds_order:
                ck(lib.kid_interp_gridded_fields_to_bergs(h), "interp")              # IB:5423
            ck(lib.kid_evolve_icebergs(h), "kid_evolve_icebergs")                    # IB:5433
            if HB.is_contact(p):
                ib.set_conglom_ids()                                                 # IB:5470
            if not p.old_interp_flds_order:
                ck(lib.kid_interp_gridded_fields_to_bergs(h), "interp")              # IB:5473
            ck(lib.kid_thermodynamics(h), "kid_thermodynamics")                      # IB:5505
            ck(lib.kid_create_gridded_icebergs_fields(h), "kid_create_gridded")      # IB:5512
        return _snapshot(ib)
    finally:
        ib.close()


@pytest.mark.parametrize("contact,old_order", [pytest.param(False, True, id="3x3"), pytest.param(True, False, id="contact-stored_environment")])
def test_phases_equal_the_step(contact, old_order):
    case = RK.box(contact, old_order)
    phases = _phase_run(case, 5)
    ib = _loaded(case)
    try:
        ib.run(5)
        fused = _snapshot(ib)
    finally:
        ib.close()
    assert np.array_equal(fused[0]["id"], phases[0]["id"]) and np.array_equal(fused[0]["alive"], phases[0]["alive"])
    for f in tuple(P.TRAJ_FIELDS) + tuple(P.SIZE_FIELDS) + OLD_FIELDS:
        assert P.rel_err(phases[0][f], fused[0][f]) <= 1e-12, f
    for k in range(fused[1].shape[0]):
        assert P.rel_err(phases[1][k], fused[1][k]) <= 1e-12, k
    for k in range(fused[2].shape[0]):
        assert P.rel_err(phases[2][k], fused[2][k]) <= 1e-12, k


# ---- the order of the rows ----
@pytest.mark.parametrize("contact", SEARCHES)
def test_row_order(contact):
    """the box uploaded in reference order and shuffled, 5 steps: a berg's sums run over its neighbours in the order of the cell
    lists -- rank and order, the reference's traversal whatever the rows -- and the per-berg fields, matched by id, come out
    identical to the bit: that is what is asserted (the parity tolerance would be the bound if the lists kept the rows' order)"""
    grid, p, b, _, _ = RK.box(contact)
    perm = np.random.default_rng(5).permutation(len(b["lon"]))
    shuffled = {k: (np.ascontiguousarray(v[perm]) if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    got = []
    for state in (b, shuffled):
        ib = _loaded((grid, p, state, None, 5))
        try:
            ib.run(5)
            got.append(ib.download_bergs())
        finally:
            ib.close()
    o0, o1 = np.argsort(got[0]["id"]), np.argsort(got[1]["id"])
    assert np.array_equal(got[0]["id"][o0], got[1]["id"][o1]) and np.array_equal(got[1]["id"], b["id"][perm])
    assert RK.pairs_in_reach(p, grid["desc"], got[0]) > 0
    for f in ALL_FIELDS:
        assert np.array_equal(got[0][f][o0], got[1][f][o1]), f


# ---- refusals that stay ----
def test_refusals_that_stay():
    from icebergs_amd.lib import KidError
    case = RK.box(False)
    grid, p = case[0], case[1]
    ib = _loaded(case)
    try:
        n_hi, n_lo = C.c_int64(), C.c_int64()
        a, c = np.full((64, 34), -7.0), np.full((64, 34), -7.0)
        dp = C.POINTER(C.c_double)
        assert ib.lib.kid_pack_halo_bergs_pair(ib.h, 0, 0, a.ctypes.data_as(dp), 64, C.byref(n_hi), c.ctypes.data_as(dp), 64, C.byref(n_lo)) == EUNSUPPORTED
        msg = ib.lib.kid_last_error(ib.h)
        assert b"kid_pack_halo_bergs_pair" in msg and b"Runge_not_Verlet" in msg, msg
        assert np.all(a == -7.0) and np.all(c == -7.0)
        assert ib.lib.kid_set_reproducible_sums(ib.h, 1) == EUNSUPPORTED
        msg = ib.lib.kid_last_error(ib.h)
        assert b"reproducible sums" in msg and b"interactive_icebergs_on" in msg, msg
        assert ib.lib.kid_set_reproducible_sums(ib.h, 0) == 0
        q = RK.box_params(False)
        q.mts, q.mts_sub_steps, q.max_bonds, q.old_interp_flds_order = 1, 4, 4, 0
        assert ib.lib.kid_set_params(ib.h, C.byref(q)) == EINVAL
        assert b"Runge_not_Verlet must be false to use MTS" in ib.lib.kid_last_error(ib.h)
        q = RK.box_params(False)
        q.footloose, q.use_operator_splitting = 1, 1
        assert ib.lib.kid_set_params(ib.h, C.byref(q)) == EINVAL
        assert b"Runge_not_Verlet must be false to use footloose" in ib.lib.kid_last_error(ib.h)
        ib.run(1)                         # the handle still steps with the parameters it had
    finally:
        ib.close()
    q = RK.box_params(False)
    q.mts, q.mts_sub_steps, q.max_bonds, q.old_interp_flds_order = 1, 4, 4, 0
    with pytest.raises(KidError, match="rc=-1 .*Runge_not_Verlet must be false to use MTS"):
        _icebergs(grid, q, 8)
    q = RK.box_params(False)
    q.footloose, q.use_operator_splitting = 1, 1
    with pytest.raises(KidError, match="rc=-1 .*Runge_not_Verlet must be false to use footloose"):
        _icebergs(grid, q, 8)
