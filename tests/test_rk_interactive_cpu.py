"""Interacting bergs under RK4, the checker and the cases, no GPU: tests/rk_interactive_ref.c pinned to the oracle's own
RK4 where nobody is in reach, its independence of the order in which the first sweep visits the rows, the branches the cases of
tests/rk_interactive.py reach, and how far interactions and the integrator move the answer.

The device is held to the checker with tests/parity.py's tolerance for trajectories, TOL_TRAJ = 1e-10 (test_rk_interactive_gpu.py):
that is "the parity tolerance" below."""
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

SEARCHES = [pytest.param(False, id="3x3"), pytest.param(True, id="contact")]
WRITTEN = tuple(P.TRAJ_FIELDS)            # what ko_evolve_icebergs writes under RK4, with ine, jne and alive
ALL_FIELDS = tuple(T.BERG_F64_NAMES) + tuple(T.BERG_I32_NAMES) + ("id",)
FAR = 9.0e3                               # no two discs of the far-apart population closer than this (reach: 3.15 km; 10 steps move one 1.8 km)
FAR_STEPS = 10


def far_population():
    """discs of the box no two of which are within FAR of each other, picked greedily in row order"""
    grid, b0 = HB.population()
    keep = []
    for k in range(len(b0["lon"])):
        if all((b0["lon"][k] - b0["lon"][o]) ** 2 + (b0["lat"][k] - b0["lat"][o]) ** 2 > FAR * FAR for o in keep):
            keep.append(k)
    keep = np.array(keep)
    return grid, {k: (np.ascontiguousarray(v[keep]) if isinstance(v, np.ndarray) else v) for k, v in b0.items()}


def _evolve_pair(grid, b, p_ia, p_plain, steps, interacting):
    """the largest relative difference per step between `interacting` (an evolve with the interactive terms, springs on) and
    ko_evolve_icebergs (without) from the same state, over WRITTEN; cells and survivors must be the same.  The next step starts
    from the interacting side's state."""
    ol = RK.oracle_lib()
    o_ia, o_plain = ol.Oracle(grid, p_ia), ol.Oracle(grid, p_plain)
    b = S.copy_bergs(b)
    worst = 0.0
    for _ in range(steps):
        assert RK.pairs_in_reach(p_ia, grid["desc"], b) == 0
        ref = S.copy_bergs(b)
        o_plain.lib.ko_evolve_icebergs(C.byref(o_plain.kg), C.byref(o_plain.params), C.byref(o_plain.soa(ref)), ol._dp(o_plain.scalars))
        interacting(o_ia, b)
        for f in ("ine", "jne", "alive"):
            assert np.array_equal(ref[f], b[f]), f
        worst = max([worst] + [P.rel_err(b[f], ref[f]) for f in WRITTEN])
    assert o_ia.scalars[T.SCALAR_NAMES["error_count"]] == o_plain.scalars[T.SCALAR_NAMES["error_count"]]
    assert o_ia.scalars[T.SCALAR_NAMES["nspeeding_tickets"]] == o_plain.scalars[T.SCALAR_NAMES["nspeeding_tickets"]]
    return worst


@pytest.mark.parametrize("old_order", [pytest.param(1, id="old_interp_flds_order"), pytest.param(0, id="stored_environment")])
def test_stage_driver_pinned_to_the_oracle(old_order):
    """Nobody within reach, interactive_icebergs_on = 1, springs on: the checker gives what ko_evolve_icebergs (RK4) gives.  The
    tolerance is measured in this run: the largest relative difference of ko_evolve_icebergs_interactive against ko_evolve_icebergs
    under Verlet on the same population -- the same two restatements of accel, called once per step there and four times here --
    times 4, or zero if that is zero.  Measured: 0 for both orders, and the RK4 pair is identical to the bit."""
    grid, b = far_population()
    assert len(b["lon"]) >= 12
    ol = RK.oracle_lib()
    if not old_order:                     # the stored environment, once (neither evolve changes it)
        o = ol.Oracle(grid, RK.box_params(False, old_order=False))
        o.lib.ko_interp_gridded_fields_to_bergs(C.byref(o.kg), C.byref(o.params), C.byref(o.soa(b)))
    lib = RK.checker()
    lib.tko_set_traversal(0, 0)

    def verlet(o, state):
        o.lib.ko_evolve_icebergs_interactive(C.byref(o.kg), C.byref(o.params), C.byref(o.soa(state)), None, ol._dp(o.scalars))

    def rk4(o, state):
        lib.tko_evolve_icebergs_interactive_rk(C.byref(o.kg), C.byref(o.params), C.byref(o.soa(state)), None, ol._dp(o.scalars))

    measured = _evolve_pair(grid, b, RK.box_params(False, old_order, rk=False), RK.box_params(False, old_order, rk=False, interactive=False),
                            FAR_STEPS, verlet)
    got = _evolve_pair(grid, b, RK.box_params(False, old_order), RK.box_params(False, old_order, interactive=False), FAR_STEPS, rk4)
    print("far-apart population of %d: Verlet pair %.3e, RK4 pair %.3e" % (len(b["lon"]), measured, got))
    assert got <= 4.0 * measured, "RK4 pair %.3e, Verlet pair %.3e" % (got, measured)


def _run_in_order(case, mode, seed, steps):
    grid, p, b, bonds, _ = case
    c = RK.Composed(grid, p, S.copy_bergs(b), S.copy_bonds(bonds) if bonds is not None else None)
    RK.checker().tko_set_traversal(mode, seed)
    try:
        for _ in range(steps):
            c.step()
    finally:
        RK.checker().tko_set_traversal(0, 0)
    return c.snapshot()


@pytest.mark.parametrize("name", ["box-3x3", "box-contact", "polar"])
def test_order_free(name):
    """the first sweep over the rows reversed and shuffled: every field of every row, the planes and the scalars identical to the bit
    (5 steps: the pair forces of steps 2 .. 5 read what the sweeps of the step before left)"""
    case = {"box-3x3": lambda: RK.box(False), "box-contact": lambda: RK.box(True), "polar": RK.polar}[name]()
    ref = _run_in_order(case, 0, 0, 5)
    assert RK.pairs_in_reach(case[1], case[0]["desc"], ref[0]) > 0
    for mode, seed in ((1, 0), (2, 11), (2, 12)):
        got = _run_in_order(case, mode, seed, 5)
        for f in ALL_FIELDS:
            assert np.array_equal(ref[0][f], got[0][f]), (mode, seed, f)
        for k in (1, 2, 3):
            assert np.array_equal(ref[k], got[k]), (mode, seed, k)


@pytest.mark.parametrize("contact", SEARCHES)
def test_box_reaches_its_branches(contact):
    """(a): pairs inside crit_dist on every step, bergs whose stage cell is not their cell at the start of the step.  The box has no
    land: no bounce to count."""
    _, st = RK.box_run(contact)
    print("box %s: %s" % ("contact" if contact else "3x3", {k: v for k, v in st.items() if k != "contact_steps"}))
    assert st["finite"] and st["berg_steps"] == 247 * RK.NSTEPS
    assert st["pairs"] > 0 and st["contact_steps"][-1] == RK.NSTEPS
    assert st["cell_changes"] > 0


def test_collision_reaches_its_branches_and_its_step_count():
    """(b): COLLISION_STEPS is the first multiple of 50 at which the two conglomerates have been in contact for at least 20 steps
    (a pair of elements of different conglomerates within R1 + R2 before the step).  No land in this case either."""
    _, st = RK.collision_run()
    print("collision: %s" % {k: v for k, v in st.items() if k != "contact_steps"})
    cs = st["contact_steps"]
    assert st["finite"] and st["berg_steps"] == 16 * RK.COLLISION_STEPS
    assert st["first_contact"] == 495 and cs[514 - 1] == 20
    assert RK.COLLISION_STEPS % 50 == 0 and cs[RK.COLLISION_STEPS - 1] >= 20 and cs[RK.COLLISION_STEPS - 50 - 1] < 20
    assert st["pairs"] > 0 and st["cell_changes"] > 0


def test_polar_reaches_the_tangent_plane_with_a_pair_in_reach():
    """(c) is kept because it does: steps on the tangent plane (lat > 89) and pairs inside crit_dist on every step"""
    _, st = RK.polar_run()
    print("polar: %s" % {k: v for k, v in st.items() if k != "contact_steps"})
    assert st["finite"] and st["tangent_steps"] > 0 and st["tangent_steps"] < st["berg_steps"], "some elements above 89, some below"
    assert st["pairs"] > 0 and st["contact_steps"][-1] == RK.POLAR_STEPS


@pytest.mark.parametrize("n", RK.SHAPES)
def test_shapes(n):
    """(d): the checker leaves dead and static rows as they were (the second sweep writes nothing to a static row); a row with
    fl_k = -1 moves but feels nobody"""
    grid, p, b, _, _ = RK.shapes(n)
    snaps, st = RK.shapes_run(n)
    got = snaps[1][0]
    untouched = (b["alive"] == 0) | (b["static_berg"] >= 0.5)
    assert st["berg_steps"] == int((~untouched).sum())
    if n >= 63:
        assert st["pairs"] > 0 and untouched.sum() >= 9 and (b["fl_k"] == -1.0).sum() == 1
    for f in tuple(T.BERG_F64_NAMES) + ("ine", "jne", "alive", "id"):
        if f in P.ENV_FIELDS or f == "od":
            continue                      # (the interpolation of IB:5473 and the thermodynamics store the environment of every live row)
        assert np.array_equal(got[f][untouched], b[f][untouched]), f
    if n > 4:
        assert got["lon"][4] != b["lon"][4] and got["lon_old"][4] == got["lon"][4]


@pytest.mark.parametrize("contact", SEARCHES)
def test_sensitivity(contact):
    """interactions and the integrator move uvel by orders of magnitude more than the parity tolerance: RK4 with against RK4 without
    interactions, RK4 against Verlet, each at least 1e3 x TOL_TRAJ after the 40 steps of the box"""
    rk = RK.box_run(contact)[0][RK.NSTEPS][0]
    plain = RK.box_run(contact, interactive=False)[0][RK.NSTEPS][0]
    verlet = RK.box_run(contact, rk=False)[0][RK.NSTEPS][0]
    for name, other in (("interactions off", plain), ("Verlet", verlet)):
        assert np.array_equal(rk["id"], other["id"])
        ratio = P.rel_err(other["uvel"], rk["uvel"]) / P.TOL_TRAJ
        print("box %s: RK4 against %s: uvel differs by %.3e x the parity tolerance" % ("contact" if contact else "3x3", name, ratio))
        assert ratio >= 1.0e3
