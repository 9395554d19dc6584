"""Bonded bergs on lat-lon grids, on the CPU: the cases of tests/latlon_bonded.py are what they claim to be -- admissible (the
oracle's own spread under one-ulp changes of the initial positions stays under the cap, the discrete outcome is the same in all
nine runs, the run is clean), they reach the branch each exists for, and the derived tolerances see a metric wrong by 1e-5 from
at least 100 x away.  Oracle only; the device is held to these cases in tests/test_latlon_bonded_gpu.py.  The spread and so the
tolerances are measured on the day of the run: nothing here is a recorded figure (DESIGN.md section 4 has the table of one run;
`pytest -s` or `-rP` shows today's, one line per case).

The second control: the pair metric (grid_to_meters) is a static function of oracle/kid_oracle_mts.c and cannot be handed another
latitude without touching oracle/, so it is Rearth on one side only -- params.Rearth (pair metric, position and velocity maps)
scaled while the grid's dx / dy / area stay; the first control scales both."""
import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
import latlon_bonded as LB
import parity as P

CASES = LB.NAMES


def _scalar(ref, name):
    return ref[3][T.SCALAR_NAMES[name]]


def _bonded_sides(bd):
    return int(bd["count"].sum())


def test_builder_maps_the_metre_pattern():
    """rows in reference order, in-cell coordinates from the cell's own corners, bonds those of the metre pattern (by id) and the
    bonded pairs 2 r apart under the reference's own pair metric, up to the shear of the map (x tan(lat) dlat)"""
    for name in CASES:
        grid, p, b, bd, _ = LB.case(name)
        d, st = grid["desc"], grid["static"]
        assert d.grid_is_latlon == 1 and d.grid_is_regular == 0 and p.Rearth == 6.36e6
        n = len(b["lon"])
        assert n <= 60 and np.all(np.diff(b["jne"].astype(np.int64) * 1000 + b["ine"]) >= 0)
        jj, ii = b["jne"] - d.jsd, b["ine"] - d.isd
        assert np.all((st["lon"][jj, ii - 1] <= b["lon"]) & (b["lon"] < st["lon"][jj, ii]))
        assert np.all((st["lat"][jj - 1, ii] <= b["lat"]) & (b["lat"] < st["lat"][jj, ii]))
        assert np.all((b["xi"] >= 0) & (b["xi"] < 1) & (b["yj"] >= 0) & (b["yj"] < 1))
        assert np.array_equal(b["n_bonds"], bd["count"]) and bd["count"].min() >= 2
        row = {int(i): k for k, i in enumerate(b["id"])}
        worst = 0.0
        for (a, o), slot in P.bond_set(b, bd).items():
            assert (o, a) in P.bond_set(b, bd)
            ka, ko = row[a], row[o]
            worst = max(worst, abs(LB.pair_metres(p, b["lon"][ka], b["lat"][ka], b["lon"][ko], b["lat"][ko]) / 3000.0 - 1.0))
        bound = 0.02 if abs(b["lat"]).max() < 80 else 0.6     # tan(70) = 2.7, tan(89) = 57: the map shears the pattern near the pole
        assert worst < bound, (name, worst)
        if p.mts:
            assert p.dt / p.mts_sub_steps in (18.0, 90.0)     # config 4's DEM sub-step; its implicit inner scheme (20 per step)


@pytest.mark.parametrize("name", CASES)
def test_case_is_admissible(oracle, name):
    m = LB.measured(name)
    ref, b0 = m["ref"], m["case"][2]
    sp, same = LB.spread(name)
    print(LB.table_line(name))
    assert all(same.values()), (name, same)                     # cells, conglomerates, partners, broken bonds, counters: all nine agree
    assert not LB.over_cap(name), (name, LB.over_cap(name))     # 10 x spread <= 100 x today's tolerance
    assert _scalar(ref, "error_count") == 0 and _scalar(ref, "nspeeding_tickets") == 0
    assert np.all(ref[0]["alive"] != 0) and np.array_equal(ref[0]["id"], b0["id"])
    for f in P.TRAJ_FIELDS + P.MTS_FIELDS:
        assert np.isfinite(ref[0][f]).all(), (name, f)
    tol, base = LB.tolerances(name), P.mts_tolerances()
    assert set(tol) == set(base) and all(base[k] <= tol[k] <= LB.SPREAD_CAP * base[k] for k in base)


@pytest.mark.parametrize("name", CASES)
def test_controls_are_far_outside_the_tolerances(oracle, name):
    """a metric wrong by 1e-5 fails the derived tolerances by at least 100 x in lon or uvel"""
    for which in ("both", "params"):
        c = LB.control(name, which)
        print("%s control %s: lon %.1e x tol, uvel %.1e x tol" % (name, which, c["lon"], c["uvel"]))
        assert max(c["lon"], c["uvel"]) >= 100.0, (name, which, c["lon"], c["uvel"])


# ---- reach: each case shows from the oracle's output what it exists for ----
def _moved(name):
    m = LB.measured(name)
    b0, rb = m["case"][2], m["ref"][0]
    return int(((rb["ine"] != b0["ine"]) | (rb["jne"] != b0["jne"])).sum())


def _gap_between_conglomerates(p, b):
    """the smallest distance between elements of different conglomerates, in the reference's metres"""
    other = b["conglom_id"][:, None] != b["conglom_id"][None, :]
    dist = LB.pair_metres(p, b["lon"][:, None], b["lat"][:, None], b["lon"][None, :], b["lat"][None, :])
    return float(dist[other].min())


def test_reach_two_bergs_70S(oracle):
    m = LB.measured("two_bergs_70S")
    grid, p, b0, bd, _ = m["case"]
    rb = m["ref"][0]
    assert _moved("two_bergs_70S") >= 1
    assert len(np.unique(rb["conglom_id"])) == 2
    b0 = S.copy_bergs(b0)
    b0["conglom_id"][:] = rb["conglom_id"]
    before, after = _gap_between_conglomerates(p, b0), _gap_between_conglomerates(p, rb)
    print("two_bergs_70S: %d elements changed cell; gap between the conglomerates %.0f m -> %.0f m (contact_distance %.0f m)" % (
        _moved("two_bergs_70S"), before, after, p.contact_distance))
    assert before > p.contact_distance > after       # (R1 + R2 = 3 km < contact_distance: the range is the distance)
    assert abs(p.omega) > 0 and not p.use_f_plane and abs(rb["lat"]).min() > 69.0     # Coriolis from the latitude


def test_reach_hex_grounded_60S(oracle):
    m = LB.measured("hex_grounded_60S")
    p, rb, bd = m["case"][1], m["ref"][0], m["refbd"]
    grounded = rb["od"] < (p.rho_bergs / 1025.0) * rb["thickness"]       # the draught, D = rho_bergs / rho_seawater T (IB:4900)
    print("hex_grounded_60S: od %.0f .. %.0f m, %d elements over less water than their draught" % (rb["od"].min(), rb["od"].max(), int(grounded.sum())))
    assert grounded.any() and not grounded.all()
    assert _scalar(m["ref"], "nbonds_broken") == 0 and not (bd["broken"] != 0).any() and _bonded_sides(bd) == _bonded_sides(m["case"][3])
    assert m["case"][0]["desc"].grid_is_regular == 0   # the depth goes through calc_xiyj


def test_reach_hex_fracture(oracle):
    m = LB.measured("hex_fracture")
    sides = _bonded_sides(m["case"][3])
    broken = int(_scalar(m["ref"], "nbonds_broken"))
    print("hex_fracture: %d of %d bond sides broken, %d still listed (%d of them broken, kept for contact)" % (
        broken, sides, _bonded_sides(m["refbd"]), int((m["refbd"]["broken"] != 0).sum())))
    assert 1 <= broken <= sides // 2
    assert LB.spread("hex_fracture")[1]["broken_bonds"] and LB.spread("hex_fracture")[1]["bond_partners"] and LB.spread("hex_fracture")[1]["scalars"]


def test_reach_polar_89N(oracle):
    """initial latitudes on both sides of 89; whether a row crosses it is looked at step by step.  A run the cap on the spread
    admits is two steps long (the velocities' spread passes the cap in the third), in which the elements travel about 150 m, and
    the row nearest to 89 starts 390 m south of it: no row crosses, and none could in a run of this length at this drift."""
    import oracle_lib
    grid, p, b, bd, nsteps = LB.case("polar_89N")
    assert (b["lat"] > 89.0).sum() >= 6 and (b["lat"] < 89.0).sum() >= 6
    o = oracle_lib.Oracle(grid, p)
    b, bd = S.copy_bergs(b), S.copy_bonds(bd)
    side0 = b["lat"] > 89.0
    crossed = np.zeros(len(side0), dtype=bool)
    for _ in range(nsteps):
        o.run_step_mts(b, bd, 1)
        crossed |= (b["lat"] > 89.0) != side0
    nearest = float(np.abs(LB.case("polar_89N")[2]["lat"] - 89.0).min()) * p.Rearth * np.pi / 180.0
    print("polar_89N: %d rows above 89, %d below, %d crossed in %d steps (nearest starts %.0f m from it)" % (
        int(side0.sum()), int((~side0).sum()), int(crossed.sum()), nsteps, nearest))
    assert ((b["lat"] > 89.0).any() and (b["lat"] < 89.0).any())     # both branches of the position and velocity maps run in one launch
    assert not crossed.any() and nearest > 0.1 * p.dt * nsteps       # said so: the drift of 0.1 m/s cannot carry a row that far


def test_reach_polar_depth(oracle):
    m = LB.measured("polar_depth")
    grid, p, b0 = m["case"][:3]
    top0, top1 = LB.depth_stencil_top(grid, p, b0), LB.depth_stencil_top(grid, p, m["ref"][0])
    print("polar_depth: highest centre of the depth stencil %.4f (start), %.4f (end); od %s" % (top0.max(), top1.max(), m["ref"][0]["od"]))
    assert (top0 >= 89.999).all() and (top1 >= 89.999).all()
    assert top1.max() < 90.0                                          # the map's radii 90 - lat stay positive
    assert _scalar(m["ref"], "error_count") == 0
    assert np.ptp(m["ref"][0]["od"]) > 1.0                            # the depth the form interpolates is not flat


def test_reach_c2_forcing_60S(oracle):
    m = LB.measured("c2_forcing_60S")
    grid, p, _, _, _ = m["case"]
    rb = m["ref"][0]
    assert p.diag_mask == (1 << 20) - 1
    assert np.ptp(rb["uo"]) > 0 and np.ptp(rb["sst"]) > 0             # the stored environment holds gradients
    uv = m["ref"][1][T.ACC_NAMES["uvel_on_ocean"]:T.ACC_NAMES["uvel_on_ocean"] + 9]
    assert np.abs(uv).max() > 0                                       # the velocity-weighted planes hold something
    assert _moved("c2_forcing_60S") >= 1


def test_wrapped_longitudes():
    a, b = np.array([359.9999, 0.5, 10.0]), np.array([-0.0001, 360.5, 10.0])
    assert P.wrapped_lon_err(a, b) < 1e-12 and P.rel_err(a, b) > 0.9
    assert abs(P.wrapped_lon_err(np.array([10.0, 20.0]), np.array([10.0, 20.5])) - 0.5 / 20.5) < 1e-15


def test_default_tolerances_are_todays():
    """compare_mts without a mapping asserts what it always has"""
    t = P.mts_tolerances()
    assert t["lon"] == t["uvel"] == t["od"] == t["mass"] == t["bond_length"] == 1.0e-9
    assert t["axn"] == t["ang_accel"] == t["bond_nstress"] == t["bond_f_x"] == 1.0e-4
    assert t["ang_vel"] == t["rot"] == 1.0e-6 and t["acc"] == t["out"] == 10 * P.TOL_GRID
