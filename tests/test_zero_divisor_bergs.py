"""Live bergs whose mass or volume is zero: the call sites that hand kid_rcp a zero divisor ("call sites").

kid_rcp(0) is NaN where IEEE's 1/0 is inf.  accel_pre forms 1/M and thermodynamics 1/(T W L); a step never makes such a berg
(thermodynamics removes a berg in the step in which its mass reaches zero), an upload can.  Twelve bergs on the curvilinear lat-lon
patch, ten ordinary ones in a block of cells and, each alone in a cell away from them, one with mass = 0 and one with thickness = 0,
three steps, RK4 and Verlet.

The CPU half holds the reference's side: its inf does not survive to a result.  1/M = inf makes the drag coefficients infinite and
the implicit solve 0 * inf: position and velocity are NaN after the first step, and the berg is removed by thermodynamics (its new
mass is 0).  The berg without volume keeps mass 0/0 = NaN and stays, NaN in position, velocity and mass.  Every other berg is finite,
and so is every per-cell sum outside the two cells.
The GPU half: the library does the same -- the same survivors, the berg without volume NaN in the same fields, every other berg
within the parity tolerances, the per-cell sums within TOL_GRID outside the 3 x 3 cells around the two bergs, the same counters.  So
the deviation of kid_rcp at 0 changes no result the reference keeps finite."""
import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
import parity as P
import test_wave_mix_gpu as W

NSTEPS = 3
CELLS = [(37, 7), (38, 7), (37, 8), (38, 8), (37, 7), (38, 8), (37, 9), (38, 9), (37, 8), (38, 7)]
CELL_M0, CELL_V0 = (43, 8), (43, 11)      # the berg without mass, the berg without volume: four cells from the others
ID_M0, ID_V0 = 11, 12
NAN_FIELDS = ["lon", "lat", "uvel", "vvel"]
_case = {}


def population():
    if "b" not in _case:
        g = W.grid()
        d, st = g["desc"], g["static"]
        cells = CELLS + [CELL_M0, CELL_V0]
        n = len(cells)
        rng = np.random.default_rng(3)
        b = S.empty_bergs(n)
        b["ine"][:] = [c[0] for c in cells]
        b["jne"][:] = [c[1] for c in cells]
        xi, yj = rng.uniform(0.2, 0.8, n), rng.uniform(0.2, 0.8, n)
        S._fill_classes(b, rng.integers(0, 10, size=n))
        jj, ii = b["jne"] - d.jsd, b["ine"] - d.isd
        for name in ("lon", "lat"):
            b[name][:] = W._bilinear(st[name], ii, jj, xi, yj)
        b["xi"][:], b["yj"][:] = xi, yj
        b["start_mass"][:] = b["mass"]
        b["mass"][ID_M0 - 1] = 0.0
        b["thickness"][ID_V0 - 1] = 0.0
        b["start_lon"][:], b["start_lat"][:] = b["lon"], b["lat"]
        b["start_day"][:] = 1.0e-6 * np.arange(n)
        b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"]
        _case["b"] = S.sort_reference_order(b)
    return _case["b"]


def oracle_run(verlet):
    if verlet not in _case:
        _case[verlet] = P.run_oracle(W.grid(), W._params(verlet), population(), NSTEPS)
    return _case[verlet]


def near_bad_cells():
    """True on the 3 x 3 cells around the two bergs (mass spreading reaches the neighbours)"""
    d = W.grid()["desc"]
    m = np.zeros(W.grid()["static"]["lon"].shape, dtype=bool)
    for (i, j) in (CELL_M0, CELL_V0):
        m[j - d.jsd - 1:j - d.jsd + 2, i - d.isd - 1:i - d.isd + 2] = True
    return m


def by_id(b):
    n = int(b.get("_n", len(b["lon"])))
    live = np.flatnonzero(b["alive"][:n] != 0)
    o = live[np.argsort(b["id"][live], kind="stable")]
    return {f: b[f][o] for f in P.TRAJ_FIELDS + P.SIZE_FIELDS + ["id", "ine", "jne"]}


def check_degenerate(run, label):
    """what both sides must show: the massless berg gone, the berg without volume NaN, everything else finite"""
    rb, acc, out, scal = run
    r = by_id(rb)
    assert ID_M0 not in r["id"] and ID_V0 in r["id"] and len(r["id"]) == len(CELLS) + 1, (label, r["id"])
    bad = r["id"] == ID_V0
    for f in NAN_FIELDS + ["mass"]:
        assert np.isnan(r[f][bad]).all(), (label, f, r[f][bad])
    for f in P.TRAJ_FIELDS + P.SIZE_FIELDS:
        assert np.isfinite(r[f][~bad]).all(), (label, f)
    far = ~near_bad_cells()
    assert np.isfinite(acc[:, far]).all() and np.isfinite(out[:, far]).all(), label
    assert scal[T.SCALAR_NAMES["nbergs_melted"]] == 1, (label, scal)
    return r, bad


@pytest.mark.parametrize("verlet", [False, True])
def test_reference_turns_a_zero_mass_or_volume_into_nan_not_into_a_result(oracle, verlet):
    b = population()
    assert b["mass"][b["id"] == ID_M0] == 0.0 and b["thickness"][b["id"] == ID_V0] == 0.0 and (b["alive"] != 0).all()
    r, bad = check_degenerate(oracle_run(verlet), "oracle")
    # already after one step the massless berg is NaN and gone: 1/M = inf does not reach a stored number
    one = P.run_oracle(W.grid(), W._params(verlet), b, 1)[0]
    k = np.flatnonzero(one["id"] == ID_M0)[0]
    assert one["alive"][k] == 0 and np.isnan(one["lon"][k]) and np.isnan(one["uvel"][k])


@pytest.mark.gpu
@pytest.mark.parametrize("verlet", [False, True])
def test_library_agrees_with_the_reference_on_zero_mass_and_volume(oracle, verlet):
    g, p, b = W.grid(), W._params(verlet), population()
    ref = oracle_run(verlet)
    got = P.run_hip(g, p, b, NSTEPS)
    label = "zero divisors/%s" % ("verlet" if verlet else "rk4")
    r, bad = check_degenerate(ref, label + "/oracle")
    q, bad_q = check_degenerate(got, label + "/library")
    assert np.array_equal(r["id"], q["id"]) and np.array_equal(bad, bad_q)
    assert np.array_equal(r["ine"], q["ine"]) and np.array_equal(r["jne"], q["jne"])
    for f in P.TRAJ_FIELDS + P.SIZE_FIELDS:
        e = P.rel_err(q[f][~bad], r[f][~bad])
        assert e <= (P.TOL_TRAJ if f in P.TRAJ_FIELDS else P.TOL_SIZE), (label, f, e)
    far = ~near_bad_cells()
    racc, gacc = np.where(far, ref[1], 0.0), np.where(far, got[1], 0.0)
    sc = P.acc_scales(racc)
    from icebergs_amd.distributed import needs_footprint_planes
    a0 = T.ACC_NAMES["area_on_ocean"]
    dead = set() if needs_footprint_planes(p) else set(range(a0, a0 + 27))
    for k in range(racc.shape[0]):
        if k not in dead:
            assert P.acc_err(gacc, racc, k, sc) <= P.TOL_GRID, (label, "acc plane", k)
    for k in range(ref[2].shape[0]):
        assert P.rel_err(np.where(far, got[2][k], 0.0), np.where(far, ref[2][k], 0.0)) <= P.TOL_GRID, (label, "out plane", k)
    for name in ("nbergs_melted", "nbergs_alive", "nspeeding_tickets"):
        assert ref[3][T.SCALAR_NAMES[name]] == got[3][T.SCALAR_NAMES[name]], (label, name)
