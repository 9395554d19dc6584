"""The library on curvilinear, rotated grids (tests/curvilinear.py) against the oracle: the interpolated rotation of
interp_flds with rotated and unrotated cells inside one wave, the flag word of the hot build's packets for all four classes
of cell, calc_xiyj's quadratic branch in the hot build, re-indexing across sheared edges, the bounce off a sheared coast, mass
spreading with unequal areas, and lat_terms_cell on both sides of |d| = 0.02 rad.  tests/test_curvilinear_cpu.py shows that
the oracle itself is frame-invariant on these grids and that it sees a wrong sign of sin or a dropped rotation at 1e4 x the
tolerances used here.  DESIGN.md ("Curvilinear, rotated grids") records the measured figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
import curvilinear as CV
import parity as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(ROOT, "icebergs_amd", "csrc", "libkid_hip_exact.so")
N, NSTEPS = 6000, 48
_grids, _refs = {}, {}


def _params(kind, verlet, old_order=True):
    p = CV.patch_params(kind)
    if verlet:
        p.Runge_not_Verlet = 0
    p.old_interp_flds_order = 1 if old_order else 0
    return p


def _case(kind):
    if kind not in _grids:
        grid = CV.patch_grid(kind)
        _grids[kind] = (grid, CV.place_bilinear(grid, N, seed=21))
    return _grids[kind]


def _oracle_run(kind, verlet, old_order):
    """one oracle run per (grid, integrator, order), shared by the cases below and left unchanged"""
    key = (kind, verlet, old_order)
    if key not in _refs:
        grid, b = _case(kind)
        _refs[key] = P.run_oracle(grid, _params(kind, verlet, old_order), b, NSTEPS)
    return _refs[key]


def _lib_run(grid, p, b, nsteps, mode="fused", store=True):
    """parity.run_hip with the stored environment switched on or off; also returns how many bergs the hot build handed to
    the general build in the last step (fused mode)"""
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        if not store:
            ib.set_store_environment(False)
        redo = None
        if mode == "fused":
            ib.run(nsteps)
            redo = ib.last_redo_count()
        else:
            ib.run_phases(nsteps)
        acc, out, scal = ib.fetch()
        return (ib.download_bergs(), acc.copy(), out.copy(), scal.copy()), redo
    finally:
        ib.close()


def _check_parity(kind, verlet, old_order, mode, store):
    grid, b = _case(kind)
    p = _params(kind, verlet, old_order)
    ref = _oracle_run(kind, verlet, old_order)
    got, redo = _lib_run(grid, p, b, NSTEPS, mode, store)
    label = "%s/%s/%s/%s/store=%d" % (kind, "verlet" if verlet else "rk4", "old" if old_order else "new", mode, store)
    if not store:   # kid_set_store_environment(0): berg%uo .. hi stay as uploaded, everything else is compared
        rb = S.copy_bergs(ref[0])
        for f in P.ENV_FIELDS:
            rb[f] = b[f].copy()
        ref = (rb,) + tuple(ref[1:])
    else:
        assert np.abs(ref[0]["ssh_x"]).max() > 0 and np.abs(ref[0]["ui"]).max() > 0   # the rotated pairs carry a signal
    rep = P.compare(ref, got, label, params=p)
    print(label, "redo", redo, {f: "%.1e" % rep[f] for f in P.TRAJ_FIELDS + P.ENV_FIELDS + ["mass"]},
          "planes %.1e" % max(v for k, v in rep.items() if k.startswith(("acc", "out"))))
    if redo is not None:   # the hot build kept at least half of the bergs: this is not the general build alone
        assert 0 <= redo <= N // 2, redo


_LATLON_CASES = [(v, o, m, s) for v in (False, True) for o in (True, False) for m in ("fused", "phases") for s in (True, False)
                 if not (m == "phases" and not s and not o)]   # (the phase entry points read the stored environment under the new order)


@pytest.mark.parametrize("verlet,old_order,mode,store", _LATLON_CASES)
def test_latlon_patch_matches_the_oracle(oracle, verlet, old_order, mode, store):
    _check_parity("latlon", verlet, old_order, mode, store)


@pytest.mark.parametrize("verlet", [False, True])
def test_cartesian_patch_matches_the_oracle(oracle, verlet):
    _check_parity("cartesian", verlet, True, "fused", True)


@pytest.mark.parametrize("verlet", [False, True])
def test_library_does_not_depend_on_the_frame_of_the_velocities(oracle, verlet):
    """the run with one angle theta at every corner (every cell takes the interpolated rotation) against the run with theta = 0
    (every cell passes through): the same cells, fields within TOL_TRAJ -- without the oracle"""
    p = _params("latlon", verlet)
    g0 = CV.frame_grid("latlon", 0.0)
    b = CV.place_bilinear(g0, 3000, seed=33)
    ref = CV.by_id(_lib_run(g0, p, b, 24)[0][0], P.TRAJ_FIELDS + P.SIZE_FIELDS)
    worst = {}
    for theta in (0.4, -1.1, 2.5):
        got = CV.by_id(_lib_run(CV.frame_grid("latlon", theta), p, b, 24)[0][0], P.TRAJ_FIELDS + P.SIZE_FIELDS)
        assert np.array_equal(got["id"], ref["id"])
        assert np.array_equal(got["ine"], ref["ine"]) and np.array_equal(got["jne"], ref["jne"]), theta
        for f in P.TRAJ_FIELDS + P.SIZE_FIELDS:
            worst[f] = max(worst.get(f, 0.0), P.rel_err(got[f], ref[f]))
    print("verlet" if verlet else "rk4", {f: "%.1e" % e for f, e in worst.items()})
    for f, e in worst.items():
        assert e <= P.TOL_TRAJ, (f, e)


def test_a_bergs_result_does_not_depend_on_the_class_of_other_cells(oracle):
    """interp_flds: "the result does not depend on which other bergs share the wave".  cos = 1, sin = 1e-300 at one corner of
    the unrotated region turns the four cells around it from flag 7 to flag 3; the waves that hold their bergs now take the
    rotation branch with most lanes unrotated.  Every berg that never comes near those cells must come back bit for bit."""
    grid, b = _case("latlon")
    p = _params("latlon", False)
    d = grid["desc"]
    ic, jc = 40, 9                       # the corner: north-east of cell (40, 9), far from the rotated disc
    planted = CV.patch_grid("latlon")
    planted["static"]["sin"][jc - d.jsd, ic - d.isd] = 1.0e-300
    f0, f1 = CV.cell_flags(grid), CV.cell_flags(planted)
    changed = np.argwhere(f0 != f1)
    assert len(changed) == 4 and set(f0[f0 != f1]) == {7} and set(f1[f0 != f1]) == {3}
    nsteps = 24
    # bergs that come within one cell of the four cells at any step (an RK4 stage may look into a neighbouring cell)
    import oracle_lib
    o = oracle_lib.Oracle(grid, p)
    t = S.copy_bergs(b)
    near = np.zeros(N, dtype=bool)
    for _ in range(nsteps + 1):
        near |= (np.abs(t["ine"] - (ic + 0.5)) <= 2) & (np.abs(t["jne"] - (jc + 0.5)) <= 2)
        o.run_step(t, 1)
    assert np.array_equal(t["id"], b["id"])
    inside = (np.abs(b["ine"] - (ic + 0.5)) <= 1) & (np.abs(b["jne"] - (jc + 0.5)) <= 1)
    assert inside.sum() >= 4 and 0 < near.sum() < N // 20
    n = N // 64 * 64   # their waves hold other bergs too
    assert (inside[:n].reshape(-1, 64).any(axis=1) & ~near[:n].reshape(-1, 64).all(axis=1)).any()
    fields = [f for f in T.BERG_F64_NAMES]
    a = CV.by_id(_lib_run(grid, p, b, nsteps)[0][0], fields)
    c = CV.by_id(_lib_run(planted, p, b, nsteps)[0][0], fields)
    assert np.array_equal(a["id"], c["id"])
    far = ~np.isin(a["id"], b["id"][near])
    for f in fields + ["ine", "jne"]:
        assert np.array_equal(a[f][far], c[f][far]), f


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/oracle"); sys.path.insert(0, %(root)r + "/tests")
from icebergs_amd import lib
import curvilinear as CV, parity as P
import test_curvilinear_gpu as G
assert b"exact-math" in lib.load().kid_version(), lib.load().kid_version()
def ulps(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2**63) - ia, ia); ib = np.where(ib < 0, np.int64(-2**63) - ib, ib)
    return int(np.abs(ia - ib).max()) if a.size else 0
out = {}
for kind, melt in (("cartesian", False), ("cartesian", True), ("latlon", True)):
    grid, b = G._case(kind)
    for verlet in (0, 1):
        p = CV.patch_params(kind)
        p.Runge_not_Verlet = 1 - verlet
        p.set_melt_rates_to_zero = 0 if melt else 1
        r = CV.by_id(P.run_oracle(grid, p, b, G.NSTEPS)[0], P.TRAJ_FIELDS + P.SIZE_FIELDS)
        g = CV.by_id(P.run_hip(grid, p, b, G.NSTEPS, mode="fused")[0], P.TRAJ_FIELDS + P.SIZE_FIELDS)
        assert np.array_equal(r["id"], g["id"]), "survivors differ"
        res = {f: {"ulps": ulps(g[f], r[f]), "rel": P.rel_err(g[f], r[f]), "nbad": int((g[f] != r[f]).sum())} for f in P.TRAJ_FIELDS + P.SIZE_FIELDS}
        res["cells_equal"] = bool(np.array_equal(r["ine"], g["ine"]) and np.array_equal(r["jne"], g["jne"]))
        out[kind + ("" if melt else "_nomelt") + ("_verlet" if verlet else "_rk4")] = res
out["calving_env"] = {f: list(v) for f, v in G._calving_run().items()}
print("RESULT " + json.dumps(out))
"""


def test_exact_math_twin_on_the_patch_grids(oracle):
    """-DKID_EXACT_MATH (tests/test_exact_math_gpu.py) on the curvilinear grids.

    Cartesian patch, f-plane, melt rates set to zero: no libm call anywhere on a berg's path, calc_xiyj's sqrt and divisions are
    IEEE on both sides -- trajectories equal the oracle's bit for bit, RK4 and Verlet.
    With the melt laws on, their pow (ocml on the device, glibc on the host; both within an ulp, not the same bits) reaches the
    trajectory through the berg's mass, width and length (the drag coefficients of accel): measured on an MI355X, 2 of 6000 bergs
    end with mass / width / length 1-2 ulps from the oracle's, and exactly those two carry bxn / byn a few ulps off (2.0e-16 of
    the field's maximum) from the step in which their size first differed; Verlet came out equal.  That case is held to the 1e-13
    (sizes 1e-14) that file uses wherever libm is on the path, as is the lat-lon patch (sincos of the latitude every step).
    The calving source's in-cell position and stored environment (test_calving_stores_the_rotated_environment_bit_for_bit below)
    are equal bit for bit on this build too."""
    assert os.path.exists(EXACT), "libkid_hip_exact.so is not built (build() makes it)"
    env = dict(os.environ, KID_HIP_SO=EXACT)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    print(json.dumps({c: {f: (v["ulps"], v["nbad"]) for f, v in res.items() if isinstance(v, dict) and v["nbad"]} for c, res in out.items() if c != "calving_env"}))
    print("calving_env", out["calving_env"])
    for case in ("cartesian_nomelt_rk4", "cartesian_nomelt_verlet"):
        assert out[case]["cells_equal"], case
        for f in P.TRAJ_FIELDS + P.SIZE_FIELDS:
            assert out[case][f]["ulps"] == 0, (case, f, out[case][f])
    for case in ("cartesian_rk4", "cartesian_verlet", "latlon_rk4", "latlon_verlet"):
        assert out[case]["cells_equal"], case
        for f in P.TRAJ_FIELDS:
            assert out[case][f]["rel"] <= 1e-13, (case, f, out[case][f])
        for f in P.SIZE_FIELDS:
            assert out[case][f]["rel"] <= (1e-14 if case.startswith("cartesian") else 1e-13), (case, f, out[case][f])
    for f, (nbad, worst) in out["calving_env"].items():
        assert nbad == 0, ("calving, exact-math build", f, nbad, worst)


def _rotate_frame(grid):
    """a smooth angle field on a grid whose cells are not rotated: the velocities are stored in the turned frame"""
    d, st, f = grid["desc"], grid["static"], grid["forcing"]
    i, j = S._ij(d)
    ang = 0.2 + 0.5 * np.sin(2.0 * np.pi * i / 23.0) * np.cos(2.0 * np.pi * j / 19.0)
    c, s = np.cos(ang), np.sin(ang)
    st["cos"][:], st["sin"][:] = c, s
    for a, b in (("uo", "vo"), ("ui", "vi"), ("ua", "va")):
        u, v = f[a].copy(), f[b].copy()
        f[a][:] = c * u - s * v
        f[b][:] = s * u + c * v
    return grid


@pytest.mark.parametrize("case", ["mts_two_bergs", "sts_two_bergs"])
def test_interacting_bergs_on_rotated_velocities(oracle, case):
    """interp_flds as the interacting-berg paths call it: two colliding conglomerates of config 4 under MTS (the stored
    environment of interp_gridded_fields_to_bergs) and under the single-time-step scheme (sts_ia_velocity_kernel)"""
    kw = dict(bump=(150e3, 150e3), two_bergs=True, hexagonal=False, nx=4, ny=6)
    if case == "mts_two_bergs":
        kw.update(sub_steps=100)
        nsteps = 3
    else:
        kw.update(dem=False, mts=False, contact=True, spring_coef=1e-5, dt=60.0)
        nsteps = 40
    grid, p, b, bd = S.config_c4(**kw)
    _rotate_frame(grid)
    S.set_diag_all(p)
    ref, refbd = P.run_oracle_mts(grid, p, b, bd, nsteps)
    flipped = _rotate_frame(S.config_c4(**kw)[0])   # control: a wrong sign of sin shows in this case
    flipped["static"]["sin"] *= -1.0
    other, _ = P.run_oracle_mts(flipped, p, b, bd, nsteps)
    assert P.rel_err(other[0]["uvel"], ref[0]["uvel"]) > 1.0e-6
    got, gotbd = P.run_hip_mts(grid, p, b, bd, nsteps)
    rep = P.compare_mts(ref, refbd, got, gotbd, "C4 rotated/" + case)
    print(case, {k: "%.1e" % v for k, v in rep.items() if v > 0})


def _with_room(b, capacity):
    out = S.empty_bergs(capacity)
    n = len(b["lon"])
    for k, v in b.items():
        out[k][:n] = v
    out["alive"][n:] = 0
    out["_n"] = n
    return out


_calving = {}


def _calving_run():
    """the stored_env variant of tests/test_calving.py's parity on the lat-lon patch grid (.not.old_interp_flds_order: a new berg
    interpolates its environment where it is born, IB:6353-6364), four calls.  Asserted here: planes, counters, ids and integer
    members equal, every real member of the bergs equal but for the in-cell position and the environment (1e-12, as that file).
    Returns {xi, yj or environment field: (new bergs whose value differs from the oracle's, largest difference)} over the four
    calls."""
    if _calving:
        return _calving
    import oracle_lib
    from icebergs_amd.framework import Icebergs
    grid, b0 = _case("latlon")
    b = {k: (v[:200].copy() if hasattr(v, "copy") else v) for k, v in b0.items()}
    p = _params("latlon", False, old_order=False)
    p.current_year, p.current_yearday = 7, 123.25
    cp = S.calving_params(p)
    orc = oracle_lib.Oracle(grid, p)
    st = orc.new_calving_state()
    cap = 12000
    worst = {f: (0, 0.0) for f in ["xi", "yj"] + P.ENV_FIELDS + ["od"]}
    ib = Icebergs(grid, p, capacity=cap)
    try:
        ib.set_forcing(grid["forcing"])
        ib.set_calving_params(cp)
        bergs = _with_room(b, cap)
        ib.upload_bergs(b)
        for step in range(4):
            calv, hflx = S.coupler_calving(grid, seed=step % 2, frac=0.08)
            rc, rscal = orc.calving(cp, calv, hflx, st, bergs, cap)
            assert rc == 0
            gscal = ib.calving(calv, hflx)
            label = "rotated stored_env step %d" % step
            gst = ib.get_calving_state()
            for name in ("calving", "calving_hflx", "stored_ice", "stored_heat", "real_calving", "rmean_calving", "rmean_calving_hflx"):
                assert np.array_equal(gst[name], st[name]), (label, name, float(np.abs(gst[name] - st[name]).max()))
            assert np.allclose(gscal, rscal, rtol=1e-12, atol=0), (label, gscal, rscal)
            assert np.array_equal(ib.get_iceberg_counter(), orc.iceberg_counter), label
            nr = bergs["_n"]
            gb = ib.download_bergs()
            assert len(gb["lon"]) == nr, (label, len(gb["lon"]), nr)
            orr, org = np.argsort(bergs["id"][:nr], kind="stable"), np.argsort(gb["id"], kind="stable")
            assert np.array_equal(bergs["id"][:nr][orr], gb["id"][org]), label
            new = bergs["id"][:nr][orr] >= (1 << 32)
            for f in T.BERG_I32_NAMES:
                assert np.array_equal(bergs[f][:nr][orr], gb[f][org]), (label, f)
            for f in T.BERG_F64_NAMES:
                r, g = bergs[f][:nr][orr], gb[f][org]
                if f in worst:
                    assert np.allclose(g, r, rtol=1e-12, atol=1e-13), (label, f, float(np.abs(g - r).max()))
                else:
                    assert np.array_equal(g, r), (label, f, np.nonzero(g != r)[0][:4])
                if f in worst:
                    nbad, dmax = int((r[new] != g[new]).sum()), float(np.abs(g[new] - r[new]).max())
                    worst[f] = (max(worst[f][0], nbad), max(worst[f][1], dmax))
        fl = CV.flags_of(grid, {"ine": bergs["ine"][200:nr], "jne": bergs["jne"][200:nr]})
        assert nr > 400 and ((fl & 4) == 0).sum() >= 20 and ((fl & 4) != 0).sum() >= 20   # born in rotated and in unrotated cells
        assert np.abs(bergs["ui"][200:nr]).max() > 0 and np.abs(bergs["ssh_x"][200:nr]).max() > 0
    finally:
        ib.close()
    _calving.update(worst)
    return _calving


def test_calving_on_the_patch_grid_matches_the_oracle(oracle):
    """planes, counters and ids bit for bit, the new bergs' members bit for bit but for the in-cell position and the
    interpolated (here: rotated) environment, which tests/test_calving.py holds to 1e-12"""
    print(_calving_run())


def test_calving_stores_the_rotated_environment_bit_for_bit(oracle):
    """The new bergs' in-cell position and stored environment against the oracle's, bit for bit, in rotated and in unrotated cells.

    The calving source calls the cell search and interp_flds with the reference's own operations (their IEEE instances,
    kid_device.hpp: a rounded product and sum instead of the fused multiply-add, the correctly rounded quotient and root, every
    cell rotated) -- once per calving cell, nowhere near the hot path.  With the per-berg builds' fused instance it was one ulp
    off, measured on an MI355X (most new bergs that differed after any of the four calls, largest difference): uo 174, 1.1e-16;
    vo 186, 3.5e-17; ui 79, 6.9e-18; vi 68, 1.4e-17; ua 196, 1.8e-15; va 159, 4.4e-16; ssh_x 118, 1.7e-21; ssh_y 220, 8.5e-22."""
    worst = _calving_run()
    print(worst)
    for f, (nbad, dmax) in worst.items():
        assert nbad == 0, (f, nbad, dmax)
