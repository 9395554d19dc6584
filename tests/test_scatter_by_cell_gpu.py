"""The hot build's scatter by distinct cell (kid_berg_kernel.hpp: the slot walk ranks the lanes, seg_flush adds once per cell).

Small populations on config 2's grid and forcing, confined to a block of C neighbouring ocean cells, so that a wave holds a
known number of distinct cells: 1, 2, 6, 11 (= KID_HOT3_SLOTS), 12 (the lanes of the twelfth cell go to the general build) and
18 (> KID_MAXRUN).  1573 = 64 * 24 + 37 bergs: the last wave is partial.  The same bergs are handed over in four row orders --
sorted by cell, round-robin over the cells (no two adjacent lanes share a cell: runs and distinct cells differ most), a seeded
shuffle, round-robin with every 7th row dead -- and stepped 8 times without re-binning, so that the order decays further; the
round-robin order once more with a re-binning every 3 steps (the re-binning instance of the plain builds runs in between).

Every run is held against the CPU oracle with the project's tolerances (parity.compare: TOL_TRAJ, TOL_SIZE, TOL_GRID with
acc_scales, error_count = 0); between the row orders the per-berg fields are bit for bit the same and the per-cell sums agree
within 1e-11 of the field's maximum (a change of summation order); and the melt budget closes to 1e-9 over the last, most
decayed step.  The block sits at 72 S, where a cell is 34 km wide: in the oracle's run at least 20 bergs end in another cell
than they started in (asserted), otherwise the decayed order would never be exercised."""
import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
import parity as P

pytestmark = pytest.mark.gpu

N = 64 * 24 + 37
NSTEPS = 8
I0, J0 = 100, 9                      # lat -72.8 .. -70.4: dx = 33 - 37 km, the bergs reach ~0.2 m/s within the 8 steps
BLOCKS = {1: (1, 1), 2: (2, 1), 6: (3, 2), 11: (11, 1), 12: (12, 1), 18: (6, 3)}   # C: cells in i, cells in j
VARIANTS = ("plain", "store_env", "diag_all", "verlet")                              # K = 1, K = 3, K = 0 (RK4), K = 0 (Verlet)
PER_BERG = P.TRAJ_FIELDS + P.SIZE_FIELDS + ["ine", "jne"]
SUM_TOL = 1.0e-11                    # per-cell sums between two row orders (test_results_do_not_depend_on_the_row_order_at_1e6)
_grid, _pops, _refs = [], {}, {}


def grid():
    if not _grid:
        _grid.append(S.c2_forcing(S.latlon_grid()))
    return _grid[0]


def params(variant):
    p = S.default_params()
    p.dt = 1800.0
    if variant == "diag_all":
        S.set_diag_all(p)
    if variant == "verlet":
        p.Runge_not_Verlet = 0
    return p


def _take(b, rows):
    return {k: (np.ascontiguousarray(v[rows]) if hasattr(v, "dtype") else v) for k, v in b.items()}


def populations(C):
    """the bergs of block C in the row orders a - e: {"a": sorted by cell, "b": round-robin over the cells, "c": shuffled,
    "d": order b with every 7th row dead, "e": order a with the same bergs dead}"""
    if C not in _pops:
        ni, nj = BLOCKS[C]
        a = S.place_bergs(grid(), N, 100 + C, (I0, I0 + ni - 1), (J0, J0 + nj - 1))   # (sorted by cell: sort_reference_order)
        cell = a["ine"].astype(np.int64) + 1000 * a["jne"].astype(np.int64)
        assert len(np.unique(cell)) == C
        # round-robin: the k-th berg of every cell, cell after cell
        nth = np.arange(N) - np.searchsorted(cell, cell, side="left")
        b = _take(a, np.lexsort((cell, nth)))
        if C > 1:
            cb = b["ine"].astype(np.int64) + 1000 * b["jne"].astype(np.int64)
            assert (cb[1:64 * 4] != cb[:64 * 4 - 1]).all()      # no two adjacent lanes share a cell while every cell still has bergs
        c = _take(a, np.random.default_rng(7).permutation(N))
        d = S.copy_bergs(b)
        d["alive"][::7] = 0
        e = S.copy_bergs(a)
        e["alive"][np.isin(a["id"], d["id"][::7])] = 0
        _pops[C] = {"a": a, "b": b, "c": c, "d": d, "e": e}
    return _pops[C]


def oracle_run(C, variant, order):
    """one oracle run per (block, variant, set of live bergs), shared and left unchanged"""
    key = (C, variant, "d" if order in ("d", "e") else "a")
    if key not in _refs:
        _refs[key] = P.run_oracle(grid(), params(variant), populations(C)[key[2]], NSTEPS)
    return _refs[key]


def cells_changed(start, end):
    """bergs alive at the end that sit in another cell than they started in"""
    o1 = np.flatnonzero(end["alive"] != 0)
    o1 = o1[np.argsort(end["id"][o1], kind="stable")]
    o0 = np.flatnonzero(np.isin(start["id"], end["id"][o1]) & (start["alive"] != 0))
    o0 = o0[np.argsort(start["id"][o0], kind="stable")]
    o1 = o1[np.isin(end["id"][o1], start["id"][o0])]          # (a footloose child has no start)
    assert np.array_equal(start["id"][o0], end["id"][o1])
    return int(((start["ine"][o0] != end["ine"][o1]) | (start["jne"][o0] != end["jne"][o1])).sum())


def _lib_run(p, b, store, interval, budget=False):
    """NSTEPS steps of the fused step; budget: the melt budget of the last step (test_melt_budget_closes_at_1e6; interval 0)"""
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(grid(), p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.set_store_environment(store)
        ib.set_resort_interval(interval)
        if budget:
            ib.run(NSTEPS - 1)
            before = ib.download_bergs()
            ib.run(1)
        else:
            ib.run(NSTEPS)
        acc, out, scal = ib.fetch()
        after = ib.download_bergs()
        if budget:
            assert np.array_equal(before["id"], after["id"])          # interval 0: rows stay put
            lost = before["mass_scaling"] * ((before["mass"] + before["mass_of_bits"]) - (after["mass"] + after["mass_of_bits"]))
            total_lost = float(np.sum(np.where(before["alive"] != 0, lost, 0.0)))
            received = float(np.sum(acc[T.ACC_NAMES["floating_melt"]] * grid()["static"]["area"])) * p.dt
            print("melt budget: lost %.17g received %.17g" % (total_lost, received))
            assert total_lost > 0.0
            assert abs(received - total_lost) <= 1.0e-9 * total_lost, (received, total_lost)
        return after, acc.copy(), out.copy(), scal.copy()
    finally:
        ib.close()


def _by_id(b):
    live = np.flatnonzero(b["alive"] != 0)
    o = live[np.argsort(b["id"][live], kind="stable")]
    return {f: b[f][o] for f in PER_BERG + ["id"]}


def _same_sums(got, ref, label):
    """acc and out of two row orders of the same live bergs: within SUM_TOL of the field's maximum"""
    for name, k in ((("acc", 1), ("out", 2))):
        for q in range(ref[k].shape[0]):
            scale = np.abs(ref[k][q]).max()
            err = np.abs(got[k][q] - ref[k][q]).max()
            assert err <= SUM_TOL * scale, "%s: %s plane %d differs by %.3e of its maximum %.3e" % (label, name, q, err / scale if scale else err, scale)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("C", sorted(BLOCKS))
def test_row_orders_agree_with_the_oracle_and_each_other(oracle, C, variant):
    p, pops = params(variant), populations(C)
    store = variant != "plain"
    runs = {}
    for order, interval in (("a", 0), ("b", 0), ("c", 0), ("d", 0), ("e", 0), ("b", 3)):
        b = pops[order]
        ref = oracle_run(C, variant, order)
        moved = cells_changed(b, ref[0])
        assert moved >= 20, (order, moved)            # the case's own coverage: the order does decay
        if not store:   # kid_set_store_environment(0): berg%uo .. hi stay as uploaded, everything else is compared
            rb = S.copy_bergs(ref[0])
            for f in P.ENV_FIELDS:
                rb[f] = pops["d" if order in ("d", "e") else "a"][f].copy()
            ref = (rb,) + tuple(ref[1:])
        label = "C=%d/%s/order %s/interval %d" % (C, variant, order, interval)
        got = _lib_run(p, b, store, interval, budget=(order == "b" and interval == 0))
        rep = P.compare(ref, got, label, params=p)      # (error_count = 0 is among its scalars)
        assert got[3][T.SCALAR_NAMES["error_count"]] == 0
        print(label, "moved", moved, "planes %.1e" % max(v for k, v in rep.items() if k.startswith(("acc", "out"))))
        runs[(order, interval)] = got
    first = _by_id(runs[("a", 0)][0])
    for key in (("b", 0), ("c", 0), ("b", 3)):
        other = _by_id(runs[key][0])
        for f in PER_BERG + ["id"]:
            assert np.array_equal(first[f], other[f]), (key, f)      # per-berg arithmetic does not see the order at all
        _same_sums(runs[key], runs[("a", 0)], "C=%d/%s/%s against a" % (C, variant, key))
    d, e = _by_id(runs[("d", 0)][0]), _by_id(runs[("e", 0)][0])
    keep = np.isin(first["id"], d["id"])
    for f in PER_BERG + ["id"]:
        assert np.array_equal(d[f], e[f]), f
        assert np.array_equal(d[f], first[f][keep]), f               # ... nor which other bergs are alive
    _same_sums(runs[("d", 0)], runs[("e", 0)], "C=%d/%s/d against e" % (C, variant))


def test_footloose_profile_matches_its_oracle(oracle):
    """K = 2, the hot build of the footloose profile (config 3 with FL bits): sparse bergs, many cells per wave"""
    grid3, p, b = S.config_c3(n=64 * 8 + 37, seed=3, fl_style="fl_bits")
    ref = P.run_oracle(grid3, p, b, 24)
    got = P.run_hip(grid3, p, b, 24)
    rep = P.compare(ref, got, "C3/fl_bits", params=p)
    assert got[3][T.SCALAR_NAMES["error_count"]] == 0
    n = ref[0]["_n"]
    assert cells_changed({k: (v[:n] if hasattr(v, "dtype") else v) for k, v in b.items()}, {k: (v[:n] if hasattr(v, "dtype") else v) for k, v in ref[0].items()}) >= 20
    print("C3/fl_bits planes %.1e" % max(v for k, v in rep.items() if k.startswith(("acc", "out"))))
