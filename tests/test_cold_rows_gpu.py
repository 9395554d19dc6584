"""Cold fields (csrc/kid_rows_plan.hpp): a re-binning of a handle whose step is the plain fused launch leaves the members that
step never touches where they are and moves `origin` instead; whoever reads them by row gets them gathered first.  Held
against the same library with KID_COLD_EAGER=1, in which no field is cold.

Every scenario runs in two child processes, default and KID_COLD_EAGER, and the two results are compared row by row after
sorting by id: every member of download_bergs() bit for bit, dead rows included, and -- in the scenarios whose population
never puts more than two bergs into a cell -- every accumulator plane, gathered plane and scalar bit for bit as well (one or
two terms add to the same bits in either order, tests/test_zero_fields_gpu.py; a denser population compares members only).

Population: config-2 physics on a 24 x 16 lat-lon grid of 400 m cells under a uniform current of (0.55, 0.4) m/s and
dt = 600 s, so that a berg crosses a cell edge in most steps and goes to the general build (the child counts them), bergs
leave the domain through the east and north edges and die, and a tenth of the bergs are thin enough to melt within the run.
dense: 3001 bergs, eight per cell on average; sparse: one berg in every second cell of every second row and a second one in
every fifth of those, 100 bergs of one class, which drift together.

No scenario may pass by falling back: kid_cold_state says whether fields are deferred and how many times they were gathered;
the default child must show them deferred before the first read, the KID_COLD_EAGER child never.

One child process runs all the scenarios of one environment, so the suite pays for two processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, tempfile
sys.path.insert(0, %(root)r)
import numpy as np
from icebergs_amd import synthetic as S, types as T
from icebergs_amd.framework import Icebergs
scenarios, path = json.loads(sys.argv[1]), sys.argv[2]
NI, NJ, DT = 24, 16, 600.0
COLD_F64 = ["start_lon", "start_lat", "start_day", "start_mass", "uvel_old", "vvel_old", "lon_old", "lat_old", "uvel_prev", "vvel_prev",
            "axn_fast", "ayn_fast", "bxn_fast", "byn_fast", "ang_vel", "ang_accel", "rot"]
COLD_I32 = ["start_year", "n_bonds", "conglom_id"]

def setup(kind, distinctive=False):
    grid = S.c2_forcing(S.latlon_grid(ni=NI, nj=NJ, lon0=10.0, dlon=0.0072, lat0=-60.0, dlat=0.0036))
    grid["forcing"]["uo"][:] = 0.55
    grid["forcing"]["vo"][:] = 0.4
    p = S.default_params()
    p.dt = DT
    if kind == "dense":
        b = S.place_bergs(grid, 3001, 21, (2, NI - 1), (2, NJ - 1))
    else:   # sparse: a lattice, one class
        cells = [(i, j) for j in range(2, NJ, 2) for i in range(2, NI, 2)]
        cells += cells[::5]
        n = len(cells)
        b = S.place_bergs(grid, n, 22, (2, 2), (2, 2), klass=np.full(n, 4))
        d, st = grid["desc"], grid["static"]
        ine, jne = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
        lon0, lon1 = st["lon"][jne - d.jsd, ine - 1 - d.isd], st["lon"][jne - d.jsd, ine - d.isd]
        lat0, lat1 = st["lat"][jne - 1 - d.jsd, ine - d.isd], st["lat"][jne - d.jsd, ine - d.isd]
        b["ine"][:], b["jne"][:] = ine, jne
        b["lon"][:], b["lat"][:] = lon0 + b["xi"] * (lon1 - lon0), lat0 + b["yj"] * (lat1 - lat0)
        b["start_lon"][:], b["start_lat"][:], b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"], b["lon"], b["lat"]
        assert n > 64 and np.unique(jne * 1000 + ine, return_counts=True)[1].max() == 2
    n = len(b["lon"])
    b["uvel"][:], b["vvel"][:] = 0.55, 0.4
    thin = np.arange(n) %% 10 == 3            # ... melt within the run
    b["thickness"][thin], b["width"][thin], b["length"][thin] = 0.02, 0.5, 0.75
    b["mass"][thin] = p.rho_bergs * 0.02 * 0.5 * 0.75
    rng = np.random.default_rng(23)
    order = rng.permutation(n)                # uploaded shuffled: the first re-binning moves every row
    for k in list(b):
        b[k] = np.ascontiguousarray(b[k][order])
    if distinctive:                           # something else than zeros, and different in every row, in every member the step leaves alone
        for name in COLD_F64:
            b[name][:] = 1.0 + rng.random(n) + 1.0e-3 * np.arange(n)
        for name in COLD_I32:
            b[name][:] = rng.integers(1, 1 << 30, n)
        b["id"][:] = (rng.permutation(n).astype(np.int64) << 32) + 12345
    return grid, p, b

def run(sc):
    grid, p, b = setup(sc["kind"], bool(sc.get("distinctive")))
    n = len(b["lon"])
    if sc.get("diag"):
        p.diag_mask = T.ENUMS[sc["diag"]]
    cap = 2 * n
    ib = Icebergs(grid, p, capacity=cap)
    ib.upload_bergs(b)
    ib.set_store_environment(bool(sc.get("store_env")))
    ib.set_resort_interval(0)
    extra, states = {}, []
    redo = 0
    def steps(k):
        nonlocal redo
        for _ in range(k):
            ib.run(1); redo += ib.last_redo_count()
    def rebin():
        ib.move_berg_between_cells(); states.append(list(ib.cold_state()))
    for _ in range(3):                         # three re-binnings, two steps apart; nothing reads a row in between
        steps(2); rebin()
    steps(1)
    before = ib.cold_state()
    reader = sc.get("reader")
    if reader == "download":
        extra["r_mass"] = np.sort(ib.download_bergs()["start_mass"])
    elif reader == "restart":
        with tempfile.TemporaryDirectory() as tmp:
            ib.write_restart(tmp)
            extra["r_files"] = np.array([len(os.listdir(tmp))])
    elif reader == "chksum":
        extra["r_chk"] = np.array(ib.bergs_chksum(), dtype=np.int64)
    elif reader == "chksum_device":
        extra["r_chk"] = np.array(ib.bergs_chksum_device(), dtype=np.int64)
    elif reader == "traj":
        tp = T.TrajParams()
        tp.traj_area_thres, tp.traj_area_thres_sntbc, tp.traj_area_thres_fl, tp.save_all_traj_year = 0.0, 0.0, 1.0e9, 1.0e30
        tp.save_short_traj, tp.save_fl_traj, tp.save_nonfl_traj_by_class = 1, 1, 0
        ib.set_traj_params(tp)
        before = ib.cold_state()
        ib.record_posn()
        extra["r_traj"] = np.array([ib.num_traj_records()])
    elif reader == "budget":
        extra["r_budget"] = np.array([v for _, v in sorted(ib.budget().items())], dtype=np.float64)
    elif reader == "emigrants":
        rec = ib.pack_emigrants(T.ENUMS["KID_DIR_E"])
        extra["r_emig"] = rec[np.lexsort(rec.T[::-1])] if len(rec) else rec
    elif reader == "calving":
        ib.set_calving_params(S.calving_params(p))
        before = ib.cold_state()
        calv, hflx = S.coupler_calving(grid, seed=5, frac=0.2, dt=DT)
        scal = ib.calving(calv, hflx)
        extra["r_calved"] = np.array([scal[T.ENUMS["KID_CS_NBERGS_CALVED"]]])
    elif reader == "reserve":
        ib.reserve(3 * n)
    elif reader == "compact":
        ib.compact()
    elif reader == "count_tail":               # a re-binning just sorted the dead to the tail: the count drops them
        rebin()
        before = ib.cold_state()
        extra["r_num"] = np.array(ib.num_bergs(), dtype=np.int64)
    elif reader == "count_plain":              # after a step nothing is known about a tail: the count moves nothing
        extra["r_num"] = np.array(ib.num_bergs(), dtype=np.int64)
    elif reader == "rebin":
        ib.move_berg_between_cells()
    elif reader == "upload":
        grid2, p2, b2 = setup(sc["kind"], True)
        ib.upload_bergs(b2)
    elif reader == "params_diag":
        q = S.params_copy(p); q.diag_mask = T.ENUMS["KID_DIAG_MELT_BY_CLASS"]; ib.set_params(q)
    elif reader == "params_general":
        q = S.params_copy(p); q.bergy_bit_erosion_fraction = 0.5; ib.set_params(q)
    else:
        assert reader is None, reader
    after = ib.cold_state()
    steps(2); rebin(); steps(2)
    fused = ib.rebin_fused_count()
    mid = ib.cold_state()
    got = ib.download_bergs()
    acc, outp, scal = ib.fetch()
    end = ib.cold_state()
    ib.close()
    extra.update(acc=acc.copy(), out=outp.copy(), scal=scal.copy(), redo=np.array([redo]), fused=np.array([fused]), n0=np.array([n]),
                 states=np.array(states, dtype=np.int64), before=np.array(before, dtype=np.int64), after=np.array(after, dtype=np.int64),
                 mid=np.array(mid, dtype=np.int64), end=np.array(end, dtype=np.int64))
    extra.update({"b_" + k: v for k, v in got.items() if hasattr(v, "dtype")})
    return extra

out = {}
for name, sc in scenarios.items():
    for k, v in run(sc).items():
        out[name + "/" + k] = v
np.savez(path, **out)
'''

# reader -> times the call gathers the cold fields (0: it must leave them deferred)
READERS = {"download": 1, "restart": 1, "chksum": 1, "chksum_device": 1, "traj": 1, "budget": 1, "emigrants": 1, "calving": 1, "reserve": 1,
           "compact": 1, "count_tail": 1, "upload": 1, "params_diag": 1, "params_general": 1, "count_plain": 0, "rebin": 0}
SCENARIOS = {
    "dense-k1": dict(kind="dense", store_env=0),
    "dense-k3": dict(kind="dense", store_env=1),
    "sparse-k1": dict(kind="sparse", store_env=0),
    "sparse-k3": dict(kind="sparse", store_env=1),
    "set-k1": dict(kind="sparse", store_env=0, distinctive=1),
    "set-k3": dict(kind="sparse", store_env=1, distinctive=1),
    "set-melt-by-class": dict(kind="sparse", store_env=0, distinctive=1, diag="KID_DIAG_MELT_BY_CLASS"),
}
SCENARIOS.update({"reader-" + r: dict(kind="dense", store_env=0, reader=r) for r in READERS})


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cold_rows")
    env = {k: v for k, v in os.environ.items() if k not in ("KID_COLD_EAGER", "KID_REBIN_EAGER", "KID_STABLE_RESORT", "KID_NO_PLAIN_BUILD")}
    res = {}
    for eager in (False, True):
        e = dict(env, KID_COLD_EAGER="1") if eager else env
        path = str(tmp / ("eager.npz" if eager else "deferred.npz"))
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, json.dumps(SCENARIOS), path], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(path) as z:
            res[eager] = {k: z[k] for k in z.files}
    return res


def _case(res, case):
    return {k[len(case) + 1:]: v for k, v in res.items() if k.startswith(case + "/")}


def _members_equal(a, e, what):
    """every member of every row, dead ones included, matched by id, bit for bit"""
    members = sorted(k for k in a if k.startswith("b_"))
    assert members == sorted(k for k in e if k.startswith("b_")) and "b_id" in members and "b_start_mass" in members and "b_conglom_id" in members
    assert len(a["b_id"]) == len(e["b_id"]) > 0, (what, "row counts differ", len(a["b_id"]), len(e["b_id"]))
    oa, oe = np.argsort(a["b_id"], kind="stable"), np.argsort(e["b_id"], kind="stable")
    assert np.array_equal(a["b_id"][oa], e["b_id"][oe]) and len(np.unique(a["b_id"])) == len(a["b_id"]), what
    for k in members:
        assert np.array_equal(a[k][oa], e[k][oe], equal_nan=True), (what, k, int((a[k][oa] != e[k][oe]).sum()))


def _sums_equal(a, e, what):
    for c in (a, e):   # the precondition of a bit-for-bit comparison of the sums (module docstring): the cells the last step's sums were keyed by.
        # A row whose cell lies outside the 24 x 16 domain left it in the evolve and added nothing to any sum in that step or since;
        # a dead row inside melted there, perhaps in the last step: it counts
        term = (c["b_alive"] != 0) | ((c["b_ine"] >= 1) & (c["b_ine"] <= 24) & (c["b_jne"] >= 1) & (c["b_jne"] <= 16))
        assert int(term.sum()) > 16
        occupancy = np.unique(c["b_jne"][term].astype(np.int64) * 100000 + c["b_ine"][term], return_counts=True)[1]
        assert occupancy.max() <= 2, (what, "a cell ended with %d bergs: the order of its three atomics is not fixed" % occupancy.max())
    for k in ("acc", "out", "scal"):
        assert a[k].shape == e[k].shape and np.array_equal(a[k], e[k], equal_nan=True), (what, k, int((a[k] != e[k]).sum()))
    assert np.abs(a["acc"]).max() > 0


def _exercised(a, e, what):
    """the scenario did what the comparison is about: bergs crossed cells, some died -- melted inside the domain among them --
    and the cold fields were deferred behind a permutation before anything read them (never in the KID_COLD_EAGER child)"""
    n0 = int(a["n0"][0])
    print("%s: %d bergs, %d general-build rows in 11 steps, %d rows left, %d of them dead, %d re-binnings fused" %
          (what, n0, int(a["redo"][0]), len(a["b_id"]), int((a["b_alive"] == 0).sum()), int(a["fused"][0])))
    dead = a["b_alive"] == 0
    melted = int((dead & (a["b_ine"] >= 1) & (a["b_ine"] <= 24) & (a["b_jne"] >= 1) & (a["b_jne"] <= 16)).sum())
    print("%s: %d dead rows inside the domain (melted)" % (what, melted))
    assert n0 > 64
    if "upload" not in what and "compact" not in what and "count_tail" not in what:   # (those replace or drop the rows that melted early)
        assert melted > 0, (what, "no berg melted")
    assert int(a["redo"][0]) >= 11 * n0 // 4, (what, "too few bergs change cells for the general build to matter", int(a["redo"][0]))
    assert len(a["b_id"]) < n0 or int((a["b_alive"] == 0).sum()) > 0, (what, "no berg died: no dead tail")
    assert a["states"][:3, 0].tolist() == [1, 1, 1] and a["states"][:3, 1].tolist() == [0, 0, 0], (what, a["states"])   # deferred, never gathered
    assert a["before"].tolist() == [1, 0], (what, a["before"])
    assert int(a["fused"][0]) >= 3
    for k in ("states", "before", "after", "mid", "end"):
        assert not e[k].any(), (what, "the KID_COLD_EAGER child deferred or gathered something", k, e[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dense-k1", "dense-k3", "sparse-k1", "sparse-k3"])
def test_deferred_matches_eager(runs, case):
    """Test 1 of the round: three re-binnings two steps apart, then the first read"""
    a, e = _case(runs[False], case), _case(runs[True], case)
    _exercised(a, e, case)
    assert a["mid"].tolist() == [1, 0] and a["end"].tolist() == [0, 1], (case, a["mid"], a["end"])   # the download gathered them, once
    _members_equal(a, e, case)
    if case.startswith("sparse"):
        _sums_equal(a, e, case)


@pytest.mark.gpu
@pytest.mark.parametrize("reader", sorted(READERS))
def test_every_reader_materialises_once(runs, reader):
    """Test 2: one entry point between two re-binnings, stepping on afterwards"""
    case = "reader-" + reader
    a, e = _case(runs[False], case), _case(runs[True], case)
    _exercised(a, e, case)
    gathered = int(a["after"][1]) - int(a["before"][1])
    assert gathered == READERS[reader], (reader, "gathered %d times" % gathered, a["before"], a["after"])
    assert int(a["after"][0]) == (0 if READERS[reader] else 1), (reader, a["after"])
    _members_equal(a, e, case)
    for k in sorted(k for k in a if k.startswith("r_")):
        if k == "r_budget":   # sums over all bergs in the order of the rows
            assert np.allclose(a[k], e[k], rtol=1.0e-12, atol=0.0, equal_nan=True), (reader, a[k], e[k])
        else:
            assert np.array_equal(a[k], e[k], equal_nan=True), (reader, k, a[k], e[k])
    if reader in ("count_tail",):
        assert a["r_num"][0] == a["r_num"][1], "the dead tail was not dropped"
    if reader == "calving":
        assert a["r_calved"][0] > 0
    if reader == "emigrants":
        assert len(a["r_emig"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["set-k1", "set-k3", "set-melt-by-class"])
def test_cold_set_is_right(runs, case):
    """Test 3: distinctive values in every member the plain step leaves alone.  A kernel of the step that read one of them by
    row would compute something else than the KID_COLD_EAGER child; with the melt-by-class diagnostic the step reads start_mass,
    which must then be in row order."""
    a, e = _case(runs[False], case), _case(runs[True], case)
    if case == "set-melt-by-class":   # the diagnostic is not in the plain namelist: nothing may be deferred at all
        for k in ("states", "before", "after", "mid", "end"):
            assert not a[k].any() and not e[k].any(), (case, k, a[k], e[k])
    else:
        _exercised(a, e, case)
    _members_equal(a, e, case)
    _sums_equal(a, e, case)
    for k in ("b_start_mass", "b_rot", "b_conglom_id", "b_n_bonds"):
        assert a[k].all(), (case, k)
