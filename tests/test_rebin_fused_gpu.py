"""The re-binning folded into the plain hot build that follows it (kid_move_berg_between_cells leaves the permutation
pending; berg_kernel<..., REBIN = true> reads its rows through it) against the eager copy (KID_REBIN_EAGER=1).

Every scenario runs twice in fresh child processes, default and eager, and the two results are compared:
* every per-berg member of every live berg, matched by id, bit for bit (row order never enters a berg's arithmetic);
  with KID_STABLE_RESORT set in both runs the row order is the same too and whole arrays are compared row for row;
* per-cell accumulators and gathered planes within 1e-11 of the plane's largest value: the bound the order-independence
  tests of tests/test_properties_gpu.py use for the same sums (summation order only);
* observers: what download, count, checksum, compaction, a phase-by-phase step and a step under a non-plain namelist see
  right after a re-binning, with no step in between.

No case may pass by falling back: kid_rebin_fused_count says how many re-binnings the hot build took over, and every default
run must show all the ones its schedule can fuse, every KID_REBIN_EAGER run none.  (The compile-time budget of the new
instantiations is tests/test_rebin_build_budget.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_TOL = 1.0e-11   # tests/test_properties_gpu.py, "per-cell sums: summation order only"

CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
from icebergs_amd import synthetic as S, types as T
from icebergs_amd.framework import Icebergs
sc = json.loads(sys.argv[1])
grid, p, b = S.config_c2(n=sc["n"], seed=sc["seed"])
n = sc["n"]
if sc.get("kill"):
    b["alive"][np.random.default_rng(11).choice(n, n // 20, replace=False)] = 0
if sc.get("fat"):   # members the plain step never touches, not zero: more moved fields than the kernel's head copies hold
    rng = np.random.default_rng(13)
    for name in ("uvel_old", "vvel_old", "uvel_prev", "vvel_prev", "axn_fast", "ayn_fast", "bxn_fast", "byn_fast", "ang_vel", "ang_accel", "rot"):
        b[name][:] = rng.standard_normal(n)
ib = Icebergs(grid, p, capacity=n)
ib.upload_bergs(b)
ib.set_store_environment(bool(sc["store_env"]))
extra = {}
mode = sc["mode"]
if mode == "run":
    ib.set_resort_interval(sc["interval"])
    ib.run(sc["steps"])
elif mode == "twice":
    ib.set_resort_interval(0)
    for _ in range(3):
        ib.run(4)
        ib.move_berg_between_cells()
        ib.move_berg_between_cells()
    ib.run(2)
else:   # observers: a re-binning, then `mode` with no step in between
    ib.set_resort_interval(0)
    ib.run(5)
    ib.move_berg_between_cells()
    if mode == "num":
        extra["num"] = np.array(ib.num_bergs(), dtype=np.int64)
    elif mode == "chksum":
        extra["chksum"] = np.array(ib.bergs_chksum(), dtype=np.int64)
    elif mode == "compact":
        ib.compact()
    elif mode == "phases":
        ib.run_phases(1)
    elif mode == "namelist":
        p.diag_mask = T.ENUMS["KID_DIAG_MASS"]
        ib.set_params(p)
        ib.run(1)
    else:
        assert mode == "download", mode
extra["redo"] = np.array([ib.last_redo_count()], dtype=np.int64)
extra["fused"] = np.array([ib.rebin_fused_count()], dtype=np.int64)
got = ib.download_bergs()
acc, out, scal = ib.fetch()
ib.close()
np.savez(sys.argv[2], acc=acc, out=out, scal=scal, **{"b_" + k: v for k, v in got.items() if hasattr(v, "dtype")}, **extra)
'''


def _run(tmp_path, tag, sc, eager, stable):
    env = {k: v for k, v in os.environ.items() if k not in ("KID_REBIN_EAGER", "KID_STABLE_RESORT")}
    if eager:
        env["KID_REBIN_EAGER"] = "1"
    if stable:
        env["KID_STABLE_RESORT"] = "1"
    path = str(tmp_path / (tag + ".npz"))
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, json.dumps(sc), path], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _fusable(sc):
    """re-binnings of the scenario that are followed by a fused RK4 step of the whole population (the ones the hot build can take)"""
    if sc["mode"] == "run":      # kid_run_step re-bins after every `interval` steps; the last one counts only if a step follows
        return (sc["steps"] - 1) // sc["interval"]
    if sc["mode"] == "twice":    # of two in a row the first is copied at once (the second sorts its rows), the second waits for the step
        return 3
    return 0                     # observers look before any step: the copy runs for them


def _compare(a, e, stable, dead_present=False, fused=None):
    """a: default (deferred) run, e: eager run"""
    assert int(e["fused"][0]) == 0, "KID_REBIN_EAGER run took the fused launch"
    if fused is not None:
        assert int(a["fused"][0]) == fused, "the default run fused %d re-binnings, its schedule has %d" % (int(a["fused"][0]), fused)
    members = sorted(k for k in a if k.startswith("b_"))
    assert members == sorted(k for k in e if k.startswith("b_")) and "b_id" in members and "b_alive" in members
    assert len(a["b_id"]) == len(e["b_id"]), "row counts differ"
    if stable:   # same permutation: the arrays are the same, dead rows included
        for k in members:
            assert np.array_equal(a[k], e[k], equal_nan=True), k
    la, le = a["b_alive"] != 0, e["b_alive"] != 0
    assert int(la.sum()) == int(le.sum()) > 0
    if dead_present:
        assert int(la.sum()) < len(la)
    oa, oe = np.flatnonzero(la)[np.argsort(a["b_id"][la], kind="stable")], np.flatnonzero(le)[np.argsort(e["b_id"][le], kind="stable")]
    assert np.array_equal(a["b_id"][oa], e["b_id"][oe])
    for k in members:
        assert np.array_equal(a[k][oa], e[k][oe], equal_nan=True), k          # bit for bit, berg by berg
    for name in ("acc", "out"):
        for q in range(a[name].shape[0]):
            scale = np.abs(e[name][q]).max()
            err = np.abs(a[name][q] - e[name][q]).max()
            assert err <= PLANE_TOL * scale, (name, q, err, scale)
    for k in ("num", "chksum"):
        if k in e:
            assert np.array_equal(a[k], e[k]), (k, a[k], e[k])


# n is never a multiple of the 64-thread workgroup.  300 001 bergs on the 360 x 200 grid: ~4 per cell, a wave spans more cells
# than it has packet slots, so a share of every wave goes to the general build on top of the bergs that cross a cell edge;
# 1 000 003: ~14 per cell, the headline's regime in small.  fat-rows: eleven more live members per berg, which the re-binning
# instance copies as `surplus` (kid_berg_kernel.hpp).
RUNS = {
    "k1-sparse": dict(n=300_001, seed=7, store_env=0, mode="run", interval=4, steps=14),
    "k1-dense": dict(n=1_000_003, seed=5, store_env=0, mode="run", interval=4, steps=14),
    "k3-store-env": dict(n=300_001, seed=8, store_env=1, mode="run", interval=4, steps=14),
    "k1-dead": dict(n=300_001, seed=9, store_env=0, mode="run", interval=3, steps=11, kill=1),
    "k3-dead": dict(n=300_001, seed=9, store_env=1, mode="run", interval=3, steps=11, kill=1),
    "k1-fat-rows": dict(n=300_001, seed=14, store_env=0, mode="run", interval=4, steps=14, fat=1, kill=1),
    "k3-fat-rows": dict(n=300_001, seed=14, store_env=1, mode="run", interval=4, steps=14, fat=1, kill=1),
    "k1-twice": dict(n=300_001, seed=10, store_env=0, mode="twice"),
    "k3-twice": dict(n=300_001, seed=10, store_env=1, mode="twice"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("stable", [False, True], ids=["counting-sort", "stable-resort"])
@pytest.mark.parametrize("case", sorted(RUNS))
def test_fused_rebinning_matches_eager(tmp_path, case, stable):
    sc = RUNS[case]
    a = _run(tmp_path, "deferred", sc, eager=False, stable=stable)
    e = _run(tmp_path, "eager", sc, eager=True, stable=stable)
    assert int(e["redo"][0]) > 0, "no berg went to the general build: the case does not exercise the bail path"
    assert _fusable(sc) >= 3
    _compare(a, e, stable, dead_present=bool(sc.get("kill")), fused=_fusable(sc))


@pytest.mark.gpu
@pytest.mark.parametrize("store_env", [0, 1], ids=["k1", "k3"])
@pytest.mark.parametrize("mode", ["download", "num", "chksum", "compact", "phases", "namelist"])
def test_observers_see_the_eager_state(tmp_path, mode, store_env):
    """KID_STABLE_RESORT in both runs: the row order is the same, so whatever the observer returns is compared as it is"""
    sc = dict(n=300_001, seed=12, store_env=store_env, mode=mode, kill=1)
    a = _run(tmp_path, "deferred", sc, eager=False, stable=True)
    e = _run(tmp_path, "eager", sc, eager=True, stable=True)
    _compare(a, e, stable=True, fused=0)
