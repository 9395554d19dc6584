"""Reproducible per-cell sums (kid_set_reproducible_sums, the device side of parallel_reprod; icebergs_amd/csrc/kid_repro.inc).

With the switch on, every accumulator plane, output plane and step scalar is a function of the set of bergs only: the same
bergs uploaded in another row order, re-binned at another interval, compacted mid-run, stepped fused or phase by phase give
the same bits.  Each per-cell sum is the reference's: a left fold of the bergs' terms in `inorder` order (start_year,
start_day, start_mass, start_lon, start_lat, then the id), checked bit for bit against the oracle on the exact-math build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from icebergs_amd import synthetic as S
import parity as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.path.join(ROOT, "icebergs_amd", "csrc", "libkid_hip_exact.so")
KID_EUNSUPPORTED = -5
FIELDS = P.TRAJ_FIELDS + P.SIZE_FIELDS + ["ine", "jne"]


def _permuted(b, perm):
    out = {k: (v[perm].copy() if isinstance(v, np.ndarray) and v.shape[:1] == b["lon"].shape else v) for k, v in b.items()}
    return out


def _cell_sorted(b):
    return _permuted(b, np.lexsort((b["id"], b["ine"], b["jne"])))


def _shuffled(b, seed=99):
    return _permuted(b, np.random.default_rng(seed).permutation(len(b["lon"])))


def _run(grid, p, b, nsteps, repro=True, resort=16, compact_at=None, calving=None, phases=False, capacity=None):
    """nsteps of the fused step (or the phase-by-phase calls); returns (bergs by id, acc, out, scalars)"""
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(grid, p, capacity=capacity or len(b["lon"]))
    try:
        ib.set_resort_interval(resort)
        if repro:
            ib.set_reproducible_sums(True)
        if calving is not None:
            ib.set_calving_params(calving)
        ib.upload_bergs(b)
        for step in range(nsteps):
            if calving is not None:
                calv, hflx = S.coupler_calving(grid, seed=step % 3, frac=0.03)
                ib.calving(calv, hflx)
            if phases:
                ib.run_phases(1)   # (kid_create_gridded_icebergs_fields ends with the gather)
            else:
                ib.run(1)
            if compact_at == step:
                ib.compact()
        acc, out, scal = ib.fetch()
        got = ib.download_bergs()
    finally:
        ib.close()
    live = np.nonzero(got["alive"] != 0)[0]
    live = live[np.argsort(got["id"][live])]
    return {f: got[f][live].copy() for f in FIELDS + ["id"]}, acc.copy(), out.copy(), scal.copy()


def _assert_same(a, c, label):
    assert np.array_equal(a[0]["id"], c[0]["id"]), label + ": survivors differ"
    for f in FIELDS:
        assert np.array_equal(a[0][f], c[0][f]), (label, f)
    for k in range(a[1].shape[0]):
        assert np.array_equal(a[1][k], c[1][k]), (label, "acc plane %d" % k, P.rel_err(a[1][k], c[1][k]))
    for k in range(a[2].shape[0]):
        assert np.array_equal(a[2][k], c[2][k]), (label, "out plane %d" % k)
    assert np.array_equal(a[3], c[3]), (label, "scalars", a[3], c[3])


def _c2(verlet=False, hexagonal=False, new_order=False, static=False, spread_melt=False, no_decay=False, taw=False, heat=False):
    grid, p, b = S.config_c2(n=40000, seed=21, continents=True)
    S.set_diag_all(p)
    if verlet:
        p.Runge_not_Verlet, p.use_new_predictive_corrective = 0, 1
    if hexagonal:
        p.hexagonal_icebergs = 1
    if new_order:
        p.old_interp_flds_order = 0
    if static:
        b["static_berg"][::9] = 1.0
    if spread_melt:
        p.find_melt_using_spread_mass = 1
        p.Iceberg_melt_without_decay = 1 if no_decay else 0
    if taw:
        p.add_weight_to_ocean, p.time_average_weight = 1, 1
    if heat:   # calving_hflx and net_heat_to_ocean (every BASELINE config carries no heat)
        b["heat_density"][:] = 3.0e5
    return grid, p, b


CASES = {
    "rk4-rect": (dict(), 0, None),
    "verlet-rect-neworder": (dict(verlet=True, new_order=True), 1, None),
    "rk4-hex-static-heat": (dict(hexagonal=True, static=True, heat=True), 5, 3),
    "verlet-hex-taw": (dict(verlet=True, hexagonal=True, taw=True), 1, None),
    "spread-melt": (dict(spread_melt=True), 5, None),
    "spread-melt-no-decay": (dict(spread_melt=True, no_decay=True), 0, 4),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_row_order_invariance(oracle, case):
    kw, resort, compact_at = CASES[case]
    grid, p, b = _c2(**kw)
    a = _run(grid, p, _cell_sorted(b), 8, resort=3 if resort == 0 else 0)   # another re-binning interval than the shuffled run's
    c = _run(grid, p, _shuffled(b), 8, resort=resort, compact_at=compact_at)
    _assert_same(a, c, case)
    if case == "rk4-rect":   # control: the default sums do see the row order, so the test can see a difference
        d = _run(grid, p, _shuffled(b), 8, repro=False, resort=resort)
        assert not np.array_equal(a[1], d[1]), "the default path gave the same planes: the control cannot tell orders apart"


def test_row_order_invariance_with_calving(oracle):
    grid, p, b = S.config_c2(n=40000, seed=23, continents=True)
    S.set_diag_all(p)
    p.current_year, p.current_yearday = 7, 123.25
    cp = S.calving_params(p, tau_calving=0.0, restarted=False)
    cap = 400000
    a = _run(grid, p, _cell_sorted(b), 8, resort=5, calving=cp, capacity=cap)
    c = _run(grid, p, _shuffled(b), 8, resort=1, calving=cp, capacity=cap, compact_at=4)
    assert len(a[0]["id"]) > 40000, "the calving source must add bergs"
    _assert_same(a, c, "calving")


def test_phases_equal_fused_bitwise(oracle):
    grid, p, b = S.config_c2(n=20000, seed=7)
    S.set_diag_all(p)
    a = _run(grid, p, b, 5)
    c = _run(grid, p, b, 5, phases=True)
    _assert_same(a, c, "phases vs fused")


@pytest.mark.parametrize("verlet", [False, True])
def test_same_per_berg_arithmetic(oracle, verlet):
    """plain namelist: the berg state is that of the default path bit for bit, the planes agree to summation order"""
    grid, p, b = S.config_c2(n=20000, seed=5)
    if verlet:
        p.Runge_not_Verlet = 0
    on = _run(grid, p, b, 6)
    off = _run(grid, p, b, 6, repro=False)
    assert np.array_equal(on[0]["id"], off[0]["id"])
    for f in FIELDS:
        assert np.array_equal(on[0][f], off[0][f]), f
    for k in range(on[1].shape[0]):
        assert P.rel_err(on[1][k], off[1][k]) <= 1e-12, k
    for k in range(on[2].shape[0]):
        assert P.rel_err(on[2][k], off[2][k]) <= 1e-12, k
    ref = P.run_oracle(grid, p, b, 6)
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.set_reproducible_sums(True)
        ib.upload_bergs(b)
        ib.run(6)
        acc, out, scal = ib.fetch()
        got = (ib.download_bergs(), acc.copy(), out.copy(), scal.copy())
    finally:
        ib.close()
    P.compare(ref, got, "repro/verlet=%s" % verlet, params=p)


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/oracle"); sys.path.insert(0, %(root)r + "/tests")
from icebergs_amd import synthetic as S, lib
from icebergs_amd.framework import Icebergs
import parity as P
assert b"exact-math" in lib.load().kid_version(), lib.load().kid_version()
out = {}
for name, verlet, zero in (("rk4", False, True), ("verlet", True, True), ("rk4-melt", False, False), ("verlet-melt", True, False)):
    grid, p, b = S.config_c1(n=3000, seed=3)
    S.set_diag_all(p)
    if verlet:
        p.Runge_not_Verlet, p.old_bug_bilin = 0, 0
    p.set_melt_rates_to_zero = 1 if zero else 0
    res = []
    for nsteps in (1, 3, 8):
        ref = P.run_oracle(grid, p, b, nsteps)
        ib = Icebergs(grid, p, capacity=len(b["lon"]))
        ib.set_reproducible_sums(True)
        ib.upload_bergs(b)
        ib.run(nsteps)
        acc, o, scal = ib.fetch()
        ib.close()
        diff = []
        for k in range(acc.shape[0]):
            if not np.array_equal(acc[k], ref[1][k]):
                diff.append(["acc", k, P.rel_err(acc[k], ref[1][k])])
        for k in range(o.shape[0]):
            if not np.array_equal(o[k], ref[2][k]):
                diff.append(["out", k, P.rel_err(o[k], ref[2][k])])
        if not np.array_equal(scal, ref[3]):
            diff.append(["scalars", -1, P.rel_err(scal, ref[3])])
        res.append({"nsteps": nsteps, "diff": diff, "mass_on_ocean_max": float(np.abs(acc[10:19]).max())})
    out[name] = res
print("RESULT " + json.dumps(out))
'''


def test_oracle_order_bit_for_bit(oracle):
    """exact-math build, config 1 with thousands of bergs on 13 x 13 cells (many per cell): with the melt rates zeroed every
    plane, output and scalar is the oracle's bit for bit after 1, 3 and 8 steps; with melt on within 1e-14 after 1 and 3
    steps and 1e-13 after 8 (pow differs in the last bit between the device and the host libm)"""
    assert os.path.exists(EXACT), "libkid_hip_exact.so is not built (build() makes it)"
    env = dict(os.environ, KID_HIP_SO=EXACT)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    print(json.dumps(out))
    for case, res in out.items():
        for step in res:
            assert step["mass_on_ocean_max"] > 0
            if case.endswith("-melt"):
                # the melt laws' pow is ocml's here, glibc's in the oracle: the bergs' masses drift apart by an ulp now and
                # then, and the melt planes (differences of masses) follow; the sums themselves add in the same order
                tol = 1e-14 if step["nsteps"] <= 3 else 1e-13
                assert all(d[2] <= tol for d in step["diff"]), (case, step)
            else:
                assert not step["diff"], (case, step)


@pytest.mark.parametrize("switch", ["mts", "interactive_icebergs_on", "footloose"])
def test_refusals(switch):
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=2000, seed=3)
    q = S.params_copy(p)
    q.Runge_not_Verlet = 0
    if switch == "mts":
        q.mts, q.old_interp_flds_order, q.mts_sub_steps, q.max_bonds = 1, 0, 1, 4
    elif switch == "interactive_icebergs_on":
        q.interactive_icebergs_on, q.max_bonds = 1, 4
    else:
        q.footloose, q.use_operator_splitting = 1, 1
    # turned on while the switch is set
    ib = Icebergs(grid, q, capacity=len(b["lon"]))
    try:
        rc = ib.lib.kid_set_reproducible_sums(ib.h, 1)
        msg = ib.lib.kid_last_error(ib.h).decode()
        assert rc == KID_EUNSUPPORTED and switch in msg, (rc, msg)
    finally:
        ib.close()
    # the switch set later through kid_set_params: refused at the step
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.set_reproducible_sums(True)
        ib.upload_bergs(b)
        ib.run(1)
        ib.set_params(q)
        rc = ib.lib.kid_run_step(ib.h, 1)
        msg = ib.lib.kid_last_error(ib.h).decode()
        assert rc == KID_EUNSUPPORTED and switch in msg, (rc, msg)
        # switched off (and the namelist back): the handle steps normally
        ib.set_params(p)
        ib.set_reproducible_sums(False)
        ib.run(2)
        got = ib.download_bergs()
    finally:
        ib.close()
    ref = _run(grid, p, b, 3, repro=False)
    live = np.nonzero(got["alive"] != 0)[0]
    live = live[np.argsort(got["id"][live])]
    assert np.array_equal(got["id"][live], ref[0]["id"])
    for f in P.TRAJ_FIELDS:
        assert np.array_equal(got[f][live], ref[0][f]), f
