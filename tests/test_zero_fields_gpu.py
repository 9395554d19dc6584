"""The plain hot builds skip the per-berg fields a launch knows to hold zeros (axn, ayn, mass_of_bits, heat_density: Redo::zero,
kid_rows_plan.hpp) against the same library with KID_NO_ZERO_SKIP=1, which loads and stores everything.

Every scenario runs in two fresh child processes, default and KID_NO_ZERO_SKIP, both with KID_STABLE_RESORT (same row order):
S.config_c2(n = 4096 + 37), 8 steps, a re-binning after step 4.  Every downloaded berg member, every accumulator plane, every
gathered plane and every scalar must compare equal (np.array_equal) between the two, row for row and cell for cell.

The planes in a form that is deterministic.  A plane's cell is the sum of the terms of the bergs IN that cell (every cell_add
of the thermodynamics and of the spreading is keyed by the berg's own cell; the nine spreading slots are planes of their own,
which the gather folds in a fixed order), and the waves add their partial sums with atomics in whatever order they arrive.
From zero, one or two terms give the same bits in either order (a + b = b + a); three or more need not, and with a seed
that put three bergs into some cell np.array_equal on the planes failed once in 24 pairs of runs of the SAME binaries (one
cell of one plane, equal again in the next run).  The population is therefore one in which no cell ever holds more than two
bergs: seed 7 of S.config_c2 at this size (118 cells with two), checked by the child at the upload and by the test on the
cells of the downloaded rows, dead ones included -- the cells that the last step's sums were keyed by.  The dynamics are
bit-reproducible, so this holds in every run or in none.

No case may pass by falling back:
kid_hot_zero_mask says which fields the last hot build skipped, it is recorded after every step and held to what the rule
gives for the scenario; the KID_NO_ZERO_SKIP child must show 0 throughout.  (The rule alone: tests/test_zero_fields_cpu.py.)

One child process runs all the scenarios of one environment, so the suite pays for four processes, not twenty."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096 + 37
ACCEL = {"axn", "ayn"}
ALL = ACCEL | {"mass_of_bits", "heat_density"}
SEED = 7             # no cell of S.config_c2(n=N, seed=SEED) holds more than two bergs (module docstring)

CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
from icebergs_amd import synthetic as S, types as T
from icebergs_amd.framework import Icebergs
cases, path = json.loads(sys.argv[1]), sys.argv[2]
N = %(n)d
out = {}
for case in cases:
    grid, p, b = S.config_c2(n=N, seed=%(seed)d)
    assert np.unique(b["jne"].astype(np.int64) * 100000 + b["ine"], return_counts=True)[1].max() == 2, "the seed's population: two bergs per cell at most, and some cells with two"
    masks, moved = [], []
    def rebin():   # ... and the fp64 members the permutation moved (kid_perm_moved_fields: a hook for tests, not in include/kid.h)
        ib.move_berg_between_cells()
        fn = ib.lib.kid_perm_moved_fields
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_int64)], C.c_int
        c = C.c_int64(-1)
        assert fn(ib.h, C.byref(c)) == 0
        moved.append(c.value)
    if case == "axn-uploaded":
        b["axn"][1234] = 1.0e-6
    elif case == "neg-zero":
        b["ayn"][4000] = -0.0
    elif case == "heat-density":
        b["heat_density"][77] = 3.0e5
    elif case == "dead-rows":
        b["alive"][np.random.default_rng(5).choice(N, N // 16, replace=False)] = 0
        b["alive"][128:192] = 0          # one wave of the hot build with no live row
    ib = Icebergs(grid, p, capacity=N)
    side = None
    if case in ("two-halves", "slow-lane"):
        ib.set_stream(torch.cuda.current_stream().cuda_stream)
        side = torch.cuda.Stream(torch.device("cuda", 0))
        ib.set_side_stream(side.cuda_stream, 1 if case == "two-halves" else 2)
    ib.set_resort_interval(0)
    ib.set_store_environment(case == "store-env")
    if case == "repro":
        ib.set_reproducible_sums(True)
    if case == "sequence":   # every row with axn, ayn and bits: the first re-binning moves the three fields into the second set of arrays
        b0 = S.copy_bergs(b)
        rng = np.random.default_rng(3)
        for name in ("axn", "ayn", "mass_of_bits"):
            b0[name][:] = 1.0e-7 * rng.standard_normal(N) if name != "mass_of_bits" else 1.0e3 * rng.random(N)
        ib.upload_bergs(b0)
        for s in range(2):
            ib.run(1); masks.append(sorted(ib.hot_zero_mask()))
        rebin()
        ib.run(1); masks.append(sorted(ib.hot_zero_mask()))
    ib.upload_bergs(b)
    def steps(k):
        for _ in range(k):
            ib.run(1); masks.append(sorted(ib.hot_zero_mask()))
    def with_params(change, k):
        q = S.params_copy(p)
        change(q)
        ib.set_params(q)
        steps(k)
        ib.set_params(p)
    if case == "erosion":
        with_params(lambda q: setattr(q, "bergy_bit_erosion_fraction", 0.5), 2)
        steps(2)
    elif case == "verlet":
        with_params(lambda q: setattr(q, "Runge_not_Verlet", 0), 2)
        steps(2)
    else:
        steps(4)
    rebin()
    steps(4)
    ib.sync()
    torch.cuda.synchronize()
    got = ib.download_bergs()
    acc, outp, scal = ib.fetch()
    fused = ib.rebin_fused_count()
    ib.close()
    out.update({case + "/acc": acc.copy(), case + "/out": outp.copy(), case + "/scal": scal.copy(), case + "/fused": np.array([fused], dtype=np.int64),
                case + "/masks": np.array([json.dumps(masks)]), case + "/moved": np.array(moved, dtype=np.int64)})
    out.update({case + "/b_" + k: v for k, v in got.items() if hasattr(v, "dtype")})
np.savez(path, **out)
'''

# scenario -> (the cases of the issue it covers, the mask after every one of its steps)
PLAIN = ["plain", "axn-uploaded", "neg-zero", "heat-density", "erosion", "verlet", "store-env", "dead-rows", "two-halves", "slow-lane", "repro", "sequence"]
EXPECTED = {
    "plain": [ALL] * 8,                                                 # (a)
    "axn-uploaded": [ALL - ACCEL] * 8,                                  # (b) from the first step on, and for good: ayn goes with axn
    "neg-zero": [ALL - ACCEL] * 8,                                      # an uploaded -0. is not "zeros": a build that skipped the field would keep it where another stores +0.
    "heat-density": [ALL - {"heat_density"}] * 8,                       # (c)
    "erosion": [set()] * 2 + [ALL - {"mass_of_bits"}] * 6,              # (d) two steps of a general namelist (no plain build), then plain again
    "verlet": [set()] * 2 + [ALL - ACCEL] * 6,                          # (e) two Verlet steps (no plain build), then RK
    "store-env": [ALL] * 8,                                             # (f) K = 3
    "dead-rows": [ALL] * 8,                                             # (g)
    "two-halves": [ALL] * 8,                                            # (h) kid_set_side_stream mode 1
    "slow-lane": [ALL] * 8,                                             # (h) mode 2
    "repro": [set()] * 8,                                               # (i) the staging instance is K = 0
    "sequence": [{"heat_density"}] * 3 + [ALL] * 8,                     # (j) non-zero upload, re-binning, step; zeros uploaded, steps, re-binning, steps
}
# fp64 members that each re-binning of the scenario leaves in place because they are known as zeros when it is planned (the rule
# itself, whatever build the steps before it ran): all three; mass_of_bits alone once axn was uploaded or a Verlet step was
# launched; axn, ayn once a thermodynamics with an erosion fraction was launched; none while the upload held all three
PERM_SKIPS = {"plain": [3], "axn-uploaded": [1], "neg-zero": [1], "heat-density": [3], "erosion": [2], "verlet": [1], "store-env": [3], "dead-rows": [3],
              "two-halves": [3], "slow-lane": [3], "repro": [3], "sequence": [0, 3]}


def _children(tmp, tag, cases, extra_env):
    env = {k: v for k, v in os.environ.items() if k not in ("KID_NO_ZERO_SKIP", "KID_NO_PLAIN_BUILD", "KID_REBIN_EAGER")}
    env["KID_STABLE_RESORT"] = "1"
    res = {}
    for skip in (True, False):
        e = dict(env, **extra_env)
        if not skip:
            e["KID_NO_ZERO_SKIP"] = "1"
        path = str(tmp / ("%s-%d.npz" % (tag, skip)))
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "n": N, "seed": SEED}, json.dumps(cases), path], env=e, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        with np.load(path) as z:
            res[skip] = {k: z[k] for k in z.files}
    return res


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return _children(tmp_path_factory.mktemp("zero_fields"), "plain", PLAIN, {})


@pytest.fixture(scope="module")
def runs_no_plain(tmp_path_factory):
    return _children(tmp_path_factory.mktemp("zero_fields_np"), "noplain", ["plain"], {"KID_NO_PLAIN_BUILD": "1"})


def _case(res, case):
    return {k[len(case) + 1:]: v for k, v in res.items() if k.startswith(case + "/")}


def _equal(a, e, what):
    """a: the default child, e: the KID_NO_ZERO_SKIP child.  Everything, row for row"""
    members = sorted(k for k in a if k.startswith("b_"))
    assert members == sorted(k for k in e if k.startswith("b_")) and "b_axn" in members and "b_alive" in members
    for c in (a, e):   # the precondition of a bit-for-bit comparison of the sums (module docstring)
        occupancy = np.unique(c["b_jne"].astype(np.int64) * 100000 + c["b_ine"], return_counts=True)[1]
        assert occupancy.max() <= 2, (what, "a cell ended with %d bergs: the order of its three atomics is not fixed" % occupancy.max())
    for k in members + ["acc", "out", "scal"]:
        assert a[k].shape == e[k].shape, (what, k)
        if k in ("acc", "out") and not np.array_equal(a[k], e[k], equal_nan=True):   # the figures, before the assertion
            for q in range(a[k].shape[0]):
                d = np.abs(a[k][q] - e[k][q])
                if np.nanmax(d) > 0:
                    print("%s: %s plane %d differs in %d cells, by at most %.3e of %.3e" % (what, k, q, int((d > 0).sum()), np.nanmax(d), np.abs(e[k][q]).max()))
        assert np.array_equal(a[k], e[k], equal_nan=True), (what, k, int((a[k] != e[k]).sum()))
    assert int((a["b_alive"] != 0).sum()) > 0 and np.abs(a["acc"]).max() > 0


def _masks(c):
    return [set(m) for m in json.loads(str(c["masks"][0]))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PLAIN)
def test_skipping_known_zeros_changes_nothing(runs, case):
    a, e = _case(runs[True], case), _case(runs[False], case)
    want = EXPECTED[case]
    got = _masks(a)
    assert got == want, "default child of %s: masks %s, the rule gives %s" % (case, got, want)
    assert _masks(e) == [set()] * len(want), "the KID_NO_ZERO_SKIP child of %s skipped something" % case
    _equal(a, e, case)
    assert int(a["fused"][0]) == int(e["fused"][0])
    # the permutation's own skip: a re-binning planned while axn, ayn, mass_of_bits are known as zeros leaves them where they are,
    # the KID_NO_ZERO_SKIP child moves them (heat_density stays in both children: the older rule)
    assert len(a["moved"]) == len(e["moved"]) == len(PERM_SKIPS[case])
    for q, skipped in enumerate(PERM_SKIPS[case]):
        assert int(e["moved"][q]) - int(a["moved"][q]) == skipped, (case, q, a["moved"], e["moved"])
    if case in ("plain", "store-env", "dead-rows", "sequence"):   # the re-binning went through the re-binning instance of the hot build
        assert int(a["fused"][0]) >= 1
    if case == "dead-rows":
        assert int((a["b_alive"] == 0).sum()) > 0
    if case in ("two-halves", "slow-lane"):   # the schedule changes neither the bergs nor the order of a stable re-binning
        ref = _case(runs[True], "plain")
        for k in sorted(k for k in ref if k.startswith("b_")):
            assert np.array_equal(a[k], ref[k], equal_nan=True), (case, k)
    if case == "neg-zero":   # ... and both children end with the +0. that the step stores
        assert not np.signbit(a["b_ayn"]).any() and not np.signbit(e["b_ayn"]).any()
    if case == "sequence":   # what the second upload replaced is gone from every row, whichever array of the pair holds the field now
        for k in ("b_axn", "b_ayn", "b_mass_of_bits"):
            assert not a[k].any(), k


@pytest.mark.gpu
def test_no_plain_build_skips_nothing(runs_no_plain, runs):
    """(i) KID_NO_PLAIN_BUILD: the general-namelist hot build loads and stores everything; its results are the plain builds'"""
    a, e = _case(runs_no_plain[True], "plain"), _case(runs_no_plain[False], "plain")
    assert _masks(a) == [set()] * 8 and _masks(e) == [set()] * 8
    _equal(a, e, "no-plain-build")
