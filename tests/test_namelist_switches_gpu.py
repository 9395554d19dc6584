"""The library against the oracle at every namelist switch of tests/switch_cases.py (their admissibility is checked on the
CPU by test_namelist_switches_cpu.py), at the tolerances of parity.compare / parity.compare_mts.

  per-berg cases  both bases, mode "fused" and "phases"; a case that leaves every KID_SWITCHES member at its base's value
                  is stepped by the folded build (K = 1 plain, K = 2 footloose profile) and is run once more with
                  KID_NO_PLAIN_BUILD, so that the general build K = 0 is held to the oracle at the same value;
  bonded cases    the MTS/DEM step;
  twin            the bare bases stepped by the folded and by the general build: the same bits berg by berg;
  predicate       a KID_SWITCHES member moved alone must take the handle out of the folded build: the result then moves
                  away from the bare base's wherever the oracle's does (a build that stayed folded reproduces the base).

Every test prints the worst relative error of its case (pytest -s), the figures of the table in DESIGN.md section 4.
"""
import numpy as np
import pytest

import parity as P
import switch_cases as SC
from icebergs_amd import types as T

pytestmark = pytest.mark.gpu

BERG_FIELDS = P.TRAJ_FIELDS + P.SIZE_FIELDS


def _worst(rep):
    k = max(rep, key=rep.get)
    return "%.1e (%s)" % (rep[k], k)


def _build_of(case, general=False):
    return 0 if general or not SC.stays_folded(case) else {"plain": 1, "flprof": 2}[case.base]


def _run_case(case, mode):
    grid, p, b = SC.build(case.base, case.inputs)
    p = SC.with_settings(p, SC.all_settings(case))
    ref = SC.oracle_run(case.base, SC.all_settings(case), case.inputs)
    got = P.run_hip(grid, p, b, SC.NSTEPS, mode=mode)
    return p, ref, got


@pytest.mark.parametrize("case,mode", [(c, m) for c in SC.PER_BERG for m in ("fused", "phases") if m == "fused" or SC.runs_phase_by_phase(c)],
                         ids=lambda v: v if isinstance(v, str) else SC.case_id(v))
def test_per_berg_switch(oracle, case, mode):
    p, ref, got = _run_case(case, mode)
    label = "%s/%s" % (SC.case_id(case), mode)
    rep = P.compare(ref, got, label, params=p)
    print("SWITCH %s build K=%d worst %s" % (label, _build_of(case), _worst(rep)))


@pytest.mark.parametrize("case", [c for c in SC.PER_BERG if not SC.runs_phase_by_phase(c)], ids=SC.case_id)
def test_phase_entry_points_refuse_what_they_cannot_run(oracle, case):
    """find_melt_using_spread_mass needs the gridded mass before the melt, which only the whole step gathers: run phase by
    phase the library used to return the bergs' own melt flux as if the switch were off (floating_melt off by 0.9)."""
    from icebergs_amd import lib
    with pytest.raises(lib.KidError, match="find_melt_using_spread_mass"):
        _run_case(case, "phases")


@pytest.mark.parametrize("case", [c for c in SC.PER_BERG if SC.stays_folded(c)], ids=SC.case_id)
def test_per_berg_switch_general_build(oracle, case, monkeypatch):
    """The run-time members the folded builds read (sicn_shift, ocean_drag_scale, rho_bergs, the rolling inputs, ...) once more
    in the general build."""
    monkeypatch.setenv("KID_NO_PLAIN_BUILD", "1")   # read when the handle is created
    p, ref, got = _run_case(case, "fused")
    label = "%s/general" % SC.case_id(case)
    rep = P.compare(ref, got, label, params=p)
    print("SWITCH %s build K=0 worst %s" % (label, _worst(rep)))


@pytest.mark.parametrize("case", SC.BONDED, ids=SC.case_id)
def test_bonded_switch(oracle, case):
    grid, p, b, bd = SC.build("bonded")
    p = SC.with_settings(p, SC.all_settings(case))
    ref, refbd = SC.oracle_run("bonded", SC.all_settings(case))
    got, gotbd = P.run_hip_mts(grid, p, b, bd, SC.NSTEPS)
    rep = P.compare_mts(ref, refbd, got, gotbd, SC.case_id(case))
    print("SWITCH %s build MTS worst %s" % (SC.case_id(case), _worst(rep)))
    print(case.name, {k: "%.1e" % v for k, v in rep.items() if v > 0})


@pytest.mark.parametrize("base,inputs", [("plain", ""), ("flprof", ""), ("plain", "narrow"), ("flprof", "narrow")])
def test_folded_and_general_build_are_twins(oracle, base, inputs, monkeypatch):
    """DESIGN: a berg's result does not depend on which build stepped it (the FMAs are spelled out, -ffp-contract=off).  The
    folded build (K = 1 / K = 2) and the general one (K = 0) on the same inputs: every berg field the same bits; the per-cell
    planes, whose sums are taken in another order, within TOL_GRID."""
    grid, p, b = SC.build(base, inputs)
    folded = P.run_hip(grid, p, b, SC.NSTEPS, mode="fused")
    monkeypatch.setenv("KID_NO_PLAIN_BUILD", "1")
    general = P.run_hip(grid, p, b, SC.NSTEPS, mode="fused")
    fo, go = SC.by_id(folded[0]), SC.by_id(general[0])
    assert np.array_equal(folded[0]["id"][fo], general[0]["id"][go])
    worst = 0.0
    for f in BERG_FIELDS + ["ine", "jne"]:
        a, c = folded[0][f][fo], general[0][f][go]
        if not np.array_equal(a, c):
            k = np.nonzero(a != c)[0]
            ulps = np.max(np.abs(a[k] - c[k]) / np.spacing(np.abs(c[k]))) if a.dtype == np.float64 else -1
            worst = max(worst, float(ulps))
            print("TWIN %s/%s: %s differs on %d bergs, at most %.0f ulp" % (base, inputs, f, len(k), ulps))
    assert worst == 0.0, "the folded and the general build differ by up to %.0f ulp" % worst
    d = SC.differences(general, folded, [])
    print("TWIN %s/%s planes worst %s" % (base, inputs, _worst(d)))
    for k, e in d.items():
        assert e <= P.TOL_GRID, "%s rel err %.3e" % (k, e)
    # the twins are the library's own two builds: both are held to the oracle as well
    ref = SC.oracle_run(base, {}, inputs, keep=True)
    P.compare(ref, folded, "twin/%s/folded" % base, params=p)
    P.compare(ref, general, "twin/%s/general" % base, params=p)


_BASE_HIP = {}


def _base_hip(base, inputs):
    if (base, inputs) not in _BASE_HIP:
        grid, p, b = SC.build(base, inputs)
        _BASE_HIP[(base, inputs)] = P.run_hip(grid, p, b, SC.NSTEPS, mode="fused")
    return _BASE_HIP[(base, inputs)]


@pytest.mark.parametrize("case", [c for c in SC.PER_BERG if SC.moves_one_switch(c)], ids=SC.case_id)
def test_switch_leaves_folded_build(oracle, case):
    """plain_namelist() / fl_profile_namelist(): one KID_SWITCHES member off its folded value and nothing else changed.  Seen
    from the host only: the result agrees with the oracle, and it is as far from the library's own result on the bare base as
    the oracle's two runs are from each other -- a handle that stayed in the folded build would return the base's result."""
    assert not SC.stays_folded(case)
    base_ref = SC.oracle_run(case.base, {}, case.inputs, keep=True)
    base_got = _base_hip(case.base, case.inputs)
    p, ref, got = _run_case(case, "fused")
    P.compare(ref, got, SC.case_id(case) + "/predicate", params=p)
    if case.name in SC.COUNTER_ONLY:
        k = T.SCALAR_NAMES[SC.COUNTER_ONLY[case.name]]
        assert ref[3][k] != base_ref[3][k] and got[3][k] == ref[3][k] and got[3][k] != base_got[3][k]
        return
    d_ref = SC.differences(base_ref, ref, BERG_FIELDS)
    d_got = SC.differences(base_got, got, BERG_FIELDS)
    from icebergs_amd.distributed import needs_footprint_planes
    a0 = T.ACC_NAMES["area_on_ocean"]   # (planes the library leaves zero when nothing reads them, as parity.compare has it)
    dead = set() if needs_footprint_planes(p) else {"acc%d" % k for k in range(a0, a0 + 27)}
    moved = [k for k, e in d_ref.items() if e >= 1.0e-6 and k not in dead]
    assert moved
    print("SWITCH %s moves %s: oracle %s, library %s" % (SC.case_id(case), SC.moves_one_switch(case), _worst(d_ref), _worst(d_got)))
    for k in moved:   # both runs agree with the oracle within 1e-9 of the same scale, the oracle's runs differ by >= 1e-6
        assert k in d_got and d_got[k] >= 0.5 * d_ref[k], "%s: the oracle moves by %.1e, the library by %.1e" % (k, d_ref[k], d_got.get(k, 0.))
