"""Bonded bergs on lat-lon grids, the device against the oracle: the cases of tests/latlon_bonded.py (admitted by
tests/test_latlon_bonded_cpu.py) through kid_run_step and through the oracle, compared by parity.compare_mts under the tolerances
the oracle's own spread gives on the day of the run (latlon_bonded.tolerances: max(compare_mts's, 10 x spread); cells, bond sets,
broken bonds and counters exact; longitudes modulo 360).  Then the fused sub-step loop against the three-launch one on two of
them, and the device-side checksum of a final state against the oracle's."""
import numpy as np
import pytest

import latlon_bonded as LB
import parity as P

pytestmark = pytest.mark.gpu

_HIP = {}


def _hip(name, path="default"):
    """one device run per (case, sub-step path), shared and left unchanged (the environment selects the path: the caller sets it)"""
    if (name, path) not in _HIP:
        grid, p, b, bd, nsteps = LB.measured(name)["case"]
        _HIP[(name, path)] = P.run_hip_mts(grid, p, b, bd, nsteps)
    return _HIP[(name, path)]


def _line(label, rep, tol):
    worst = max(tol, key=lambda k: rep[k] / tol[k])
    return "%s: lon %.1e lat %.1e uvel %.1e vvel %.1e axn %.1e ang_accel %.1e od %.1e acc %.1e out %.1e | nearest to its tolerance: %s %.1e of %.1e" % (
        label, rep["lon"], rep["lat"], rep["uvel"], rep["vvel"], rep["axn"], rep["ang_accel"], rep["od"], rep["acc"], rep["out"], worst, rep[worst], tol[worst])


@pytest.mark.parametrize("name", LB.NAMES)
def test_device_against_the_oracle(oracle, name):
    m = LB.measured(name)
    tol = LB.tolerances(name)
    got, gotbd = _hip(name)
    rep, exact = P.mts_errors(m["ref"], m["refbd"], got, gotbd, wrap_lon=True)
    print(_line("lat-lon/" + name, rep, tol), {k: v for k, v in exact.items() if not v} or "")
    print(name, {k: "%.1e" % v for k, v in rep.items() if v > 0 and not k[3:].isdigit()})
    P.compare_mts(m["ref"], m["refbd"], got, gotbd, "lat-lon/" + name, tols=tol, wrap_lon=True)


@pytest.mark.parametrize("name", ["two_bergs_70S", "hex_grounded_60S"])
def test_fused_substeps_match_three_launches(oracle, name, monkeypatch):
    """the sub-step loop in one cooperative launch against three launches per sub-step (KID_MTS_NO_FUSED): held to each other by
    the tolerances each is held to the oracle by"""
    m = LB.measured(name)
    tol = LB.tolerances(name)
    monkeypatch.delenv("KID_MTS_NO_FUSED", raising=False)
    fused, fusedbd = _hip(name)
    monkeypatch.setenv("KID_MTS_NO_FUSED", "1")
    plain, plainbd = _hip(name, "three launches")
    for label, (a, abd), (b, bbd) in (("three launches against the oracle", (m["ref"], m["refbd"]), (plain, plainbd)),
                                      ("fused against three launches", (plain, plainbd), (fused, fusedbd))):
        rep, _ = P.mts_errors(a, abd, b, bbd, wrap_lon=True)
        print(_line("lat-lon/%s %s" % (name, label), rep, tol))
    P.compare_mts(m["ref"], m["refbd"], plain, plainbd, "lat-lon three launches/" + name, tols=tol, wrap_lon=True)
    P.compare_mts(plain, plainbd, fused, fusedbd, "lat-lon fused vs three launches/" + name, tols=tol, wrap_lon=True)
    for f in ("lon", "lat", "uvel", "vvel"):
        assert not np.array_equal(plain[0][f], m["case"][2][f]), f     # (the run did move the elements)


def test_device_checksum_of_the_final_state(oracle):
    """bergs_chksum on the device (kid_bergs_chksum_device) after the run of two_bergs_70S: chksum3 -- cell occupancy and
    log(mass) -- and the count are the oracle's over its own final state"""
    import oracle_lib
    from icebergs_amd.framework import Icebergs
    name = "two_bergs_70S"
    m = LB.measured(name)
    grid, p, b, bd, nsteps = m["case"]
    want = oracle_lib.Oracle(grid, p).bergs_chksum(m["ref"][0])
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(bd)
        before = ib.bergs_chksum_device()
        ib.run(nsteps)
        got = ib.bergs_chksum_device()
    finally:
        ib.close()
    start = oracle_lib.Oracle(grid, p).bergs_chksum(b)
    print("two_bergs_70S chksum: device", got, "oracle", want, "(before the run: device", before, "oracle", start, ")")
    assert before[2] == start[2] and before[5] == start[5] == len(b["lon"])
    assert got[2] == want[2] and got[5] == want[5]
    assert want[2] != start[2], "the final occupancy is not the initial one"
