"""The fused sub-step loop (mts_substeps_kernel) in the arrangement production runs it: ten workgroups over all eight XCDs, and the
bergs' rows in an order in which partners do NOT sit next to each other (tests/dem_cases.py: lattice order, a seeded shuffle with
nine bonds in ten across a workgroup boundary, an interleave with every bond across one).  The kernel exchanges the 64-byte records
point to point through a three-copy ring with no grid barrier; 1, 2, 3, 4, 7 and 40 sub-steps make the ring wrap at every phase.

* Row-order invariance.  Each side of a pair evaluates it in the primary's orientation and sums its list in list order, so what a
  berg computes cannot depend on where its row or its partners' rows are: between the three orders every per-berg field by id,
  every bond field by (id, place in the list), the broken marks, the conglomerate ids and the event scalars are EQUAL, bit for bit.
  |rot_k - rot_o| stays below 0.25 (asserted), so no wave changes between the sine series and sin().  The atomically summed planes
  are held at compare_mts' tolerance.  A record of three sub-steps earlier handed out by the ring would be a displacement of
  metres through a 1e9 N/m spring: nothing here could absorb it.
* With fracture (a lattice grounded on the seamount: bonds break inside the loop) and with idle rows (every ninth element static:
  a berg that is not swept copies its record along).
* Fused against three launches per sub-step (KID_MTS_NO_FUSED) on the shuffled order with orig_dem_moment_of_inertia = 1, where both
  paths compute theta = arg: bit for bit.
* Every order against the oracle with compare_mts at its existing tolerances.
No case may pass on the fall-back: kid_mts_fused_launches counts the cooperative launches of a handle -- one per step on the fused
path, none with KID_MTS_NO_FUSED."""
import numpy as np
import pytest

import dem_cases as D
import parity as P

pytestmark = pytest.mark.gpu
NSTEPS = 2
ORDERS = ("lattice", "shuffle", "stride")


def run_hip(grid, p, b, bd, nsteps=NSTEPS):
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(grid, p, capacity=len(b["lon"]), device=0)
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(bd)
        ib.run(nsteps)
        acc, out, scal = ib.fetch()
        got = ib.download_bergs()
        gotbd = ib.download_bonds(bd["max_bonds"])
        return (got, acc.copy(), out.copy(), scal.copy()), gotbd, ib.mts_fused_launches()
    finally:
        ib.close()


def across_orders(oracle, kind, sub_steps, monkeypatch):
    monkeypatch.delenv("KID_MTS_NO_FUSED", raising=False)
    monkeypatch.delenv("KID_MTS_FUSED_BLOCKS_CAP", raising=False)
    res = {}
    for order in ORDERS:
        grid, p, b, bd = D.lattice(kind, sub_steps, order)
        got, gotbd, launches = run_hip(grid, p, b, bd)
        assert launches == NSTEPS, "%s/%d %s: %d fused launches in %d steps (the case took the fall-back)" % (kind, sub_steps, order, launches, NSTEPS)
        arg = D.max_bond_arg(got[0], gotbd)
        assert arg < 0.25, arg
        ref, refbd = P.run_oracle_mts(grid, p, b, bd, NSTEPS)
        P.compare_mts(ref, refbd, got, gotbd, "%s/%d %s order against the oracle" % (kind, sub_steps, order))
        res[order] = (got, gotbd, ref, refbd)
    base, basebd = res["lattice"][0], res["lattice"][1]
    for order in ORDERS[1:]:
        got, gotbd = res[order][0], res[order][1]
        label = "%s/%d fused loop, %s against lattice order" % (kind, sub_steps, order)
        D.assert_same_by_id(base[0], basebd, got[0], gotbd, label)
        from icebergs_amd import types as T
        for name in P.MTS_SCALARS:
            assert base[3][T.SCALAR_NAMES[name]] == got[3][T.SCALAR_NAMES[name]], (label, name)
        sc = P.acc_scales(base[1])
        for k in range(base[1].shape[0]):
            assert P.acc_err(got[1], base[1], k, sc) <= 10 * P.TOL_GRID, (label, "accumulator plane", k)
        for k in range(base[2].shape[0]):
            assert P.rel_err(got[2][k], base[2][k]) <= 10 * P.TOL_GRID, (label, "output plane", k)
    return res


@pytest.mark.parametrize("sub_steps", D.SUB_STEPS)
@pytest.mark.parametrize("kind", ["hex", "hex_partial", "square"])
def test_fused_substeps_do_not_depend_on_the_row_order(oracle, kind, sub_steps, monkeypatch):
    res = across_orders(oracle, kind, sub_steps, monkeypatch)
    assert (res["lattice"][1]["broken"] != 0).sum() == 0   # (nothing breaks here: the seamount is out of the way)


@pytest.mark.parametrize("sub_steps", [7, 40])
def test_fused_substeps_with_fracture_do_not_depend_on_the_row_order(oracle, sub_steps, monkeypatch):
    res = across_orders(oracle, "hex_grounded", sub_steps, monkeypatch)
    gotbd, refbd = res["lattice"][1], res["lattice"][3]
    assert (gotbd["broken"] != 0).sum() > 0 and (refbd["broken"] != 0).sum() > 0   # bonds do break inside the loop


@pytest.mark.parametrize("sub_steps", [4, 40])
def test_fused_substeps_with_idle_rows_do_not_depend_on_the_row_order(oracle, sub_steps, monkeypatch):
    res = across_orders(oracle, "hex_idle", sub_steps, monkeypatch)
    got = res["shuffle"][0][0]
    start = D.lattice("hex_idle", sub_steps, "shuffle")[2]
    idle = start["static_berg"] == 1.0
    assert idle.sum() == 267 and np.array_equal(got["lon"][idle], start["lon"][idle]) and np.array_equal(got["lat"][idle], start["lat"][idle])
    assert not np.array_equal(got["lon"][~idle], start["lon"][~idle])


@pytest.mark.parametrize("sub_steps", D.SUB_STEPS)
def test_fused_substeps_equal_three_launches_bit_for_bit(oracle, sub_steps, monkeypatch):
    """orig_dem_moment_of_inertia = 1: theta = arg on both paths, which share their update functions -- the same operations in the
    same order on the same values"""
    monkeypatch.delenv("KID_MTS_NO_FUSED", raising=False)
    grid, p, b, bd = D.lattice("hex", sub_steps, "shuffle", orig_moment=1)
    fused, fusedbd, launches = run_hip(grid, p, b, bd)
    assert launches == NSTEPS
    monkeypatch.setenv("KID_MTS_NO_FUSED", "1")
    plain, plainbd, launches = run_hip(grid, p, b, bd)
    assert launches == 0
    label = "hex/%d shuffled, fused against three launches" % sub_steps
    D.assert_same_by_id(plain[0], plainbd, fused[0], fusedbd, label)
    assert np.array_equal(plain[0]["id"], fused[0]["id"])
    from icebergs_amd import types as T
    for name in P.MTS_SCALARS:
        assert plain[3][T.SCALAR_NAMES[name]] == fused[3][T.SCALAR_NAMES[name]], (label, name)
    ref, refbd = P.run_oracle_mts(grid, p, b, bd, NSTEPS)
    P.compare_mts(ref, refbd, plain, plainbd, label + ": three launches against the oracle")
