"""The populations of tests/dem_cases.py on the oracle: by id the three row orders are one and the same problem (every field, bond and
scalar bit for bit), so whatever tests/test_dem_rows_gpu.py finds between them on the device is the device's; and the orders do what
they are for -- the shuffle puts four bonds in five across a workgroup boundary of the fused sub-step kernel, the interleave all."""
import numpy as np
import pytest

import dem_cases as D
import parity as P

CASES = [("hex", 7), ("hex_partial", 3), ("square", 4), ("hex_grounded", 40), ("hex_idle", 4)]


def test_permute_bonded_keeps_lists_and_moves_rows():
    grid, p, b, bd = D.lattice("hex_partial", 3)
    n = len(b["lon"])
    perm = D.row_order("shuffle", n)
    c, cbd = D.permute_bonded(b, bd, perm)
    assert np.array_equal(c["id"], b["id"][perm]) and np.array_equal(cbd["count"], bd["count"][perm])
    mb = bd["max_bonds"]
    for r in (0, 1, n // 2, n - 1):   # row r holds what row perm[r] held, list order and all
        assert np.array_equal(cbd["other_id"].reshape(mb, n)[:, r], bd["other_id"].reshape(mb, n)[:, perm[r]])
    D.assert_same_by_id(b, bd, c, cbd, "permuted inputs")


@pytest.mark.parametrize("kind", ["hex", "hex_partial", "square"])
def test_row_orders_separate_partners(kind):
    grid, p, b, bd = D.lattice(kind, 1)
    n = len(b["lon"])
    assert (n + D.BLOCK - 1) // D.BLOCK == 10   # ten workgroups: every XCD, two of them twice
    share = {}
    for order in ("lattice", "shuffle", "stride"):
        c, cbd = D.permute_bonded(b, bd, D.row_order(order, n, b, bd))
        share[order] = D.crossing_share(c, cbd)
        rows = D.partner_rows(c, cbd)   # from other_id
        own = np.broadcast_to(np.arange(n)[None, :] // D.BLOCK, rows.shape)
        if order == "stride":
            assert not np.any((rows >= 0) & (rows // D.BLOCK == own)), "a partner shares its berg's workgroup"
    print(kind, {k: "%.3f" % v for k, v in share.items()})
    assert share["lattice"] < 0.2 and share["shuffle"] >= 0.8 and share["stride"] == 1.0


@pytest.mark.parametrize("kind,sub_steps", CASES)
def test_oracle_is_row_order_invariant(oracle, kind, sub_steps):
    res = {}
    for order in ("lattice", "shuffle", "stride"):
        grid, p, b, bd = D.lattice(kind, sub_steps, order)
        res[order] = P.run_oracle_mts(grid, p, b, bd, 2)
    (ref, refbd) = res["lattice"]
    if kind in ("hex_grounded", "hex_idle"):
        assert (refbd["broken"] != 0).sum() > 0   # bonds do break inside the loop
    if kind == "hex_idle":
        idle = ref[0]["static_berg"] == 1.0
        assert idle.sum() == 267 and np.array_equal(ref[0]["lon"][idle], D.lattice(kind, sub_steps)[2]["lon"][idle])
    assert D.max_bond_arg(ref[0], refbd) < 0.25
    for order in ("shuffle", "stride"):
        got, gotbd = res[order]
        D.assert_same_by_id(ref[0], refbd, got[0], gotbd, "%s/%d oracle, %s against lattice order" % (kind, sub_steps, order))
        assert np.array_equal(ref[3], got[3]), "scalars"
        assert P.rel_err(got[1], ref[1]) <= 1e-12 and P.rel_err(got[2], ref[2]) <= 1e-12   # per-cell sums: the order of the additions
