"""Bonded DEM populations in the arrangement production has them, for tests/test_dem_rows_cpu.py, tests/test_dem_rows_gpu.py and the
bonded cases of tests/test_exact_math_gpu.py: config_c4 lattices of ten workgroups of mts_substeps_kernel (256 rows each, so all
eight XCDs take part in the record exchange and two hold a second workgroup), uploaded in three row orders --

  lattice   the order config_c4 leaves (sort_reference_order): a berg's partners sit within a column of rows of it;
  shuffle   a seeded permutation: partners land anywhere, nine bonds in ten cross a workgroup;
  stride    a stride-10 interleave (row r of the lattice order goes to block r mod 10, or to the next block that holds none of
            its partners): EVERY partner is in another workgroup.

A permutation moves berg rows and the row index k of the slot-major bond arrays; each berg's bond list keeps its order, and the
reference's traversal order (cells, then the `inorder` keys) does not depend on rows, so by id every order is the same problem."""
import numpy as np

from icebergs_amd import synthetic as S

BLOCK = 256            # MTS_FUSED_BS: rows per workgroup of mts_substeps_kernel
SUB_STEPS = (1, 2, 3, 4, 7, 40)   # the three-copy ring wraps at every phase
FAR = (215.0e3, 215.0e3)   # a seamount nobody reaches: (150e3, 150e3), where the oracle-size cases park it, lies UNDER a lattice of this size


def permute_bonded(b, bd, perm):
    """(bergs, bonds) with row r holding what row perm[r] held; bond lists keep their order (only the row index k of the
    slot-major arrays x[s * n + k] moves)"""
    perm = np.asarray(perm)
    n = len(b["lon"])
    assert sorted(perm.tolist()) == list(range(n))
    nb = {k: (np.ascontiguousarray(v[perm]) if hasattr(v, "dtype") and v.shape[:1] == (n,) else v) for k, v in b.items()}
    mb = bd["max_bonds"]
    nbd = {"max_bonds": mb, "count": np.ascontiguousarray(bd["count"][perm])}
    for k, v in bd.items():
        if k in ("max_bonds", "count"):
            continue
        nbd[k] = np.ascontiguousarray(v.reshape(mb, n)[:, perm]).reshape(mb * n)
    return nb, nbd


def row_order(kind, n, b=None, bd=None):
    if kind == "lattice":
        return np.arange(n)
    if kind == "shuffle":
        return np.random.default_rng(20240).permutation(n)
    assert kind == "stride"
    # row r of the lattice order goes to the block with the most room left that holds none of its partners, r mod nblock first among
    # equals: a stride-nblock interleave wherever the lattice allows it, and no block closes before the others
    nblock = (n + BLOCK - 1) // BLOCK
    room = [min(BLOCK, n - q * BLOCK) for q in range(nblock)]
    row_of = {int(i): r for r, i in enumerate(b["id"])}
    block_of = np.full(n, -1)
    for r in range(n):
        near = {block_of[row_of[int(bd["other_id"][s * n + r])]] for s in range(bd["count"][r])}
        q = min((c for c in range(nblock) if room[c] > 0 and c not in near), key=lambda c: (-room[c], (c - r) % nblock))
        block_of[r] = q
        room[q] -= 1
    return np.argsort(block_of, kind="stable")


def crossing_share(b, bd):
    """the share of bonds whose two ends sit in different 256-row blocks"""
    n = len(b["lon"])
    row_of = {int(i): r for r, i in enumerate(b["id"])}
    cross = total = 0
    for r in range(n):
        for s in range(bd["count"][r]):
            total += 1
            cross += (row_of[int(bd["other_id"][s * n + r])] // BLOCK) != (r // BLOCK)
    return cross / total


def lattice(kind, sub_steps, order="lattice", orig_moment=0):
    """kind: hex (48 x 50 = 2400), hex_partial (47 x 51 = 2397: the last workgroup partial), square (48 x 50, four bonds:
    mts_substeps_kernel<4>), hex_grounded (48 x 50 on the seamount: bonds break inside the loop), hex_idle (every 9th element static)"""
    # dt: 9 s per sub-step, config 4's own (1800 s / 200): the explicit sub-steps are stable below ~70 s for these springs and masses
    kw = dict(nx=48, ny=50, sub_steps=sub_steps, dt=9.0 * sub_steps, bump=FAR)
    if kind == "hex_partial":
        kw.update(nx=47, ny=51)
    elif kind == "square":
        kw.update(hexagonal=False)
    elif kind == "hex_grounded":
        kw.update(bump=(58.0e3, 60.0e3))
    else:
        assert kind in ("hex", "hex_idle"), kind
    grid, p, b, bd = S.config_c4(**kw)
    S.set_diag_all(p)
    p.orig_dem_moment_of_inertia = orig_moment
    # melt off, as in the reference's own DEM tests: at 9 to 360 s per step the mass an element loses to erosion is 1e-9 of its mass,
    # and the melt diagnostics, differences of two masses, carry 1e-16 / 1e-9 of noise on either side (3e-8 at 9 s against the
    # planes' 1e-8: not what these cases are about)
    p.set_melt_rates_to_zero = 1
    if kind == "hex_idle":
        b["static_berg"][::9] = 1.0
    n = len(b["lon"])
    assert n == kw["nx"] * kw["ny"]
    b, bd = permute_bonded(b, bd, row_order(order, n, b, bd))
    return grid, p, b, bd


def by_id(b, bd):
    """({field: values in id order}, {bond field: (max_bonds, n) in id order, slots past a list's end zeroed}): what does not depend
    on the row order"""
    n = len(b["lon"])
    o = np.argsort(b["id"], kind="stable")
    mb = bd["max_bonds"]
    bb = {k: v[o] for k, v in b.items() if hasattr(v, "dtype") and v.shape[:1] == (n,)}
    live = np.arange(mb)[:, None] < bd["count"][o][None, :]
    bo = {"count": bd["count"][o]}
    for k, v in bd.items():
        if k not in ("max_bonds", "count"):
            bo[k] = np.where(live, v.reshape(mb, n)[:, o], 0)
    return bb, bo


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
    return bool(np.array_equal(a, b))


def partner_rows(b, bd):
    """(max_bonds, n) rows of the bonds' other ends, -1 past a list's end"""
    n, mb = len(b["lon"]), bd["max_bonds"]
    o = np.argsort(b["id"], kind="stable")
    other = bd["other_id"].reshape(mb, n)
    pos = np.clip(np.searchsorted(b["id"][o], other), 0, n - 1)
    live = np.arange(mb)[:, None] < bd["count"][None, :]
    assert np.array_equal(b["id"][o][pos][live], other[live]), "a bond names a berg that is not there"
    return np.where(live, o[pos], -1)


def max_bond_arg(b, bd):
    """the largest |rot_k - rot_o| over the bonds: below 0.25 every wave of the fused kernel takes the sine series"""
    rows = partner_rows(b, bd)
    d = np.abs(b["rot"][None, :] - b["rot"][np.maximum(rows, 0)])
    return float(np.max(np.where(rows >= 0, d, 0.0)))


def assert_same_by_id(a, abd, c, cbd, label, skip=()):
    """bit for bit: every per-berg field by id, every bond field by (id, slot of the list), counts and broken marks"""
    (fa, ba), (fc, bc) = by_id(a, abd), by_id(c, cbd)
    assert set(fa) == set(fc) and set(ba) == set(bc)
    bad = [f for f in fa if f not in skip and not same_bits(fa[f], fc[f])] + ["bond " + f for f in ba if not same_bits(ba[f], bc[f])]
    assert not bad, "%s: not bit for bit in %s" % (label, bad)
