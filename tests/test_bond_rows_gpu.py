"""Bond tables follow their rows (kid_set_bonds_follow_rows; permute_bonds_kernel and bonds_move of icebergs_amd/csrc/kid_rows.inc).

With the switch on, kid_move_berg_between_cells and kid_compact_bergs accept a handle with bond tables and carry the slot-major
tables through their permutation: every list with its row, in list order, bit for bit; partner rows through the inverse
permutation, (-1, -1) for a partner that is dead or dropped.  With it off both refuse as they always did.

Populations: the config_c4 lattices of tests/dem_cases.py (hex 2400 rows = ten workgroups, hex_partial 2397, square with four
slots, hex_grounded where bonds break and lists close up), uploaded in the seeded shuffle so that a re-binning really moves rows,
3 sub-steps (7 where bonds must break); and hand-built chains on the 48 x 40 box (1 row without a bond, a pair, 65, 257), on
which only the tables are looked at.  The capacity is always n + 37: the tables' stride is not the row count.

1. the switch: off refuses (rc=-5, "bonds keep their rows") and changes nothing, on accepts, 2 is KID_EINVAL
2. tables through a re-binning, twice in a row, and with KID_STABLE_RESORT=1
3. tables through a compaction: every seventh row dead (partners of live rows among them), nothing dead, everything dead
4. stepping does not notice: run 1, re-bin, run 1, compact, run 1 against run 3, bit for bit by id
5. compaction on the device against the survivors uploaded afresh, then two steps on either
6. bonded bergs under the single-time-step scheme (the collision case of tests/rk_interactive.py), Verlet and RK4
7. growth: re-bin, reserve(2 * capacity), re-bin, compact; after close() the process holds the memory it held before

Row-order invariance of the stepping kernels themselves is tests/test_dem_rows_gpu.py's subject; the bound on the atomically
summed planes (10 * P.TOL_GRID) is the one it uses between row orders."""
import ctypes as C
import functools

import numpy as np
import pytest

import dem_cases as D
import parity as P
from icebergs_amd import lib as L
from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from icebergs_amd.framework import Icebergs

pytestmark = pytest.mark.gpu
PAD = 37
BOND_MEMBERS = ["count", "other_id", "broken"] + list(T.BOND_F64_NAMES)


# ---- populations ----
@functools.lru_cache(maxsize=None)
def _lattice(kind, sub_steps):
    return D.lattice(kind, sub_steps, "shuffle")


def lattice(kind, sub_steps):
    grid, p, b, bd = _lattice(kind, sub_steps)
    return grid, p, S.copy_bergs(b), S.copy_bonds(bd)


def box():
    grid = S.c2_forcing(S.latlon_grid(ni=48, nj=40, lon0=10.0, dlon=0.02, lat0=-60.0, dlat=0.02))
    p = S.default_params()
    p.dt = 1800.0
    return grid, p


def chain(n):
    """n bergs in random cells of the box, berg k bonded to k - 1 and k + 1 (two slots; none at n = 1), every bond member distinct"""
    grid, p = box()
    b = S.place_bergs(grid, n, 11 + n, (4, 44), (4, 36))   # (in reference order: cells ascending)
    assert n < 2 or len(set(zip(b["jne"].tolist(), b["ine"].tolist()))) > 1
    # rows out of cell order, so that a re-binning has something to do: the pair turned round, the chains shuffled
    perm = np.arange(n)[::-1] if n <= 2 else np.random.default_rng(20240 + n).permutation(n)
    b = {k: (np.ascontiguousarray(v[perm]) if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    bd = S.empty_bonds(n, 2)
    other = bd["other_id"].reshape(2, n)
    for k in range(n):
        for o in (k - 1, k + 1):
            if 0 <= o < n:
                other[bd["count"][k], k] = b["id"][o]
                bd["count"][k] += 1
    live = np.arange(2)[:, None] < bd["count"][None, :]
    for f, name in enumerate(T.BOND_F64_NAMES):
        bd[name][:] = np.where(live, (f + 1) * 4096.0 + np.arange(2 * n).reshape(2, n) + 0.25, 0.0).reshape(2 * n)
    bd["broken"][:] = np.where(live, np.arange(2 * n).reshape(2, n) % 2, 0).reshape(2 * n)
    return grid, p, b, bd


def loaded(grid, p, b, bd, follow=True):
    ib = Icebergs(grid, p, capacity=len(b["lon"]) + PAD)
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(bd)
        if follow:
            ib.set_bonds_follow_rows(True)
    except Exception:
        ib.close()
        raise
    return ib


# ---- what is held ----
def state(ib, mb):
    return ib.download_bergs(), ib.download_bonds(mb)


def partners_by_id(b, bd):
    """(rows, slots) as kid_upload_bonds derives them: the row of the live berg a slot names, and the slot of that berg's list that
    names this one; -1 where there is none"""
    n, mb = len(b["lon"]), bd["max_bonds"]
    row_of = {int(i): r for r, i in enumerate(b["id"]) if b["alive"][r]}
    other, cnt = bd["other_id"].reshape(mb, n), bd["count"]
    rows, slots = np.full((mb, n), -1, dtype=np.int32), np.full((mb, n), -1, dtype=np.int32)
    for k in range(n):
        for s in range(cnt[k]):
            o = row_of.get(int(other[s, k]), -1)
            if o < 0:
                continue
            rows[s, k] = o
            for t in range(cnt[o]):
                if other[t, o] == b["id"][k]:
                    slots[s, k] = t
                    break
    return rows, slots


def assert_tables(ib, b, bd, label, all_alive=True):
    """the partner rows and slots on the device are those the downloaded ids give, and every matched slot names its berg back"""
    n, mb = len(b["lon"]), bd["max_bonds"]
    rows, slots = ib.bond_partner_rows()
    assert rows.shape == (mb, n) and slots.shape == (mb, n)
    want_rows, want_slots = partners_by_id(b, bd)
    assert np.array_equal(rows, want_rows), (label, "partner rows")
    assert np.array_equal(slots, want_slots), (label, "partner slots")
    if all_alive and n:
        assert np.array_equal(rows, D.partner_rows(b, bd)), (label, "partner rows against dem_cases.partner_rows")
    other = bd["other_id"].reshape(mb, n)
    s_, k_ = np.nonzero((rows >= 0) & (slots >= 0))
    assert np.array_equal(other[slots[s_, k_], rows[s_, k_]], b["id"][k_]), (label, "a matched slot does not name its berg back")
    past = np.arange(mb)[:, None] >= bd["count"][None, :]
    assert (rows[past] == -1).all() and (slots[past] == -1).all(), (label, "past a list's end")


def assert_rows_unchanged(a, abd, c, cbd, label):
    for k, v in a.items():
        if hasattr(v, "dtype"):
            assert D.same_bits(v, c[k]), (label, k)
    for k in BOND_MEMBERS:
        assert D.same_bits(abd[k], cbd[k]), (label, "bond " + k)


def snapshot(ib, mb):
    acc, out, scal = ib.fetch()
    b, bd = state(ib, mb)
    return b, bd, acc.copy(), out.copy(), scal.copy()


def assert_same_run(a, c, label):
    """as tests/test_dem_rows_gpu.py compares two row orders: bergs and bonds bit for bit by id, the event scalars equal, the
    atomically summed planes within 10 * P.TOL_GRID"""
    D.assert_same_by_id(a[0], a[1], c[0], c[1], label)
    for name in P.MTS_SCALARS:
        assert a[4][T.SCALAR_NAMES[name]] == c[4][T.SCALAR_NAMES[name]], (label, name)
    sc = P.acc_scales(c[2])
    for k in range(c[2].shape[0]):
        assert P.acc_err(a[2], c[2], k, sc) <= 10 * P.TOL_GRID, (label, "accumulator plane", k)
    for k in range(c[3].shape[0]):
        assert P.rel_err(a[3][k], c[3][k]) <= 10 * P.TOL_GRID, (label, "output plane", k)


def kill_every_seventh(b):
    b["alive"][::7] = 0
    return b


def survivors(b, bd):
    """the live rows alone, dropped on the host: rows and the row index of the slot-major bond arrays, lists untouched"""
    keep = np.nonzero(b["alive"] != 0)[0]
    n, mb = len(b["lon"]), bd["max_bonds"]
    nb = {k: (np.ascontiguousarray(v[keep]) if hasattr(v, "dtype") and v.shape[:1] == (n,) else v) for k, v in b.items()}
    nbd = {"max_bonds": mb, "count": np.ascontiguousarray(bd["count"][keep])}
    for k, v in bd.items():
        if k not in ("max_bonds", "count"):
            nbd[k] = np.ascontiguousarray(v.reshape(mb, n)[:, keep]).reshape(mb * len(keep))
    return nb, nbd


# ---- 1. the switch ----
def test_switch_off_refuses_on_accepts():
    grid, p, b, bd = chain(65)
    ib = loaded(grid, p, b, bd, follow=False)
    try:
        before = state(ib, 2)
        for call in (ib.compact, ib.move_berg_between_cells):
            with pytest.raises(L.KidError, match=r"rc=-5 .*bonds keep their rows"):
                call()
        assert_rows_unchanged(*before, *state(ib, 2), "after the refusals")
        assert_tables(ib, *before, "after the refusals")
        with pytest.raises(L.KidError, match=r"rc=-1 "):
            ib.set_bonds_follow_rows(2)
        with pytest.raises(L.KidError, match=r"rc=-1 "):
            ib.set_bonds_follow_rows(-1)
        with pytest.raises(L.KidError, match=r"rc=-5 .*bonds keep their rows"):   # a refused value leaves the switch where it was
            ib.compact()
        ib.set_bonds_follow_rows(True)
        ib.move_berg_between_cells()
        ib.compact()
        D.assert_same_by_id(*before, *state(ib, 2), "after both calls")
        ib.set_bonds_follow_rows(False)
        with pytest.raises(L.KidError, match=r"rc=-5 .*bonds keep their rows"):
            ib.move_berg_between_cells()
    finally:
        ib.close()
    grid, p = box()
    ib = Icebergs(grid, p, capacity=8)   # without bonds: accepted, and the hook has nothing to show
    try:
        ib.set_bonds_follow_rows(True)
        ib.upload_bergs(S.place_bergs(grid, 4, 5, (4, 44), (4, 36)))
        with pytest.raises(L.KidError, match=r"rc=-1 .*no bonds"):
            ib.bond_partner_rows()
        ib.move_berg_between_cells()
        ib.compact()
    finally:
        ib.close()


# ---- 2. a re-binning ----
def rebinning(case, label, twice=True):
    grid, p, b, bd = case
    mb, n = bd["max_bonds"], len(b["lon"])
    ib = loaded(grid, p, b, bd)
    try:
        assert ib.capacity == n + PAD
        before = state(ib, mb)
        assert_tables(ib, *before, label + ": as uploaded")
        for turn in range(2 if twice else 1):
            ib.move_berg_between_cells()
            after = state(ib, mb)
            D.assert_same_by_id(*before, *after, "%s: re-binning %d" % (label, turn + 1))
            assert_tables(ib, *after, "%s: re-binning %d" % (label, turn + 1))
            if turn == 0 and n > 1:
                assert not np.array_equal(after[0]["id"], before[0]["id"]), label + ": the re-binning moved no row"
            key = after[0]["jne"].astype(np.int64) * 100000 + after[0]["ine"]
            assert (np.diff(key) >= 0).all(), label + ": rows are not in cell order"
    finally:
        ib.close()


@pytest.mark.parametrize("kind,sub_steps", [("hex", 3), ("hex_partial", 3), ("square", 3)])
def test_tables_through_a_rebinning_lattice(kind, sub_steps):
    rebinning(lattice(kind, sub_steps), kind)


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_tables_through_a_rebinning_chain(n):
    rebinning(chain(n), "chain of %d" % n)


@pytest.mark.parametrize("case", ["hex", "chain"])
def test_tables_through_a_stable_resort(case, monkeypatch):
    monkeypatch.setenv("KID_STABLE_RESORT", "1")   # read when the handle is created
    rebinning(lattice("hex", 3) if case == "hex" else chain(257), case + ", KID_STABLE_RESORT")


@pytest.mark.parametrize("n", [65, 257])
def test_rebinning_drops_dead_rows_and_unmatches_their_partners(n):
    """dead rows sort to the tail, which the next count cuts off without a kernel: no reference may point into it"""
    grid, p, b, bd = chain(n)
    b = kill_every_seventh(b)
    live = int((b["alive"] != 0).sum())
    ib = loaded(grid, p, b, bd)
    try:
        ib.move_berg_between_cells()
        rows, _ = [x[:, :live] for x in _raw_partner_rows(ib, n, 2)]   # before the count: the tail is still there
        assert rows.max() < live and (rows >= 0).any()
        assert ib.num_bergs() == (live, live)
        got = state(ib, 2)
        D.assert_same_by_id(*survivors(b, bd), *got, "chain of %d, every seventh dead, re-binned" % n)
        assert_tables(ib, *got, "chain of %d, every seventh dead, re-binned" % n, all_alive=False)
    finally:
        ib.close()


def _raw_partner_rows(ib, n, mb):
    rows, slots = np.full((mb, n), -7, dtype=np.int32), np.full((mb, n), -7, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert ib.lib.kid_bond_partner_rows(ib.h, rows.ctypes.data_as(ip), slots.ctypes.data_as(ip), n) == 0
    return rows, slots


# ---- 3. a compaction ----
def compaction(case, label, kill):
    grid, p, b, bd = case
    mb, n = bd["max_bonds"], len(b["lon"])
    b = kill(b)
    live = int((b["alive"] != 0).sum())
    ib = loaded(grid, p, b, bd)
    try:
        assert_tables(ib, b, bd, label + ": as uploaded", all_alive=live == n)
        ib.compact()
        assert ib.num_bergs() == (live, live)
        if live == 0:
            return
        got = state(ib, mb)
        want = survivors(b, bd)
        assert np.array_equal(got[0]["id"], want[0]["id"]), label + ": compaction keeps the order of the rows it keeps"
        D.assert_same_by_id(*want, *got, label + ": the survivors")
        assert_tables(ib, *got, label + ": after the compaction", all_alive=live == n)
        if live < n:
            rows, _ = ib.bond_partner_rows()
            named = np.arange(mb)[:, None] < got[1]["count"][None, :]
            lost = named & (rows < 0)
            assert lost.any(), label + ": no live berg had a dead partner"   # count and other_id are kept (by id, above), the row is gone
            assert not np.isin(got[1]["other_id"].reshape(mb, live)[lost], got[0]["id"]).any()
    finally:
        ib.close()


@pytest.mark.parametrize("kind", ["hex", "hex_partial", "square"])
def test_tables_through_a_compaction_lattice(kind):
    compaction(lattice(kind, 3), kind + ", every seventh dead", kill_every_seventh)


@pytest.mark.parametrize("n", [2, 65, 257])
def test_tables_through_a_compaction_chain(n):
    compaction(chain(n), "chain of %d, every seventh dead" % n, kill_every_seventh)


def test_compaction_of_nothing_and_of_everything():
    compaction(lattice("hex", 3), "hex, nothing dead", lambda b: b)
    compaction(chain(1), "one row, nothing dead", lambda b: b)

    def everything(b):
        b["alive"][:] = 0
        return b
    compaction(lattice("hex", 3), "hex, everything dead", everything)
    compaction(chain(65), "chain of 65, everything dead", everything)


# ---- 4. stepping does not notice ----
@pytest.mark.parametrize("kind,sub_steps", [("hex", 3), ("hex_partial", 3), ("square", 3), ("hex_grounded", 7)])
def test_stepping_does_not_notice(kind, sub_steps, monkeypatch):
    monkeypatch.delenv("KID_MTS_NO_FUSED", raising=False)
    monkeypatch.delenv("KID_MTS_FUSED_BLOCKS_CAP", raising=False)
    grid, p, b, bd = lattice(kind, sub_steps)
    mb = bd["max_bonds"]
    ia = loaded(grid, p, b, bd)
    try:
        ia.run(1)
        ids = ia.download_bergs()["id"]
        ia.move_berg_between_cells()
        assert not np.array_equal(ia.download_bergs()["id"], ids), kind + ": the re-binning moved no row"
        ia.run(1)
        ia.compact()
        ia.run(1)
        moved = snapshot(ia, mb)
        assert_tables(ia, moved[0], moved[1], kind + ": after the third step")
        assert ia.mts_fused_launches() == 3, "%s: %d fused launches in 3 steps (the case took the fall-back)" % (kind, ia.mts_fused_launches())
    finally:
        ia.close()
    ib = loaded(grid, p, b, bd, follow=False)
    try:
        ib.run(3)
        still = snapshot(ib, mb)
        assert ib.mts_fused_launches() == 3
    finally:
        ib.close()
    assert np.array_equal(still[0]["id"], b["id"]) and not np.array_equal(moved[0]["id"], b["id"])
    assert (moved[0]["alive"] == 1).all() and (still[0]["alive"] == 1).all()   # melt is off: nobody dies, the compaction is the identity
    assert_same_run(moved, still, kind + ": rows moved between the steps against rows that stayed")
    if kind == "hex_grounded":
        assert (still[1]["broken"] != 0).sum() > 0 and (moved[1]["broken"] != 0).sum() > 0   # bonds do break, lists shrink
    else:
        assert (still[1]["broken"] != 0).sum() == 0


# ---- 5. compaction against a fresh upload ----
def test_compaction_against_a_fresh_upload(monkeypatch):
    monkeypatch.delenv("KID_MTS_NO_FUSED", raising=False)
    monkeypatch.delenv("KID_MTS_FUSED_BLOCKS_CAP", raising=False)
    grid, p, b, bd = lattice("hex", 3)
    mb = bd["max_bonds"]
    b = kill_every_seventh(b)
    ia = loaded(grid, p, b, bd)
    try:
        ia.compact()
        ia.run(2)
        on_device = snapshot(ia, mb)
        assert ia.mts_fused_launches() == 2
    finally:
        ia.close()
    sb, sbd = survivors(b, bd)
    ib = loaded(grid, p, sb, sbd, follow=False)
    try:
        ib.run(2)
        fresh = snapshot(ib, mb)
        assert ib.mts_fused_launches() == 2
    finally:
        ib.close()
    assert np.array_equal(on_device[0]["id"], fresh[0]["id"])
    assert_same_run(on_device, fresh, "hex, every seventh dead: compacted on the device against the survivors uploaded")


# ---- 6. bonded bergs under the single-time-step scheme ----
@pytest.mark.parametrize("rk", [False, True], ids=["verlet", "rk4"])
def test_single_time_step_bonded_bergs_do_not_notice(rk):
    import rk_interactive as RK
    grid, p, b, bd, _ = RK.collision(rk)
    assert p.interactive_icebergs_on and not p.mts and p.iceberg_bonds_on and bool(p.Runge_not_Verlet) == rk
    n, mb = len(b["lon"]), bd["max_bonds"]
    # The case leaves all five `inorder` keys at zero, so inside a cell the traversal order -- the order in which a berg meets its
    # neighbours -- would be that of the rows.  start_day makes the order total, as synthetic.place_bergs does; without
    # footloose nothing else reads it.  Both handles get the same population.
    # (This case found that the skip rule of the row permutation left uvel_old / vvel_old, uploaded as zeros and written by the
    # interacting evolve, where they were: field_never_written of kid_rows.inc now counts interactive_icebergs_on like mts.)
    b["start_day"][:] = 1.0e-6 * np.arange(n)
    b, bd = D.permute_bonded(b, bd, np.random.default_rng(20240).permutation(n))
    ia = loaded(grid, p, b, bd)
    try:
        ia.run(1)
        ia.move_berg_between_cells()
        assert not np.array_equal(ia.download_bergs()["id"], b["id"]), "the re-binning moved no row"
        ia.run(1)
        ia.compact()
        ia.run(1)
        moved = snapshot(ia, mb)
        assert_tables(ia, moved[0], moved[1], "collision: after the third step")
    finally:
        ia.close()
    ib = loaded(grid, p, b, bd, follow=False)
    try:
        ib.run(3)
        still = snapshot(ib, mb)
    finally:
        ib.close()
    assert (moved[0]["alive"] == 1).all() and (still[0]["alive"] == 1).all()
    assert (still[1]["count"] > 0).any()
    assert_same_run(moved, still, "collision under %s: rows moved between the steps against rows that stayed" % ("RK4" if rk else "Verlet"))


# ---- 7. growth ----
def _in_use():
    dev, pin = C.c_int64(), C.c_int64()
    assert L.load().kid_memory_in_use(C.byref(dev), C.byref(pin)) == 0
    return dev.value, pin.value


@pytest.mark.parametrize("case", ["hex", "chain"])
def test_tables_through_growth(case):
    grid, p, b, bd = lattice("hex", 3) if case == "hex" else chain(257)
    mb, n = bd["max_bonds"], len(b["lon"])
    start = _in_use()
    ib = loaded(grid, p, b, bd)
    try:
        before = state(ib, mb)
        held = [_in_use()[0]]
        ib.move_berg_between_cells()
        held.append(_in_use()[0])
        assert held[1] - held[0] >= (n + PAD) * (4 + mb * 116), "the second set of bond tables is not accounted for"
        first = state(ib, mb)
        assert not np.array_equal(first[0]["id"], before[0]["id"])
        ib.reserve(2 * (n + PAD))
        assert ib.capacity == 2 * (n + PAD)
        grown = state(ib, mb)
        assert_rows_unchanged(*first, *grown, case + ": kid_reserve keeps the rows")
        assert_tables(ib, *grown, case + ": after kid_reserve")
        ib.move_berg_between_cells()
        again = state(ib, mb)
        D.assert_same_by_id(*before, *again, case + ": re-binning at the new stride")
        assert_tables(ib, *again, case + ": re-binning at the new stride")
        ib.compact()
        last = state(ib, mb)
        assert_rows_unchanged(*again, *last, case + ": a compaction of nothing")
        assert_tables(ib, *last, case + ": after the compaction")
    finally:
        ib.close()
    assert _in_use() == start
