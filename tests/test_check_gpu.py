"""The debug-mode invariants on the device (icebergs_amd/csrc/kid_check.inc): kid_check_bergs and kid_sorted_ids against the planted
populations of tests/check_cases.py and the host restatement tests/check_ref.py.

Counts are compared exactly.  The position check recomputes xi, yj with the device function that kid_locate_bergs stores from, so
a located state has no mismatch, bit for bit.  The oracle's pos_within_cell differs from the device's by rounding (1e-9 in
tests/test_locate_gpu.py: a refined reciprocal against the IEEE quotient), so the host restatement of the position check is run on
the state whose unplanted xi, yj are the oracle's own, with the same plants in the same rows (tests/test_check_cpu.py): both must
give the planted numbers.  After stepping, max_dxi and max_dyj are held to parity.TOL_TRAJ, the project's standing tolerance for
xi, yj; the count of bitwise mismatches there is printed, not asserted (DESIGN 7.3 records it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import check_cases as CC                  # noqa: E402
import check_ref as CR                    # noqa: E402
import halo_bergs as HB                   # noqa: E402
import parity as P                        # noqa: E402
from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -4
MEMBERS = list(T.BERG_F64_NAMES) + list(T.BERG_I32_NAMES) + ["id"]
COUNTS = ("n_xiyj", "n_land", "n_in_halo", "n_identical", "n_same_id", "n_same_berg", "n_dup_ids")
X, L, SI, DI = 0, 1, 2, 3                # first_id / first_row: xiyj, land, same_id, dup_ids


def _icebergs(grid, p, cap):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)      # (an AttributeError from check_bergs on a library without the symbol fails the test)


def _memory(ib):
    dev, pin = C.c_int64(), C.c_int64()
    assert ib.lib.kid_memory_in_use(C.byref(dev), C.byref(pin)) == 0
    return dev.value, pin.value


def _errors(ib):
    return float(ib.fetch()[2][T.ENUMS["KID_S_ERROR_COUNT"]])


def _same_bits(a, b):
    return all(a[m].dtype == b[m].dtype and a[m].tobytes() == b[m].tobytes() for m in MEMBERS)


_located = {}


def _located_box(mask=False):
    """the 257 rows of the box after kid_locate_bergs on the device (downloaded once): xi, yj as the device function gives them"""
    if mask not in _located:
        g = CC.box_grid(mask)
        b = CC.box_bergs()
        ib = _icebergs(g, CC.box_params(), CC.N)
        try:
            ib.upload_bergs(b)
            counts = ib.locate_bergs("search")
            assert counts["found"] == CC.N - CC.N // 7
            _located[mask] = ib.download_bergs()
        finally:
            ib.close()
    return S.copy_bergs(_located[mask])


# ---- shapes ----
@pytest.mark.parametrize("n", CC.SHAPES)
def test_located_rows_are_clean(n):
    g = CC.box_grid()
    b = CC.box_bergs(n)
    ib = _icebergs(g, CC.box_params(), n)
    try:
        ib.upload_bergs(b)
        ib.locate_bergs("search")
        before = _memory(ib)
        r = ib.check_bergs()
        assert _memory(ib) == before
        assert r["n_rows"] == n - n // 7
        assert all(r[k] == 0 for k in COUNTS), r
        assert r["max_dxi"] == 0.0 and r["max_dyj"] == 0.0
        assert r["first_id"] == [-1] * 4 and r["first_row"] == [-1] * 4
        ids = ib.sorted_ids()
        assert ids.dtype == np.int64 and np.array_equal(ids, np.sort(b["id"][b["alive"] != 0]))
        for name, mask in ib.CHECKS.items():           # every part alone, by name and by mask
            assert ib.check_bergs(name) == ib.check_bergs(mask)
    finally:
        ib.close()


def test_no_rows_at_all():
    ib = _icebergs(CC.box_grid(), CC.box_params(), 8)
    try:
        r = ib.check_bergs()
        assert all(r[k] == 0 for k in COUNTS + ("n_rows",)) and r["first_id"] == [-1] * 4 and len(ib.sorted_ids()) == 0
    finally:
        ib.close()


# ---- position, planted ----
def test_planted_positions():
    g = CC.box_grid(mask=True)
    d = g["desc"]
    b = _located_box(mask=True)
    want = CC.plant_positions(b, d)
    ib = _icebergs(g, CC.box_params(), CC.N)
    try:
        ib.upload_bergs(b)
        errors = _errors(ib)
        r = ib.check_bergs("position")
        assert r["n_rows"] == CC.N - CC.N // 7
        assert (r["n_xiyj"], r["n_land"]) == (want["n_xiyj"], want["n_land"]) == (6, 1)
        assert r["first_id"][X] == want["first_xiyj"] and r["first_row"][X] in want["rows_xiyj"] and b["id"][r["first_row"][X]] == want["first_xiyj"]
        assert r["first_id"][L] == want["first_land"] and r["first_row"][L] == CC.LAND_ROW
        assert r["max_dxi"] == want["max_dxi"] and r["max_dyj"] == want["max_dyj"]      # one ulp; the NaN row does not poison it
        assert 0.0 < r["max_dxi"] <= 2.0 ** -52 and 0.0 < r["max_dyj"] <= 2.0 ** -52
        assert r["n_in_halo"] == 0 and r["n_same_id"] == 0                                # not asked for
        full = ib.check_bergs()
        assert full["n_in_halo"] == want["n_in_halo"] == CR.count_out_of_order(b, d)[0] == 1
        assert {k: full[k] for k in ("n_rows", "n_xiyj", "n_land", "max_dxi", "max_dyj")} == {k: r[k] for k in ("n_rows", "n_xiyj", "n_land", "max_dxi", "max_dyj")}
        assert _same_bits(ib.download_bergs(), b)                                          # no word of any row changed
        assert _errors(ib) == errors
    finally:
        ib.close()


# ---- duplicates, planted ----
@pytest.mark.parametrize("mts", [False, True])
def test_planted_duplicates(mts):
    g = CC.box_grid()
    d = g["desc"]
    b = CC.box_bergs()
    want = CC.plant_duplicates(b, d)
    ref = CR.report(b, d, mts)
    ib = _icebergs(g, CC.box_params(mts), CC.N)
    try:
        ib.upload_bergs(b)
        r = ib.check_bergs(("order", "duplicates", "ids"))
        print("planted duplicates, mts %s: %s" % (mts, {k: r[k] for k in COUNTS}))
        assert r["n_same_id"] == want["n_same_id"] == ref["n_same_id"] == 2086
        assert r["n_same_berg"] == (want["n_same_berg_mts"] if mts else want["n_same_berg"]) == ref["n_same_berg"]
        assert r["n_identical"] == want["n_identical"] == ref["n_identical"] == 66
        assert r["n_dup_ids"] == want["n_dup_ids"] == ref["n_dup_ids"] == 1
        assert r["n_in_halo"] == want["n_in_halo"] == ref["n_in_halo"] == 1
        assert r["n_rows"] == 0 and r["n_xiyj"] == 0
        assert r["first_id"][SI] == want["first_same_id"] and r["first_row"][SI] in want["rows_same_id"] and b["id"][r["first_row"][SI]] == want["first_same_id"]
        assert r["first_id"][DI] == want["first_dup_id"] and r["first_row"][DI] in want["rows_dup_id"]
        # each counter alone sees its own offenders only
        only = ib.check_bergs("ids")
        assert only["n_dup_ids"] == 1 and only["n_same_id"] == 0 and only["n_identical"] == 0 and only["first_id"][SI] == -1
        only = ib.check_bergs("duplicates")
        assert only["n_same_id"] == 2086 and only["n_dup_ids"] == 0 and only["n_identical"] == 0 and only["n_in_halo"] == 0
        only = ib.check_bergs("order")
        assert only["n_identical"] == 66 and only["n_in_halo"] == 1 and only["n_same_id"] == 0
        ids = ib.sorted_ids()
        assert np.array_equal(ids, np.sort(b["id"][CR.on_domain(b, d)]))       # the dead row and the two rows in halo cells are left out
        assert _same_bits(ib.download_bergs(), b)
    finally:
        ib.close()


# ---- layout ----
def test_report_does_not_depend_on_the_layout():
    g = CC.box_grid(mask=True)
    d = g["desc"]
    b = _located_box(mask=True)
    CC.plant_positions(b, d)
    free = [k for k in CC.live_rows(b) if k not in CC.XI_ROWS + (CC.YJ_ROW, CC.NAN_ROW, CC.LAND_ROW, CC.HALO_ROW)]
    # duplicates beside the position plants: three rows with one set of keys, two rows with one id
    trio = (free[0], free[100], free[200])
    assert len({(int(b["ine"][k]), int(b["jne"][k])) for k in trio}) == 3          # three cells: no identicals
    for k in trio[1:]:
        CC.copy_row(b, k, trio[0], CC.KEYS)
    b["id"][free[4]] = b["id"][free[3]]
    rng = np.random.Generator(np.random.PCG64(17))
    perm = rng.permutation(CC.N)
    shuffled = {k: (v[perm].copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}

    def strip(r):
        return {k: v for k, v in r.items() if k != "first_row"}

    reports = {}
    for name in ("reference order", "shuffled", "re-binned", "compacted", "grown"):
        ib = _icebergs(g, CC.box_params(), CC.N)
        try:
            ib.upload_bergs(shuffled if name == "shuffled" else b)
            if name == "re-binned":
                ib.move_berg_between_cells()
            elif name == "compacted":
                ib.compact()
            elif name == "grown":
                ib.reserve(4 * CC.N)
            before = _memory(ib)
            r = ib.check_bergs()
            assert _memory(ib) == before, name
            now = ib.download_bergs()
            for q in range(4):
                assert r["first_id"][q] >= 0 and now["alive"][r["first_row"][q]] != 0 and now["id"][r["first_row"][q]] == r["first_id"][q], (name, q)
            reports[name] = strip(r)
        finally:
            ib.close()
    first = reports["reference order"]
    assert first["n_xiyj"] == 6 and first["n_land"] == 1 and first["n_in_halo"] == 1 and first["n_same_id"] == 3 and first["n_identical"] == 0 and first["n_dup_ids"] == 1
    for name, r in reports.items():
        assert r == first, (name, r, first)


# ---- halo copies resident ----
def test_with_halo_copies_resident():
    import test_halo_bergs_gpu as HG
    nic, njc = 7, 5
    g, b, halo_recs, halo_cells = HG._small_population(nic, njc)
    m = len(b["lon"])
    owners = b["id"][:len(halo_cells)]                      # the copies carry ids that owned rows of this tile carry too
    halo_recs[:, 31] = (owners >> 32).astype(np.int32)
    halo_recs[:, 32] = (owners & 0xffffffff).astype(np.uint32).astype(np.int32)
    ib = _icebergs(g, HB.params(False), 128)
    try:
        ib.upload_bergs(b)
        clean = ib.check_bergs(("order", "duplicates", "ids"))
        ids = ib.sorted_ids()
        ib.unpack_immigrants(halo_recs)
        assert ib.halo_berg_count() == len(halo_cells) == 16
        r = ib.check_bergs()                                # KID_OK with halo rows resident
        assert r["n_rows"] == int((b["alive"] != 0).sum()) + 16
        for k in ("n_in_halo", "n_identical", "n_same_id", "n_same_berg", "n_dup_ids"):
            assert r[k] == clean[k] == 0, k
        assert np.array_equal(ib.sorted_ids(), ids) and len(ids) == int((b["alive"] != 0).sum()) == m - 2
        assert ib.halo_berg_count() == 16
    finally:
        ib.close()


# ---- after stepping ----
def _c2(verlet):
    grid, p, b = S.config_c2(n=300, seed=4)
    if verlet:
        p.Runge_not_Verlet = 0
    return grid, p, b, None


def _interacting_box():
    import rk_interactive as RK
    grid, p, b, bonds, _ = RK.box(False, True)
    return grid, p, b, bonds


STEPPED = {"rk4-latlon-fused": lambda: _c2(False), "verlet-latlon": lambda: _c2(True), "rk4-interacting-box": _interacting_box}


@pytest.mark.parametrize("case", sorted(STEPPED))
def test_after_sixteen_steps(case):
    grid, p, b, bonds = STEPPED[case]()
    d = grid["desc"]
    n = len(b["lon"])
    assert 240 <= n <= 300
    ib = _icebergs(grid, p, n)
    try:
        ib.upload_bergs(b)
        if bonds is not None:
            ib.upload_bonds(bonds)
        ib.run(16)
        r = ib.check_bergs()
        now = ib.download_bergs()
        ulp = max(r["max_dxi"], r["max_dyj"]) / 2.0 ** -53
        print("after 16 steps, %s: n_rows %d, n_xiyj %d (bitwise mismatches of stored xi, yj against pos_within_cell<false>), max_dxi %.3e, max_dyj %.3e (%.1f units of 2^-53), redo %d"
              % (case, r["n_rows"], r["n_xiyj"], r["max_dxi"], r["max_dyj"], ulp, ib.last_redo_count()))
        assert r["n_rows"] == int((now["alive"] != 0).sum()) > 200
        assert r["n_land"] == 0
        ref = CR.report(now, d, bool(p.mts))
        for k in ("n_same_id", "n_same_berg", "n_dup_ids", "n_identical", "n_in_halo"):
            assert r[k] == ref[k], (k, r[k], ref[k])
        assert r["max_dxi"] <= P.TOL_TRAJ and r["max_dyj"] <= P.TOL_TRAJ
    finally:
        ib.close()


# ---- arguments ----
def test_arguments():
    g = CC.box_grid()
    b = CC.box_bergs(65)
    ib = _icebergs(g, CC.box_params(), 65)
    try:
        ib.upload_bergs(b)
        rep = T.CheckReport()
        for what in (0, 16, 31, 1 << 31):
            assert ib.lib.kid_check_bergs(ib.h, what, C.byref(rep)) == EINVAL and b"kid_check_bergs" in ib.lib.kid_last_error(ib.h), what
        assert ib.lib.kid_check_bergs(ib.h, 15, None) == EINVAL
        assert ib.lib.kid_check_bergs(None, 15, C.byref(rep)) == EINVAL
        n = C.c_int64(-1)
        live = int((b["alive"] != 0).sum())
        buf = np.full(live + 3, -7, dtype=np.int64)
        p64 = buf.ctypes.data_as(C.POINTER(C.c_int64))
        assert ib.lib.kid_sorted_ids(ib.h, p64, live - 1, C.byref(n)) == ECAPACITY and n.value == live and np.all(buf == -7)
        assert ib.lib.kid_sorted_ids(ib.h, None, 0, C.byref(n)) == 0 and n.value == live
        assert ib.lib.kid_sorted_ids(ib.h, p64, live, None) == EINVAL
        assert ib.lib.kid_sorted_ids(ib.h, p64, live, C.byref(n)) == 0 and n.value == live
        assert np.array_equal(buf[:live], np.sort(b["id"][b["alive"] != 0])) and np.all(buf[live:] == -7)
    finally:
        ib.close()
    # a handle without a static grid: the position check is refused, the others run
    h = C.c_void_p()
    lib = ib.lib
    d, p = g["desc"], CC.box_params()
    assert lib.kid_create(C.byref(d), C.byref(p), 16, 0, C.byref(h)) == 0
    try:
        rep = T.CheckReport()
        assert lib.kid_check_bergs(h, T.ENUMS["KID_CHECK_POSITION"], C.byref(rep)) == EINVAL and b"kid_set_static_grid" in lib.kid_last_error(h)
        assert lib.kid_check_bergs(h, T.ENUMS["KID_CHECK_ALL"], C.byref(rep)) == EINVAL
        assert lib.kid_check_bergs(h, T.ENUMS["KID_CHECK_ALL"] - T.ENUMS["KID_CHECK_POSITION"], C.byref(rep)) == 0
    finally:
        lib.kid_destroy(h)


# ---- two HIP ranks on one GPU ----
def _worker(rank, world, port, out_dir):
    import test_decomposed as TD
    from icebergs_amd.decomposed import TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nbergs = 300
    whole, p, b = TD._population(world, nbergs)
    S.set_diag_all(p)
    sel = (b["ine"] - 1) // TD.NI == rank
    big = S.empty_bergs(nbergs)
    m = int(sel.sum())
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            big[k][:m] = v[sel]
    big["ine"][:m] -= rank * TD.NI
    big["_n"] = m
    run = TD.HipRun(TD._grid(rank, world), p, big, nbergs)
    ex = TileExchange(world, 1, dist)
    for _ in range(10):
        ex.step(run.tile)
    stepped = ex.check_duplicates(run.tile)
    # one id on both tiles: every rank gives one of its live rows the smallest id rank 0 holds
    lowest = int(run.tile.sorted_ids()[0]) if rank == 0 else 0
    box = [None] * world
    dist.all_gather_object(box, lowest)
    now = run.ib.download_bergs()
    if rank != 0:
        k = int(np.nonzero((now["alive"] != 0) & (now["ine"] >= 1) & (now["ine"] <= TD.NI) & (now["jne"] >= 1) & (now["jne"] <= TD.NJ))[0][0])
        now["id"][k] = box[0]
        run.ib.upload_bergs(now)
    planted = ex.check_duplicates(run.tile)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([stepped, planted, (ex.sent, ex.received)], dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


def test_two_hip_ranks_on_one_gpu(tmp_path):
    port = 31700 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    got = [np.load(os.path.join(str(tmp_path), "rank%d.npy" % r)) for r in range(2)]
    for g in got:
        assert tuple(g[0]) == (0, 0) and tuple(g[1]) == (0, 1), g
    assert sum(int(g[2][0]) for g in got) == sum(int(g[2][1]) for g in got) > 0      # bergs did migrate
