"""Halo bergs of a decomposed run on the device (csrc/kid_halo_bergs.inc): kid_pack_halo_bergs_pair against the numpy
selection of tests/halo_bergs.py, the lifetime of a halo row (unpacked before kid_evolve_icebergs, retired by it), 2 x 2 HIP tiles on
one GPU against the undivided handle and the undivided oracle for both searches, the control without the update, and two gloo
ranks through TileExchange.step_interactive."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import halo_bergs as HB                   # noqa: E402
import test_halo_bergs_cpu as HBC         # noqa: E402
import test_halo_planes_cpu as HC         # noqa: E402  (assemble, the five outputs)

pytestmark = pytest.mark.gpu

H = S.HALO
EINVAL, EUNSUPPORTED = -1, -5
# tiles against the undivided handle: the rule and margin of DESIGN 7.5, 4 x max(d_cpu, 1e-12).  d_cpu is the oracle's own
# tiles-versus-whole deviation (HBC.D_CPU, measured by tests/test_halo_bergs_cpu.py); 1e-12 is the level this project allows between
# two summation orders; tiles and whole share the device arithmetic, and the factor 4 covers the reduction order in the planes.
BOUND = 4.0 * max(HBC.D_CPU, 1e-12)
EMPTY = np.empty((0, 34))


def _icebergs(grid, p, cap):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)


# ---- pack ----
def _small_population(nic, njc):
    """one berg in every cell of the nic x njc tile and a second one in every third, two of them dead; and records for halo rows
    in the halo cells around it (the corner columns included), as a neighbour would have sent them"""
    g = S.cartesian_grid(ni=nic, nj=njc, gridres=HB.RES)
    rng = np.random.default_rng(3)
    cells = [(i, j) for j in range(1, njc + 1) for i in range(1, nic + 1)]
    cells += cells[::3]
    n = len(cells)
    b = S.empty_bergs(n)
    ine, jne = np.array(cells, dtype=np.int32).T
    xi, yj = rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)
    b["ine"][:], b["jne"][:], b["xi"][:], b["yj"][:] = ine, jne, xi, yj
    b["lon"][:], b["lat"][:] = (ine - 1 + xi) * HB.RES, (jne - 1 + yj) * HB.RES
    for f in T.BERG_F64_NAMES:                        # every real of the record distinct and non-zero
        if f not in ("lon", "lat", "xi", "yj", "halo_berg", "static_berg", "fl_k"):
            b[f][:] = rng.uniform(1.0, 2.0, n)
    b["start_year"][:] = 1990 + np.arange(n)
    b["id"][:] = (np.arange(n, dtype=np.int64) % 5 << 32) | (1000 + np.arange(n, dtype=np.int64))
    b["alive"][[4, 20]] = 0
    halo_cells = [(0, 2), (-1, 4), (-2, 1), (8, 1), (9, 3), (11, 5), (10, 2), (0, 5), (8, 4), (-2, 3), (11, 1), (8, 5), (3, 0), (5, 7), (-1, -1), (9, 8)]
    hb = S.empty_bergs(len(halo_cells))
    hi_, hj_ = np.array(halo_cells, dtype=np.int32).T
    hb["lon"][:], hb["lat"][:] = (hi_ - 0.5) * HB.RES, (hj_ - 0.25) * HB.RES
    hb["ine"][:], hb["jne"][:] = hi_ + 3, hj_                      # the sender's own indices: the receiver finds the cell
    for f in ("mass", "thickness", "width", "length", "uvel", "vvel"):
        hb[f][:] = rng.uniform(1.0, 2.0, len(halo_cells))
    hb["id"][:] = 5000 + np.arange(len(halo_cells))
    return g, b, HB.np_records(hb, np.arange(len(halo_cells)), halo=1.0), halo_cells


def test_pack_against_the_numpy_selection():
    """a 7 x 5 tile (halo 4), 47 rows placed cell by cell and 16 halo rows from an unpack (four of them north and south of the tile: never selected): for widths 2, 3 and 4, both axes and
    missing sides the packed ids are the numpy selection's, every record is the emigrants' record of that berg with real 30 = 1,
    and the rows are bit for bit what they were"""
    nic, njc = 7, 5
    g, b, halo_recs, halo_cells = _small_population(nic, njc)
    p = HB.params(False)
    ib = _icebergs(g, p, 128)
    other = _icebergs(g, p, 128)
    try:
        # what kid_pack_emigrants writes for a berg is the numpy record: the same rows, moved one cell east of the tile
        moved = S.copy_bergs(b)
        moved["alive"][:] = 1
        moved["ine"][:] = nic + 1
        other.upload_bergs(moved)
        east = other.pack_emigrants(T.ENUMS["KID_DIR_E"])
        want = HB.np_records(moved, np.arange(len(moved["lon"])))
        assert east.shape == want.shape and np.array_equal(east[np.argsort(HB.record_ids(east))], want[np.argsort(HB.record_ids(want))])
        ib.upload_bergs(b)
        assert ib.halo_berg_count() == 0
        ib.unpack_immigrants(halo_recs)
        assert ib.halo_berg_count() == len(halo_cells)
        before = ib.download_bergs()
        m = len(b["lon"])
        assert np.array_equal(before["halo_berg"][m:], np.ones(len(halo_cells)))
        assert [(int(i), int(j)) for i, j in zip(before["ine"][m:], before["jne"][m:])] == halo_cells
        for w in (2, 3, 4):
            for axis in (0, 1):
                hi, lo = HB.np_halo_select(before["ine"], before["jne"], before["alive"], axis, w, nic, njc)
                assert len(hi) > 0 and len(lo) > 0
                if axis == 1:
                    assert (before["halo_berg"][hi] >= 0.5).any() and (before["halo_berg"][lo] >= 0.5).any()   # halo rows are sent on
                for sides in ((True, True), (True, False), (False, True), (False, False)):
                    got = ib.pack_halo_bergs_pair(axis, w, sides)
                    for recs, rows, on in zip(got, (hi, lo), sides):
                        if not on:
                            assert len(recs) == 0
                            continue
                        want = HB.np_records(before, rows, halo=1.0)
                        assert len(recs) == len(rows), (axis, w, sides)
                        o1, o2 = np.argsort(HB.record_ids(recs)), np.argsort(HB.record_ids(want))
                        assert np.array_equal(HB.record_ids(recs)[o1], before["id"][rows][o2]), (axis, w, sides)
                        assert np.array_equal(recs[o1].view(np.int64), want[o2].view(np.int64)), (axis, w, sides)
                        assert np.all(recs[:, 29] == 1.0)
        hi0, lo0 = ib.pack_halo_bergs_pair(0, 0)                     # width 0: the grid's halo
        hi4, lo4 = ib.pack_halo_bergs_pair(0, 4)
        assert np.array_equal(hi0, hi4) and np.array_equal(lo0, lo4)
        after = ib.download_bergs()
        for k, v in before.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, after[k]), k
        # a buffer too small: the count comes back, nothing else
        n_hi, n_lo = C.c_int64(), C.c_int64()
        small = np.full((2, 34), -7.0)
        rc = ib.lib.kid_pack_halo_bergs_pair(ib.h, 0, 4, small.ctypes.data_as(C.POINTER(C.c_double)), 2, C.byref(n_hi), None, 0, C.byref(n_lo))
        assert rc == -4 and n_hi.value == len(HB.np_halo_select(before["ine"], before["jne"], before["alive"], 0, 4, nic, njc)[0]) and n_lo.value == 0
        assert np.all(small == -7.0)
    finally:
        ib.close()
        other.close()


def test_pack_refusals():
    """widths 1, 5 (> halo) and 4 on a tile of 3 rows: KID_EINVAL; bonded, mts, footloose and non-interacting namelists:
    KID_EUNSUPPORTED, each by name; nothing is written"""
    n_hi, n_lo = C.c_int64(), C.c_int64()
    a, b = np.full((64, 34), -7.0), np.full((64, 34), -7.0)
    dp = C.POINTER(C.c_double)

    def call(ib, axis, w):
        return ib.lib.kid_pack_halo_bergs_pair(ib.h, axis, w, a.ctypes.data_as(dp), 64, C.byref(n_hi), b.ctypes.data_as(dp), 64, C.byref(n_lo))
    for nic, njc, bad, good in ((7, 5, (1, 5, -1), 4), (7, 3, (4,), 3)):
        g, bergs, _, _ = _small_population(nic, njc)
        ib = _icebergs(g, HB.params(False), 128)
        try:
            ib.upload_bergs(bergs)
            for axis in (0, 1):
                for w in bad:
                    assert call(ib, axis, w) == EINVAL and b"width" in ib.lib.kid_last_error(ib.h), (axis, w)
                assert call(ib, axis, good) == 0 and n_hi.value > 0 and n_lo.value > 0
            assert call(ib, 2, good) == EINVAL and call(ib, -1, good) == EINVAL
            a[:], b[:] = -7.0, -7.0
            # (footloose and find_melt_using_spread_mass cannot be set together with interacting bergs at all: kid_set_params)
            for word, changes in ((b"iceberg_bonds_on", {"iceberg_bonds_on": 1}), (b"mts", {"mts": 1, "old_interp_flds_order": 0}),
                                  (b"footloose", {"footloose": 1, "interactive_icebergs_on": 0}), (b"interactive_icebergs_on", {"interactive_icebergs_on": 0}),
                                  (b"static_icebergs", {"static_icebergs": 1}),
                                  (b"find_melt_using_spread_mass", {"find_melt_using_spread_mass": 1, "interactive_icebergs_on": 0})):
                q = HB.params(False)
                for k, v in changes.items():
                    setattr(q, k, v)
                ib.set_params(q)
                assert call(ib, 0, good) == EUNSUPPORTED, word
                msg = ib.lib.kid_last_error(ib.h)
                assert word in msg and b"kid_pack_halo_bergs_pair" in msg, msg
                assert n_hi.value == 0 and n_lo.value == 0
            assert np.all(a == -7.0) and np.all(b == -7.0)
        finally:
            ib.close()


# ---- lifetime ----
def test_lifetime_of_halo_rows():
    """tile (0, 0) of the box takes the copies its east neighbour packs: resident until kid_evolve_icebergs, which retires them"""
    from icebergs_amd.lib import KidError
    whole, b = HB.population()
    p = HB.params(False)
    west = _icebergs(HB.tile_grid(0, 0, whole), p, 400)
    east = _icebergs(HB.tile_grid(1, 0, whole), p, 400)
    try:
        west.upload_bergs(HB.trim(HB.split_bergs(b, 0, 0, 400)))
        east.upload_bergs(HB.trim(HB.split_bergs(b, 1, 0, 400)))
        owned = west.download_bergs()
        n_owned = len(owned["id"])
        assert west.halo_berg_count() == 0
        _, to_west = east.pack_halo_bergs_pair(0, 0, (False, True))
        assert len(to_west) > 10
        west.unpack_immigrants_pair(EMPTY, to_west)
        assert west.halo_berg_count() == len(to_west) and west.num_bergs() == (n_owned + len(to_west), n_owned + len(to_west))
        got = west.download_bergs()
        halo_ids = got["id"][n_owned:]
        assert np.array_equal(np.sort(halo_ids), np.sort(HB.record_ids(to_west))) and np.all(got["ine"][n_owned:] > HB.NI)
        for name, call in (("kid_thermodynamics", lambda: west._check(west.lib.kid_thermodynamics(west.h), "kid_thermodynamics")),
                           ("kid_budget", west.budget), ("kid_stock", lambda: west.stock(T.ENUMS["KID_STOCK_WATER"])),
                           ("kid_pack_emigrants", lambda: west.pack_emigrants_pair(0)), ("kid_move_berg_between_cells", west.move_berg_between_cells),
                           ("kid_calculate_mass_on_ocean", west.calculate_mass_on_ocean), ("kid_step_gather", west.step_gather),
                           ("kid_bergs_chksum", west.bergs_chksum)):
            with pytest.raises(KidError, match="rc=-1 .*halo rows"):
                call()
        west._check(west.lib.kid_zero_accumulators(west.h), "kid_zero_accumulators")
        west._check(west.lib.kid_evolve_icebergs(west.h), "kid_evolve_icebergs")
        assert west.halo_berg_count() == 0
        after = west.download_bergs()
        assert not after["alive"][n_owned:].any() and np.all(after["ine"][n_owned:] == 1) and np.all(after["jne"][n_owned:] == 1)
        for f in ("lon", "lat", "uvel", "vvel", "axn", "bxn"):          # never moved
            assert np.array_equal(after[f][n_owned:], got[f][n_owned:]), f
        inside = (after["ine"][:n_owned] >= 1) & (after["ine"][:n_owned] <= HB.NI) & (after["jne"][:n_owned] >= 1) & (after["jne"][:n_owned] <= HB.NJ)
        assert west.num_bergs()[1] == int(inside.sum()) == int((after["alive"][:n_owned] != 0).sum())
        assert np.any(after["uvel"][:n_owned] != owned["uvel"])
        west._check(west.lib.kid_thermodynamics(west.h), "kid_thermodynamics")      # allowed again
        west.calculate_mass_on_ocean()
        west.step_gather()
        assert west.fetch()[2][T.ENUMS["KID_S_ERROR_COUNT"]] == 0.0
        for axis in (0, 1):
            for recs in west.pack_emigrants_pair(axis):
                assert not set(HB.record_ids(recs)) & set(halo_ids)
        west.compact()
        assert west.num_bergs() == (int(inside.sum()), int(inside.sum()))
        # and the re-binning drops them as well
        west.unpack_immigrants_pair(EMPTY, to_west)
        west._check(west.lib.kid_evolve_icebergs(west.h), "kid_evolve_icebergs")
        west.pack_emigrants_pair(0), west.pack_emigrants_pair(1)
        west.move_berg_between_cells()
        slots, alive = west.num_bergs()
        assert slots == alive and not set(west.download_bergs()["id"]) & set(halo_ids)
    finally:
        west.close()
        east.close()


# ---- 2 x 2 tiles against the undivided handle and the undivided oracle ----
def _swap(tiles, pack, unpack):
    moved = 0
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
        out = {}
        for (tx, ty), ib in tiles.items():
            out[(tx, ty)] = pack(ib, axis, ((tx + dx, ty + dy) in tiles, (tx - dx, ty - dy) in tiles))
        for (tx, ty), ib in tiles.items():
            lo, hi = (tx - dx, ty - dy), (tx + dx, ty + dy)
            from_lo, from_hi = out[lo][0] if lo in out else EMPTY, out[hi][1] if hi in out else EMPTY
            moved += len(from_lo) + len(from_hi)
            unpack(ib, axis, from_lo, from_hi)
    return moved


def _tiles_step(tiles, contact, update):
    """TileExchange.step_interactive for every tile (old_interp_flds_order on), the three exchanges swapped in process"""
    def call(ib, name):
        ib._check(getattr(ib.lib, name)(ib.h), name)
    copies = 0
    for ib in tiles.values():
        call(ib, "kid_zero_accumulators")
    if update:
        copies = _swap(tiles, lambda ib, axis, sides: ib.pack_halo_bergs_pair(axis, 0, sides), lambda ib, axis, lo, hi: ib.unpack_immigrants_pair(lo, hi))
    for ib in tiles.values():
        if contact:
            ib.set_conglom_ids()
        call(ib, "kid_evolve_icebergs")
    moved = _swap(tiles, lambda ib, axis, sides: ib.pack_emigrants_pair(axis), lambda ib, axis, lo, hi: ib.unpack_immigrants_pair(lo, hi))
    for ib in tiles.values():
        call(ib, "kid_thermodynamics")
        call(ib, "kid_calculate_mass_on_ocean")

    def pack_planes(ib, axis, sides):
        n = ib.halo_buffer_count(axis)
        return ib.pack_halo_pair(axis, out=tuple(np.empty(n) if s else None for s in sides))
    _swap(tiles, pack_planes, lambda ib, axis, lo, hi: ib.unpack_halo_pair(axis, lo if lo is not EMPTY else None, hi if hi is not EMPTY else None))
    for ib in tiles.values():
        call(ib, "kid_step_gather")
    return copies, moved


def _live(b):
    a = (b["alive"] != 0) & (b["halo_berg"] < 0.5)
    return {k: b[k][a] for k in HB.FIELDS + ("id",)}


def _two_by_two(contact, update, check_at):
    whole, b = HB.population()
    p = HB.params(contact)
    n = len(b["lon"])
    ref = _icebergs(whole, p, n)
    tiles = {}
    try:
        ref.upload_bergs(HB.trim(dict(b, _n=n)))
        for tx in range(HB.NTX):
            for ty in range(HB.NTY):
                ib = _icebergs(HB.tile_grid(tx, ty, whole), p, 400)
                assert ib.buffer_width() == 34
                ib.upload_bergs(HB.trim(HB.split_bergs(b, tx, ty, 400)))
                tiles[(tx, ty)] = ib
        copies = moved = 0
        res = {}
        for step in range(1, max(check_at) + 1):
            ref.run(1)
            c, m = _tiles_step(tiles, contact, update)
            copies, moved = copies + c, moved + m
            if step in check_at:
                want_out = ref.fetch()[1][:, H:H + HB.NJ * HB.NTY, H:H + HB.NI * HB.NTX].copy()
                got_out = HC.assemble({k: ib.fetch()[1][:, H:H + HB.NJ, H:H + HB.NI].copy() for k, ib in tiles.items()}, HB.NTX, HB.NTY)
                res[step] = (_live(ref.download_bergs()), HB.join([_live(ib.download_bergs()) for ib in tiles.values()]), want_out, got_out)
        for ib in tiles.values():
            assert ib.halo_berg_count() == 0 and ib.fetch()[2][T.ENUMS["KID_S_ERROR_COUNT"]] == 0.0
        return res, copies, moved
    finally:
        ref.close()
        for ib in tiles.values():
            ib.close()


@pytest.mark.parametrize("contact", [False, True])
def test_two_by_two_tiles_match_the_undivided_handle_and_oracle(contact):
    """after steps 1, 20 and 40: the same survivors, every field of the owned bergs and the five gathered outputs within BOUND of
    the undivided handle's, and the bergs within 1e-9 of the undivided oracle's.  Measured on an MI355X (one run): bergs equal to
    the bit with both searches, outputs 3.4e-16 (3 x 3) and 2.9e-16 (contact); against the oracle 3.7e-12 and 2.8e-12."""
    res, copies, moved = _two_by_two(contact, True, HB.CHECK_AT)
    oracle = HB.whole_oracle(contact)[0]
    assert copies > 1000 and moved >= 20, (copies, moved)
    worst = worst_out = worst_oracle = 0.0
    for step in HB.CHECK_AT:
        want, got, want_out, got_out = res[step]
        dev = HB.compare(got, want)
        dev_out, _ = HC.deviations(got_out, want_out)
        dev_or = HB.compare(got, oracle[step])
        print("step", step, "contact", contact, "bergs", max(dev.values()), "outputs", max(dev_out.values()), "against the oracle", max(dev_or.values()))
        worst, worst_out, worst_oracle = max(worst, max(dev.values())), max(worst_out, max(dev_out.values())), max(worst_oracle, max(dev_or.values()))
    print("tiles against the undivided handle: bergs", worst, "outputs", worst_out, "bound", BOUND, "; against the undivided oracle", worst_oracle)
    assert worst <= BOUND and worst_out <= BOUND, (worst, worst_out)
    assert worst_oracle <= 1e-9, worst_oracle


def test_two_by_two_tiles_without_the_update_are_wrong():
    """the control: the halo update skipped, the velocities differ from the undivided handle's by more than 1e-6 of the largest
    (measured: 0.17 of it after one step, 1.4 after forty)"""
    res, copies, moved = _two_by_two(False, False, (1, 40))
    dev = {step: HB.compare(res[step][1], res[step][0]) for step in (1, 40)}
    print("tiles without halo bergs:", {s: d["uvel"] for s, d in dev.items()})
    assert copies == 0 and dev[1]["uvel"] > 1e-6 and dev[40]["uvel"] > 1e-6, dev


# ---- two ranks on one GPU ----
def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from icebergs_amd.decomposed import HipTile, TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    whole, b = HB.population()
    p = HB.params(False)
    nj = HB.NJ * HB.NTY                          # 2 x 1: each rank holds a column of the box
    ib = _icebergs(HB.tile_grid(rank, 0, whole, nj=nj), p, 400)
    ib.upload_bergs(HB.trim(HB.split_bergs(b, rank, 0, 400, nj=nj)))
    tile = HipTile(ib)
    ex = TileExchange(world, 1, dist)
    for _ in range(HB.NSTEPS):
        ex.step_interactive(tile)
    assert ib.halo_berg_count() == 0
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), sent=ex.sent, received=ex.received, **_live(ib.download_bergs()))
    ib.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_step_interactive_on_one_gpu(tmp_path):
    """TileExchange.step_interactive with HIP handles, both ranks on GPU 0 and gloo for the messages (2 x 1): the bergs after 40
    steps against the undivided oracle within the 1e-9 this project uses for HIP against the oracle (measured: 3.7e-12, in axn)"""
    world = 2
    port = 31700 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert sum(int(q["sent"]) for q in parts) == sum(int(q["received"]) for q in parts) > 1000
    got = HB.join([{k: q[k] for k in HB.FIELDS + ("id",)} for q in parts])
    dev = HB.compare(got, HB.whole_oracle(False)[0][HB.NSTEPS])
    print("two HIP ranks against the undivided oracle:", max(dev.values()), {k: v for k, v in dev.items() if v > 1e-13})
    assert max(dev.values()) <= 1e-9, dev
