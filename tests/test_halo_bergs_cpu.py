"""Halo bergs of a decomposed run without a GPU (update_halo_icebergs FW:1800-2131): the numpy restatement of the strip
selection, oracle tiles with halo rows against the undivided oracle for both searches (d_cpu), the control without halo rows,
and TileExchange.update_halo_bergs / step_interactive over a one-rank fake `dist` and over gloo ranks of oracle tiles."""
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

from icebergs_amd import synthetic as S   # noqa: E402
import halo_bergs as HB                   # noqa: E402

# The bound on the oracle's own tiles-versus-whole deviation (any field of an owned berg, relative to the field's maximum): the
# 1e-12 this project allows between tiles and whole (tests/test_migration.py, tests/test_halo_planes_cpu.py).  It is set from that
# rule, not from the run: here the tiles' arrays are slices of the whole grid's and the force sums run in the same order, and
# what is measured is 0 -- every field to the bit (D_CPU below).
BOUND_CPU = 1e-12
# What test_oracle_tiles_with_halo_rows_match_the_undivided_oracle measures, d_cpu (the larger of the two searches, steps 1, 20
# and 40).  tests/test_halo_bergs_gpu.py takes its bound from it: 4 x max(D_CPU, 1e-12).
D_CPU = 0.0


def test_numpy_strip_selection():
    """7 x 5 cells, halo 4: the strips of FW:1896, 1911, 1981, 1995 cell by cell, the asymmetry (w - 1 columns go east and north,
    w go west and south), the corner columns of axis 1, dead rows left out"""
    nic, njc = 7, 5
    ii, jj = np.meshgrid(np.arange(1 - HB.H, nic + HB.H + 1), np.arange(1 - HB.H, njc + HB.H + 1))
    ine, jne = ii.reshape(-1).astype(np.int32), jj.reshape(-1).astype(np.int32)
    alive = np.ones(len(ine), dtype=np.int32)
    dead = (ine == 5) & (jne == 3)
    alive[dead] = 0
    for w in (2, 3, 4):
        hi, lo = HB.np_halo_select(ine, jne, alive, 0, w, nic, njc)
        assert set(ine[hi]) == set(range(nic - w + 2, nic + 1)) and set(ine[lo]) == set(range(1, w + 1))
        assert set(jne[hi]) == set(jne[lo]) == set(range(1, njc + 1))
        assert len(hi) == (w - 1) * njc - (1 if w == 4 else 0) and len(lo) == w * njc and not dead[hi].any()
        hi, lo = HB.np_halo_select(ine, jne, alive, 1, w, nic, njc)
        assert set(jne[hi]) == set(range(njc - w + 2, njc + 1)) and set(jne[lo]) == set(range(1, w + 1))
        assert set(ine[hi]) == set(ine[lo]) == set(range(1 - HB.H, nic + HB.H + 1))          # the halo columns too: two hops for a diagonal neighbour
        assert len(lo) == w * (nic + 2 * HB.H) - (1 if w >= 3 else 0)
    hi, lo = HB.np_halo_select(ine, jne, alive, 1, 4, nic, njc)
    assert len(np.intersect1d(hi, lo)) > 0                                                    # njc = 5, w = 4: rows 3 and 4 go both ways


def _tiles(contact, with_halo_bergs, cap=400):
    whole, b = HB.population()
    p = HB.params(contact)
    return {(tx, ty): HB.OracleTile(HB.tile_grid(tx, ty, whole), p, HB.split_bergs(b, tx, ty, cap), with_halo_bergs)
            for tx in range(HB.NTX) for ty in range(HB.NTY)}


def _swap(tiles, pack):
    """one exchange with the ranks in one process: east/west, then north/south; returns the records moved"""
    empty = np.empty((0, 34))
    moved = 0
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
        out = {}
        for (tx, ty), t in tiles.items():
            sides = ((tx + dx, ty + dy) in tiles, (tx - dx, ty - dy) in tiles)
            out[(tx, ty)] = pack(t, axis, sides)
        for (tx, ty), t in tiles.items():
            lo, hi = (tx - dx, ty - dy), (tx + dx, ty + dy)
            from_lo, from_hi = out[lo][0] if lo in out else empty, out[hi][1] if hi in out else empty
            moved += len(from_lo) + len(from_hi)
            t.unpack_pair(from_lo, from_hi)
    return moved


def _run_tiles(contact, with_halo_bergs, check_at):
    """TileExchange.step_interactive for the four oracle tiles in one process (no planes: the bergs are what is compared)"""
    tiles = _tiles(contact, with_halo_bergs)
    snaps, migrated, copies = {}, 0, 0
    for step in range(1, max(check_at) + 1):
        for t in tiles.values():
            t.zero_accumulators()
        copies += _swap(tiles, lambda t, axis, sides: t.pack_halo_bergs_pair(axis, 0, sides))
        for t in tiles.values():
            if contact:
                t.set_conglom_ids()
            t.evolve()
        migrated += _swap(tiles, lambda t, axis, sides: t.pack_pair(axis))
        for t in tiles.values():
            t.thermodynamics()
        if step in check_at:
            snaps[step] = HB.join([t.live() for t in tiles.values()])
    return snaps, migrated, copies


def test_the_population_exercises_the_edges():
    """the conditions on the undivided oracle run alone: contacts across tile edges (ordered pairs, summed over the steps),
    diagonal ones, migrations, nobody leaves the box"""
    for contact in (False, True):
        snaps, outs, stats = HB.whole_oracle(contact)
        print("undivided oracle, contact search" if contact else "undivided oracle, 3 x 3 search", stats)
        assert stats["pairs"] >= 50 and stats["diag"] >= 5 and stats["migrations"] >= 20 and stats["left"] == 0, stats
        assert sorted(snaps) == list(HB.CHECK_AT)


@pytest.mark.parametrize("contact", [False, True])
def test_oracle_tiles_with_halo_rows_match_the_undivided_oracle(contact):
    """2 x 2 oracle tiles, halo rows appended from the neighbours before each evolve (width 4, two hops for the diagonal),
    migration after it: the same survivors, no id owned twice, every field of the owned bergs.  Measured d_cpu: 0.0 with
    both searches at all three steps -- every field of every owned berg to the bit."""
    want = HB.whole_oracle(contact)[0]
    got, migrated, copies = _run_tiles(contact, True, HB.CHECK_AT)
    assert migrated >= 20 and copies > 1000, (migrated, copies)
    d_cpu = 0.0
    for step in HB.CHECK_AT:
        dev = HB.compare(got[step], want[step])
        print("step", step, "contact", contact, "largest deviation", max(dev.values()), {k: v for k, v in dev.items() if v > 0.0})
        d_cpu = max(d_cpu, max(dev.values()))
    print("d_cpu =", d_cpu)
    assert d_cpu <= BOUND_CPU, d_cpu


@pytest.mark.parametrize("contact", [False, True])
def test_oracle_tiles_without_halo_rows_differ(contact):
    """the control: the same run with no halo rows differs from the undivided run by more than 1e-6 of the largest speed"""
    want = HB.whole_oracle(contact)[0]
    got, migrated, copies = _run_tiles(contact, False, (1, 40))
    assert copies == 0
    dev = {step: HB.compare(got[step], want[step]) for step in (1, 40)}
    print("no halo rows, contact", contact, {s: (d["uvel"], d["vvel"]) for s, d in dev.items()})
    assert dev[1]["uvel"] > 1e-6 and dev[40]["uvel"] > 1e-6, dev


# ---- TileExchange ----
class _OneRank:
    def get_rank(self): return 0
    def get_world_size(self): return 1


def test_update_halo_bergs_on_one_rank_and_the_refusals():
    from icebergs_amd.decomposed import TileExchange
    whole, b = HB.population()
    p = HB.params(False)
    n = len(b["lon"])
    b["_n"] = n
    t = HB.OracleTile(whole, p, b)
    ex = TileExchange(1, 1, _OneRank())
    ex.update_halo_bergs(t)                    # no neighbour anywhere: nothing is packed, nothing arrives
    assert t.b["_n"] == n and ex.sent == ex.received == 0 and not t.halo_ids
    ex.step_interactive(t)                     # and the step is the undivided oracle's
    want = HB.whole_oracle(False)[0][1]
    assert max(HB.compare(t.live(), want).values()) == 0.0
    with pytest.raises(ValueError, match="cyclic_x"):
        TileExchange(1, 1, _OneRank(), cyclic_x=True).update_halo_bergs(t)
    for switch in ("mts", "iceberg_bonds_on", "footloose", "find_melt_using_spread_mass", "Runge_not_Verlet"):
        q = HB.params(False)
        setattr(q, switch, 1)
        t.params = q
        with pytest.raises(ValueError, match=switch):
            ex.step_interactive(t)
    t.params = S.default_params()
    with pytest.raises(ValueError, match="interactive_icebergs_on"):
        ex.step_interactive(t)
    t.params = p
    with pytest.raises(ValueError, match="interactive_icebergs_on"):
        ex.step(t)                             # the plain tile step still refuses interacting bergs


def _worker(rank, world, port, out_dir, contact):
    from icebergs_amd.decomposed import TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    whole, b = HB.population()
    p = HB.params(contact)
    ex = TileExchange(HB.NTX, HB.NTY, dist)
    tile = HB.OracleTile(HB.tile_grid(ex.tx, ex.ty, whole), p, HB.split_bergs(b, ex.tx, ex.ty, 400))
    # one update on its own: what arrives is what the numpy selection picks on the neighbours, two hops for the diagonal one
    own = tile.live()
    ex.update_halo_bergs(tile)
    arrived = np.concatenate(tile.halo_ids) if tile.halo_ids else np.empty(0, dtype=np.int64)
    sent1, received1 = ex.sent, ex.received
    tile.b["_n"] = len(own["id"])              # drop them again: the run below starts from the population
    tile.halo_ids = []
    for _ in range(HB.NSTEPS):
        ex.step_interactive(tile)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), arrived=arrived, sent1=sent1, received1=received1, sent=ex.sent, received=ex.received,
             **tile.live())
    dist.barrier()
    dist.destroy_process_group()


def _expected_arrivals(tx, ty):
    """the ids the numpy selection sends to tile (tx, ty): axis 0 from the east / west neighbour's own bergs, axis 1 from the
    north / south neighbour's own bergs and the halo rows its axis 0 brought"""
    whole, b = HB.population()
    w = HB.H
    held = {}
    for key in ((x, y) for x in range(HB.NTX) for y in range(HB.NTY)):
        t = HB.split_bergs(b, key[0], key[1], 400)
        m = t["_n"]
        held[key] = {k: t[k][:m].copy() for k in ("id", "ine", "jne", "alive")}
    got = {key: [] for key in held}
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
        sel = {key: HB.np_halo_select(h["ine"], h["jne"], h["alive"], axis, w, HB.NI, HB.NJ) for key, h in held.items()}
        new = {key: [] for key in held}
        for (x, y), h in held.items():
            for src, which, shift in (((x - dx, y - dy), 0, +1), ((x + dx, y + dy), 1, -1)):    # what the lo neighbour sent hi, and the other way round
                if src not in held:
                    continue
                rows = sel[src][which]
                s = held[src]
                new[(x, y)].append({"id": s["id"][rows], "ine": s["ine"][rows] - shift * dx * HB.NI, "jne": s["jne"][rows] - shift * dy * HB.NJ,
                                    "alive": s["alive"][rows]})
        for key, parts in new.items():
            for part in parts:
                got[key].append(part["id"])
                held[key] = {k: np.concatenate([held[key][k], part[k]]) for k in held[key]}
    return np.concatenate(got[(tx, ty)]) if got[(tx, ty)] else np.empty(0, dtype=np.int64)


@pytest.mark.parametrize("contact", [False])
def test_gloo_ranks_of_oracle_tiles_update_halo_bergs_and_step(tmp_path, contact):
    """four gloo ranks (2 x 2) of oracle tiles: after one update_halo_bergs the records sent equal the records received and the ids
    that arrived on each rank are the numpy selection's, in order; forty step_interactive then give the undivided oracle's bergs"""
    import oracle_lib
    oracle_lib.build()
    world = HB.NTX * HB.NTY
    port = 31300 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path), contact), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert sum(int(q["sent1"]) for q in parts) == sum(int(q["received1"]) for q in parts) > 100
    assert sum(int(q["sent"]) for q in parts) == sum(int(q["received"]) for q in parts)
    for r, q in enumerate(parts):
        want = _expected_arrivals(r % HB.NTX, r // HB.NTX)
        assert len(want) > 20 and np.array_equal(q["arrived"], want), r
    far = HB.split_bergs(HB.population()[1], 1, 1, 400)
    assert set(parts[0]["arrived"]) & set(far["id"][:far["_n"]])          # bergs of the diagonal tile did arrive, in two hops
    got = HB.join([{k: q[k] for k in HB.FIELDS + ("id",)} for q in parts])
    dev = HB.compare(got, HB.whole_oracle(contact)[0][HB.NSTEPS])
    print("gloo ranks against the undivided oracle:", max(dev.values()))
    assert max(dev.values()) <= BOUND_CPU, dev
