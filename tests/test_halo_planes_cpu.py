"""Halo update of the on-ocean planes of a decomposed run (mpp_update_domains(var_on_ocean) in sum_up_spread_fields,
IB:6106-6107, before the 9-point sum IB:6126-6131), without a GPU: the oracle steps the tiles, a numpy restatement of the update
sits behind the tile interface of icebergs_amd.decomposed, and what is under test is the buffer layout and the message code
of TileExchange.update_halos / TileExchange.step.  The five gathered outputs of the tiles, assembled, against the oracle on
the undivided grid."""
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

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import test_decomposed as D               # noqa: E402  (its grids, populations and OracleTile)
import test_migration as M                # noqa: E402  (the 2 x 2 lat-lon box)

H = S.HALO
A0 = T.ENUMS["KID_A_MASS_ON_OCEAN"]
OUT_NAMES = ("spread_mass", "spread_area", "spread_uvel", "spread_vvel", "ustar_iceberg")
OUT_ROWS = [T.ENUMS["KID_O_" + n.upper()] for n in OUT_NAMES]

# What the second test measures for the oracle's own tiles-versus-whole deviation of the five outputs (the largest of its
# four cases, relative to each plane's maximum): the corner coordinates of a tile are rounded differently from the whole
# grid's.  tests/test_halo_planes_gpu.py takes its bound from it: 4 x max(D_CPU_RUN, 1e-12).
D_CPU_RUN = 8.9e-13     # open box: 7.7e-14 with two tiles, 8.8e-13 with three; the Cartesian channel: 0 with two and with three


# ---- the halo update restated with numpy slices (the layout of include/kid.h) ----
def np_pack_halo_pair(acc, axis, w, npl, nic, njc):
    """(hi, lo): the strips for the east / north and the west / south neighbour; element order plane, j, i"""
    v = acc[A0:A0 + npl]
    if axis == 0:
        hi, lo = v[:, H:H + njc, H + nic - w:H + nic], v[:, H:H + njc, H:H + w]
    else:
        hi, lo = v[:, H + njc - w:H + njc, H - w:H + nic + w], v[:, H:H + w, H - w:H + nic + w]
    return hi.reshape(-1).copy(), lo.reshape(-1).copy()


def np_unpack_halo_pair(acc, axis, w, npl, nic, njc, from_lo, from_hi):
    """the neighbours' strips into the halo; None: no neighbour, that halo keeps what it holds"""
    v = acc[A0:A0 + npl]
    if axis == 0:
        if from_lo is not None:
            v[:, H:H + njc, H - w:H] = from_lo.reshape(npl, njc, w)
        if from_hi is not None:
            v[:, H:H + njc, H + nic:H + nic + w] = from_hi.reshape(npl, njc, w)
    else:
        if from_lo is not None:
            v[:, H - w:H, H - w:H + nic + w] = from_lo.reshape(npl, w, nic + 2 * w)
        if from_hi is not None:
            v[:, H + njc:H + njc + w, H - w:H + nic + w] = from_hi.reshape(npl, w, nic + 2 * w)


def np_halo_count(axis, w, npl, nic, njc):
    return npl * njc * w if axis == 0 else npl * w * (nic + 2 * w)


class OracleTile(D.OracleTile):
    """the oracle behind the whole tile interface of icebergs_amd.decomposed: the phases of a step, the berg migration of
    tests/test_decomposed.py and the numpy halo update above (test infrastructure)"""
    NPL = 36          # the oracle fills all four groups of nine, as the reference does

    def __init__(self, grid, p, bergs):
        super().__init__(grid, p, bergs)
        self.params = p
        d = grid["desc"]
        self.nic, self.njc = d.iec - d.isc + 1, d.jec - d.jsc + 1

    def _args(self):
        return C.byref(self.o.kg), C.byref(self.o.params), C.byref(self.o.soa(self.b))

    def zero_accumulators(self):
        self.o.acc[:] = 0.0

    def interp(self):
        self.o.lib.ko_interp_gridded_fields_to_bergs(*self._args())

    def thermodynamics(self):
        from oracle_lib import _dp
        self.o.lib.ko_thermodynamics(*self._args(), _dp(self.o.acc), _dp(self.o.scalars))

    def calculate_mass_on_ocean(self):
        from oracle_lib import _dp
        self.o.lib.ko_calculate_mass_on_ocean(*self._args(), _dp(self.o.acc))

    def gather(self):
        self.o.step_gather()

    def halo_buffer_count(self, axis, width=1):
        return np_halo_count(axis, width, self.NPL, self.nic, self.njc)

    def pack_halo_pair(self, axis, width=1, sides=(True, True)):
        hi, lo = np_pack_halo_pair(self.o.acc, axis, width, self.NPL, self.nic, self.njc)
        return (hi if sides[0] else None), (lo if sides[1] else None)

    def unpack_halo_pair(self, axis, from_lo, from_hi, width=1):
        np_unpack_halo_pair(self.o.acc, axis, width, self.NPL, self.nic, self.njc, from_lo, from_hi)

    def out_comp(self):
        return self.o.out[:, H:H + self.njc, H:H + self.nic].copy()


def split_bergs(b, tx, ty, ni, nj, cap=None):
    """the live bergs of `b` (whole-grid cell indices) that sit on tile (tx, ty), with the tile's own indices"""
    sel = (b["alive"] != 0) & ((b["ine"] - 1) // ni == tx) & ((b["jne"] - 1) // nj == ty)
    m = int(sel.sum())
    big = S.empty_bergs(m if cap is None else cap)
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            big[k][:m] = v[sel]
    big["ine"][:m] -= tx * ni
    big["jne"][:m] -= ty * nj
    big["_n"] = m
    return big


def assemble(parts, ntx, nty):
    """{(tx, ty): (5, njc, nic)} -> (5, nty * njc, ntx * nic)"""
    return np.concatenate([np.concatenate([parts[(tx, ty)] for tx in range(ntx)], axis=2) for ty in range(nty)], axis=1)


def deviations(got, want):
    """per output, the largest deviation as a fraction of the plane's maximum, and the cells off by more than 1e-3 of it"""
    dev, cells = {}, {}
    for name, k in zip(OUT_NAMES, OUT_ROWS):
        scale = float(np.max(np.abs(want[k])))
        assert scale > 0.0, name + ": the undivided plane is empty, the comparison would see nothing"
        e = np.abs(got[k] - want[k]) / scale
        dev[name], cells[name] = float(e.max()), int((e > 1e-3).sum())
    return dev, cells


def test_numpy_halo_update_closes_the_gap_between_oracle_tiles_and_the_undivided_oracle():
    """The 2 x 2 box of tests/test_migration.py, 6 000 bergs (two oracle steps on the undivided grid give them velocities),
    set_diag_all, default namelist: calculate_mass_on_ocean per tile, the halo update, the gather, against the same on the
    undivided grid.  The bound with the update is the 1e-12 this project allows between tiles and whole
    (tests/test_migration.py): only the rounding of the tiles' corner coordinates separates them.  Measured d_cpu: 6.4e-13
    (ustar_iceberg; spread_mass 5.0e-13); without the update 161 cells of spread_mass are off by more than 1e-3 of its maximum,
    the largest by 0.24 of it."""
    import oracle_lib
    oracle_lib.build()
    from oracle_lib import Oracle, _dp
    ntx = nty = 2
    NI, NJ = M.NI, M.NJ
    whole = M._grid(None, None, ntx, nty)
    p = S.set_diag_all(S.default_params())
    p.dt = 1800.0
    b = S.place_bergs(whole, 6000, 11, (2, NI * ntx - 1), (2, NJ * nty - 1))
    ref = Oracle(whole, p)
    ref.run_step(b, 2)
    ref.acc[:] = 0.0
    ref.lib.ko_calculate_mass_on_ocean(C.byref(ref.kg), C.byref(ref.params), C.byref(ref.soa(b)), _dp(ref.acc))
    ref.step_gather()
    want = ref.out[:, H:H + NJ * nty, H:H + NI * ntx]
    tiles = {}
    for tx in range(ntx):
        for ty in range(nty):
            t = OracleTile(M._grid(tx, ty, ntx, nty), p, split_bergs(b, tx, ty, NI, NJ))
            t.zero_accumulators()
            t.calculate_mass_on_ocean()
            tiles[(tx, ty)] = t
    for t in tiles.values():                                       # the control: what a decomposed run returned without the update
        t.gather()
    dev0, cells0 = deviations(assemble({k: t.out_comp() for k, t in tiles.items()}, ntx, nty), want)
    print("no halo update: deviation", dev0, "cells off by > 1e-3 of the maximum", cells0)
    assert cells0["spread_mass"] > 100 and dev0["spread_mass"] > 1e-3, (cells0, dev0)
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):             # the update, in process
        packed = {k: t.pack_halo_pair(axis) for k, t in tiles.items()}
        for (tx, ty), t in tiles.items():
            lo, hi = (tx - dx, ty - dy), (tx + dx, ty + dy)
            t.unpack_halo_pair(axis, packed[lo][0] if lo in packed else None, packed[hi][1] if hi in packed else None)
    for t in tiles.values():
        t.gather()
    dev, cells = deviations(assemble({k: t.out_comp() for k, t in tiles.items()}, ntx, nty), want)
    print("with the halo update: d_cpu =", max(dev.values()), dev)
    assert max(dev.values()) <= 1e-12, dev


def _worker(rank, world, port, nbergs, nsteps, out_dir, cyclic):
    from icebergs_amd.decomposed import TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    whole, p, b = D._population(world, nbergs, cyclic)
    S.set_diag_all(p)
    if cyclic:
        p.periodic_reentry = 0            # on a tile the seam is a real boundary between ranks
    g = D._channel(rank, world) if cyclic else D._grid(rank, world)
    tile = OracleTile(g, p, split_bergs(b, rank, 0, D.NI, D.NJ, cap=nbergs))
    ex = TileExchange(world, 1, dist, cyclic_x=cyclic)
    for _ in range(nsteps):
        ex.step(tile)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), out=tile.out_comp(), sent=ex.sent, received=ex.received)
    dist.barrier()
    dist.destroy_process_group()


def whole_oracle_out(world, nbergs, nsteps, cyclic):
    """the five outputs of the undivided oracle run (ko_run_step; periodic_reentry = 1 on the channel) after the last step"""
    import oracle_lib
    whole, p, b = D._population(world, nbergs, cyclic)
    S.set_diag_all(p)
    ref = oracle_lib.Oracle(whole, p)
    ref.run_step(b, nsteps)
    return ref.out[:, H:H + D.NJ, H:H + D.NI * world].copy()


@pytest.mark.parametrize("cyclic,world", [(False, 2), (False, 3), (True, 2), (True, 3)])
def test_gloo_ranks_of_oracle_tiles_step_and_update_halos(tmp_path, cyclic, world):
    """TileExchange.step over gloo ranks: 30 steps on the open box, 60 on the cyclic channel of tests/test_decomposed.py (with
    two tiles east and west are the same rank).  The bound is that file's for the bergs of the same runs (1e-12 on the box,
    1e-11 on the channel, whose coordinates are metres up to 1e5): the outputs are sums of smooth functions of the berg state
    over a cell's bergs, relative to the plane's maximum.  Measured d_cpu_run: D_CPU_RUN above."""
    import oracle_lib
    oracle_lib.build()
    nbergs, nsteps = (300, 60) if cyclic else (400, 30)
    port = 30500 + (os.getpid() % 2000) + 10 * int(cyclic) + world
    mp.spawn(_worker, args=(world, port, nbergs, nsteps, str(tmp_path), cyclic), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert sum(int(q["sent"]) for q in parts) == sum(int(q["received"]) for q in parts) > 20
    got = assemble({(r, 0): parts[r]["out"] for r in range(world)}, world, 1)
    dev, _ = deviations(got, whole_oracle_out(world, nbergs, nsteps, cyclic))
    print("cyclic" if cyclic else "open", "world", world, ": d_cpu_run =", max(dev.values()), dev)
    assert max(dev.values()) <= (1e-11 if cyclic else 1e-12), dev


def test_step_refuses_what_the_tile_step_does_not_cover():
    from icebergs_amd.decomposed import TileExchange

    class FakeDist:
        def get_rank(self): return 0
        def get_world_size(self): return 1

    class Tile:
        pass
    ex = TileExchange(1, 1, FakeDist())
    for switch in ("find_melt_using_spread_mass", "mts", "interactive_icebergs_on"):
        t = Tile()
        t.params = S.default_params()
        setattr(t.params, switch, 1)
        with pytest.raises(ValueError, match=switch):
            ex.step(t)
