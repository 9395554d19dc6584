"""Halo update of the on-ocean planes of a decomposed run on the device (csrc/kid_halo.inc): kid_pack_halo_pair /
kid_unpack_halo_pair against the numpy slicing of tests/test_halo_planes_cpu.py, kid_calculate_mass_on_ocean + kid_step_gather
against kid_create_gridded_icebergs_fields, and the five gathered outputs of tiles (2 x 2 in one process, two gloo ranks on one
GPU) against the undivided grid."""
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
import parity as P                        # noqa: E402
import test_decomposed as D               # noqa: E402
import test_halo_planes_cpu as HC         # noqa: E402  (the numpy restatement, the oracle tile, the assembly helpers)
import test_migration as M                # noqa: E402

pytestmark = pytest.mark.gpu

H = S.HALO
# tiles against the undivided handle: 4 x max(d_cpu_run, 1e-12).  d_cpu_run is the oracle's own tiles-versus-whole deviation
# (HC.D_CPU_RUN, measured by tests/test_halo_planes_cpu.py); 1e-12 is the level this project allows between two summation orders
# (test_same_per_berg_arithmetic) and between tiles and whole (tests/test_migration.py); the factor 4 is for the tiles and the
# whole handle adding a cell's bergs in different orders on top of the corner-coordinate rounding.
BOUND = 4.0 * max(HC.D_CPU_RUN, 1e-12)


def _small_tile(nic, njc, diag_all):
    from icebergs_amd.framework import Icebergs
    g = S.c2_forcing(S.latlon_grid(ni=nic, nj=njc, lon0=10.0, dlon=0.02, lat0=-60.0, dlat=0.02))
    p = S.default_params()
    if diag_all:
        S.set_diag_all(p)
    return Icebergs(g, p, capacity=8)


def _coded_block(ib):
    """a device tensor bound as the accumulator block, every double of it encoding (plane, j, i)"""
    import torch
    count = T.NSCALAR + T.NACC * ib.ncell
    pl, j, i = np.meshgrid(np.arange(T.NACC), np.arange(ib.nj), np.arange(ib.ni), indexing="ij")
    host = np.concatenate([-(np.arange(T.NSCALAR) + 1.0), (pl * 10000.0 + j * 100.0 + i + 0.5).reshape(-1)])
    block = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    ib.bind_accum_buffer(block.data_ptr(), count)
    return block, host


def _planes(host, ib):
    return host[T.NSCALAR:].reshape(T.NACC, ib.nj, ib.ni)


@pytest.mark.parametrize("diag_all,on_device", [(False, False), (False, True), (True, False), (True, True)])
def test_pack_and_unpack_against_slicing(diag_all, on_device):
    """one handle on a 7 x 5 tile (halo 4: the smallest on which a width-4 strip, the corner columns and both axes are all
    distinct): the packed buffers are the numpy slices element for element, unpack changes exactly the addressed halo cells"""
    import torch
    nic, njc = 7, 5
    npl = 36 if diag_all else 9
    ib = _small_tile(nic, njc, diag_all)
    try:
        assert ib.halo_plane_count() == npl
        block, host = _coded_block(ib)

        def buf(n, fill):
            a = fill + np.zeros(n)
            return torch.from_numpy(a).cuda() if on_device else a

        def to_np(b):
            return b.cpu().numpy() if on_device else b
        for axis in (0, 1):
            for w in (1, 4):
                count = ib.halo_buffer_count(axis, w)
                assert count == HC.np_halo_count(axis, w, npl, nic, njc)
                want_hi, want_lo = HC.np_pack_halo_pair(_planes(host, ib), axis, w, npl, nic, njc)
                assert len(want_hi) == len(want_lo) == count
                hi, lo = ib.pack_halo_pair(axis, w, out=(buf(count, -7.0), buf(count, -7.0)))
                assert np.array_equal(to_np(hi), want_hi) and np.array_equal(to_np(lo), want_lo), (axis, w)
                if not on_device:                                              # the default: two new numpy arrays
                    hi, lo = ib.pack_halo_pair(axis, w)
                    assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo), (axis, w)
                none, lo = ib.pack_halo_pair(axis, w, out=(None, buf(count, -7.0)))   # no neighbour on the high side
                assert none is None and np.array_equal(to_np(lo), want_lo)
                hi, none = ib.pack_halo_pair(axis, w, out=(buf(count, -7.0), None))
                assert none is None and np.array_equal(to_np(hi), want_hi)
                assert np.array_equal(block.cpu().numpy().view(np.int64), host.view(np.int64))   # packing writes nothing into the block
                # a second coded pattern comes back: exactly the addressed halo cells change
                in_lo, in_hi = -1.0e6 - np.arange(count) - 0.25, -2.0e6 - np.arange(count) - 0.75
                for from_lo, from_hi in ((in_lo, in_hi), (None, in_hi), (in_lo, None), (None, None)):
                    want = host.copy()
                    HC.np_unpack_halo_pair(_planes(want, ib), axis, w, npl, nic, njc, from_lo, from_hi)
                    changed = int((want != host).sum())
                    assert changed == count * ((from_lo is not None) + (from_hi is not None))
                    ib.unpack_halo_pair(axis, None if from_lo is None else buf(count, from_lo), None if from_hi is None else buf(count, from_hi), w)
                    ib.sync()
                    got = block.cpu().numpy()
                    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (axis, w, from_lo is None, from_hi is None)
                    block.copy_(torch.from_numpy(host))
                    torch.cuda.synchronize()
    finally:
        ib.close()


def test_widths_outside_the_halo_or_the_tile_are_refused():
    """width 0, width 5 (> halo 4) and a width larger than njc: KID_EINVAL from all three calls, nothing written"""
    n = C.c_int64(-1)
    for nic, njc, bad, good in ((7, 5, (0, 5, -1), 4), (7, 3, (4,), 3)):
        ib = _small_tile(nic, njc, True)
        try:
            block, host = _coded_block(ib)
            a, b = np.full(4096, -7.0), np.full(4096, -7.0)
            for axis in (0, 1):
                for w in bad:
                    assert ib.lib.kid_halo_buffer_count(ib.h, axis, w, C.byref(n)) == -1 and n.value == -1, (axis, w)
                    assert ib.lib.kid_pack_halo_pair(ib.h, axis, w, a.ctypes.data, b.ctypes.data, 0) == -1, (axis, w)
                    assert ib.lib.kid_unpack_halo_pair(ib.h, axis, w, a.ctypes.data, b.ctypes.data, 0) == -1, (axis, w)
                assert ib.halo_buffer_count(axis, good) == HC.np_halo_count(axis, good, 36, nic, njc)
            for axis in (2, -1):
                assert ib.lib.kid_halo_buffer_count(ib.h, axis, 1, C.byref(n)) == -1
            ib.sync()
            assert np.all(a == -7.0) and np.all(b == -7.0)
            assert np.array_equal(block.cpu().numpy().view(np.int64), host.view(np.int64))
        finally:
            ib.close()


def test_calculate_mass_on_ocean_and_gather_equal_create_gridded_icebergs_fields():
    """an undivided handle with reproducible sums, three phase-by-phase steps: the two halves give the bits of the whole"""
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=20000, seed=7)
    S.set_diag_all(p)
    res = []
    for split in (False, True):
        ib = Icebergs(grid, p, capacity=len(b["lon"]))
        try:
            ib.set_reproducible_sums(True)
            ib.upload_bergs(b)
            for _ in range(3):
                if not split:
                    ib.run_phases(1)
                    continue
                for name in ("kid_zero_accumulators", "kid_evolve_icebergs", "kid_thermodynamics", "kid_calculate_mass_on_ocean", "kid_step_gather"):
                    ib._check(getattr(ib.lib, name)(ib.h), name)
            res.append([x.copy() for x in ib.fetch()])
        finally:
            ib.close()
    assert p.old_interp_flds_order == 1
    for x, y, name in zip(res[0], res[1], ("acc", "out", "scalars")):
        assert np.abs(x).max() > 0.0, name
        assert np.array_equal(x, y), name


# ---- 2 x 2 tiles against the undivided grid, one process ----
def _halo_swap(tiles, on_device):
    """TileExchange.update_halos with the ranks in one process"""
    import torch
    for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
        packed = {}
        for (tx, ty), ib in tiles.items():
            n = ib.halo_buffer_count(axis)
            sides = ((tx + dx, ty + dy) in tiles, (tx - dx, ty - dy) in tiles)
            new = (lambda: torch.empty(n, dtype=torch.float64, device="cuda")) if on_device else (lambda: np.empty(n))
            packed[(tx, ty)] = ib.pack_halo_pair(axis, out=tuple(new() if s else None for s in sides))
        for (tx, ty), ib in tiles.items():
            lo, hi = (tx - dx, ty - dy), (tx + dx, ty + dy)
            ib.unpack_halo_pair(axis, packed[lo][0] if lo in packed else None, packed[hi][1] if hi in packed else None)


def _tiles_step(tiles, exchange, update, on_device=False):
    """TileExchange.step for every tile, the two exchanges swapped in process"""
    def call(ib, name):
        ib._check(getattr(ib.lib, name)(ib.h), name)
    p = next(iter(tiles.values())).params
    for ib in tiles.values():
        call(ib, "kid_zero_accumulators")
        if not p.old_interp_flds_order:
            call(ib, "kid_interp_gridded_fields_to_bergs")
        call(ib, "kid_evolve_icebergs")
    moved = exchange(tiles)
    for ib in tiles.values():
        if not p.old_interp_flds_order:
            call(ib, "kid_interp_gridded_fields_to_bergs")
        call(ib, "kid_thermodynamics")
        call(ib, "kid_calculate_mass_on_ocean")
    if update:
        _halo_swap(tiles, on_device)
    for ib in tiles.values():
        call(ib, "kid_step_gather")
    return moved


def _two_by_two(old_order, update, on_device, check_at):
    """the run of test_two_by_two_tiles_match_the_undivided_grid with the halo update before the gather; returns the deviations
    {step: {plane: rel_err}} of the assembled tiles' outputs from the undivided handle's"""
    from icebergs_amd.framework import Icebergs
    ntx = nty = 2
    NI, NJ = M.NI, M.NJ
    whole = M._grid(None, None, ntx, nty)
    p = S.set_diag_all(S.default_params())
    p.dt, p.old_interp_flds_order = 1800.0, old_order
    n = 6000
    b = S.place_bergs(whole, n, 11, (2, NI * ntx - 1), (2, NJ * nty - 1))
    ref = Icebergs(whole, p, capacity=n)
    tiles = {}
    try:
        ref.upload_bergs(b)
        for tx in range(ntx):
            for ty in range(nty):
                bt = HC.split_bergs(b, tx, ty, NI, NJ)
                ib = Icebergs(M._grid(tx, ty, ntx, nty), p, capacity=n)
                assert ib.buffer_width() == 34
                ib.upload_bergs(bt)
                tiles[(tx, ty)] = ib
        assert ref.buffer_width() == 34
        exchange = M._exchange(ntx, nty, pair=True)
        moved, dev = 0, {}
        for step in range(1, max(check_at) + 1):
            ref.run_phases(1)
            moved += _tiles_step(tiles, exchange, update, on_device)
            if step in check_at:
                want = ref.fetch()[1][:, H:H + NJ * nty, H:H + NI * ntx]
                got = HC.assemble({k: ib.fetch()[1][:, H:H + NJ, H:H + NI].copy() for k, ib in tiles.items()}, ntx, nty)
                dev[step] = {}
                for name, k in zip(HC.OUT_NAMES, HC.OUT_ROWS):
                    assert np.abs(want[k]).max() > 0.0, name
                    dev[step][name] = P.rel_err(got[k], want[k])
        rb = ref.download_bergs()
        ids = np.concatenate([q["id"][q["alive"] != 0] for q in (ib.download_bergs() for ib in tiles.values())])
        # the old checks: the same survivors, bergs did cross tile boundaries
        assert len(np.unique(ids)) == len(ids) and np.array_equal(np.sort(ids), np.sort(rb["id"][rb["alive"] != 0])) and len(ids) < n
        assert moved > 500, moved
        return dev
    finally:
        ref.close()
        for ib in tiles.values():
            ib.close()


@pytest.mark.parametrize("old_order,on_device", [(1, False), (0, False), (1, True)])
def test_two_by_two_tiles_outputs_match_the_undivided_grid(old_order, on_device):
    """after steps 1, 20 and 40 the five gathered outputs of the tiles agree with the undivided handle's within BOUND.
    Measured on an MI355X (the largest of the three steps and five planes): 1.44e-12 with old_interp_flds_order on (host and
    device buffers alike), 1.08e-12 with it off; spread_mass 6.9e-13 at most."""
    dev = _two_by_two(old_order, True, on_device, (1, 20, 40))
    print("tiles against the undivided handle, old_interp_flds_order", old_order, "device buffers", on_device, ":", dev)
    worst = max(max(d.values()) for d in dev.values())
    print("largest deviation:", worst, "bound:", BOUND)
    assert sorted(dev) == [1, 20, 40]
    assert worst <= BOUND, dev


def test_two_by_two_tiles_without_the_halo_update_are_wrong():
    """the control: the same run with the update skipped differs by more than 1e-3 of the plane maximum in spread_mass
    (measured: 0.21 after one step, 0.14 after forty)"""
    dev = _two_by_two(1, False, False, (1, 40))
    print("tiles without the halo update:", dev)
    assert dev[1]["spread_mass"] > 1e-3 and dev[40]["spread_mass"] > 1e-3, dev


# ---- two ranks on one GPU ----
def _worker(rank, world, port, nbergs, nsteps, out_dir, cyclic):
    import torch.distributed as dist
    from icebergs_amd.decomposed import HipTile, TileExchange
    from icebergs_amd.framework import Icebergs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    whole, p, b = D._population(world, nbergs, cyclic)
    S.set_diag_all(p)
    if cyclic:
        p.periodic_reentry = 0            # on a tile the seam is a real boundary between ranks
    g = D._channel(rank, world) if cyclic else D._grid(rank, world)
    ib = Icebergs(g, p, capacity=nbergs)
    ib.upload_bergs(HC.split_bergs(b, rank, 0, D.NI, D.NJ))
    tile = HipTile(ib)
    ex = TileExchange(world, 1, dist, cyclic_x=cyclic)
    for _ in range(nsteps):
        ex.step(tile)
    out = ib.fetch()[1][:, H:H + D.NJ, H:H + D.NI].copy()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), out=out, sent=ex.sent, received=ex.received)
    ib.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("cyclic", [False, True])
def test_two_ranks_hip_tiles_outputs_on_one_gpu(tmp_path, cyclic):
    """TileExchange.step with HIP handles, both ranks on GPU 0 and gloo for the messages, on the open box and the cyclic channel
    of tests/test_decomposed.py: the assembled outputs against the undivided oracle within the 1e-9 that file uses for HIP
    against the oracle (measured: 7.7e-14 on the box, 9.2e-15 on the channel)"""
    import oracle_lib
    oracle_lib.build()
    world = 2
    nbergs, nsteps = (300, 60) if cyclic else (400, 30)
    port = 30900 + (os.getpid() % 2000) + int(cyclic)
    mp.spawn(_worker, args=(world, port, nbergs, nsteps, str(tmp_path), cyclic), nprocs=world, join=True)
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert sum(int(q["sent"]) for q in parts) == sum(int(q["received"]) for q in parts) > 20
    got = HC.assemble({(r, 0): parts[r]["out"] for r in range(world)}, world, 1)
    dev, _ = HC.deviations(got, HC.whole_oracle_out(world, nbergs, nsteps, cyclic))
    print("two HIP ranks against the undivided oracle,", "cyclic channel" if cyclic else "open box", ":", max(dev.values()), dev)
    assert max(dev.values()) <= 1e-9, dev
