"""The tripolar north fold of a decomposed run on the device (csrc/kid_halo.inc): kid_unpack_halo_fold and
kid_fold_halo_self on a 7 x 5 tile against the numpy fold of tests/north_fold.py, HIP tiles of the folded grid through
TileExchange(fold_north=True).step against the undivided handle and the undivided oracle on the unfolded grid, and two gloo
ranks on one GPU."""
import os
import sys
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import halo_bergs as HB                   # noqa: E402  (its box of interacting bergs, for resident halo rows)
import north_fold as NF                   # noqa: E402
import test_halo_bergs_gpu as HBG         # noqa: E402
import test_halo_planes_cpu as HC         # noqa: E402
import test_north_fold_cpu as NFC         # noqa: E402  (D_CPU)

pytestmark = pytest.mark.gpu

H = S.HALO
EINVAL = -1
# tiles against the undivided handle: the rule and margin of DESIGN 7.5, 4 x max(d_cpu, 1e-12).  d_cpu is the oracle's own deviation
# between tiles of the folded grid and the undivided unfolded grid (NFC.D_CPU); 1e-12 is the level this project allows between two
# summation orders; tiles and whole share the device arithmetic, and the factor 4 covers the order of the 9-point sum in the turned half.
BOUND = 4.0 * max(NFC.D_CPU, 1e-12)
S_ERR = T.ENUMS["KID_S_ERROR_COUNT"]


def _icebergs(grid, p, cap):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)


# ---- 5. the two calls on a 7 x 5 tile ----
def _spread_tile(nic, njc, diag_all, seed):
    """a handle on an nic x njc tile of 5 km cells with two bergs per cell on average, the on-ocean planes spread and the
    east/west halo columns filled with the tile's own strips (as a cyclic row of one tile would), so that the corner columns of
    the north strip hold something"""
    g = S.c1_forcing(S.cartesian_grid(ni=nic, nj=njc, gridres=5000.0))
    p = S.default_params()
    p.dt, p.lat_ref, p.use_f_plane = 600.0, -70.0, 1
    if diag_all:
        S.set_diag_all(p)
    b = S.place_bergs(g, 2 * nic * njc, seed, (1, nic), (1, njc))
    b["uvel"][:], b["vvel"][:] = 0.1 + 0.01 * np.arange(len(b["lon"])), -0.2 + 0.01 * np.arange(len(b["lon"]))
    ib = _icebergs(g, p, len(b["lon"]))
    ib.upload_bergs(b)
    return ib


def _respread(ib, w):
    ib.calculate_mass_on_ocean()
    hi, lo = ib.pack_halo_pair(0, w)
    ib.unpack_halo_pair(0, hi, lo, w)


@pytest.mark.parametrize("diag_all", [False, True], ids=["9planes", "36planes"])
def test_fold_calls_against_the_numpy_fold(diag_all):
    """a second handle's north strip unpacked over the fold, widths 1 to 4, slots swapped and not, host and device buffers:
    every element of the fold rows is the numpy fold's bit for bit and nothing else of the accumulator block changes;
    kid_fold_halo_self equals a pack and a fold-unpack on the same handle"""
    import torch
    nic, njc = 7, 5
    npl = 36 if diag_all else 9
    mine, partner = _spread_tile(nic, njc, diag_all, 5), _spread_tile(nic, njc, diag_all, 6)
    try:
        assert mine.halo_plane_count() == npl
        for w in (1, 2, 3, 4):
            count = mine.halo_buffer_count(1, w)
            _respread(partner, w)
            strip, _ = partner.pack_halo_pair(1, w)
            want_strip, _ = HC.np_pack_halo_pair(partner.fetch()[0], 1, w, npl, nic, njc)
            assert np.array_equal(strip, want_strip) and int((strip != 0.0).sum()) > count // 5
            for swap in (True, False):
                for on_device in (False, True):
                    _respread(mine, w)
                    before = mine.fetch()[0].copy()
                    buf = torch.from_numpy(strip).cuda() if on_device else strip.copy()
                    mine.unpack_halo_fold(buf, w, swap)
                    after = mine.fetch()[0].copy()
                    want = before.copy()
                    NF.np_unpack_halo_fold(want, w, npl, nic, njc, strip, swap)
                    assert int((want != before).sum()) > count // 5                  # the fold rows did change
                    assert np.array_equal(after.view(np.int64), want.view(np.int64)), (w, swap, on_device)
                    rows = np.zeros(after.shape, dtype=bool)
                    rows[NF.A0:NF.A0 + npl, H + njc:H + njc + w] = True
                    assert np.array_equal(after[~rows].view(np.int64), before[~rows].view(np.int64))   # nothing outside rows jec+1 .. jec+w
                # the handle as its own partner
                _respread(mine, w)
                own, _ = mine.pack_halo_pair(1, w)
                mine.unpack_halo_fold(own, w, swap)
                two_calls = mine.fetch()[0].copy()
                mine.unpack_halo_fold(np.full(count, -7.0), w, swap)            # (a second spreading would add the bergs in another order)
                assert np.all(mine.fetch()[0][NF.A0:NF.A0 + npl, H + njc:H + njc + w, H - w:H + nic + w] == -7.0)
                mine.fold_halo_self(w, swap)
                one_call = mine.fetch()[0].copy()
                assert np.array_equal(one_call.view(np.int64), two_calls.view(np.int64)), (w, swap)
                assert np.abs(one_call[NF.A0:NF.A0 + npl, H + njc:H + njc + w]).max() > 0.0
        assert mine.fetch()[2][S_ERR] == 0.0
    finally:
        mine.close()
        partner.close()


def test_fold_calls_refuse_bad_widths_null_buffers_and_resident_halo_rows():
    """the widths kid_unpack_halo_pair refuses (0, 5 > halo, -1; 4 on a tile of 3 rows) and a NULL buffer: KID_EINVAL from both
    calls, nothing written; with halo rows resident both calls are refused by name until kid_evolve_icebergs has retired them"""
    from icebergs_amd.lib import KidError
    for nic, njc, bad, good in ((7, 5, (0, 5, -1), 4), (7, 3, (4,), 3)):
        ib = _spread_tile(nic, njc, True, 5)
        try:
            ib.calculate_mass_on_ocean()
            before = ib.fetch()[0].copy()
            a = np.full(8192, -7.0)
            for w in bad:
                assert ib.lib.kid_unpack_halo_pair(ib.h, 1, w, a.ctypes.data, None, 0) == EINVAL, w
                for swap in (0, 1):
                    assert ib.lib.kid_unpack_halo_fold(ib.h, w, a.ctypes.data, swap, 0) == EINVAL, w
                    assert b"width" in ib.lib.kid_last_error(ib.h)
                    assert ib.lib.kid_fold_halo_self(ib.h, w, swap) == EINVAL, w
            assert ib.lib.kid_unpack_halo_fold(ib.h, good, None, 1, 0) == EINVAL and b"NULL" in ib.lib.kid_last_error(ib.h)
            assert ib.lib.kid_unpack_halo_fold(ib.h, good, None, 1, 1) == EINVAL
            assert np.array_equal(ib.fetch()[0].view(np.int64), before.view(np.int64))
            ib.fold_halo_self(good)                                                # and the largest width is taken
            ib.unpack_halo_fold(np.zeros(ib.halo_buffer_count(1, good)), good)
        finally:
            ib.close()
    # tile (0, 0) of the box of tests/halo_bergs.py takes the copies its east neighbour packs (tests/test_halo_bergs_gpu.py has the lifetime)
    whole, b = HB.population()
    p = HB.params(False)
    west, east = _icebergs(HB.tile_grid(0, 0, whole), p, 400), _icebergs(HB.tile_grid(1, 0, whole), p, 400)
    try:
        west.upload_bergs(HB.trim(HB.split_bergs(b, 0, 0, 400)))
        east.upload_bergs(HB.trim(HB.split_bergs(b, 1, 0, 400)))
        west.calculate_mass_on_ocean()
        strip = np.zeros(west.halo_buffer_count(1, 2))
        west.unpack_halo_fold(strip, 2)
        _, to_west = east.pack_halo_bergs_pair(0, 0, (False, True))
        west.unpack_immigrants_pair(HBG.EMPTY, to_west)
        assert west.halo_berg_count() == len(to_west) > 10
        for call in (lambda: west.unpack_halo_fold(strip, 2), lambda: west.fold_halo_self(2)):
            with pytest.raises(KidError, match="rc=-1 .*halo rows"):
                call()
        west._check(west.lib.kid_zero_accumulators(west.h), "kid_zero_accumulators")
        west._check(west.lib.kid_evolve_icebergs(west.h), "kid_evolve_icebergs")
        assert west.halo_berg_count() == 0
        west._check(west.lib.kid_thermodynamics(west.h), "kid_thermodynamics")
        west.calculate_mass_on_ocean()
        west.unpack_halo_fold(strip, 2)
        west.fold_halo_self(2)
        assert west.fetch()[2][S_ERR] == 0.0
    finally:
        west.close()
        east.close()


# ---- 6. HIP tiles of the folded grid in one process ----
def _snapshot(ib, tx, ntx):
    nic = NF.NI // ntx
    acc, out, scalars = ib.fetch()
    return {"bergs": NF.live_unfolded(ib.download_bergs(), tx, ntx), "out": out[:, H:H + NF.NJ, H:H + nic].copy(), "errors": float(scalars[S_ERR])}


def _whole_handle(rk):
    """the undivided handle on U, phase by phase as the tiles are stepped: {step: (bergs, outputs)}"""
    g, b, p = NF.unfolded_grid(), NF.population(), NF.params(rk)
    ref = _icebergs(g, p, NF.N_BERGS)
    try:
        ref.upload_bergs(b)
        res = {}
        for step in range(1, NF.NSTEPS + 1):
            ref.run_phases(1)
            if step in NF.CHECK_AT:
                res[step] = (NF.live_unfolded(ref.download_bergs(), 0, 1), ref.fetch()[1][:, H:H + 2 * NF.NJ, H:H + NF.HALF].copy())
        assert ref.fetch()[2][S_ERR] == 0.0
        return res
    finally:
        ref.close()


def _hip_tiles(ntx, rk):
    from icebergs_amd.decomposed import HipTile
    whole = NF.folded_grid()
    bf = NF.to_folded(NF.population())
    p = NF.params(rk)
    handles, folded = {}, []

    def make_tile(tx):
        ib = _icebergs(NF.tile_grid(tx, ntx, whole), p, 2 * NF.N_BERGS)
        assert ib.buffer_width() == 34
        ib.upload_bergs(NF.trim(NF.split_bergs(bf, tx, ntx, NF.N_BERGS)))
        handles[tx] = ib
        return HipTile(ib)

    def after_step(tile, tx, ex, step):
        """every record that came over the fold sits in the cell its rewritten indices name: the first guess of the unpack held"""
        recs = ex.fold_records
        if not len(recs):
            return
        b = tile.ib.download_bergs()
        row = {int(i): k for k, i in enumerate(b["id"]) if b["alive"][k]}
        for r, i in zip(recs, HB.record_ids(recs)):
            k = row[int(i)]
            assert (int(b["ine"][k]), int(b["jne"][k])) == (int(r[NF.W_INE]), int(r[NF.W_JNE])), (step, tx, int(i))
            assert 1 <= r[NF.W_INE] <= NF.NI // ntx and r[NF.W_JNE] == NF.NJ
        folded.append(len(recs))
    try:
        ranks = NF.step_tiles(ntx, make_tile, NF.NSTEPS, after_step=after_step, snapshot=lambda tile, tx: _snapshot(tile.ib, tx, ntx))
        return ranks, sum(folded)
    finally:
        for ib in handles.values():
            ib.close()


@pytest.mark.parametrize("rk", [0, 1], ids=["verlet", "rk4"])
@pytest.mark.parametrize("ntx", [1, 2])
def test_hip_tiles_over_the_fold_match_the_undivided_handle_and_oracle(ntx, rk):
    """layouts 1 x 1 (kid_fold_halo_self, records straight back) and 2 x 1 (kid_unpack_halo_fold) of F after steps 1, 20 and
    40: the same survivors, berg fields and the five outputs within BOUND of the undivided handle on U and within 1e-9 of the
    undivided oracle on U; sent == received, no error counted, every fold record in the cell its rewritten indices name.
    Measured on an MI355X: DESIGN 7.5."""
    oracle_snaps, oracle_outs, stats, _ = NF.whole_oracle(rk)
    ref = _whole_handle(rk)
    ranks, folded = _hip_tiles(ntx, rk)
    sent, received = sum(r[1] for r in ranks), sum(r[2] for r in ranks)
    print("ntx", ntx, "rk", rk, ": records sent", sent, "received", received, "over the fold", folded, "; U alone:", stats)
    assert sent == received and folded >= 20
    worst = worst_oracle = 0.0
    for step in NF.CHECK_AT:
        parts = [r[0][step] for r in ranks]
        assert all(q["errors"] == 0.0 for q in parts)
        bergs = NF.join([q["bergs"] for q in parts])
        out = NF.out_to_unfolded(HC.assemble({(tx, 0): q["out"] for tx, q in enumerate(parts)}, ntx, 1))
        dev, dev_out = NF.compare(bergs, ref[step][0]), HC.deviations(out, ref[step][1])[0]
        dev_or, dev_or_out = NF.compare(bergs, oracle_snaps[step]), HC.deviations(out, oracle_outs[step])[0]
        print("step", step, "against the handle: bergs", max(dev.values()), "outputs", max(dev_out.values()),
              "; against the oracle: bergs", max(dev_or.values()), "outputs", max(dev_or_out.values()))
        worst = max(worst, max(dev.values()), max(dev_out.values()))
        worst_oracle = max(worst_oracle, max(dev_or.values()), max(dev_or_out.values()))
    print("ntx", ntx, "rk", rk, ": against the undivided handle", worst, "bound", BOUND, "; against the undivided oracle", worst_oracle)
    assert worst <= BOUND, worst
    assert worst_oracle <= 1e-9, worst_oracle


# ---- 7. two ranks on one GPU ----
def _worker(rank, world, port, rk, out_dir):
    import torch.distributed as dist
    from icebergs_amd.decomposed import HipTile, TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bf = NF.to_folded(NF.population())
    ib = _icebergs(NF.tile_grid(rank, world), NF.params(rk), 2 * NF.N_BERGS)
    ib.upload_bergs(NF.trim(NF.split_bergs(bf, rank, world, NF.N_BERGS)))
    tile = HipTile(ib)
    ex = TileExchange(world, 1, dist, fold_north=True)
    for _ in range(NF.NSTEPS):
        ex.step(tile)
    snap = _snapshot(ib, rank, world)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), sent=ex.sent, received=ex.received, out=snap["out"], errors=snap["errors"], **snap["bergs"])
    ib.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_over_the_fold_on_one_gpu(tmp_path):
    """TileExchange(fold_north=True).step with HIP handles, both ranks on GPU 0 and gloo for the messages (2 x 1, RK4): bergs and
    outputs after 40 steps against the undivided oracle on U within the 1e-9 this project uses for HIP against the oracle"""
    world, rk = 2, 1
    want_bergs, want_out = NF.whole_oracle(rk)[0][NF.NSTEPS], NF.whole_oracle(rk)[1][NF.NSTEPS]
    port = 32300 + (os.getpid() % 2000)
    ctx = mp.spawn(_worker, args=(world, port, rk, str(tmp_path)), nprocs=world, join=False)
    deadline = time.monotonic() + 120.0
    while not ctx.join(timeout=5.0):
        if time.monotonic() > deadline:
            for proc in ctx.processes:
                proc.kill()
            pytest.fail("the two ranks did not finish in 120 s")
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    assert sum(int(q["sent"]) for q in parts) == sum(int(q["received"]) for q in parts) >= 20
    assert all(float(q["errors"]) == 0.0 for q in parts)
    got = NF.join([{k: q[k] for k in NF.FIELDS + ("id",)} for q in parts])
    out = NF.out_to_unfolded(HC.assemble({(r, 0): parts[r]["out"] for r in range(world)}, world, 1))
    dev, dev_out = NF.compare(got, want_bergs), HC.deviations(out, want_out)[0]
    print("two HIP ranks over the fold against the undivided oracle: bergs", max(dev.values()), "outputs", max(dev_out.values()))
    assert max(dev.values()) <= 1e-9 and max(dev_out.values()) <= 1e-9, (dev, dev_out)
