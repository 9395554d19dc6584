"""The tripolar north fold of a decomposed run without a GPU: the numpy restatement of the fold of the on-ocean
planes against coded strips, the oracle behind the tile interface stepped through TileExchange(fold_north=True).step on the
folded grid of tests/north_fold.py against the undivided oracle on the unfolded grid, mass conservation over the fold, and the
partner table.  What is under test is the routing, the cell-index rewrite and the message code of icebergs_amd.decomposed."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import north_fold as NF                   # noqa: E402
import test_halo_planes_cpu as HC         # noqa: E402

H = S.HALO
K_MASS = T.ENUMS["KID_O_SPREAD_MASS"]
# The oracle's own deviation between tiles of the folded grid and the undivided unfolded grid, the largest over the six runs of
# test_oracle_tiles_over_the_fold (berg fields and the five outputs, relative to each field's maximum).
# tests/test_north_fold_gpu.py takes its bound against the undivided handle from it: 4 x max(D_CPU, 1e-12).
D_CPU = 1.2e-14   # Verlet 2.0e-15, RK4 1.1e-14, the same in the three layouts (the five outputs alone: 2.8e-16)


# ---- 1. the strip mapping ----
def _code(npl, nrow, ncol):
    """an array that holds its own (plane, row, column) code, rows and columns counted over the whole data domain"""
    pl, r, c = np.meshgrid(np.arange(npl), np.arange(nrow), np.arange(ncol), indexing="ij")
    return (pl * 10000.0 + r * 100.0 + c).astype(np.float64)


@pytest.mark.parametrize("npl", [9, 36])
@pytest.mark.parametrize("swap", [True, False])
def test_fold_strip_mapping(npl, swap):
    """a 7 x 5 tile with halo 4: after the fold every cell of rows njc+1 .. njc+w, columns 1-w .. nic+w holds the code of the
    partner's cell (nic+1-i, njc+1-k), of the mirrored slot with swap_slots; nothing else of the planes changes"""
    nic, njc = 7, 5
    nrow, ncol = njc + 2 * H, nic + 2 * H
    for w in (1, 2, 3, 4):
        partner = np.zeros((NF.A0 + 36, nrow, ncol))
        partner[NF.A0:NF.A0 + npl] = _code(npl, nrow, ncol)
        mine = np.full((NF.A0 + 36, nrow, ncol), -1.0)
        strip, _ = HC.np_pack_halo_pair(partner, 1, w, npl, nic, njc)
        assert strip.size == HC.np_halo_count(1, w, npl, nic, njc)
        NF.np_unpack_halo_fold(mine, w, npl, nic, njc, strip, swap)
        touched = np.zeros(mine.shape, dtype=bool)
        for pl in range(npl):
            src_pl = pl - pl % 9 + (8 - pl % 9) if swap else pl      # the slot that points the opposite way
            for k in range(1, w + 1):
                for i in range(1 - w, nic + w + 1):
                    jr, ic = H + njc + k - 1, H + i - 1                # 0-based places of (i, njc+k) in the data domain
                    want = src_pl * 10000.0 + (H + (njc + 1 - k) - 1) * 100.0 + (H + (nic + 1 - i) - 1)
                    assert mine[NF.A0 + pl, jr, ic] == want, (w, pl, k, i)
                    touched[NF.A0 + pl, jr, ic] = True
        assert touched.sum() == npl * w * (nic + 2 * w) and np.all(mine[~touched] == -1.0)


# ---- 2. and 3.: oracle tiles over the fold ----
_RUNS = {}


def _run(ntx, rk, fold):
    """the ntx x 1 layout of F stepped by the oracle through TileExchange.step, ranks as threads of this process (computed once
    and shared): per check step the bergs in U's terms, the five outputs unfolded, the bergs' mass and sum(spread_mass area)"""
    key = (ntx, rk, fold)
    if key in _RUNS:
        return _RUNS[key]
    NF._oracle_lib()
    whole = NF.folded_grid()
    bf = NF.to_folded(NF.population())
    p = NF.params(rk)
    nic = NF.NI // ntx

    def make_tile(tx):
        return NF.OracleTile(NF.tile_grid(tx, ntx, whole), p, NF.split_bergs(bf, tx, ntx, 3 * NF.N_BERGS))   # arrivals take new rows

    def snapshot(tile, tx):
        area = tile.o.grid["static"]["area"][H:H + NF.NJ, H:H + nic]
        return {"bergs": NF.live_unfolded(tile.b, tx, ntx), "out": tile.out_comp(), "mass": NF.total_mass(NF.trim(tile.b)),
                "terms": (tile.out_comp()[K_MASS] * area).reshape(-1)}
    ranks = NF.step_tiles(ntx, make_tile, NF.NSTEPS, fold_north=fold, snapshot=snapshot)
    res = {"sent": sum(r[1] for r in ranks), "received": sum(r[2] for r in ranks), "fold_calls": sum(r[3].fold_calls for r in ranks)}
    for step in NF.CHECK_AT:
        parts = [r[0][step] for r in ranks]
        res[step] = {"bergs": NF.join([q["bergs"] for q in parts]),
                     "out": NF.out_to_unfolded(HC.assemble({(tx, 0): q["out"] for tx, q in enumerate(parts)}, ntx, 1)),
                     "mass": math.fsum(q["mass"] for q in parts), "spread": math.fsum(np.concatenate([q["terms"] for q in parts]))}
    _RUNS[key] = res
    return res


@pytest.mark.parametrize("rk", [0, 1], ids=["verlet", "rk4"])
@pytest.mark.parametrize("ntx", NF.LAYOUTS)
def test_oracle_tiles_over_the_fold(ntx, rk):
    """layouts 1 x 1 (the tile is its own partner), 2 x 1 and 4 x 1 of F against the undivided oracle on U after steps 1, 20 and
    40: the same survivors, every id owned once, berg fields and the five gathered outputs within 1e-9 (the bound of DESIGN 7.6
    for tile runs against the undivided oracle; a larger value means the construction is wrong).  Measured d_cpu: DESIGN 7.5.
    The control, the same run with fold_north=False, loses the crossers: its spread_mass along the rows either side of the fold
    is off by more than 100 x d_cpu of the plane's maximum."""
    snaps, outs, stats, _ = NF.whole_oracle(rk)
    print("U alone:", stats)
    got = _run(ntx, rk, True)
    assert got["sent"] == got["received"] >= 20, (got["sent"], got["received"])
    assert got["fold_calls"] == NF.NSTEPS * ntx
    d_cpu = 0.0
    for step in NF.CHECK_AT:
        dev = NF.compare(got[step]["bergs"], snaps[step])
        dev_out, _ = HC.deviations(got[step]["out"], outs[step])
        print("ntx", ntx, "rk", rk, "step", step, "bergs", max(dev.values()), "outputs", max(dev_out.values()))
        d_cpu = max(d_cpu, max(dev.values()), max(dev_out.values()))
    print("ntx", ntx, "rk", rk, ": d_cpu =", d_cpu)
    assert d_cpu <= 1e-9, d_cpu
    ctl = _run(ntx, rk, False)
    want = outs[NF.NSTEPS][K_MASS]
    rows = slice(NF.NJ - 1, NF.NJ + 1)                 # row NJ of F in both halves: rows NJ and NJ+1 of U
    off = float(np.abs(ctl[NF.NSTEPS]["out"][K_MASS][rows] - want[rows]).max() / np.abs(want).max())
    print("ntx", ntx, "rk", rk, ": without the fold spread_mass along the fold is off by", off, "of the plane's maximum")
    assert ctl["fold_calls"] == 0 and off > 100.0 * d_cpu and off > 1e-6, (off, d_cpu)
    assert len(ctl[NF.NSTEPS]["bergs"]["id"]) < len(snaps[NF.NSTEPS]["id"])


@pytest.mark.parametrize("rk", [0, 1], ids=["verlet", "rk4"])
def test_mass_is_conserved_over_the_fold(rk):
    """sum(spread_mass area) over F against the bergs' mass with every kind of bits times mass_scaling, both summed exactly
    (math.fsum): after steps 1, 20 and 40 the relative gap stays within four times the largest the oracle on U alone shows for
    the same sum over the 40 steps of its run.  With exact sums the gap is what the rounding of the per-cell quotient and
    product leaves, 0 or one unit in the last place of the total (1.7e-16: U shows it at 3 of its 40 steps with Verlet, at 2
    with RK4, and at none of the three check steps, which is why the whole run is taken); measured on F: 0 or 1.7e-16 in every
    layout.  Without the fold what the last row spreads northward is lost: a deficit of 3.2 to 3.4 %."""
    gaps = NF.whole_oracle(rk)[3]
    bound = 4.0 * max(gaps.values())
    for ntx in NF.LAYOUTS:
        got, ctl = _run(ntx, rk, True), _run(ntx, rk, False)
        for step in NF.CHECK_AT:
            gap = abs(got[step]["spread"] - got[step]["mass"]) / got[step]["mass"]
            deficit = (ctl[step]["mass"] - ctl[step]["spread"]) / ctl[step]["mass"]
            print("ntx", ntx, "rk", rk, "step", step, "gap", gap, "U's own", gaps[step], "bound", bound, "; deficit without the fold", deficit)
            assert deficit > 1e-6 and deficit > 100.0 * bound, (ntx, step, deficit)
            assert gap <= bound, (ntx, step, gap, bound)


# ---- 4. routing ----
class FakeDist:
    def __init__(self, rank, world): self.r, self.w = rank, world
    def get_rank(self): return self.r
    def get_world_size(self): return self.w


def test_partner_table_and_refusals():
    from icebergs_amd.decomposed import TileExchange
    for ntx, table in ((1, [0]), (2, [1, 0]), (3, [2, 1, 0]), (4, [3, 2, 1, 0])):
        for nty in (1, 2):
            for tx in range(ntx):
                top = TileExchange(ntx, nty, FakeDist((nty - 1) * ntx + tx, ntx * nty), fold_north=True, tile_widths=[5] * ntx)
                assert top.fold_partner() == (nty - 1) * ntx + table[tx], (ntx, nty, tx)
                assert top.neighbour(0, 1) is None                       # the fold is no ordinary neighbour
                if nty == 2:
                    assert TileExchange(ntx, nty, FakeDist(tx, ntx * nty), fold_north=True).fold_partner() is None   # below the top row
                    assert TileExchange(ntx, nty, FakeDist(tx, ntx * nty), fold_north=True).neighbour(0, 1) == ntx + tx
    with pytest.raises(AssertionError, match="uniform in x"):
        TileExchange(3, 1, FakeDist(0, 3), fold_north=True, tile_widths=[6, 5, 5])
    TileExchange(3, 1, FakeDist(0, 3), tile_widths=[6, 5, 5])           # without the fold any widths do

    class Tile:
        params = S.default_params()

        def comp_domain(self):
            return 1, 6, 1, 5
    ex = TileExchange(1, 1, FakeDist(0, 1), fold_north=True, tile_widths=[5])
    with pytest.raises(AssertionError, match="uniform in x"):         # the tile is not of the width the layout was given
        ex.update_halos(Tile())
    ex = TileExchange(2, 1, FakeDist(0, 2), fold_north=True)
    t = Tile()
    t.params = S.default_params()
    t.params.interactive_icebergs_on = 1
    with pytest.raises(ValueError, match="fold_north"):
        ex.update_halo_bergs(t)
    with pytest.raises(ValueError, match="fold_north"):
        ex.step_interactive(t)
    # the default: the object of before
    plain = TileExchange(2, 1, FakeDist(1, 2))
    assert plain.fold_north is False and plain.fold_partner() is None and plain.neighbour(0, 1) is None and plain.neighbour(-1, 0) == 0
    assert len(plain.fold_records) == 0
