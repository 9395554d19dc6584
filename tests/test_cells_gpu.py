"""The per-cell module on the device (icebergs_amd/csrc/kid_cells.inc): the device tables rebuilt while the forcing records of
the ODD set are the current ones.  With a side stream in use every prepass alternates between two sets of records, cell packets
and grid descriptors; kid_set_params dirties the tables, and the rebuild (refresh_tables) has to write the descriptor of either
set with that set's own pointers whichever of them is current.  Three steps leave the parity at 1; then one diagnostic bit that
adds accumulator planes is switched on and two more steps run, on forcing that alternates between two sets of planes.  A handle
on one stream, given the same calls, is the reference: what a berg does never depends on the schedule (bit for bit), the
atomically summed planes agree to the tolerances of test_pipelined_stepper_matches_plain (parity.compare).

37 x 9 computational cells with a halo of 2: one row of cells crosses the 32-cell wave of pack_packets_kernel and is no multiple
of its 8-cell unroll; 4096 bergs: the smallest population that takes two halves or the slow lane."""
import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
import parity as P

pytestmark = pytest.mark.gpu

N = 4096


def _config(monkeypatch):
    monkeypatch.setattr(S, "HALO", 2)
    grid = S.c2_forcing(S.latlon_grid(ni=37, nj=9, lat0=-64.0))
    d = grid["desc"]
    assert (d.iec - d.isc + 1, d.jec - d.jsc + 1, d.isc - d.isd, d.jed - d.jec) == (37, 9, 2, 2)
    p = S.default_params()
    p.dt = 1800.0
    b = S.place_bergs(grid, N, 41, (3, 35), (3, 7))
    return grid, p, b


@pytest.mark.parametrize("mode", [1, 2], ids=["two_halves", "slow_lane"])
def test_tables_rebuilt_at_parity_one(monkeypatch, mode):
    import torch
    from icebergs_amd.framework import Icebergs
    grid, p, b = _config(monkeypatch)
    dev = torch.device("cuda", 0)
    sets = []
    for scale in (1.0, 0.5):   # the second set, used on odd steps: half the ocean and wind velocities
        sets.append([torch.from_numpy(np.ascontiguousarray(grid["forcing"][name] * (scale if name in ("uo", "vo", "ua", "va") else 1.0))).to(dev)
                     for name in T.FORCING_NAMES])
    ptrs = [[t.data_ptr() for t in s] for s in sets]
    q = S.params_copy(p)
    q.diag_mask |= T.ENUMS["KID_DIAG_MASS"]   # one bit that adds planes: the live prefix grows from the core planes to all of them

    def run(side_mode):
        ib = Icebergs(grid, p, capacity=N, device=0)
        try:
            ib.set_stream(torch.cuda.current_stream().cuda_stream)
            side = torch.cuda.Stream(dev)
            if side_mode:
                ib.set_side_stream(side.cuda_stream, side_mode)
            ib.upload_bergs(b)
            for k in range(5):
                if k == 3:   # three prepasses so far: the odd set is current
                    ib.set_params(q)
                ib.step_prepare(ptrs[k & 1])
                ib.run(1)
            ib.sync()
            torch.cuda.synchronize()
            acc, out, scal = ib.fetch()
            return ib.download_bergs(), acc.copy(), out.copy(), scal.copy()
        finally:
            ib.close()
    ref, got = run(0), run(mode)
    assert (ref[0]["alive"] != 0).sum() == N
    assert np.abs(ref[1][T.ENUMS["KID_A_MASS"]]).max() > 0   # the added plane is filled
    P.compare(ref, got, "cells/parity 1/mode %d" % mode, params=q)
    o1, o2 = np.argsort(ref[0]["id"], kind="stable"), np.argsort(got[0]["id"], kind="stable")
    differ = [f for f in sorted(ref[0]) if not f.startswith("_") and not np.array_equal(np.asarray(ref[0][f])[o1], np.asarray(got[0][f])[o2])]
    print("fields that differ between the schedules:", differ)
    assert not differ
