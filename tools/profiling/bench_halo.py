#!/usr/bin/env python3
"""Times the halo update of the on-ocean planes (kid_pack_halo_pair / kid_unpack_halo_pair, both axes: four calls per step;
DESIGN 7.5) on one handle: a 1440 x 1080 tile, 36 live planes, width 1.  The handle's own strips come back as its neighbours'
(a doubly periodic exchange with itself), so the calls and their sizes are those of an interior tile.  Three routes:
  device   device buffers (on_device = 1): the four calls only enqueue; the clock stops after a kid_sync
  host     host buffers: each call goes through the pinned staging buffer and waits for it
  parent   the only route a host had before these calls: kid_get_accumulators of the whole block, numpy strips, and the block
           uploaded again into a bound accumulator buffer
One JSON line; a timing tool, nothing is asserted on the times."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from icebergs_amd import synthetic as S  # noqa: E402
from icebergs_amd import types as T  # noqa: E402
from icebergs_amd.framework import Icebergs, _dp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ni", type=int, default=1440)
ap.add_argument("--nj", type=int, default=1080)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--parent-iters", type=int, default=3)
a = ap.parse_args()
import torch  # noqa: E402

grid = S.c2_forcing(S.latlon_grid(ni=a.ni, nj=a.nj, lon0=0.0, dlon=360.0 / a.ni, lat0=-75.0, dlat=140.0 / a.nj))
p = S.set_diag_all(S.default_params())
ib = Icebergs(grid, p, capacity=8)
assert ib.halo_plane_count() == 36
count = T.NSCALAR + T.NACC * ib.ncell
block = torch.zeros(count, dtype=torch.float64, device="cuda")
block[T.NSCALAR:] = torch.arange(T.NACC * ib.ncell, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
ib.bind_accum_buffer(block.data_ptr(), count)
n = [ib.halo_buffer_count(axis, 1) for axis in (0, 1)]
lib, h = ib.lib, ib.h


def four_calls(bufs, on_device):
    for axis in (0, 1):
        hi, lo = bufs[axis]
        ib._check(lib.kid_pack_halo_pair(h, axis, 1, hi, lo, on_device), "kid_pack_halo_pair")
        ib._check(lib.kid_unpack_halo_pair(h, axis, 1, hi, lo, on_device), "kid_unpack_halo_pair")   # what went east comes in from the west


def timed(bufs, on_device, iters):
    for _ in range(5):
        four_calls(bufs, on_device)
    ib.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        four_calls(bufs, on_device)
    ib.sync()
    return (time.perf_counter() - t0) * 1e6 / iters


dev = [tuple(torch.empty(n[axis], dtype=torch.float64, device="cuda") for _ in range(2)) for axis in (0, 1)]
torch.cuda.synchronize()
t_dev = timed([tuple(t.data_ptr() for t in pair) for pair in dev], 1, a.iters)
host = [tuple(np.empty(n[axis]) for _ in range(2)) for axis in (0, 1)]
t_host = timed([tuple(x.ctypes.data for x in pair) for pair in host], 0, a.iters)

# the parent commit's route: the whole block to the host, the strips moved with numpy, the whole block back
acc = np.zeros((T.NACC, ib.nj, ib.ni))
HL, A0 = S.HALO, T.ENUMS["KID_A_MASS_ON_OCEAN"]
t_parent = 0.0
for it in range(a.parent_iters + 1):
    ib.sync()
    t0 = time.perf_counter()
    ib._check(lib.kid_get_accumulators(h, _dp(acc), None, None), "kid_get_accumulators")
    v = acc[A0:A0 + 36]
    v[:, HL:HL + a.nj, HL - 1] = v[:, HL:HL + a.nj, HL + a.ni - 1]
    v[:, HL:HL + a.nj, HL + a.ni] = v[:, HL:HL + a.nj, HL]
    v[:, HL - 1, HL - 1:HL + a.ni + 1] = v[:, HL + a.nj - 1, HL - 1:HL + a.ni + 1]
    v[:, HL + a.nj, HL - 1:HL + a.ni + 1] = v[:, HL, HL - 1:HL + a.ni + 1]
    block[T.NSCALAR:].copy_(torch.from_numpy(acc.reshape(-1)))
    torch.cuda.synchronize()
    if it:
        t_parent += time.perf_counter() - t0
print(json.dumps({"what": "halo update of the on-ocean planes, both axes: 2 x (kid_pack_halo_pair + kid_unpack_halo_pair)", "ni": a.ni, "nj": a.nj, "planes": 36,
                  "width": 1, "doubles_per_direction": n, "iters": a.iters, "device_buffers_us_per_step": round(t_dev, 1),
                  "host_buffers_us_per_step": round(t_host, 1),
                  "parent_route_us_per_step": round(t_parent * 1e6 / a.parent_iters, 1), "parent_iters": a.parent_iters,
                  "parent_route": "kid_get_accumulators(acc), numpy strips, upload into the bound accumulator buffer"}))
ib.close()
