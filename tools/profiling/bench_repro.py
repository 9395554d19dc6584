"""Cost of reproducible sums (kid_set_reproducible_sums): bench.py's plain one-GPU population (config 2 physics, 1e7 bergs,
re-binning every 16 steps, forcing resident on the device) stepped with the switch off and on, ms per step for each.
Also reports how the bergs spread over the cells (the fold walks each cell's list in one thread: skewed lists are its
long pole).  Prints one JSON line.

    python tools/profiling/bench_repro.py [--bergs N] [--steps K] [--warmup W] [--only off|on]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from icebergs_amd import synthetic as S, types as T            # noqa: E402
from icebergs_amd.framework import Icebergs                     # noqa: E402
from icebergs_amd.distributed import ShardedStepper             # noqa: E402


def run(grid, params, bergs, repro, steps, warmup, spinup):
    dev = torch.device("cuda", 0)
    ib = Icebergs(grid, params, capacity=len(bergs["lon"]), device=0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ib.set_stream(stream.cuda_stream)
    ib.upload_bergs(bergs)
    ib.set_store_environment(False)
    if repro:
        ib.set_reproducible_sums(True)
    forcing = [torch.from_numpy(np.ascontiguousarray(grid["forcing"][name])).to(dev) for name in T.FORCING_NAMES]
    ptrs = [t.data_ptr() for t in forcing]
    _, count = ib.accum_device_ptr()
    acc_t = torch.zeros(count, dtype=torch.float64, device=dev)
    ib.bind_accum_buffer(acc_t.data_ptr(), count)
    stepper = ShardedStepper(ib, acc_t, ib.ncell, params.diag_mask, None, params=params, resort_interval=16)

    def step():
        stepper.set_forcing_device(ptrs)
        stepper.step()

    for _ in range(spinup + warmup):
        step()
    stepper.flush()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    stepper.flush()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / steps
    ib.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bergs", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--spinup", type=int, default=24)
    ap.add_argument("--only", choices=["off", "on"], default=None)
    args = ap.parse_args()
    grid, params, bergs = S.config_c2(n=args.bergs, seed=2)
    d = grid["desc"]
    ni = d.ied - d.isd + 1
    cells = np.bincount((bergs["ine"] - d.isd) + (bergs["jne"] - d.jsd) * ni)
    occ = cells[cells > 0]
    res = {"bergs": args.bergs, "steps": args.steps, "bergs_per_cell_median": float(np.median(occ)), "bergs_per_cell_max": int(occ.max()),
           "cells_occupied": int(occ.size)}
    for mode in ("off", "on"):
        if args.only and mode != args.only:
            continue
        res["ms_per_step_" + mode] = run(grid, params, bergs, mode == "on", args.steps, args.warmup, args.spinup)
    if "ms_per_step_off" in res and "ms_per_step_on" in res:
        res["ratio"] = res["ms_per_step_on"] / res["ms_per_step_off"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
