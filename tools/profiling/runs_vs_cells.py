#!/usr/bin/env python3
"""Runs of equal cell against distinct cells per wave as the row order decays (host-side count, config 2).

The hot build's scatter used to add once per RUN of adjacent lanes with equal cell and staged value; its packet slots go by
DISTINCT cell.  This counts both for every 64 consecutive rows (one wave of the hot build) of the population bench.py runs:
    python3 tools/profiling/runs_vs_cells.py [--bergs 10000000] [--spinup 24] [--ages 0,4,8,12,15]
After the spin-up (bergs start at rest) the population is re-binned once, the re-binning is switched off, and after k steps
download_bergs() gives the rows as the next hot build would read them.  A dead row is a key of its own (-1) in the run count,
as in make_runs, and no cell."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def count(b):
    key = np.where(b["alive"] != 0, b["ine"].astype(np.int64) + 100000 * b["jne"].astype(np.int64), -1)
    n = len(key)
    pad = (-n) % 64
    if pad:
        key = np.concatenate([key, np.full(pad, -1, dtype=np.int64)])
    key = key.reshape(-1, 64)
    key = key[(key >= 0).any(axis=1)]                     # (a wave without a live lane leaves at once)
    runs = 1 + (key[:, 1:] != key[:, :-1]).sum(axis=1)
    s = np.sort(key, axis=1)
    cells = (s[:, 0] >= 0).astype(np.int64) + ((s[:, 1:] != s[:, :-1]) & (s[:, 1:] >= 0)).sum(axis=1)
    return runs, cells


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bergs", type=int, default=10_000_000)
    ap.add_argument("--spinup", type=int, default=24)
    ap.add_argument("--ages", default="0,4,8,12,15")
    a = ap.parse_args()
    from icebergs_amd import synthetic as S
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=a.bergs, seed=2)
    ib = Icebergs(grid, p, capacity=a.bergs)
    try:
        ib.upload_bergs(b)
        del b
        ib.set_store_environment(False)
        ib.set_resort_interval(16)
        ib.run(a.spinup)
        ib.move_berg_between_cells()
        ib.set_resort_interval(0)
        print("# config_c2(n=%d, seed=2), %d spin-up steps, re-binned once, then no re-binning; per 64 consecutive rows" % (a.bergs, a.spinup))
        print("%-5s %10s %9s %9s %9s %10s %9s %9s %14s %14s" % ("steps", "waves", "runs_mean", "runs_p99", "runs_max", "cells_mean", "cells_p99", "cells_max",
                                                                    "waves_cells>11", "waves_runs>16"))
        done = 0
        for k in [int(x) for x in a.ages.split(",")]:
            if k > done:
                ib.run(k - done)
                done = k
            runs, cells = count(ib.download_bergs())
            print("%-5d %10d %9.2f %9.0f %9d %10.2f %9.0f %9d %14d %14d" % (k, len(runs), runs.mean(), np.percentile(runs, 99), runs.max(), cells.mean(),
                                                                            np.percentile(cells, 99), cells.max(), int((cells > 11).sum()), int((runs > 16).sum())))
            sys.stdout.flush()
    finally:
        ib.close()


if __name__ == "__main__":
    main()
