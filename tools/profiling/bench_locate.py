"""Time kid_locate_bergs (cells from positions, csrc/kid_locate.inc) in both modes.  One process, ended by its own alarm.

  python tools/profiling/bench_locate.py [case ...] [--json=PATH]

Cases (default: all):
  c2-1e6, c2-1e7    config 2's 360 x 200 lat-lon grid.  Uniform in index space: find_cell's guess hits and mode 2 never scans.
  fine-1e6          1440 x 1080 lat-lon grid (0.25 x 0.15 degrees), 1e6 bergs: the walk is four times as long.
  curvi-1e5, curvi-1e6
                    336 x 300 cells (about 1e5), rows stretched towards the north and corners sheared as on the patch grid of
                    tests/curvilinear.py: the guess misses nearly everywhere, so mode 2 is the scan -- where the cooperative
                    scan matters.  With KID_HIP_SO naming a build whose scan is one lane's loop, the same case times that.

Each figure is the median of `reps` calls on freshly uploaded rows (cell (1, 1), xi = yj = 0), a host clock around the call,
which ends in the read of its three counts after a stream synchronise; the upload is outside the clock.  The first call of a
case (code object load) is discarded.  Every call must find every berg in the cell it was placed in.
Prints one JSON line."""
import json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
signal.alarm(1100)   # the process's own time limit
import numpy as np
from icebergs_amd import synthetic as S
from icebergs_amd import lib as L
from icebergs_amd.framework import Icebergs


def curvilinear_grid(ni=336, nj=300):
    grid = S.latlon_grid(ni=ni, nj=nj, lon0=10.0, dlon=0.05, lat0=-75.0, dlat=0.03)
    d, st = grid["desc"], grid["static"]
    i, j = S._ij(d)
    one = S.zeros(d) + 1.0
    i, j = i * one, j * one
    st["lat"] = -75.0 + 0.03 * (j + 0.35 * j * j / nj)                                  # rows 1.0 to 1.7 times the first one's height
    st["lon"] = st["lon"] + 0.12 * 0.05 * np.sin(2.0 * np.pi * j / 13.0 + 0.4) * np.sin(2.0 * np.pi * i / 29.0)
    st["lat"] = st["lat"] + 0.10 * 0.03 * np.cos(2.0 * np.pi * i / 11.0 + 0.3) * np.sin(2.0 * np.pi * j / 31.0)
    lon, lat = st["lon"], st["lat"]
    for name, a in (("lonc", lon), ("latc", lat)):                                      # FW:1153-1158
        st[name][1:, 1:] = 0.25 * ((a[1:, 1:] + a[:-1, :-1]) + (a[1:, :-1] + a[:-1, 1:]))
    return grid


def place(grid, n, seed):
    """n bergs strictly inside cells of the computational domain, through the bilinear map of the cell's corners"""
    d, st = grid["desc"], grid["static"]
    rng = np.random.Generator(np.random.PCG64(seed))
    b = S.empty_bergs(n)
    ine, jne = rng.integers(d.isc + 1, d.iec, size=n), rng.integers(d.jsc + 1, d.jec, size=n)
    xi, yj = rng.uniform(0.02, 0.98, size=n), rng.uniform(0.02, 0.98, size=n)
    jj, ii = jne - d.jsd, ine - d.isd
    for name in ("lon", "lat"):
        a = st[name]
        b[name][:] = (a[jj, ii] * xi + a[jj, ii - 1] * (1.0 - xi)) * yj + (a[jj - 1, ii] * xi + a[jj - 1, ii - 1] * (1.0 - xi)) * (1.0 - yj)
    b["ine"][:], b["jne"][:] = ine, jne
    b["mass"][:], b["thickness"][:], b["width"][:], b["length"][:], b["mass_scaling"][:] = 1.0e9, 100.0, 100.0, 150.0, 1.0
    return b


def c2(n):
    grid, p, b = S.config_c2(n=n, seed=2)
    return grid, p, b


CASES = {
    "c2-1e6": lambda: c2(1_000_000) + (5,),
    "c2-1e7": lambda: c2(10_000_000) + (3,),
    "fine-1e6": lambda: (lambda g: (g, S.default_params(), place(g, 1_000_000, 4), 5))(S.latlon_grid(ni=1440, nj=1080, lon0=0.0, dlon=0.25, lat0=-81.0, dlat=0.15)),
    "curvi-1e5": lambda: (lambda g: (g, S.default_params(), place(g, 100_000, 6), 5))(curvilinear_grid()),
    "curvi-1e6": lambda: (lambda g: (g, S.default_params(), place(g, 1_000_000, 7), 3))(curvilinear_grid()),
}
names = [a for a in sys.argv[1:] if not a.startswith("--")] or list(CASES)
out = {"tool": "bench_locate", "library": os.path.relpath(L.SO_PATH, ROOT), "cases": {}}
for name in names:
    grid, p, b, reps = CASES[name]()
    n = len(b["lon"])
    d = grid["desc"]
    true_i, true_j = b["ine"].copy(), b["jne"].copy()
    b["ine"][:], b["jne"][:], b["xi"][:], b["yj"][:] = 1, 1, 0.0, 0.0
    ib = Icebergs(grid, p, capacity=n, device=0)
    r = {"n": n, "cells": int((d.iec - d.isc + 1) * (d.jec - d.jsc + 1))}
    for mode in ("search", "scan"):
        ms = []
        for rep in range(reps + 1):
            ib.upload_bergs(b)
            ib.sync()
            t0 = time.perf_counter(); counts = ib.locate_bergs(mode); dt = 1e3 * (time.perf_counter() - t0)
            assert counts == {"found": n, "lost": 0, "grounded": 0}, (name, mode, counts)
            if rep:
                ms.append(dt)
        got = ib.download_bergs()
        assert np.array_equal(got["ine"], true_i) and np.array_equal(got["jne"], true_j), (name, mode)
        r[mode + "_ms"], r[mode + "_ms_all"] = float(np.median(ms)), ms
        r[mode + "_ns_per_berg"] = 1e6 * r[mode + "_ms"] / n
    out["cases"][name] = r
    ib.close()
    del b, got
    print(name, json.dumps(r), flush=True)
print(json.dumps(out), flush=True)
for a in sys.argv[1:]:
    if a.startswith("--json="):
        open(a.split("=", 1)[1], "w").write(json.dumps(out, indent=1) + "\n")
