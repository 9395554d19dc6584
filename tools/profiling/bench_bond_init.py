"""Time kid_initialize_bonds against the host route (synthetic.bond_neighbours + kid_upload_bonds) on the population of
bench_c4.py: 224x224 square-packed elements (50 176) on a 60x60 grid of 20 km cells.  One process, ended by its own alarm.

  python tools/profiling/bench_bond_init.py [nx] [--json PATH]

Prints one JSON line: device_ms (median of 5 calls on fresh populations), host_ms (KD-tree + upload), their ratio, and the
device time with the threshold given as a length and as twice that length.  With the doubled length every interior element
has 12 candidates, more than max_bonds: that call ends after its counting pass (KID_ECAPACITY), which is the search itself."""
import json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
signal.alarm(600)   # the process's own time limit
import numpy as np
from icebergs_amd import lib as L
from icebergs_amd import synthetic as S
from icebergs_amd.framework import Icebergs

args = [a for a in sys.argv[1:] if not a.startswith("--")]
nx = int(args[0]) if args else 224
radius = 1500.0
grid, p, b, _ = S.config_c4(nx=4, ny=4, hexagonal=False, radius=radius, ni=60, nj=60, gridres=20000.0, sub_steps=90,
                            origin=(100137.0, 100211.0), bump=(900.0e3, 440.0e3))   # (grid and namelist; the elements follow)
xs, ys = np.meshgrid(100137.0 + radius + 2 * radius * np.arange(nx), 100211.0 + radius + 2 * radius * np.arange(nx), indexing="ij")
n = nx * nx
b = S.empty_bergs(n)
b["lon"][:], b["lat"][:] = xs.ravel(), ys.ravel()
b["ine"][:] = np.floor(b["lon"] / 20000.0).astype(np.int32) + 1
b["jne"][:] = np.floor(b["lat"] / 20000.0).astype(np.int32) + 1
b["xi"][:], b["yj"][:] = b["lon"] / 20000.0 - (b["ine"] - 1), b["lat"] / 20000.0 - (b["jne"] - 1)
b["thickness"][:], b["width"][:], b["length"][:] = 200.0, 2 * radius, 2 * radius
b["mass"][:] = 200.0 * 850.0 * (2 * radius) ** 2
b["start_mass"][:], b["mass_scaling"][:] = b["mass"], 1.0
b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"]
b["start_lon"][:], b["start_lat"][:], b["start_year"][:] = b["lon"], b["lat"], 1
b = S.sort_reference_order(b)

ib = Icebergs(grid, p, capacity=n, device=0)


def timed(fn):
    ib.sync(); t0 = time.perf_counter(); r = fn(); ib.sync()
    return 1e3 * (time.perf_counter() - t0), r


ib.upload_bergs(b); ib.initialize_bonds(from_radii=True)   # warm-up: allocations, the static grid's extents
dev, formed = [], None
for _ in range(5):
    ib.upload_bergs(b)
    ms, formed = timed(lambda: ib.initialize_bonds(from_radii=True))
    dev.append(ms)
dev_tab = ib.download_bonds(int(p.max_bonds))
host = []
for _ in range(3):
    ib.upload_bergs(b)
    bb = S.copy_bergs(b)
    t0 = time.perf_counter()
    bd = S.bond_neighbours(bb, n, 2.0 * radius * 1.05, int(p.max_bonds))
    t_tree = 1e3 * (time.perf_counter() - t0)
    ms, _ = timed(lambda: ib.upload_bonds(bd))
    host.append((t_tree + ms, t_tree, ms))
assert int(bd["count"].sum()) == formed == int(dev_tab["count"].sum())
by_len = {}
for f in (1.0, 2.0):
    ib.upload_bergs(b); ib.sync()
    t0, outcome = time.perf_counter(), "formed"
    try:
        ib.initialize_bonds(from_radii=False, length=f * 2.0 * radius * 1.05)
    except L.KidError as e:
        assert "rc=-4" in str(e)
        outcome = "counting pass only (KID_ECAPACITY)"
    ib.sync()
    by_len[f] = (1e3 * (time.perf_counter() - t0), outcome)
host.sort()
out = {"tool": "bench_bond_init", "elements": n, "bond_sides": formed, "device_ms": float(np.median(dev)), "device_ms_all": dev,
       "host_ms": host[len(host) // 2][0], "host_tree_ms": host[len(host) // 2][1], "host_upload_ms": host[len(host) // 2][2],
       "device_ms_length": by_len[1.0][0], "device_ms_length_doubled": by_len[2.0][0], "length_doubled_outcome": by_len[2.0][1]}
out["host_over_device"] = out["host_ms"] / out["device_ms"]
out["doubled_over_single"] = out["device_ms_length_doubled"] / out["device_ms_length"]
print(json.dumps(out), flush=True)
for a in sys.argv[1:]:
    if a.startswith("--json="):
        open(a.split("=", 1)[1], "w").write(json.dumps(out, indent=1) + "\n")
ib.close()
