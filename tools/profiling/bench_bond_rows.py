"""Time the two row permutations of a bonded handle (kid_set_bonds_follow_rows: kid_move_berg_between_cells and kid_compact_bergs
carry the bond tables, csrc/kid_rows.inc) against the only route there was before -- download bergs and bonds, permute on the
host, upload both again (kid_upload_bonds hashes the ids on the host) -- and config 4's step on a shuffled upload before and
after one re-binning.  One process, ended by its own alarm.

  python tools/profiling/bench_bond_rows.py [nx ...] [--steps=K] [--json=PATH]

nx: the lattice is nx x nx square-packed elements of config 4 (tools/profiling/bench_c4.py: 224 is BASELINE's 50 176; 1000 is 1e6),
uploaded in a seeded shuffle.  Prints one JSON line per size and one at the end.  Every time is the host clock around a
synchronised call; one warm-up, then REPEATS windows in which the device route and the host route alternate, each on a freshly
uploaded shuffled population (the uploads between the windows are not timed); the median and all windows are reported.
bytes: what permute_bonds_kernel moves, from the shapes -- per list slot 116 B (other_id 8, broken 4, partner row 4, partner slot 4,
twelve fields of 8) read and written for the slots in use and 116 B written for the others, the counts both ways, and per slot in
use the 12 B of perm-independent lookups (keep, alive, inverse) -- and the bandwidth that the whole entry point reaches on
them, a lower bound of the kernel's own (the entry point also sorts and moves the berg SoA)."""
import json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
signal.alarm(1100)   # the process's own time limit
import numpy as np
from icebergs_amd import synthetic as S
from icebergs_amd.framework import Icebergs

sizes = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [224, 1000]
opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--") and "=" in a)
STEPS = int(opts.get("steps", 5))
REPEATS = 5
SLOT_BYTES = 8 + 4 + 4 + 4 + 12 * 8


def rows_of(b, bd, rows):
    """(bergs, bonds) with the given rows, lists untouched"""
    n, mb = len(b["lon"]), bd["max_bonds"]
    nb = {k: (np.ascontiguousarray(v[rows]) if hasattr(v, "dtype") and v.shape[:1] == (n,) else v) for k, v in b.items()}
    nbd = {"max_bonds": mb, "count": np.ascontiguousarray(bd["count"][rows])}
    for k, v in bd.items():
        if k not in ("max_bonds", "count"):
            nbd[k] = np.ascontiguousarray(v.reshape(mb, n)[:, rows]).reshape(mb * len(rows))
    return nb, nbd


def timed(ib, call):
    ib.sync(); t0 = time.perf_counter(); call(); ib.sync()
    return 1e3 * (time.perf_counter() - t0)


def host_route(ib, mb, compact):
    b, bd = ib.download_bergs(), ib.download_bonds(mb)
    if compact:
        rows = np.nonzero(b["alive"] != 0)[0]
    else:
        rows = np.lexsort((b["ine"], b["jne"], b["alive"] == 0))   # by cell, j-major; the dead last
        rows = rows[: int((b["alive"] != 0).sum())]
    nb, nbd = rows_of(b, bd, rows)
    ib.upload_bergs(nb); ib.upload_bonds(nbd)


def med(v):
    return {"median": float(np.median(v)), "windows": [float(x) for x in v]}


out = {"tool": "bench_bond_rows", "config": 4, "repeats": REPEATS, "steps": STEPS, "sizes": {}}
for nx in sizes:
    t0 = time.time()
    grid, p, b, bd = S.config_c4(nx=nx, ny=nx, hexagonal=False, radius=1500.0, ni=60, nj=60, gridres=20000.0, sub_steps=90,
                                 origin=(100137.0, 100211.0), bump=(900.0e3, 440.0e3))
    n, mb = len(b["lon"]), bd["max_bonds"]
    shuffled = rows_of(b, bd, np.random.default_rng(20240).permutation(n))
    holed = (S.copy_bergs(shuffled[0]), shuffled[1])
    holed[0]["alive"][::7] = 0
    r = {"elements": n, "bond_sides": int(bd["count"].sum()), "max_bonds": mb, "generated_s": time.time() - t0}
    used = int(bd["count"].sum())
    r["permute_bonds_bytes"] = used * (2 * SLOT_BYTES + 12) + (n * mb - used) * SLOT_BYTES + n * (4 + 4 + 4)
    ib = Icebergs(grid, p, capacity=n + 37, device=0)

    def fresh(pop):
        ib.upload_bergs(pop[0]); ib.upload_bonds(pop[1])
    ib.set_bonds_follow_rows(True)
    ms = {k: [] for k in ("move_device", "move_host", "compact_device", "compact_host")}
    for rep in range(REPEATS + 1):   # (window 0 is the warm-up: code objects, rocprim, the second sets of arrays, pinned staging)
        w = {}
        fresh(shuffled); w["move_device"] = timed(ib, ib.move_berg_between_cells)
        fresh(shuffled); w["move_host"] = timed(ib, lambda: host_route(ib, mb, False))
        fresh(holed); w["compact_device"] = timed(ib, ib.compact)
        fresh(holed); w["compact_host"] = timed(ib, lambda: host_route(ib, mb, True))
        if rep:
            for k, v in w.items():
                ms[k].append(v)
    for k, v in ms.items():
        r[k + "_ms"] = med(v)
    r["move_host_over_device"] = r["move_host_ms"]["median"] / r["move_device_ms"]["median"]
    r["compact_host_over_device"] = r["compact_host_ms"]["median"] / r["compact_device_ms"]["median"]
    r["move_entry_point_GBps_on_bond_bytes"] = r["permute_bonds_bytes"] / (1e6 * r["move_device_ms"]["median"])
    # config 4's step on the shuffled upload, before and after one re-binning; and on the lattice order, for scale
    def step_ms():
        ib.run(1)
        return med([timed(ib, lambda: ib.run(1)) for _ in range(STEPS)])
    fresh(shuffled); r["step_shuffled_ms"] = step_ms()
    ib.move_berg_between_cells(); r["step_rebinned_ms"] = step_ms()
    fresh((b, bd)); r["step_lattice_order_ms"] = step_ms()
    r["fused_launches"] = ib.mts_fused_launches()
    ib.close()
    out["sizes"][str(n)] = r
    print(json.dumps({str(n): r}), flush=True)
    del b, bd, shuffled, holed
print(json.dumps(out), flush=True)
if "json" in opts:
    os.makedirs(os.path.dirname(os.path.abspath(opts["json"])), exist_ok=True)
    open(opts["json"], "w").write(json.dumps(out, indent=1) + "\n")
from icebergs_amd import lib as _kl
_kl.device_reset()   # see lib.device_reset: the exit order after a cooperative launch
