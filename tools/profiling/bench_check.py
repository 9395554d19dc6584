"""Time kid_check_bergs (the debug-mode invariants on the device, csrc/kid_check.inc) on the resident state of config 2, at 1e6 and
1e7 bergs after two steps: all four checks in one call, each check alone, kid_sorted_ids, and -- the route a host had before --
kid_download_bergs of the same population, in the same run.  One process, ended by its own alarm.

  python tools/profiling/bench_check.py [n ...] [--json=PATH]

Prints one JSON line.  Per size and call: the host clock around a synchronised call, one warm-up, then five windows; the median
and all five.  The check calls are interleaved with each other; the downloads are timed after them, three windows, and one more
KID_CHECK_ALL directly behind a download (all_after_download).  The report of the timed state is included (n_xiyj after two steps of the fused build is a measurement
too)."""
import json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
signal.alarm(900)   # the process's own time limit
import numpy as np
from icebergs_amd import synthetic as S
from icebergs_amd.framework import Icebergs

sizes = [int(float(a)) for a in sys.argv[1:] if not a.startswith("--")] or [1_000_000, 10_000_000]
WINDOWS = 5


def timed(ib, call):
    ib.sync(); t0 = time.perf_counter(); call(); ib.sync()
    return 1e3 * (time.perf_counter() - t0)


out = {"tool": "bench_check", "config": 2, "grid": "360x200", "windows": WINDOWS, "sizes": {}}
for n in sizes:
    grid, p, b = S.config_c2(n=n, seed=2)
    ib = Icebergs(grid, p, capacity=n, device=0)
    ib.upload_bergs(b)
    del b
    ib.run(2)
    calls = {"all": lambda: ib.check_bergs("all"), "position": lambda: ib.check_bergs("position"), "order": lambda: ib.check_bergs("order"),
             "duplicates": lambda: ib.check_bergs("duplicates"), "ids": lambda: ib.check_bergs("ids"), "sorted_ids": ib.sorted_ids}
    for call in calls.values():     # warm-up: the kernels' code objects, rocprim's
        call()
    ms = {name: [] for name in calls}
    for _ in range(WINDOWS):        # interleaved: a drift of the machine lands on every call alike
        for name, call in calls.items():
            ms[name].append(timed(ib, call))
    ib.download_bergs()             # warm-up: the pinned staging of the download
    ms["download_bergs"] = [timed(ib, ib.download_bergs) for _ in range(3)]
    ms["all_after_download"] = [timed(ib, calls["all"])]
    rep = ib.check_bergs("all")
    r = {name + "_ms": {"median": float(np.median(v)), "windows": v} for name, v in ms.items()}
    r["download_over_all"] = float(np.median(ms["download_bergs"]) / np.median(ms["all"]))
    r["report"] = {k: rep[k] for k in ("n_rows", "n_xiyj", "n_land", "n_in_halo", "n_identical", "n_same_id", "n_same_berg", "n_dup_ids", "max_dxi", "max_dyj")}
    out["sizes"][str(n)] = r
    print(json.dumps({str(n): r}), flush=True)
    ib.close()
print(json.dumps(out), flush=True)
for a in sys.argv[1:]:
    if a.startswith("--json="):
        open(a.split("=", 1)[1], "w").write(json.dumps(out, indent=1) + "\n")
