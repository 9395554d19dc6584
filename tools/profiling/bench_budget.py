"""Time kid_budget against the route a host had before it (download_bergs + fetch + the numpy sums) on config 2, at 1e6 and
1e7 bergs, on the same handle after two steps.  One process, ended by its own alarm.

  python tools/profiling/bench_budget.py [n ...] [--json=PATH]

Prints one JSON line: per size budget_ms (median of 20 calls, each ended by the call's own 96-byte read), host_ms (median of 3:
the downloads and the sums, the calving state left out as the handle has none), their ratio, and the two floating masses; then,
with reproducible sums turned on on the same handle, budget_repro_first_ms (the call that also builds the mode's static order)
and budget_repro_ms (median of 20: the key kernel and the one-bit radix pass every call of that mode adds to the sweep)."""
import json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
signal.alarm(900)   # the process's own time limit
import numpy as np
from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from icebergs_amd.framework import Icebergs

sizes = [int(float(a)) for a in sys.argv[1:] if not a.startswith("--")] or [1_000_000, 10_000_000]


def host_route(ib):
    """what a host could do without kid_budget: the whole population and the planes over the bus, then numpy"""
    d = ib.grid["desc"]
    b = ib.download_bergs()
    _, _, scal = ib.fetch()
    on = (b["alive"] != 0) & (b["ine"] >= d.isc) & (b["ine"] <= d.iec) & (b["jne"] >= d.jsc) & (b["jne"] <= d.jec)
    ms = b["mass_scaling"][on]
    dm = (b["mass"][on] + b["mass_of_bits"][on] + b["mass_of_fl_bits"][on] + b["mass_of_fl_bergy_bits"][on]) * ms
    return {"nbergs": int(on.sum()), "floating_mass": float(dm.sum()), "icebergs_mass": float((b["mass"][on] * ms).sum()),
            "bergy_mass": float(((b["mass_of_bits"][on] + b["mass_of_fl_bergy_bits"][on]) * ms).sum()),
            "fl_bits_mass": float((b["mass_of_fl_bits"][on] * ms).sum()), "floating_heat": float((dm * b["heat_density"][on]).sum()),
            "net_heat_to_ocean": float(scal[T.SCALAR_NAMES["net_heat_to_ocean"]])}


out = {"tool": "bench_budget", "config": 2, "sizes": {}}
for n in sizes:
    grid, p, b = S.config_c2(n=n, seed=2)
    ib = Icebergs(grid, p, capacity=n, device=0)
    ib.upload_bergs(b)
    del b
    ib.run(2)
    ib.budget(); ib.sync()   # warm-up: the sweep's buffers
    dev = []
    for _ in range(20):
        t0 = time.perf_counter(); bud = ib.budget(); dev.append(1e3 * (time.perf_counter() - t0))
    host = []
    for _ in range(3):
        ib.sync(); t0 = time.perf_counter(); ref = host_route(ib); host.append(1e3 * (time.perf_counter() - t0))
    assert bud["nbergs"] == ref["nbergs"]
    assert abs(bud["floating_mass"] - ref["floating_mass"]) <= 1e-12 * ref["floating_mass"]
    r = {"budget_ms": float(np.median(dev)), "budget_ms_min": min(dev), "host_ms": float(np.median(host)), "host_ms_all": host,
         "floating_mass_budget": bud["floating_mass"], "floating_mass_host": ref["floating_mass"], "nbergs": bud["nbergs"]}
    r["host_over_budget"] = r["host_ms"] / r["budget_ms"]
    ib.set_reproducible_sums(True); ib.sync()
    t0 = time.perf_counter(); rep = ib.budget(); r["budget_repro_first_ms"] = 1e3 * (time.perf_counter() - t0)
    dev = []
    for _ in range(20):
        t0 = time.perf_counter(); rep = ib.budget(); dev.append(1e3 * (time.perf_counter() - t0))
    assert rep["nbergs"] == bud["nbergs"]
    assert abs(rep["floating_mass"] - bud["floating_mass"]) <= 1e-12 * bud["floating_mass"]
    r["budget_repro_ms"], r["budget_repro_ms_min"] = float(np.median(dev)), min(dev)
    r["repro_over_default"] = r["budget_repro_ms"] / r["budget_ms"]
    out["sizes"][str(n)] = r
    ib.close()
print(json.dumps(out), flush=True)
for a in sys.argv[1:]:
    if a.startswith("--json="):
        open(a.split("=", 1)[1], "w").write(json.dumps(out, indent=1) + "\n")
