#!/usr/bin/env python3
"""Duration of the hot build by the age of the row order: steps since the last re-binning.

Reads a rocprofv3 --kernel-trace CSV of bench.py (kernel trace only, the program after `--`):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 48 --warmup 12
    python3 tools/profiling/hot_by_age.py DIR/*/*_kernel_trace.csv --skip 36
Every launch of a hot build (berg_kernel<..., FAST = true, ...>) is one step.  A launch of the re-binning instance
(berg_kernel<..., true, K, false, true>) starts an interval at age 0; the plain hot builds that follow have age 1, 2, ...
--skip: the step launches of the spin-up and the warm-up (bench.py: --spinup + --warmup, 24 + 5 by default), which are counted
for the age but left out of the figures.  Prints count, mean, min and max in microseconds per age, and what the growth over
the interval costs: the mean over the plain launches against the youngest age seen."""
import argparse
import collections
import csv


def template_args(name):
    if "berg_kernel<" not in name:
        return None
    return [a.strip() for a in name.split("berg_kernel<")[1].split(">")[0].split(",")]


def classify(name):
    """None: not a hot build; "rebin": the re-binning instance; "hot": any other hot build"""
    a = template_args(name)
    if a is None or len(a) < 4 or a[3] != "true":
        return None
    return "rebin" if len(a) >= 7 and a[6] == "true" else "hot"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("csv")
    ap.add_argument("--skip", type=int, default=29, help="step launches of spin-up + warm-up, excluded from the figures")
    ap.add_argument("--steps", type=int, default=0, help="count this many step launches after the skipped ones (0: all)")
    a = ap.parse_args()
    rows = [r for r in csv.DictReader(open(a.csv)) if classify(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by_age = collections.defaultdict(list)
    rebin = []
    age, seen = None, 0          # age None: no re-binning seen yet, the order's age is unknown
    for r in rows:
        kind = classify(r["Kernel_Name"])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1.0e3
        age = 0 if kind == "rebin" else (None if age is None else age + 1)
        seen += 1
        if seen <= a.skip or (a.steps and seen > a.skip + a.steps) or age is None:
            continue
        (rebin if kind == "rebin" else by_age[age]).append(us)
    print("# %s: %d hot-build launches, %d skipped (spin-up, warm-up)" % (a.csv.split("/")[-1], len(rows), min(a.skip, len(rows))))
    print("%-22s %5s %9s %9s %9s" % ("steps since re-binning", "n", "mean_us", "min_us", "max_us"))
    if rebin:
        print("%-22s %5d %9.1f %9.1f %9.1f" % ("0 (re-binning inst.)", len(rebin), sum(rebin) / len(rebin), min(rebin), max(rebin)))
    allv = []
    for k in sorted(by_age):
        v = by_age[k]
        allv += v
        print("%-22d %5d %9.1f %9.1f %9.1f" % (k, len(v), sum(v) / len(v), min(v), max(v)))
    if allv:
        k0 = min(by_age)
        young = sum(by_age[k0]) / len(by_age[k0])
        mean = sum(allv) / len(allv)
        print("plain hot build: mean %.1f us over %d launches; age %d: %.1f us; growth over the interval: %.1f us per launch (%.1f %%)"
              % (mean, len(allv), k0, young, mean - young, 100.0 * (mean - young) / mean))


if __name__ == "__main__":
    main()
