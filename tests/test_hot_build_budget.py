"""Compile-only guard on the plain hot build of the fused RK4 step (berg_kernel<true, true, evolve|thermo|spread, true, K>).

It compiles tools/profiling/hot_only.hip the way tools/profiling/hot.sh does (hipcc --cuda-device-only -S, the max-ILP
scheduler of the product's hot translation unit) and holds the listing to the budget DESIGN section 4 records: static VALU
count, 168 VGPRs at most (the third wave per SIMD), no spill, occupancy 3.  No GPU is needed; it skips without hipcc."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HAVE_HIPCC = os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)

# static VALU instructions of the kernel after the round-4 trims (K = 1: 3576, K = 3: 3676; before them 3708, 3808), ~3 % of slack
VALU_BUDGET = {1: 3680, 3: 3780}
MAX_VGPRS = 168


def _compile(tmp_path, k):
    out = tmp_path / ("hot_k%d.s" % k)
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
           "-DKID_HOT_ARGS=true,true,(PH_EVOLVE|PH_THERMO|PH_SPREAD),true,%d" % k,
           "-o", str(out), os.path.join(ROOT, "tools", "profiling", "hot_only.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out.read_text(), r.stderr


def _remarks(stderr):
    """kernel-resource-usage remarks of the berg_kernel instantiation: {name: int}"""
    res, inside = {}, False
    for line in stderr.splitlines():
        if "Function Name:" in line:
            inside = "berg_kernel" in line
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[", line)
        if inside and m:
            res[m.group(1)] = int(m.group(2))
    return res


def _ops(listing, want="berg_kernel"):
    """static opcode counts of one kernel in the listing (the logic of tools/profiling/isa_stats.py)"""
    ops, inside = collections.Counter(), False
    for line in listing.split("\n"):
        if re.match(r"^_Z\w*%s\w*:" % re.escape(want), line):
            inside = True
            continue
        if inside and line.startswith(".Lfunc_end"):
            break
        if not inside:
            continue
        t = line.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        ops[t.split()[0]] += 1
    return ops


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not found")
@pytest.mark.parametrize("k", [1, 3])
def test_plain_hot_build_budget(tmp_path, k):
    listing, stderr = _compile(tmp_path, k)
    ops = _ops(listing)
    assert ops, "berg_kernel not found in the listing"
    valu = sum(v for op, v in ops.items() if op.startswith("v_"))
    assert valu <= VALU_BUDGET[k], "K=%d: %d static VALU instructions > budget %d" % (k, valu, VALU_BUDGET[k])
    rem = _remarks(stderr)
    assert rem.get("VGPRs", 999) <= MAX_VGPRS, rem
    assert rem.get("VGPRs Spill", 1) == 0, rem
    assert rem.get("SGPRs Spill", 1) == 0, rem
    assert rem.get("Occupancy [waves/SIMD]", 0) == 3, rem
