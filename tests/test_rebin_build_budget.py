"""Compile-only guard on the re-binning instances of the plain hot build, berg_kernel<true, true, evolve|thermo|spread, true, K,
false, true> (K = 1, 3), in the manner of tests/test_hot_build_budget.py: compiled the way the product compiles them (the
max-ILP scheduler of the hot translation unit) they keep three waves per SIMD -- 168 VGPRs at most, LDS within 12 800 B per
one-wave workgroup -- with no spill and no scratch beyond the 16 B of the plain builds.  A two-wave re-binning launch would
cost about what the saved copy is worth.  No GPU is needed; it skips without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HAVE_HIPCC = os.path.isfile(HIPCC) and os.access(HIPCC, os.X_OK)


def _remarks(stderr):
    res, inside = {}, False
    for line in stderr.splitlines():
        if "Function Name:" in line:
            inside = "berg_kernel" in line
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[", line)
        if inside and m:
            res[m.group(1)] = int(m.group(2))
    return res


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not found")
@pytest.mark.parametrize("k", [1, 3])
def test_rebinning_instance_keeps_three_waves(tmp_path, k):
    """berg_kernel<true, true, evolve|thermo|spread, true, K, false, true> compiled the way the product compiles it: three
    waves per SIMD (<= 168 VGPRs, LDS <= 12 800 B per one-wave workgroup), no spill, no scratch beyond the 16 B of the plain build"""
    out = tmp_path / ("rebin_k%d.s" % k)
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", "-mllvm", "-amdgpu-sched-strategy=max-ilp",
           "-DKID_HOT_ARGS=true,true,(PH_EVOLVE|PH_THERMO|PH_SPREAD),true,%d,false,true" % k,
           "-o", str(out), os.path.join(ROOT, "tools", "profiling", "hot_only.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rem = _remarks(r.stderr)
    assert rem, "no resource-usage remarks for berg_kernel"
    assert rem.get("VGPRs", 999) <= 168, rem
    assert rem.get("VGPRs Spill", 1) == 0 and rem.get("SGPRs Spill", 1) == 0, rem
    assert rem.get("ScratchSize [bytes/lane]", 999) <= 16, rem
    assert rem.get("LDS Size [bytes/block]", 99999) <= 12800, rem
    assert rem.get("Occupancy [waves/SIMD]", 0) == 3, rem
