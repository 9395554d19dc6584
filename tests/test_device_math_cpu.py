"""The iterations behind the trimmed division, square roots and fifth-root forms, on the host: tests/device_math_host.cpp restates
them in plain C++ with the hardware's first guess as an argument, and this test runs it as a program under AddressSanitizer and
UndefinedBehaviorSanitizer over the input sets of the GPU test (tests/device_math_sets.py), with the seed at exact * (1 + delta)
for delta swept across the whole band the GPU test allows the hardware (2^-23 for v_rcp_f64 and v_rsq_f64, 3e-6 for the single-
precision fifth-root seed).  The worst error against long double must stay inside the bounds the source comments claim: the
bounds then belong to the algorithm, whatever a chip's seeds are inside the band.  tests/test_device_math_gpu.py ties the
restatement to the device code: fed the device's own seeds it reproduces the device's results bit for bit.

kid_div_r must give the bits of kid_div, and kid_sqrt_nn those of kid_sqrt for x >= 1e-300.  The program also counts quotients of
a >= b > 0 that come out below 1 (a in {b, the next eight doubles}) and fails on the first: accel's short cut of cr_q leans on there
being none, for any seed in the band."""
import os
import shutil
import subprocess

import pytest

import device_math_sets as D

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_iterations_hold_their_bounds_for_every_seed_in_the_band(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe, sets = str(tmp_path / "device_math_host"), str(tmp_path / "sets.bin")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "device_math_host.cpp")],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    D.write_host_sets(sets)
    run = subprocess.run([exe, sets, repr(D.BAND_RCP), repr(D.BAND_RSQ), repr(D.BAND_RPOW5)], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    seen = {}
    for l in lines:
        if l.startswith("WORST "):
            w = l.split()
            seen[w[1]] = float(w[2])
    for name in ("kid_rcp", "mul_rcp", "kid_div", "kid_sqrt", "kid_rsqrt", "kid_rpow5", "kid_pow08"):
        assert seen[name] <= D.BOUND[name], (name, seen[name])
