"""Which berg_kernel a launch gets (icebergs_amd/csrc/kid_launch_select.hpp), the selection alone: tests/launch_select_host.cpp
enumerates every input under AddressSanitizer and UndefinedBehaviorSanitizer -- the K choice against the four ifs of the launch
macro it replaced, instance_exists against the list of call sites and the dead set, the part count and the slow-lane eligibility
against their former expressions (n = 4095 / 4096 included).  Host code with its own main; no GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_launch_selection_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "launch_select_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "launch_select_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
