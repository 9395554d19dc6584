"""The layout of the accumulator block (icebergs_amd/csrc/kid_planes.hpp), the layout alone: tests/planes_host.cpp enumerates
every input under AddressSanitizer and UndefinedBehaviorSanitizer -- the named plane ranges against the literals they replaced,
footprint_needed, nacc_live, plane_range_live and halo_plane_count against their former expressions for every diag_mask bit alone
and in pairs, and the nine-point stencil (entries and order of the additions) against the pairing of sum_up_spread_fields.
Host code with its own main; no GPU, no HIP."""
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


def test_plane_layout_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "planes_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "planes_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
