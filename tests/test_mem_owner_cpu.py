"""The owner of a handle's device and pinned memory (icebergs_amd/csrc/kid_mem.hpp), its bookkeeping alone: tests/mem_owner_host.cpp
drives it with malloc / free under AddressSanitizer and UndefinedBehaviorSanitizer -- record and forget, an unknown pointer, swapped
holders, grow keeps the prefix, byte counts back at zero, a second drain.  Host code with its own main; no GPU, no HIP."""
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


def test_mem_owner_bookkeeping_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "mem_owner_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "mem_owner_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
