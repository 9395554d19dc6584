"""ignore_ij_restart through the Fortran glue (icebergs_amd/fortran/kid_locate_test.F90): &icebergs_nml with
ignore_ij_restart = .true. -> kid_icebergs_init, which hands the switch (and use_slow_find) to the handle -> kid_read_restart of a
file whose ine, jne are wrong.  The number of bergs kept and the checksum of their cells in row order equal what the Python host
gets from the same file, and what the generator placed; with ignore_ij_restart = .false. the same file keeps the wrong cells."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from icebergs_amd import lib as L
from icebergs_amd import synthetic as S
from icebergs_amd.framework import Icebergs
from test_fortran_gpu import icebergs_nml_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCATE = os.path.join(ROOT, "icebergs_amd", "fortran", "kid_locate_test")


def _checksum(ine, jne):
    k = np.arange(1, len(ine) + 1, dtype=np.int64)
    return int((k * (ine.astype(np.int64) + 1000 * jne.astype(np.int64))).sum())


def _run(tmp_path, p, grid, n, **nml):
    (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, **nml))
    r = subprocess.run([LOCATE, "20", "20", "1000.0", str(n), str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"kid_locate_test: kept=(\d+) checksum=(-?\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    return int(m.group(1)), int(m.group(2))


@pytest.mark.gpu
def test_namelist_switch_reaches_the_restart_read(tmp_path):
    n = 300
    grid, p, b = S.config_c1(n=n, seed=7)
    b["id"][:] = (np.int64(3) << 32) + np.arange(1, n + 1)
    junk = S.copy_bergs(b)
    junk["ine"][:], junk["jne"][:] = np.where(np.arange(n) % 2 == 0, 1, -5), np.where(np.arange(n) % 2 == 0, 1, 10000)
    lib = L.load()
    assert lib.kid_restart_write_bergs(str(tmp_path / "icebergs.res.nc").encode(), C.byref(p), C.byref(Icebergs._soa(junk))) == 0
    want = (n, _checksum(b["ine"], b["jne"]))
    host = {}
    for mode in ("search", "scan"):
        ib = Icebergs(grid, p, capacity=n)
        try:
            ib.set_restart_locate(mode)
            ib.read_restart(tmp_path)
            got = ib.download_bergs()
        finally:
            ib.close()
        host[mode] = (len(got["id"]), _checksum(got["ine"], got["jne"]))
        assert host[mode] == want, mode
    assert _run(tmp_path, p, grid, n, ignore_ij_restart=".true.", use_slow_find=".false.") == host["search"]
    assert _run(tmp_path, p, grid, n, ignore_ij_restart=".true.", use_slow_find=".true.") == host["scan"]
    kept, chk = _run(tmp_path, p, grid, n, ignore_ij_restart=".false.")
    assert kept == n // 2 and chk == _checksum(np.ones(kept, dtype=np.int32), np.ones(kept, dtype=np.int32))
