"""The checksum lines of the Fortran glue under the namelist's `debug` (kid_glue_checksums in kid_icebergs_run_local and
kid_icebergs_run_finish): kid_chksum_test.F90 reads icebergs_nml, builds the stand-alone driver's grid, holds a population and
runs one coupling step.  With debug = T it prints three labelled groups in the reference's formats (FW:6975, 6876, 6691, 6817);
the bergs line of the first group, taken before anything has moved, is the line the Python host makes of the same population;
with debug = F nothing is printed."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from test_fortran_gpu import icebergs_nml_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "icebergs_amd", "fortran", "kid_chksum_test")
MAGIC = 1263093767
LABELS = ("top of s/r run", "s/r run after calving", "end of s/r run")


def _write_case(path, gni, gnj, nsteps, gridres, dt, sst, sss, cap, b):
    n = len(b["lon"])
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", MAGIC, gni, gnj, 0, nsteps))
        f.write(struct.pack("<4d", gridres, dt, sst, sss))
        f.write(struct.pack("<qq", cap, n))
        for name in T.BERG_F64_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.float64).tobytes())
        for name in T.BERG_I32_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(b["id"], dtype=np.int64).tobytes())


def _read_result(path):
    with open(path, "rb") as f:
        d = T.GridDesc.from_buffer_copy(f.read(C.sizeof(T.GridDesc)))
        p = T.Params.from_buffer_copy(f.read(C.sizeof(T.Params)))
        ni, nj = d.ied - d.isd + 1, d.jed - d.jsd + 1
        st = {name: np.frombuffer(f.read(8 * ni * nj), dtype=np.float64).reshape(nj, ni).copy() for name in T.GRID_STATIC_NAMES}
        assert f.read() == b""
    return d, p, st


@pytest.mark.gpu
def test_glue_prints_the_checksum_groups_under_debug(tmp_path):
    from icebergs_amd.framework import Icebergs, format_bergs_chksum
    gni = gnj = 20
    grid, p, b = S.config_c1(n=300, seed=5)
    n = len(b["lon"])
    case, res = str(tmp_path / "chksum.bin"), str(tmp_path / "chksum.out")
    _write_case(case, gni, gnj, 1, 1000.0, p.dt, 2.0, 34.0, n, b)
    out = {}
    for debug in (".true.", ".false."):
        (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, debug=debug))
        r = subprocess.run([EXE, case, res], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        assert "kid_chksum_test: done" in r.stdout
        out[debug] = r.stdout.splitlines()
    assert not [line for line in out[".false."] if line.startswith("KID")]
    lines = out[".true."]
    heads = [line for line in lines if line.startswith("KID: checksumming gridded data @ ")]
    assert heads == ["KID: checksumming gridded data @ " + label for label in LABELS]
    bergs = [line for line in lines if line.startswith("KID, bergs_chksum: ")]
    assert [line[19:37] for line in bergs] == [label[:18].rjust(18) for label in LABELS]
    assert all(re.fullmatch(r"KID, bergs_chksum: .{18}( (chksum[2-5]?|#)= *-?\d+){6}", line) and len(line) == len(format_bergs_chksum("", (0,) * 6)) for line in bergs)
    starts = [lines.index(h) for h in heads] + [len(lines)]
    for s, e in zip(starts[:-1], starts[1:]):                     # a group: the bergs line, the count record, the header, the fields
        assert lines[s - 2].startswith("KID, bergs_chksum: ") and lines[s - 1].startswith("KID, grd_chksum2: " + "# of bergs/cell".rjust(18))
        fields = list(itertools.takewhile(lambda line: line.startswith("KID, grd_chksum"), lines[s + 1:e]))
        assert [line[18:36].strip() for line in fields] == T.CHK_LABELS      # calving is configured by kid_icebergs_init: all 59
        assert all(line.startswith("KID, grd_chksum%d: " % (3 if line[18:36].strip() in T.CHK_3D else 2)) for line in fields)
    # the same population in a handle of the Python host, on the grid and with the parameters kid_icebergs_init derived
    d, fp, st = _read_result(res)
    ib = Icebergs({"desc": d, "static": st, "forcing": {k: np.zeros_like(st["lon"]) for k in T.FORCING_NAMES}}, fp, capacity=n)
    try:
        ib.upload_bergs(b)
        six = ib.bergs_chksum_device()
        assert six == ib.bergs_chksum() and six[5] == n
        assert bergs[0] == format_bergs_chksum(LABELS[0], six)
    finally:
        ib.close()
