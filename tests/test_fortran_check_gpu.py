"""The debug-mode invariants in the Fortran glue (kid_glue_check_bergs): kid_check_test.F90 reads icebergs_nml, builds the
stand-alone driver's grid, holds a population and runs one coupling step.  With debug = T each of the three checksum groups ends
with the two lines of count_out_of_order and check_for_duplicates in the reference's formats (FW:4083-4084, 4154-4155), with the
numbers Icebergs.check_bergs gives for the same population; with debug = F no line starts with KID.  Called with check_position
included on a population with one xi planted wrong, the program stops with the reference's message and the planted id."""
import os
import re
import subprocess

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from test_fortran_chksum_gpu import LABELS, ROOT, _read_result, _write_case
from test_fortran_gpu import icebergs_nml_text

EXE = os.path.join(ROOT, "icebergs_amd", "fortran", "kid_check_test")
ORDER = re.compile(r"KID, count_out_of_order: # out of order= {5}0 # in halo=( *\d+) # identicals=( *\d+) (.*)")
DUPS = re.compile(r"KID, check_for_duplicates: # with same id=( *\d+) # identical bergs=( *\d+) (.*)")


def _population():
    """config 1, 300 bergs; three of them share their start keys (3 pairs), two of those in one cell (1 identical), and one of
    the pair is a copy of the other in every member but the id (1 identical berg)"""
    grid, p, b = S.config_c1(n=300, seed=5)
    for f in T.BERG_F64_NAMES + T.BERG_I32_NAMES:
        b[f][11] = b[f][10]
    for f in ("start_year", "start_day", "start_mass", "start_lon", "start_lat"):
        b[f][200] = b[f][10]
    assert (b["ine"][200], b["jne"][200]) != (b["ine"][10], b["jne"][10])
    return grid, p, b


@pytest.mark.gpu
def test_glue_prints_the_two_lines_under_debug(tmp_path):
    from icebergs_amd.framework import Icebergs
    grid, p, b = _population()
    n = len(b["lon"])
    case, res = str(tmp_path / "check.bin"), str(tmp_path / "check.out")
    _write_case(case, 20, 20, 1, 1000.0, p.dt, 2.0, 34.0, n, b)
    out = {}
    for debug in (".true.", ".false."):
        (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, debug=debug))
        r = subprocess.run([EXE, case, res], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout + r.stderr
        assert "kid_check_test: done" in r.stdout
        out[debug] = r.stdout.splitlines()
    assert not [line for line in out[".false."] if line.startswith("KID")]
    lines = out[".true."]
    d, fp, st = _read_result(res)
    ib = Icebergs({"desc": d, "static": st, "forcing": {k: np.zeros_like(st["lon"]) for k in T.FORCING_NAMES}}, fp, capacity=n)
    try:
        ib.upload_bergs(b)
        want = ib.check_bergs(("order", "duplicates", "ids"))
    finally:
        ib.close()
    assert (want["n_same_id"], want["n_same_berg"], want["n_identical"], want["n_in_halo"]) == (3, 1, 1, 0)
    heads = [k for k, line in enumerate(lines) if line.startswith("KID: checksumming gridded data @ ")]
    assert len(heads) == 3
    order = [k for k, line in enumerate(lines) if line.startswith("KID, count_out_of_order:")]
    assert len(order) == 3
    for q, (k, label) in enumerate(zip(order, LABELS)):
        # the end of its group: behind the last grd_chksum line, before the next group's bergs line
        assert lines[k - 1].startswith("KID, grd_chksum") and k > heads[q] and (q == 2 or k < heads[q + 1])
        assert q == 2 or lines[k + 2].startswith("KID, bergs_chksum: ")
        m1, m2 = ORDER.fullmatch(lines[k]), DUPS.fullmatch(lines[k + 1])
        assert m1 and m2, (lines[k], lines[k + 1])
        assert len(m1.group(1)) == 6 and len(m1.group(2)) == 6 and len(m2.group(1)) == 9 and len(m2.group(2)) == 9      # i6, i9
        assert m1.group(3) == label and m2.group(3) == label
        if q == 0:          # before anything has moved: the numbers of the Python host for the same population
            assert (int(m1.group(1)), int(m1.group(2))) == (want["n_in_halo"], want["n_identical"])
            assert (int(m2.group(1)), int(m2.group(2))) == (want["n_same_id"], want["n_same_berg"])
        else:               # the keys never change, and the ocean is at rest: the same pairs
            assert int(m2.group(1)) == want["n_same_id"]


@pytest.mark.gpu
def test_glue_stops_on_a_wrong_xi(tmp_path):
    """xi, yj as the device computes them (kid_locate_bergs), so that check_position passes; then one xi moved by an ulp"""
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c1(n=300, seed=5)
    n = len(b["lon"])
    ib = Icebergs(grid, p, capacity=n)
    try:
        ib.upload_bergs(b)
        assert ib.locate_bergs("search")["found"] == n
        located = ib.download_bergs()
        assert np.array_equal(located["ine"], b["ine"]) and np.array_equal(located["jne"], b["jne"])
    finally:
        ib.close()
    (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, debug=".false."))
    case, res = str(tmp_path / "check.bin"), str(tmp_path / "check.out")
    _write_case(case, 20, 20, 1, 1000.0, p.dt, 2.0, 34.0, n, located)
    r = subprocess.run([EXE, case, res, "position"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "kid_check_test: done" in r.stdout, r.stdout + r.stderr
    assert "KID, count_out_of_order:" in r.stdout and "FATAL" not in r.stderr
    wrong = S.copy_bergs(located)
    wrong["xi"][123] = np.nextafter(wrong["xi"][123], 2.0)
    _write_case(case, 20, 20, 1, 1000.0, p.dt, 2.0, 34.0, n, wrong)
    r = subprocess.run([EXE, case, res, "position"], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode != 0 and "kid_check_test: done" not in r.stdout
    assert "KID, check_position, kid_check_test: berg has inconsistent xi,yj! id=%d " % int(wrong["id"][123]) in r.stderr, r.stderr
