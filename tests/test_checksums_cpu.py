"""Device-side checksums, the part that needs no GPU: the numpy restatement of grd_chksum2 / grd_chksum3 (tests/chksum_ref.py)
against a plane worked by hand, the 59 labels of checksum_gridded (tests/golden/checksum_gridded_names.json) against the
KID_CHK_* enum and the Python and Fortran label tables, the declarations of the two entry points through every host layer, and
the report lines of a known record character by character (the expected lines were printed by a Fortran program with the
reference's format strings, FW:6691, 6817, 6876, 6975)."""
import json
import os
import re
import struct

import numpy as np

import chksum_ref as R
from icebergs_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _desc(isc, iec, jsc, jec, halo):
    d = T.GridDesc()
    d.isc, d.iec, d.jsc, d.jec = isc, iec, jsc, jec
    d.isd, d.ied, d.jsd, d.jed = isc - halo, iec + halo, jsc - halo, jec + halo
    return d


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_restatement_against_a_plane_worked_by_hand():
    """computational domain (1:2, 1:2) with one halo cell; fld(1,1) = 1 + 2**-32, fld(2,1) = 2, fld(1,2) = -(1 + 2**-32) / 2,
    fld(2,2) = 4, the halo full of 9.  Bit patterns: 3FF0000000100000, 4000000000000000, BFE0000000100000, 4010000000000000:
    the low words add to 00200000.  Weights i + 2 j = 3, 4, 5, 6 and the products are exact: 3 (1 + 2**-32) = 4008000000180000,
    8 = 4020.., -2.5 (1 + 2**-32) = C004000000140000, 24 = 4038..: the low words add to 002C0000.  The sum of the four values
    is 6.5 + 2**-33, exact at every step."""
    d = _desc(1, 2, 1, 2, 1)
    e = 2.0 ** -32
    fld = np.full((4, 4), 9.0)
    fld[1, 1], fld[1, 2], fld[2, 1], fld[2, 2] = 1.0 + e, 2.0, -(1.0 + e) / 2.0, 4.0      # [j - jsd, i - isd]
    assert [_bits(v) for v in (fld[1, 1], fld[1, 2], fld[2, 1], fld[2, 2])] == [0x3FF0000000100000, 0x4000000000000000, 0xBFE0000000100000, 0x4010000000000000]
    assert [_bits(v) for v in (3.0 * fld[1, 1], 8.0, 5.0 * fld[2, 1], 24.0)] == [0x4008000000180000, 0x4020000000000000, 0xC004000000140000, 0x4038000000000000]
    r = R.grd_chksum(d, fld)
    assert r["chksum"] == 0x00200000 and r["chksum2"] == 0x002C0000
    assert r["minv"] == -(1.0 + e) / 2.0 and r["maxv"] == 4.0
    mean = (6.5 + 2.0 ** -33) / 4.0
    assert r["mean"] == mean
    s2 = sd = 0.0
    for v in (fld[1, 1], fld[1, 2], fld[2, 1], fld[2, 2]):      # the loop order: j outer, i inner
        s2 = s2 + v ** 2
    for v in (fld[1, 1], fld[1, 2], fld[2, 1], fld[2, 2]):
        sd = sd + (v - mean) ** 2
    assert r["rms"] == (s2 / 4.0) ** 0.5 and r["sd"] == (sd / 4.0) ** 0.5
    # a sum that wraps: the sign bit of the low word is the sign of the printed integer
    neg = np.full((4, 4), -(2.0 ** -1022) * (2.0 ** -30))        # a subnormal: bit pattern 8000000000400000
    assert _bits(neg[0, 0]) == 0x8000000000400000
    assert R.grd_chksum(d, neg)["chksum"] == 4 * 0x00400000
    big = np.full((4, 4), float(np.array([0x3FF00000C0000000], dtype=np.uint64).view(np.float64)[0]))
    assert R.grd_chksum(d, big)["chksum"] == (4 * 0xC0000000) % (1 << 32) - 0      # 0x300000000 -> low word 0
    one = np.full((4, 4), float(np.array([0x3FF00000A0000000], dtype=np.uint64).view(np.float64)[0]))
    assert R.grd_chksum(d, one)["chksum"] == ((4 * 0xA0000000) % (1 << 32)) - (1 << 32)   # low word 0x80000000: negative


def test_restatement_3d_weights():
    """grd_chksum3: float(i + 2 j + 3 (k - 1)) with the data-domain indices; on a field of ones the weighted field is the weights"""
    d = _desc(3, 5, 2, 3, 2)
    nk = 3
    fld = np.ones((nk, d.jed - d.jsd + 1, d.ied - d.isd + 1))
    want = 0
    for k in range(1, nk + 1):
        for j in range(d.jsc, d.jec + 1):
            for i in range(d.isc, d.iec + 1):
                want += _bits(float(i + 2 * j + 3 * (k - 1)))
    r = R.grd_chksum(d, fld)
    assert r["chksum2"] == R._i32(want) and r["sums"]["n"] == nk * 3 * 2
    assert r["mean"] == 1.0 and r["rms"] == 1.0 and r["sd"] == 0.0 and r["minv"] == r["maxv"] == 1.0
    b = R.bounds(r)
    assert b["rms"][0] <= 1.0 <= b["rms"][1] and b["sd"][0] == 0.0 and b["sd"][1] < 1.0e-7


def test_names_file_against_the_enum_and_the_label_tables():
    golden = json.load(open(os.path.join(HERE, "golden", "checksum_gridded_names.json")))
    names = golden["names"]
    assert len(names) == 59 == T.ENUMS["KID_NCHK"] == T.NCHK
    enum = [k[len("KID_CHK_"):] for k, v in sorted(((k, v) for k, v in T.ENUMS.items() if k.startswith("KID_CHK_")), key=lambda kv: kv[1])]
    assert [T.ENUMS["KID_CHK_" + n] for n in enum] == list(range(59))
    assert enum == [n.upper() for n in names]
    assert T.CHK_LABELS == names and list(T.CHK_3D) == golden["three_d"]
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    m = re.search(r"labels\(KID_NCHK\) = \[character\(len=18\) ::(.*?)\]", mod, re.S)
    assert m and re.findall(r"'([^']*)'", m.group(1)) == names
    assert all(len(n) <= 18 for n in names)                      # a18 prints every one of them whole
    # grd_chksum3 fields are consecutive in the enum, which is what kid_chk_is_3d of the Fortran module relies on
    idx = sorted(names.index(n) for n in golden["three_d"])
    assert idx == list(range(T.ENUMS["KID_CHK_MASS_ON_OCEAN"], T.ENUMS["KID_CHK_STORED_ICE"] + 1)) + [T.ENUMS["KID_CHK_MELT_BY_CLASS"]]


def test_record_has_no_implicit_padding():
    import ctypes
    assert ctypes.sizeof(T.GrdChksum) == sum(ctypes.sizeof(t) for _, t in T.GrdChksum._fields_) == 64
    assert [n for n, _ in T.GrdChksum._fields_] == ["chksum", "chksum2", "minv", "maxv", "mean", "rms", "sd", "present", "pad_"]


def test_entry_points_are_declared_in_every_host_layer():
    from icebergs_amd import lib as L
    from icebergs_amd.framework import Icebergs
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kid.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kid_bergs_chksum_device\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s+out\[6\]\s*,\s*kid_grd_chksum\s*\*\s*per_cell\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+kid_checksum_gridded\s*\(\s*kid_handle\s*\*\s*h\s*,\s*kid_grd_chksum\s*\*\s*out\s*,\s*int32_t\s+n_out\s*\)\s*;", hdr)
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    public = set()
    for m in re.finditer(r"^\s*public ::(.*)$", mod, re.M):
        public |= {x.strip() for x in m.group(1).split(",")}
    for name in ("kid_bergs_chksum_device", "kid_checksum_gridded"):
        assert name in L.SYMBOLS
        assert re.search(r"bind\(C,\s*name='%s'\)" % name, mod) and name in public
    assert "kid_grd_chksum" in public
    inc = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_types_gen.inc")).read()
    assert re.search(r"type, bind\(C\) :: kid_grd_chksum", inc) and re.search(r"KID_NCHK = 59\b", inc)
    for method in ("bergs_chksum_device", "checksum_gridded", "checksum_report"):
        assert callable(getattr(Icebergs, method))
    glue = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_icebergs_glue.F90")).read()
    assert re.search(r"subroutine kid_glue_checksums\(g, label\)", glue) and re.search(r"public ::[^!]*kid_glue_checksums", glue, re.S)
    assert len(re.findall(r"if \(debug\) call kid_glue_checksums\(", glue)) == 3
    make = open(os.path.join(ROOT, "icebergs_amd", "fortran", "Makefile")).read()
    assert re.search(r"^kid_chksum_test:", make, re.M) and re.search(r"^all:.*\bkid_chksum_test\b", make, re.M)


def test_report_lines_character_by_character():
    from icebergs_amd.framework import format_bergs_chksum, format_grd_chksum
    rec = {"chksum": -123456789, "chksum2": 2883584, "minv": -0.5, "maxv": 4.0, "mean": 1.625, "rms": 1.0e100, "sd": 0.0}
    assert format_grd_chksum("rmean_calving_hflx", rec) == (
        "KID, grd_chksum2: rmean_calving_hflx chksum=            -123456789 chksum2=               2883584"
        " min=-5.000000000E-01 max= 4.000000000E+00 mean= 1.625000000E+00 rms= 1.000000000+100 sd= 0.000000000E+00")
    rec.update(maxv=1.0e-5, rms=123456.789, sd=-0.0)
    assert format_grd_chksum("Uvel_on_ocean", rec, three_d=True) == (
        "KID, grd_chksum3:      Uvel_on_ocean chksum=            -123456789 chksum2=               2883584"
        " min=-5.000000000E-01 max= 1.000000000E-05 mean= 1.625000000E+00 rms= 1.234567890E+05 sd=-0.000000000E+00")
    assert format_bergs_chksum("s/r run after calving", (1, -2, 3, 3, 0, 69)) == (
        "KID, bergs_chksum: s/r run after calv chksum=                     1 chksum2=                    -2"
        " chksum3=                     3 chksum4=                     3 chksum5=                     0 #=                    69")


def test_hand_made_population_in_the_restatement():
    """the population tests/test_checksums_gpu.py uploads, checked here without a GPU: six bergs count, cell counts [3, 1, 2, 0, ...]
    leave rank 2 of the first cell and both bergs of the third in fld, the last cell decides chksum5, a tie is broken by the row"""
    import test_checksums_gpu as G
    from test_chksum import numpy_bergs_chksum
    grid = G._tile()
    d = grid["desc"]
    assert (d.iec - d.isc + 1, d.jec - d.jsc + 1, d.isc - d.isd) == (7, 5, 2)
    base = G._hand_population(G._HAND)
    want = numpy_bergs_chksum(grid, base)
    assert want[5] == 6 and want[4] == 0 and want[2] == want[3]
    counts = G._count_plane(grid, base)[d.jsc - d.jsd:d.jec - d.jsd + 1, d.isc - d.isd:d.iec - d.isd + 1].ravel()
    assert counts[:4].tolist() == [3.0, 1.0, 2.0, 0.0] and counts.sum() == 6.0
    kept = [k for k in range(len(G._HAND)) if numpy_bergs_chksum(grid, G._perturbed(base, k))[:2] != want[:2]]
    assert kept == [2, 6, 7]
    occupied = numpy_bergs_chksum(grid, G._hand_population(G._HAND + [G._LAST]))
    assert occupied[4] != 0 and occupied[5] == 7
    assert numpy_bergs_chksum(grid, G._ties_swapped(base))[0] != want[0]
