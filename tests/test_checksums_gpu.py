"""Device-side checksums on the GPU: kid_bergs_chksum_device gives the six integers of kid_bergs_chksum (the checker: a download
and a host sort) and of the numpy restatement of tests/test_chksum.py on every population, and kid_checksum_gridded gives the
records of tests/chksum_ref.py (grd_chksum2 / grd_chksum3 restated) for every field the handle holds.

Integers, min and max are compared exactly.  mean, rms and sd come from sums the device takes in a tree and the restatement one
element after the other: the sums may differ by 2 (N-1) 2**-53 sum|term| (the bound for two orders of N terms), and
chksum_ref.bounds turns that into bounds on the three printed values."""
import ctypes as C
import struct

import numpy as np
import pytest

import chksum_ref as R
from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from test_chksum import _population, numpy_bergs_chksum

pytestmark = pytest.mark.gpu


def _icebergs(grid, p, cap):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=cap)


def _mem(ib):
    a, b = C.c_int64(), C.c_int64()
    assert ib.lib.kid_memory_in_use(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _count_plane(grid, b):
    d = grid["desc"]
    plane = np.zeros((d.jed - d.jsd + 1, d.ied - d.isd + 1))
    for k in range(len(b["lon"])):
        if b["alive"][k] and d.isc <= b["ine"][k] <= d.iec and d.jsc <= b["jne"][k] <= d.jec:
            plane[b["jne"][k] - d.jsd, b["ine"][k] - d.isd] += 1.0
    return plane


def _check_record(name, got, ref):
    """one record of the device against the restatement's"""
    assert got["present"] == ref["present"], name
    assert (got["chksum"], got["chksum2"]) == (ref["chksum"], ref["chksum2"]), (name, got, ref["chksum"], ref["chksum2"])
    assert got["minv"] == ref["minv"] and got["maxv"] == ref["maxv"], (name, got, ref["minv"], ref["maxv"])
    if not ref["present"]:
        assert got["mean"] == got["rms"] == got["sd"] == 0.0, name
        return
    b = R.bounds(ref)
    assert abs(got["mean"] - ref["mean"]) <= b["mean"], (name, got["mean"], ref["mean"], b["mean"])
    assert b["rms"][0] <= got["rms"] <= b["rms"][1], (name, got["rms"], ref["rms"], b["rms"])
    assert b["sd"][0] <= got["sd"] <= b["sd"][1], (name, got["sd"], ref["sd"], b["sd"])


def _all_three(ib, grid, b):
    """device == checker == numpy on the population `b` that the handle holds; the per-cell record; memory unchanged"""
    before = _mem(ib)
    dev, per_cell = ib.bergs_chksum_device(per_cell=True)
    assert ib.bergs_chksum_device() == dev
    assert _mem(ib) == before
    host, want = ib.bergs_chksum(), numpy_bergs_chksum(grid, b)
    assert dev == host == want, (dev, host, want)
    _check_record("# of bergs/cell", per_cell, R.grd_chksum(grid["desc"], _count_plane(grid, b)))
    return dev


# ---- bergs ----
def test_population_before_and_after_steps():
    grid, p, b = _population(seed=11, n=5000)
    ib = _icebergs(grid, p, len(b["lon"]))
    try:
        ib.upload_bergs(b)
        c = _all_three(ib, grid, b)
        assert c[5] == int((b["alive"] != 0).sum())
        ib.run(3)                                    # rows re-binned, dead rows dropped
        c = _all_three(ib, grid, ib.download_bergs())
        assert c[5] > 0
    finally:
        ib.close()


def _tile(ni=7, nj=5, halo=2, gridres=1000.0):
    """a Cartesian tile whose halo is not the default one"""
    d = T.GridDesc()
    d.isc, d.iec, d.jsc, d.jec = 1, ni, 1, nj
    d.isd, d.ied, d.jsd, d.jed = 1 - halo, ni + halo, 1 - halo, nj + halo
    d.grid_is_latlon, d.grid_is_regular, d.Lx = 0, 1, -1.0
    i, j = S._ij(d)
    one = S.zeros(d) + 1.0
    st = {"lon": gridres * i * one, "lat": gridres * j * one}
    st["lonc"], st["latc"] = st["lon"] - 0.5 * gridres, st["lat"] - 0.5 * gridres
    st["dx"], st["dy"], st["area"] = one * gridres, one * gridres, one * gridres * gridres
    st["msk"], st["cos"], st["sin"], st["ocean_depth"] = one.copy(), one.copy(), S.zeros(d), one * 1000.0
    return {"desc": d, "static": st, "forcing": {k: S.zeros(d) for k in T.FORCING_NAMES}}


# (ine, jne, alive, start_year, start_day, start_mass, start_lon, start_lat): the hand-made population, in row order.
# Traversal: cell (1,1) holds rows 3, 0, 2 in that order (row 3 by its year; rows 0 and 2 differ in the sign of a zero start_lon
# only, which `<` does not see: the row decides), cell (2,1) row 4, cell (3,1) rows 6, 7 (equal in all five keys).  Counts
# [3, 1, 2, 0, ...]: rank 2 of the first cell (row 2) and both bergs of the third are what fld still holds at the end.
_HAND = [(1, 1, 1, 1, 10.0, 1.0e8, 0.0, -60.0),
         (1, 1, 0, 0, 1.0, 1.0e8, 5.0, -60.0),      # dead
         (1, 1, 1, 1, 10.0, 1.0e8, -0.0, -60.0),
         (1, 1, 1, 0, 300.0, 3.0e8, 7.0, -61.0),
         (2, 1, 1, 2, 20.0, 2.0e8, 8.0, -62.0),
         (0, 1, 1, 0, 2.0, 1.0e8, 1.0, -60.0),      # live, in the halo
         (3, 1, 1, 1, 30.0, 4.0e8, 9.0, -63.0),
         (3, 1, 1, 1, 30.0, 4.0e8, 9.0, -63.0),
         (8, 6, 1, 0, 3.0, 1.0e8, 2.0, -60.0),      # live, beyond the other corner
         (3, 1, 0, 1, 30.0, 4.0e8, 9.0, -63.0)]     # dead
_LAST = (7, 5, 1, 3, 40.0, 5.0e8, 11.0, -64.0)      # (iec, jec)


def _hand_population(rows):
    n = len(rows)
    rng = np.random.default_rng(3)
    b = S.empty_bergs(n)
    for name in ("lon", "lat", "uvel", "vvel", "thickness", "width", "length", "axn", "ayn", "bxn", "byn", "uvel_old", "vvel_old", "lon_old", "lat_old"):
        b[name][:] = rng.normal(0.0, 100.0, n)
    b["mass"][:] = rng.uniform(1.0e6, 1.0e9, n)
    b["id"][:] = (rng.integers(1, 1 << 20, n).astype(np.int64) << 32) + rng.integers(1, 70000, n)
    for k, r in enumerate(rows):
        b["ine"][k], b["jne"][k], b["alive"][k], b["start_year"][k] = r[0], r[1], r[2], r[3]
        b["start_day"][k], b["start_mass"][k], b["start_lon"][k], b["start_lat"][k] = r[4], r[5], r[6], r[7]
    return b


def _perturbed(b, k):
    c = S.copy_bergs(b)
    c["uvel"][k] = np.nextafter(c["uvel"][k], np.inf)      # a member of fld that is neither a sort key nor part of a hash; the last
    return c                                                  # bit, because the printed integers are the LOW words of the sums


def _ties_swapped(b):
    """the bergs that are equal in all five keys, in the other row order: rows 6 and 7 (ranks 0 and 1: weights 1 and 2, and a
    factor 2 leaves the low word of a bit pattern alone) and rows 0 and 2 (ranks 1 and 2 of the first cell, of which only rank 2
    is kept: here the row order decides the integers)"""
    c = S.copy_bergs(b)
    for name in c:
        c[name][[6, 7, 0, 2]] = c[name][[7, 6, 2, 0]]
    return c


def test_hand_made_population_on_a_tile():
    grid, p = _tile(), S.default_params()
    base = _hand_population(_HAND)
    want = numpy_bergs_chksum(grid, base)
    assert want[5] == 6 and want[4] == 0 and want[2] == want[3]
    # which bergs the integers depend on, from the restatement alone: rows 2, 6, 7
    kept = [k for k in range(len(_HAND)) if numpy_bergs_chksum(grid, _perturbed(base, k))[:2] != want[:2]]
    assert kept == [2, 6, 7], kept
    pops = {"base": base, "last cell occupied": _hand_population(_HAND + [_LAST])}
    ties = _ties_swapped(base)
    pops["ties swapped"] = ties
    zeros = S.copy_bergs(base)                      # -0.0 in the earlier row
    zeros["start_lon"][0], zeros["start_lon"][2] = -0.0, 0.0
    pops["zeros swapped"] = zeros
    assert numpy_bergs_chksum(grid, ties) != want and numpy_bergs_chksum(grid, pops["last cell occupied"])[4] != 0
    assert numpy_bergs_chksum(grid, zeros) == want   # rows 0 and 2 keep their places: the sign of the zero is not a key
    ib = _icebergs(grid, p, 16)
    try:
        for name, b in pops.items():
            ib.upload_bergs(b)
            _all_three(ib, grid, b)
        for k in range(len(_HAND)):                 # the same dependence on the device
            ib.upload_bergs(_perturbed(base, k))
            got = ib.bergs_chksum_device()
            assert (got[:2] != want[:2]) == (k in kept), (k, got, want)
            assert got == numpy_bergs_chksum(grid, _perturbed(base, k))
    finally:
        ib.close()


def test_one_cell_holding_300_bergs():
    """ranks 0 .. 299 of one cell cross waves and blocks; a later cell of two bergs leaves ranks 2 .. 299 in fld"""
    grid, p = _tile(), S.default_params()
    rng = np.random.default_rng(5)
    rows = [(2, 2, 1, int(rng.integers(0, 3)), float(rng.uniform(0, 300)), 1.0e8, 4.0, -60.0) for _ in range(300)]
    rows += [(5, 4, 1, 0, 1.0, 1.0e8, 4.0, -60.0), (5, 4, 1, 0, 2.0, 1.0e8, 4.0, -60.0)]
    b = _hand_population([rows[k] for k in rng.permutation(len(rows))])
    ib = _icebergs(grid, p, 512)
    try:
        ib.upload_bergs(b)
        c = _all_three(ib, grid, b)
        assert c[5] == 302
    finally:
        ib.close()


def test_no_bergs():
    grid, p = _tile(), S.default_params()
    ib = _icebergs(grid, p, 8)
    try:
        assert _all_three(ib, grid, S.empty_bergs(0)) == (0, 0, 0, 0, 0, 0)
    finally:
        ib.close()


def test_bonded_elements_with_bond_tables_resident():
    grid, p, b, bd = S.config_c4(reference_pattern=True)
    ib = _icebergs(grid, p, len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(bd)
        c = _all_three(ib, grid, b)
        assert c[5] == 69 and c[2] == c[3]
    finally:
        ib.close()


def test_halo_rows_are_refused():
    import halo_bergs as HB
    from icebergs_amd.lib import KidError
    whole, b = HB.population()
    p = HB.params(False)
    west, east = _icebergs(HB.tile_grid(0, 0, whole), p, 400), _icebergs(HB.tile_grid(1, 0, whole), p, 400)
    try:
        west.upload_bergs(HB.trim(HB.split_bergs(b, 0, 0, 400)))
        east.upload_bergs(HB.trim(HB.split_bergs(b, 1, 0, 400)))
        _, to_west = east.pack_halo_bergs_pair(0, 0, (False, True))
        west.unpack_immigrants_pair(np.empty((0, 34)), to_west)
        messages = []
        for call in (west.bergs_chksum, west.bergs_chksum_device):
            with pytest.raises(KidError, match="rc=-1 .*halo rows") as e:
                call()
            messages.append(str(e.value))
        assert "kid_bergs_chksum_device: " in messages[1]
        assert messages[1].replace("kid_bergs_chksum_device", "kid_bergs_chksum") == messages[0]
    finally:
        west.close()
        east.close()


# ---- gridded fields ----
_ACC = {"mass": "mass", "mass_on_ocean": "mass_on_ocean", "area_on_ocean": "area_on_ocean", "Uvel_on_ocean": "uvel_on_ocean", "Vvel_on_ocean": "vvel_on_ocean",
        "melt_b": "melt_buoy", "melt_e": "melt_eros", "melt_v": "melt_conv", "bergy_src": "bergy_src", "bergy_melt": "bergy_melt", "bergy_mass": "bergy_mass",
        "fl_bits_src": "fl_bits_src", "fl_bits_melt": "fl_bits_melt", "fl_bits_mass": "fl_bits_mass", "fl_bergy_bits_mass": "fl_bergy_bits_mass",
        "u_iceberg": "u_iceberg", "v_iceberg": "v_iceberg", "varea": "virtual_area", "floating_melt": "floating_melt", "berg_melt": "berg_melt",
        "melt_by_class": "melt_by_class", "melt_b_fl": "melt_buoy_fl", "melt_e_fl": "melt_eros_fl", "melt_v_fl": "melt_conv_fl",
        "fl_parent_melt": "fl_parent_melt", "fl_child_melt": "fl_child_melt"}
_NK = {"mass_on_ocean": 9, "area_on_ocean": 9, "Uvel_on_ocean": 9, "Vvel_on_ocean": 9, "melt_by_class": 10}
_CALV = ("calving", "calving_hflx", "stored_ice", "rmean_calving", "rmean_calving_hflx", "stored_heat")
_DIAG_ONLY = ("mass", "u_iceberg", "v_iceberg", "varea", "melt_b", "melt_e", "melt_v", "melt_b_fl", "melt_e_fl", "melt_v_fl", "fl_parent_melt",
              "fl_child_melt", "melt_by_class")
_FOOTPRINT = ("area_on_ocean", "Uvel_on_ocean", "Vvel_on_ocean")


def _reference_planes(ib, grid, calving):
    """{label: the plane kid_get_forcing / kid_get_calving* / kid_get_accumulators returns or the static grid, None if not held}"""
    planes = dict(ib.get_forcing())
    cs = ib.get_calving_state() if calving else {}
    for name in _CALV:
        planes[name] = cs.get(name)
    acc, out, _ = (a.copy() for a in ib.fetch())
    for label, name in _ACC.items():
        k = T.ACC_NAMES[name]
        planes[label] = acc[k:k + _NK[label]] if label in _NK else acc[k]
    for name, k in T.OUT_NAMES.items():
        planes[name] = out[k]
    for name in T.GRID_STATIC_NAMES:
        planes["depth" if name == "ocean_depth" else name] = grid["static"][name]
    assert sorted(planes) == sorted(T.CHK_LABELS)
    return planes


def _bits(recs):
    return [(n, r["chksum"], r["chksum2"], r["present"]) + tuple(struct.pack("<5d", r["minv"], r["maxv"], r["mean"], r["rms"], r["sd"])) for n, r in recs.items()]


def _check_gridded(ib, grid, calving):
    before = _mem(ib)
    recs = ib.checksum_gridded()
    assert _mem(ib) == before
    assert _bits(ib.checksum_gridded()) == _bits(recs)          # a tree of fixed shape: the same bits twice
    assert list(recs) == T.CHK_LABELS
    planes = _reference_planes(ib, grid, calving)
    refs = {}
    for name in T.CHK_LABELS:
        refs[name] = R.absent() if planes[name] is None else R.grd_chksum(grid["desc"], planes[name])
        if planes[name] is not None:
            assert (np.ndim(planes[name]) == 3) == (name in T.CHK_3D), name
        _check_record(name, recs[name], refs[name])
    return recs, refs


def test_checksum_gridded_with_diagnostics_and_calving():
    grid, p, b = S.config_c2(n=3000, seed=4)
    S.set_diag_all(p)
    ib = _icebergs(grid, p, 200000)
    try:
        ib.set_calving_params(S.calving_params(p))
        ib.upload_bergs(b)
        calv, hflx = S.coupler_calving(grid, seed=1, dt=p.dt)
        for _ in range(3):
            ib.calving(calv, hflx)
            ib.run(1)
        recs, _ = _check_gridded(ib, grid, calving=True)
        assert all(r["present"] == 1 for r in recs.values())
        for name in ("stored_ice", "mass_on_ocean", "area_on_ocean", "Uvel_on_ocean", "melt_by_class", "mass", "spread_mass", "berg_melt", "uo", "sst", "calving", "lon", "area"):
            assert recs[name]["rms"] > 0.0, name              # the planes the check is about hold something
        six, per_cell = ib.bergs_chksum_device(per_cell=True)
        got = ib.download_bergs()
        assert six == numpy_bergs_chksum(grid, got) and six[5] > 3000      # calved bergs among them
        _check_record("# of bergs/cell", per_cell, R.grd_chksum(grid["desc"], _count_plane(grid, got)))
        lines = ib.checksum_report("top of s/r run")
        assert len(lines) == 3 + 59 and lines[2] == "KID: checksumming gridded data @ top of s/r run"
        assert lines[0].startswith("KID, bergs_chksum: " + "top of s/r run".rjust(18) + " chksum=") and lines[0].endswith(" #=" + str(six[5]).rjust(22))
        assert lines[1].startswith("KID, grd_chksum2: " + "# of bergs/cell".rjust(18) + " chksum=")
        assert lines[3 + T.ENUMS["KID_CHK_STORED_ICE"]].startswith("KID, grd_chksum3: " + "stored_ice".rjust(18) + " chksum=")
    finally:
        ib.close()


def test_checksum_gridded_without_diagnostics_and_calving():
    grid, p, b = S.config_c2(n=3000, seed=4)
    p.diag_mask = 0
    ib = _icebergs(grid, p, len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.run(3)
        recs, _ = _check_gridded(ib, grid, calving=False)
        zero = dict(R.absent(), present=1)
        for name in _CALV:
            assert recs[name] == R.absent(), name             # calving was never configured
        for name in _DIAG_ONLY + (() if p.pass_fields_to_ocean_model else _FOOTPRINT):
            assert recs[name] == zero, (name, recs[name])     # a plane nobody fills reads as zeros
        assert recs["mass_on_ocean"]["rms"] > 0.0 and recs["floating_melt"]["present"] == 1
        assert len(ib.checksum_report("end of s/r run")) == 3 + 59 - len(_CALV)
    finally:
        ib.close()


def test_checksum_gridded_static_planes_with_halo_values_and_a_negative_zero():
    """a tile smaller than one block of the sweep, planes whose halo is not zero (only the computational domain may count) and
    a -0.0 inside the domain: its bit pattern is the sign bit alone, it is the minimum's equal and adds nothing to the sums"""
    grid, p = _tile(), S.default_params()
    st = grid["static"]
    rng = np.random.default_rng(9)
    d = grid["desc"]
    for name in ("sin", "cos", "msk"):
        st[name][:] = rng.normal(0.0, 1.0, st[name].shape) if name != "msk" else 7.0
    comp = (slice(d.jsc - d.jsd, d.jec - d.jsd + 1), slice(d.isc - d.isd, d.iec - d.isd + 1))
    st["msk"][comp] = 1.0
    st["sin"][comp] = np.abs(st["sin"][comp])
    st["sin"][3, 4] = -0.0
    ib = _icebergs(grid, p, 8)
    try:
        recs, refs = _check_gridded(ib, grid, calving=False)
        assert recs["msk"]["mean"] == 1.0 and recs["msk"]["sd"] == 0.0 and recs["msk"]["minv"] == recs["msk"]["maxv"] == 1.0
        assert recs["sin"]["minv"] == 0.0 and refs["sin"]["minv"] == 0.0
        assert recs["cos"]["chksum"] != 0 and recs["cos"]["chksum2"] != recs["cos"]["chksum"]      # (whole multiples of 1000 m, as lon, have empty low words)
    finally:
        ib.close()
