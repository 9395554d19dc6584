"""kid_initialize_bonds / kid_count_bonds: the bonded tail of icebergs_init (initialize_iceberg_bonds IB:356-441, form_a_bond
FW:4818-4883, count_bonds FW:5172-5285, assign_n_bonds FW:4617-4637) formed on the device.

What the comparisons are against: the host-built tables of icebergs_amd/reference_tests.py (a Python double loop over all
pairs) for the reference's own populations, a numpy all-pairs restatement of IB:413-431 written here for the lat-lon cases,
and the upload path (kid_upload_bonds) for the state a step starts from.  Everything is exact: bond tables are integers, and
the lat-lon generator asserts on the CPU that no pair lies within a relative 1e-6 of its threshold, far outside what the last
bits of cos() could move.
"""
import re

import numpy as np
import pytest

from icebergs_amd import lib as L
from icebergs_amd import reference_tests as RT
from icebergs_amd import synthetic as S
from icebergs_amd import types as T

pytestmark = pytest.mark.gpu


def _handle(grid, p, n):
    from icebergs_amd.framework import Icebergs
    return Icebergs(grid, p, capacity=max(n, 1))


def _as_icebergs_init_sees_them(case):
    """The bergs of a reference_tests case at the point where icebergs_init forms the bonds (IB:153-171): no bond counts
    yet, and start_lon / start_lat still the restart file's zeros -- dem_tests_init (IB:173, FW:4687-4710) stamps them after
    the bonds exist, so the traversal that formed the host table saw equal `inorder` keys, i.e. row order."""
    b = S.copy_bergs(case["bergs"])
    b["n_bonds"][:] = 0
    b["start_lon"][:] = 0.0
    b["start_lat"][:] = 0.0
    return b


def _lists(bd, n):
    return [[int(bd["other_id"][s * n + k]) for s in range(int(bd["count"][k]))] for k in range(n)]


def _assert_new_bond_members_zero(bd, n):
    assert not bd["broken"].any()
    for name in T.BOND_F64_NAMES:
        assert not bd[name].any(), name


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = {"ss": lambda: RT.dem_beam("ss"), "c": lambda: RT.dem_beam("c"), "collision": lambda: RT.collision("MTS_KID"),
                        "ground_frac": RT.dem_ground_frac}[name]()
    return _CASES[name]


# ---- 1. the reference's own populations --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nelem,length", [("ss", 29, None), ("c", 90, None), ("collision", 16, 800.0), ("ground_frac", 69, None)])
def test_reference_populations(name, nelem, length):
    case = _case(name)
    want = case["bonds"]
    b = _as_icebergs_init_sees_them(case)
    n = len(b["lon"])
    assert n == nelem
    mb = int(case["params"].max_bonds)
    ib = _handle(case["grid"], case["params"], n)
    try:
        ib.upload_bergs(b)
        nformed = ib.initialize_bonds(from_radii=length is None, length=length)
        got = ib.download_bonds(mb)
        gb = ib.download_bergs()
        nbonds, unmatched = ib.count_bonds()
    finally:
        ib.close()
    print(name, "formed", nformed, "count_bonds", nbonds, unmatched)
    assert np.array_equal(got["count"], want["count"])
    assert _lists(got, n) == _lists(want, n)                     # other_id, slot by slot
    assert np.array_equal(gb["n_bonds"], case["bergs"]["n_bonds"])
    _assert_new_bond_members_zero(got, n)
    assert nformed == int(want["count"].sum()) > 0
    assert unmatched == 0
    d = case["grid"]["desc"]
    on_c = (b["ine"] >= d.isc) & (b["ine"] <= d.iec) & (b["jne"] >= d.jsc) & (b["jne"] <= d.jec)
    assert nbonds == int(want["count"][on_c].sum())


# ---- 2. the state a step starts from is that of the upload path ----------------------------------------------------------------
def test_same_state_as_upload_path():
    grid, p, b, _ = S.config_c4()
    n = len(b["lon"])
    assert n == 55
    mb = int(p.max_bonds)
    a = _handle(grid, p, n)
    bb = _handle(grid, p, n)
    try:
        b0 = S.copy_bergs(b)
        b0["n_bonds"][:] = 0
        a.upload_bergs(b0)
        assert a.initialize_bonds(from_radii=True) > 0
        tab, rows = a.download_bonds(mb), a.download_bergs()
        assert a.count_bonds()[1] == 0
        bb.upload_bergs(rows)
        bb.upload_bonds(tab)
        a.run(3)
        bb.run(3)
        ra, rb = a.download_bergs(), bb.download_bergs()
        ta, tb = a.download_bonds(mb), bb.download_bonds(mb)
    finally:
        a.close()
        bb.close()
    assert tab["count"].sum() > 4 * n
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    for k in ta:
        if k != "max_bonds":
            assert ta[k].tobytes() == tb[k].tobytes(), k
    assert np.abs(ta["length"]).max() > 0.0                       # the Visited block ran (orig_bond_length)


# ---- 3. lat-lon metric, a window wider than a cell ---------------------------------------------------------------------------
REARTH, DLON, DLAT, LAT0 = 6.36e6, 1.0, 0.8, -80.0               # synthetic.latlon_grid (the config_c2 grid)


def _latlon_triples(seed=7):
    """~100 triples; the members of a triple lie ~1.2 local cell widths (or heights) apart along lon, along lat or diagonally;
    triples start 12 columns and 5 rows apart: more than 4 cells between any two of them at every latitude from 10 to 75
    degrees.  Rows in traversal order (cells j outer, i inner; zero `inorder` keys keep ties in row order)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rad = np.pi / 180.0
    lon, lat = [], []
    for jrow, lat_c in enumerate(np.arange(10.0, 75.01, 5.0 * DLAT)):                 # 17 latitudes, 4 degrees apart
        for icol in range(6):                                                        # 6 triples per latitude, 12 degrees apart
            x0, y0 = 30.3 + 12.0 * icol + rng.uniform(0.0, 0.4), lat_c + rng.uniform(0.05, 0.35)
            kind = (jrow + icol) % 3
            f = 1.2 * rng.uniform(0.93, 1.07)
            for m in range(3):
                if kind == 0:
                    lon.append(x0 + f * DLON * m), lat.append(y0 + 0.02 * m)
                elif kind == 1:
                    lon.append(x0 + 0.03 * m), lat.append(y0 + f * DLAT * m * np.cos(lat_c * rad))   # (heights scaled: the metre distance is that of the zonal triples)
                else:
                    lon.append(x0 + f * DLON * m * np.sqrt(0.5)), lat.append(y0 + f * DLAT * m * np.sqrt(0.5) * np.cos(lat_c * rad))
    lon, lat = np.array(lon), np.array(lat)
    n = len(lon)
    b = S.empty_bergs(n)
    b["lon"][:], b["lat"][:] = lon, lat
    b["ine"][:] = np.floor(lon / DLON).astype(np.int32) + 1
    b["jne"][:] = np.floor((lat - LAT0) / DLAT).astype(np.int32) + 1
    b["xi"][:] = lon / DLON - (b["ine"] - 1)
    b["yj"][:] = (lat - LAT0) / DLAT - (b["jne"] - 1)
    b["lon_old"][:], b["lat_old"][:] = lon, lat
    sep = 1.2 * DLON * rad * REARTH * np.cos(lat * rad)                               # nominal separation in metres at the berg
    side = sep                                                                        # radius = sqrt(L W / 4) ~ half the separation: threshold ~ 1.25 separations
    b["length"][:] = side * rng.uniform(0.7, 1.3, n)
    b["width"][:] = side * rng.uniform(0.7, 1.3, n)
    b["thickness"][:] = 200.0
    b["mass"][:] = 850.0 * 200.0 * b["length"] * b["width"]
    b["mass_scaling"][:] = 1.0
    order = np.lexsort((np.arange(n), b["ine"], b["jne"]))
    for k in list(b.keys()):
        b[k] = np.ascontiguousarray(b[k][order])
    return b


def _all_pairs(b, p, length):
    """IB:413-431 for every ordered pair, in numpy; returns (bond matrix, smallest relative distance of a pair from its threshold)"""
    rad = p.pi / 180.0
    lon, lat = b["lon"], b["lat"]
    dlon, dlat = lon[:, None] - lon[None, :], lat[:, None] - lat[None, :]
    lat_ref = 0.5 * (lat[:, None] + lat[None, :])
    dx_dlon = (p.pi / 180.0) * p.Rearth * np.cos(lat_ref * rad)
    dy_dlat = (p.pi / 180.0) * p.Rearth
    rx, ry = dlon * dx_dlon, dlat * dy_dlat
    r = np.sqrt((rx ** 2) + (ry ** 2))
    if length is None:
        rdenom = 1.0 / (2.0 * np.sqrt(3.0)) if p.hexagonal_icebergs else 1.0 / 4.0
        radius = np.sqrt(b["length"] * b["width"] * rdenom)
        thr = 1.25 * (radius[:, None] + radius[None, :])
    else:
        thr = np.full_like(r, length)
    bond = r < thr
    np.fill_diagonal(bond, False)
    margin = np.abs(r - thr) / thr
    np.fill_diagonal(margin, 1.0)
    return bond, float(margin.min())


def _expected_lists(b, bond):
    """a berg's partners in reverse traversal (= reverse row) order: form_a_bond inserts at the head"""
    n = len(b["lon"])
    return [[int(b["id"][o]) for o in range(n - 1, -1, -1) if bond[k, o]] for k in range(n)]


_LATLON = {}


def _latlon_case():
    if not _LATLON:
        grid = S.latlon_grid(Rearth=REARTH)
        _LATLON.update(grid=grid, bergs=_latlon_triples())
    return _LATLON["grid"], _LATLON["bergs"]


@pytest.mark.parametrize("mode", ["length", "radii", "radii_hex"])
def test_latlon_metric_and_wide_window(mode):
    grid, b = _latlon_case()
    n = len(b["lon"])
    assert 280 <= n <= 320
    p = S.default_params()
    assert p.Rearth == REARTH
    p.iceberg_bonds_on, p.interactive_icebergs_on, p.max_bonds = 1, 1, 6
    p.Runge_not_Verlet, p.use_new_predictive_corrective = 0, 1                      # bonded bergs are Verlet only (as in every bonded configuration)
    p.hexagonal_icebergs = 1 if mode == "radii_hex" else 0
    length = 1.5 * DLON * (p.pi / 180.0) * p.Rearth if mode == "length" else None   # 1.5 cell widths at the equator
    # conditions on the input, checked on the CPU before anything is compared
    bond, margin = _all_pairs(b, p, length)
    print(mode, "bond sides", int(bond.sum()), "max partners", int(bond.sum(axis=1).max()), "smallest relative margin %.3e" % margin)
    assert margin > 1.0e-6
    assert bond.sum(axis=1).max() <= p.max_bonds
    assert bond.sum() >= n // 2                                                     # and the case is not empty
    assert np.array_equal(bond, bond.T)
    dij = np.abs(b["ine"][:, None] - b["ine"][None, :])
    assert dij[bond].max() >= 2                                                     # partners more than one cell away: a 3x3 window would miss them
    want = _expected_lists(b, bond)
    ib = _handle(grid, p, n)
    try:
        ib.upload_bergs(b)
        nformed = ib.initialize_bonds(from_radii=length is None, length=length)
        got = ib.download_bonds(6)
        gb = ib.download_bergs()
        nbonds, unmatched = ib.count_bonds()
    finally:
        ib.close()
    assert nformed == int(bond.sum())
    assert _lists(got, n) == want
    assert np.array_equal(gb["n_bonds"], bond.sum(axis=1).astype(np.int32))
    _assert_new_bond_members_zero(got, n)
    assert (nbonds, unmatched) == (int(bond.sum()), 0)


# ---- 4. existing bonds stay behind the new ones; the call is idempotent ------------------------------------------------------
def test_existing_bonds_and_idempotence():
    case = _case("c")
    full = case["bonds"]
    b = _as_icebergs_init_sees_them(case)
    n = len(b["lon"])
    mb = int(case["params"].max_bonds)
    ids = [int(x) for x in b["id"]]
    row_of = {i: k for k, i in enumerate(ids)}
    full_lists = _lists(full, n)
    pairs = sorted({(min(i, o), max(i, o)) for k, i in enumerate(ids) for o in full_lists[k]})
    dropped = set(pairs[1::2])                                                        # every second pair, on both its ends
    kept_lists = [[o for o in full_lists[k] if (min(ids[k], o), max(ids[k], o)) not in dropped] for k in range(n)]
    part = S.empty_bonds(n, mb)
    for k in range(n):
        part["count"][k] = len(kept_lists[k])
        for s, o in enumerate(kept_lists[k]):
            part["other_id"][s * n + k] = o
            part["length"][s * n + k] = 1000.0 + s * n + k                            # something to recognise a moved record by
    b["n_bonds"][:] = part["count"]
    ib = _handle(case["grid"], case["params"], n)
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(part)
        nformed = ib.initialize_bonds(from_radii=True)
        got = ib.download_bonds(mb)
        gb = ib.download_bergs()
        again = ib.initialize_bonds(from_radii=True)
        got2 = ib.download_bonds(mb)
        unmatched = ib.count_bonds()[1]
    finally:
        ib.close()
    assert nformed == 2 * len(dropped) > 0
    got_lists = _lists(got, n)
    for k in range(n):
        assert sorted(got_lists[k]) == sorted(full_lists[k]), k
        new = [o for o in full_lists[k] if o not in kept_lists[k]]
        new.sort(key=lambda o: -row_of[o])                                            # reverse traversal order (rows are in traversal order)
        assert got_lists[k] == new + kept_lists[k], k
        for s, o in enumerate(got_lists[k]):
            was = kept_lists[k].index(o) if o in kept_lists[k] else None
            assert got["length"][s * n + k] == (0.0 if was is None else 1000.0 + was * n + k)
    assert np.array_equal(gb["n_bonds"], full["count"])
    assert unmatched == 0
    assert again == 0
    for k in got:
        if k != "max_bonds":
            assert got[k].tobytes() == got2[k].tobytes(), k


# ---- 5. more partners than max_bonds ---------------------------------------------------------------------------------------------
def test_overflow_is_refused_and_the_handle_stays_usable():
    case = _case("collision")
    grid, p = case["grid"], case["params"]
    assert p.max_bonds == 6
    n = 8
    ang = 2.0 * np.pi * np.arange(n) / n
    b = S.empty_bergs(n)
    b["lon"][:], b["lat"][:] = 5500.0 + 100.0 * np.cos(ang), 5500.0 + 100.0 * np.sin(ang)   # a ring of radius 100 m inside one cell
    b["ine"][:], b["jne"][:] = 6, 6
    b["xi"][:], b["yj"][:] = b["lon"] / 1000.0 - 5, b["lat"] / 1000.0 - 5
    b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"]
    b["length"][:] = b["width"][:] = 50.0
    b["thickness"][:], b["mass"][:], b["mass_scaling"][:] = 100.0, 850.0 * 100.0 * 2500.0, 1.0
    empty = S.empty_bonds(n, 6)
    ib = _handle(grid, p, n)
    try:
        ib.upload_bergs(b)
        ib.upload_bonds(empty)
        with pytest.raises(L.KidError) as e:
            ib.initialize_bonds(from_radii=False, length=800.0)      # the ring's diameter is 200 m: seven partners each
        msg = str(e.value)
        print(msg)
        assert "rc=-4" in msg                                        # KID_ECAPACITY
        assert max(int(x) for x in re.findall(r"\d+", msg.split("rc=-4")[1].split("max_bonds")[0])) == 7
        after = ib.download_bonds(6)
        for k in after:
            if k != "max_bonds":
                assert after[k].tobytes() == empty[k].tobytes(), k
        assert not ib.download_bergs()["n_bonds"].any()
        # chords of the ring: 76.5, 141.4, 184.8, 200 m -- 190 m leaves out the berg opposite
        assert ib.initialize_bonds(from_radii=False, length=190.0) == 6 * n
        got = ib.download_bonds(6)
        assert ib.count_bonds() == (6 * n, 0)
    finally:
        ib.close()
    assert (got["count"] == 6).all()
    lists = _lists(got, n)
    for k in range(n):
        assert lists[k] == [int(b["id"][o]) for o in range(n - 1, -1, -1) if o != k and o != (k + 4) % n]


# ---- 6. refusal ----------------------------------------------------------------------------------------------------------------
def test_needs_iceberg_bonds_on():
    grid, p, b = S.config_c1()
    assert not p.iceberg_bonds_on
    ib = _handle(grid, p, len(b["lon"]))
    try:
        ib.upload_bergs(b)
        with pytest.raises(L.KidError) as e:
            ib.initialize_bonds(from_radii=False, length=1000.0)
        assert "rc=-1" in str(e.value)                               # KID_EINVAL
    finally:
        ib.close()
