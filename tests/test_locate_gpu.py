"""Cells from positions on the device (icebergs_amd/csrc/kid_locate.inc): kid_locate_bergs and kid_read_restart under
kid_set_restart_locate, against the host restatement of find_cell_by_search / find_cell (tests/locate_ref.py, itself held against
the generators' cells in tests/test_locate_cpu.py) and against the oracle library's ko_pos_within_cell / ko_is_point_in_cell.

Cells are compared exactly.  xi, yj are compared to 1e-9, the restart tolerance of DESIGN section 2 (the device divides by a
refined reciprocal, the oracle by the IEEE quotient).  Where two handles run the same device routine on the same inputs --
the restart read with and without the search, the steps after it -- the comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import curvilinear as CV
import locate_ref as LR
from icebergs_amd import lib as L
from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from icebergs_amd.framework import Icebergs

pytestmark = pytest.mark.gpu

MEMBERS = list(T.BERG_F64_NAMES) + list(T.BERG_I32_NAMES) + ["id"]
MODES = {"search": LR.SEARCH, "scan": LR.SCAN}
XIYJ_TOL = 1.0e-9


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _unlocated(b):
    """the population as a host with positions only would upload it: every berg in cell (1, 1), xi = yj = 0"""
    up = S.copy_bergs(b)
    up["ine"][:], up["jne"][:] = 1, 1
    up["xi"][:], up["yj"][:] = 0.0, 0.0
    return up


def _bilinear(grid, ine, jne, xi, yj):
    """lon, lat of (xi, yj) in cell (ine, jne): the map of curvilinear.place_bilinear (FW:7071-7088 without old_bug_bilin)"""
    d, st = grid["desc"], grid["static"]
    jj, ii = jne - d.jsd, ine - d.isd
    out = []
    for name in ("lon", "lat"):
        a = st[name]
        out.append((a[jj, ii] * xi + a[jj, ii - 1] * (1.0 - xi)) * yj + (a[jj - 1, ii] * xi + a[jj - 1, ii - 1] * (1.0 - xi)) * (1.0 - yj))
    return out


# ---- the three grids of the main comparison: built once, their host references computed once ----
def _make_patch(kind):
    grid = CV.patch_grid(kind)
    return grid, CV.patch_params(kind), CV.place_bilinear(grid, 6000, 5)     # 93 waves and a partial one


def _make_c2():
    grid, p, b = S.config_c2(n=2000, seed=3)
    k = np.arange(2000)
    b["lon"][k % 3 == 1] += 360.0
    b["lon"][k % 3 == 2] -= 360.0
    return grid, p, b


_MAKERS = {"patch-latlon": lambda: _make_patch("latlon"), "patch-cartesian": lambda: _make_patch("cartesian"), "c2": _make_c2}
_cases, _refs = {}, {}


def _case(name):
    if name not in _cases:
        grid, p, b = _MAKERS[name]()
        _cases[name] = (grid, p, b, LR.LocateRef(grid, p))
    return _cases[name]


def _reference(name, mode):
    if (name, mode) not in _refs:
        _, _, b, ref = _case(name)
        _refs[(name, mode)] = ref.locate_all(b["lon"], b["lat"], MODES[mode])
    return _refs[(name, mode)]


@pytest.mark.parametrize("name", sorted(_MAKERS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_locate_bergs_matches_the_reference_search(name, mode):
    grid, p, b, _ = _case(name)
    want_i, want_j, want_xi, want_yj, status, branches = _reference(name, mode)
    n = len(b["lon"])
    assert np.all(status == LR.FOUND) and np.array_equal(want_i, b["ine"]) and np.array_equal(want_j, b["jne"])   # the generator's cells
    up = _unlocated(b)
    ib = Icebergs(grid, p, capacity=n)
    try:
        ib.upload_bergs(up)
        counts = ib.locate_bergs(mode)
        got = ib.download_bergs()
    finally:
        ib.close()
    assert counts == {"found": n, "lost": 0, "grounded": 0}
    bad = np.nonzero((got["ine"] != want_i) | (got["jne"] != want_j))[0]
    assert len(bad) == 0, [(int(k), int(got["ine"][k]), int(got["jne"][k]), int(want_i[k]), int(want_j[k]), branches[k]) for k in bad[:10]]
    dxi, dyj = float(np.abs(got["xi"] - want_xi).max()), float(np.abs(got["yj"] - want_yj).max())
    print("%s / %s: max |xi - oracle| %.3e, |yj - oracle| %.3e; branches %s" % (name, mode, dxi, dyj, {br: branches.count(br) for br in sorted(set(branches))}))
    assert dxi <= XIYJ_TOL and dyj <= XIYJ_TOL
    for m in MEMBERS:
        if m not in ("ine", "jne", "xi", "yj"):
            assert _same_bits(got[m], up[m]), m


# ---- drops ----
def _drop_case():
    grid = CV.patch_grid("latlon")
    d, st = grid["desc"], grid["static"]
    i0, i1, j0, j1 = CV.LAND
    st["area"][j0 - d.jsd:j1 + 1 - d.jsd, i0 - d.isd:i1 + 1 - d.isd] = 0.0
    rng = np.random.Generator(np.random.PCG64(11))
    inside = CV.place_bilinear(grid, 200, 12)
    gi, gj = rng.integers(i0, i1 + 1, size=40), rng.integers(j0, j1 + 1, size=40)
    glon, glat = _bilinear(grid, gi, gj, rng.uniform(0.02, 0.98, size=40), rng.uniform(0.02, 0.98, size=40))
    lon, lat = st["lon"], st["lat"]
    olon, olat = [], []
    for k in range(50):          # beyond the computational domain to the west, east, south and north; some in the halo, some off the grid
        jj, ii = int(rng.integers(d.jsc, d.jec + 1)) - d.jsd, int(rng.integers(d.isc, d.iec + 1)) - d.isd
        far = 0.5 + 6.0 * float(rng.uniform())
        if k % 4 == 0:
            olon.append(lon[jj, d.isc - 1 - d.isd] - far * 0.5); olat.append(lat[jj, ii])
        elif k % 4 == 1:
            olon.append(lon[jj, d.iec - d.isd] + far * 0.5); olat.append(lat[jj, ii])
        elif k % 4 == 2:
            olon.append(lon[jj, ii]); olat.append(lat[d.jsc - 1 - d.jsd, ii] - far * 0.3)
        else:
            olon.append(lon[jj, ii]); olat.append(lat[d.jec - d.jsd, ii] + far * 0.3)
    n = 290
    b = S.empty_bergs(n)
    order = rng.permutation(n)       # the three kinds mixed through the rows
    for name in MEMBERS:
        if name in ("lon", "lat", "id", "alive"):
            continue
        b[name][order[:200]] = inside[name]
        b[name][order[200:]] = inside[name][:90]
    b["lon"][order], b["lat"][order] = np.concatenate([inside["lon"], glon, olon]), np.concatenate([inside["lat"], glat, olat])
    kind = np.empty(n, dtype=np.int32)
    kind[order] = np.concatenate([np.full(200, LR.FOUND), np.full(40, LR.GROUNDED), np.full(50, LR.LOST)])
    return grid, CV.patch_params("latlon"), b, kind


@pytest.mark.parametrize("mode", sorted(MODES))
def test_lost_and_grounded_bergs_are_dropped(mode):
    grid, p, b, kind = _drop_case()
    ref = LR.LocateRef(grid, p)
    want_i, want_j, _, _, status, _ = ref.locate_all(b["lon"], b["lat"], MODES[mode])
    assert np.array_equal(status, kind)                  # what the points were built to be
    up = _unlocated(b)
    ib = Icebergs(grid, p, capacity=len(kind))
    try:
        ib.upload_bergs(up)
        counts = ib.locate_bergs(mode)
        assert counts == {"found": 200, "lost": 50, "grounded": 40}
        got = ib.download_bergs()
        assert np.array_equal(got["alive"] != 0, status == LR.FOUND)
        keep = status == LR.FOUND
        assert np.array_equal(got["ine"][keep], want_i[keep]) and np.array_equal(got["jne"][keep], want_j[keep])
        d = grid["desc"]
        assert np.all(got["ine"][~keep] == d.isc) and np.all(got["jne"][~keep] == d.jsc)     # a dead row's cell is put back inside
        assert ib.num_bergs()[1] == 200
        ib.compact()
        assert ib.num_bergs() == (200, 200)
        after = ib.download_bergs()
        assert np.array_equal(after["id"], b["id"][keep])                                      # the survivors, in file order
        assert np.array_equal(after["ine"], want_i[keep]) and np.array_equal(after["jne"], want_j[keep])
        again = ib.locate_bergs(mode)                                                          # and they are found again
        assert again == {"found": 200, "lost": 0, "grounded": 0}
    finally:
        ib.close()


# ---- points on corners and edges ----
def _edge_points(grid, n_each=(100, 50, 50)):
    d, st = grid["desc"], grid["static"]
    lon, lat = st["lon"], st["lat"]
    rng = np.random.Generator(np.random.PCG64(21))
    xs, ys = [], []
    while len(xs) < n_each[0]:            # corners
        i, j = int(rng.integers(6, 44)), int(rng.integers(6, 36))
        xs.append(lon[j - d.jsd, i - d.isd]); ys.append(lat[j - d.jsd, i - d.isd])
    while len(xs) < n_each[0] + n_each[1]:   # on a west / east edge that runs along a meridian: lon copied, lat between its two corners
        i, j = int(rng.integers(6, 44)), int(rng.integers(6, 36))
        if lon[j - d.jsd, i - d.isd] == lon[j + 1 - d.jsd, i - d.isd]:
            xs.append(lon[j - d.jsd, i - d.isd]); ys.append(0.5 * (lat[j - d.jsd, i - d.isd] + lat[j + 1 - d.jsd, i - d.isd]))
    while len(xs) < sum(n_each):          # on a south / north edge that runs along a parallel
        i, j = int(rng.integers(6, 44)), int(rng.integers(6, 36))
        if lat[j - d.jsd, i - d.isd] == lat[j - d.jsd, i + 1 - d.isd]:
            xs.append(0.5 * (lon[j - d.jsd, i - d.isd] + lon[j - d.jsd, i + 1 - d.isd])); ys.append(lat[j - d.jsd, i - d.isd])
    return np.array(xs), np.array(ys)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_points_on_corners_and_edges(mode):
    """mode 2: the scan order decides the cell, so it equals the reference's exactly.  mode 1: the walk is the same expression and
    every cell is expected to agree, but on an edge a difference of one ulp in dcost may legitimately pick the other cell that
    holds the point: the cell must hold the point (ko_is_point_in_cell); how many equal the reference's is printed."""
    grid, p, _, ref = _case("patch-latlon")
    x, y = _edge_points(grid)
    n = len(x)
    b = CV.place_bilinear(grid, n, 23)
    b["lon"][:], b["lat"][:] = x, y
    want_i, want_j, _, _, status, _ = ref.locate_all(x, y, MODES[mode])
    ib = Icebergs(grid, p, capacity=n)
    try:
        ib.upload_bergs(_unlocated(b))
        counts = ib.locate_bergs(mode)
        got = ib.download_bergs()
    finally:
        ib.close()
    live = got["alive"] != 0
    same = int(((got["ine"] == want_i) & (got["jne"] == want_j) & live & (status == LR.FOUND)).sum())
    print("edge points / %s: found %d (reference %d) of %d, %d in the reference's cell" % (mode, counts["found"], int((status == LR.FOUND).sum()), n, same))
    assert counts["found"] == int(live.sum()) and counts["grounded"] == 0
    for k in np.nonzero(live)[0]:
        assert ref.in_cell(x[k], y[k], got["ine"][k], got["jne"][k]), (k, x[k], y[k])
    if mode == "scan":
        assert np.array_equal(live, status == LR.FOUND)
        assert np.array_equal(got["ine"][live], want_i[live]) and np.array_equal(got["jne"][live], want_j[live])


# ---- kid_read_restart with kid_set_restart_locate ----
def _write(path, p, b):
    lib = L.load()
    assert lib.kid_restart_write_bergs(str(path / "icebergs.res.nc").encode(), C.byref(p), C.byref(Icebergs._soa(b))) == 0


def _garbage(b):
    """the indices of a file from somewhere else: (1, 1), a cell of this grid that holds none of the bergs, and (-5, 10000)"""
    g = S.copy_bergs(b)
    k = np.arange(len(b["lon"]))
    g["ine"][:] = np.where(k % 2 == 0, 1, -5)
    g["jne"][:] = np.where(k % 2 == 0, 1, 10000)
    return g


def _memory():
    dev, pin = C.c_int64(), C.c_int64()
    assert L.load().kid_memory_in_use(C.byref(dev), C.byref(pin)) == 0
    return dev.value, pin.value


def test_restart_with_garbage_indices_equals_restart_with_true_ones(tmp_path):
    """Two files from one host SoA of 3000 bergs: the true cells, and garbage.  Handle A reads the first as always, handle B the
    second with the search (mode 1, then mode 2): every member B holds equals A's bit for bit -- both run pos_within_cell<false>
    on the same lon, lat, cell.  Without the mode the garbage is trusted: the (-5, 10000) half is not on the grid and the (1, 1)
    half comes back in cell (1, 1), so not one berg is where it belongs.  The temporary blocks are gone on return."""
    grid, p = CV.patch_grid("latlon"), CV.patch_params("latlon")
    b = CV.place_bilinear(grid, 3000, 31)
    rng = np.random.default_rng(5)
    for name in ("uvel", "vvel", "heat_density", "mass_of_bits"):
        b[name][:] = rng.normal(0.0, 1.0, 3000)
    true_dir, junk_dir = tmp_path / "true", tmp_path / "junk"
    true_dir.mkdir(), junk_dir.mkdir()
    _write(true_dir, p, b)
    _write(junk_dir, p, _garbage(b))
    A, B = Icebergs(grid, p, capacity=3000), Icebergs(grid, p, capacity=3000)
    try:
        m0 = _memory()
        A.read_restart(true_dir)
        m1 = _memory()
        want = A.download_bergs()
        assert len(want["id"]) == 3000 and np.array_equal(want["ine"], b["ine"]) and np.array_equal(want["jne"], b["jne"])
        B.read_restart(junk_dir)                                  # the parent commit's behaviour, and today's default
        naive = B.download_bergs()
        assert len(naive["id"]) == 1500 and np.all(naive["ine"] == 1) and np.all(naive["jne"] == 1)
        assert not np.any((b["ine"] == 1) & (b["jne"] == 1))
        deltas = []
        for mode in ("search", "scan"):
            B.set_restart_locate(mode)
            m2 = _memory()
            B.read_restart(junk_dir)
            deltas.append(tuple(x - y for x, y in zip(_memory(), m2)))
            got = B.download_bergs()
            for m in MEMBERS:
                assert _same_bits(got[m], want[m]), (mode, m)
        print("memory in use: plain read %+d / %+d bytes, located reads %s" % (m1[0] - m0[0], m1[1] - m0[1], deltas))
        assert deltas == [(0, 0), (0, 0)]
        B.set_restart_locate(None)                                # and back: bit for bit what it was
        B.read_restart(junk_dir)
        back = B.download_bergs()
        for m in MEMBERS:
            assert _same_bits(back[m], naive[m]), m
    finally:
        A.close()
        B.close()


def test_restart_of_a_legacy_id_file(tmp_path):
    """every id 0: replace_iceberg_num (IO2:743, 917-918) hands out ids from the per-cell counters in file order, before the
    grounded filter; the cells the counters are taken from are the searched ones, so ids and counters equal the plain read's"""
    grid, p = CV.patch_grid("latlon"), CV.patch_params("latlon")
    b = CV.place_bilinear(grid, 500, 41)
    b["id"][:] = 0
    true_dir, junk_dir = tmp_path / "true", tmp_path / "junk"
    true_dir.mkdir(), junk_dir.mkdir()
    _write(true_dir, p, b)
    _write(junk_dir, p, _garbage(b))
    A, B = Icebergs(grid, p, capacity=500), Icebergs(grid, p, capacity=500)
    try:
        A.read_restart(true_dir)
        B.set_restart_locate("search")
        B.read_restart(junk_dir)
        want, got = A.download_bergs(), B.download_bergs()
        assert len(np.unique(want["id"])) == 500 and np.all(want["id"] != 0)
        for m in MEMBERS:
            assert _same_bits(got[m], want[m]), m
        assert np.array_equal(A.get_iceberg_counter(), B.get_iceberg_counter()) and A.get_iceberg_counter().sum() == 500
    finally:
        A.close()
        B.close()


def test_two_tiles_read_one_global_file(tmp_path):
    """the undivided grid of tests/test_migration_cpu.py and its two tiles, one after the other on the same device: each tile keeps
    the bergs of its own columns out of a global file whose indices mean nothing, the two sets are disjoint, their union is what the
    undivided handle keeps"""
    from test_migration_cpu import NI, NJ, _grid
    whole = _grid(None, 2)
    p = S.default_params()
    b = S.place_bergs(whole, 400, 51, (1, 2 * NI), (1, NJ))
    b["id"][:] = (np.int64(7) << 32) + np.arange(1, 401)
    _write(tmp_path, p, _garbage(b))
    kept = {}
    for tx in (None, 0, 1):
        ib = Icebergs(whole if tx is None else _grid(tx, 2), p, capacity=400)
        try:
            ib.set_restart_locate("search")
            ib.read_restart(tmp_path)
            kept[tx] = ib.download_bergs()
        finally:
            ib.close()
    by_id = {int(i): k for k, i in enumerate(b["id"])}
    assert set(kept[None]["id"]) == set(b["id"])
    for tx in (0, 1):
        rows = np.array([by_id[int(i)] for i in kept[tx]["id"]], dtype=np.int64)
        assert len(rows) > 100
        assert np.all((b["ine"][rows] > tx * NI) & (b["ine"][rows] <= (tx + 1) * NI))          # its own columns, all of them
        assert len(rows) == int(((b["ine"] > tx * NI) & (b["ine"] <= (tx + 1) * NI)).sum())
        assert np.array_equal(kept[tx]["ine"], b["ine"][rows] - tx * NI) and np.array_equal(kept[tx]["jne"], b["jne"][rows])
        assert np.all(np.diff(rows) > 0)                                                         # file order
    assert not set(kept[0]["id"]) & set(kept[1]["id"])
    assert set(kept[0]["id"]) | set(kept[1]["id"]) == set(kept[None]["id"])


# ---- refusals ----
def test_refusals_write_nothing():
    import halo_bergs as HB
    grid, p, b, _ = _case("patch-latlon")
    small = {k: (v[:64].copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    up = _unlocated(small)
    ib = Icebergs(grid, p, capacity=64)
    try:
        ib.upload_bergs(up)
        cnt = (C.c_int64 * 3)(-7, -7, -7)
        for mode in (0, 3, -1):
            assert ib.lib.kid_locate_bergs(ib.h, mode, cnt) == -1 and b"mode" in ib.lib.kid_last_error(ib.h)
            assert ib.lib.kid_set_restart_locate(ib.h, mode if mode else 3) == -1
        with pytest.raises(ValueError):
            ib.locate_bergs("fast")
        bd = S.empty_bonds(64, 2)
        bd["count"][1] = bd["count"][2] = 1
        bd["other_id"][1], bd["other_id"][2] = up["id"][2], up["id"][1]
        ib.upload_bonds(bd)
        with pytest.raises(L.KidError, match=r"rc=-5 .*bonds keep their rows"):
            ib.locate_bergs("search")
        assert list(cnt) == [-7, -7, -7]
        got = ib.download_bergs()
        for m in MEMBERS:
            assert _same_bits(got[m], up[m]), m
    finally:
        ib.close()
    # halo rows resident: the copies a neighbour packed, between the unpack and the evolve that retires them
    whole, pop = HB.population()
    hp = HB.params(False)
    west, east = Icebergs(HB.tile_grid(0, 0, whole), hp, capacity=400), Icebergs(HB.tile_grid(1, 0, whole), hp, capacity=400)
    try:
        west.upload_bergs(HB.trim(HB.split_bergs(pop, 0, 0, 400)))
        east.upload_bergs(HB.trim(HB.split_bergs(pop, 1, 0, 400)))
        _, to_west = east.pack_halo_bergs_pair(0, 0, (False, True))
        west.unpack_immigrants_pair(np.zeros((0, 34)), to_west)
        assert west.halo_berg_count() == len(to_west) > 0
        before = west.download_bergs()
        with pytest.raises(L.KidError, match=r"rc=-1 .*halo rows are resident"):
            west.locate_bergs("scan")
        after = west.download_bergs()
        for m in MEMBERS:
            assert _same_bits(after[m], before[m]), m
    finally:
        west.close()
        east.close()


# ---- a run goes on from located bergs as from uploaded ones ----
def test_steps_after_locate_equal_steps_after_upload():
    """20 steps of config 2 from bergs that kid_locate_bergs placed, and from the same bergs uploaded with their true cells (and the
    xi, yj the device gives them: a function of lon, lat and the cell, held against the oracle above).  Per berg, bit for bit: the
    rows are the same bergs in both handles and results do not depend on the row order."""
    grid, p, b = S.config_c2(n=2000, seed=9)
    A, B = Icebergs(grid, p, capacity=2000), Icebergs(grid, p, capacity=2000)
    try:
        A.upload_bergs(_unlocated(b))
        assert A.locate_bergs("search") == {"found": 2000, "lost": 0, "grounded": 0}
        placed = A.download_bergs()
        assert np.array_equal(placed["ine"], b["ine"]) and np.array_equal(placed["jne"], b["jne"])
        direct = S.copy_bergs(b)
        direct["xi"][:], direct["yj"][:] = placed["xi"], placed["yj"]
        B.upload_bergs(direct)
        A.run(20)
        B.run(20)
        ga, gb = A.download_bergs(), B.download_bergs()
    finally:
        A.close()
        B.close()
    fa, fb = CV.by_id(ga, MEMBERS[:-1]), CV.by_id(gb, MEMBERS[:-1])
    assert len(fa["id"]) == len(fb["id"]) > 1900
    start = CV.by_id(b, ["lon"])
    assert not np.array_equal(fa["lon"], start["lon"][np.isin(start["id"], fa["id"])])       # they moved
    for m in fa:
        assert _same_bits(fa[m], fb[m]), m
