"""Cells from positions without a GPU: the host restatement of find_cell_by_search and find_cell (tests/locate_ref.py), which
the device tests compare kid_locate_bergs with, is itself held against something it did not produce -- the cell every berg
of the generators was placed in through the bilinear map of that cell's corners, strictly inside it (xi, yj in [0.02, 0.98]).
Both modes must return that cell for every berg; that is a condition on the restatement and on the inputs, not a measurement."""
import numpy as np
import pytest

import curvilinear as CV
import locate_ref as LR
from icebergs_amd import synthetic as S


def _patch(kind):
    grid = CV.patch_grid(kind)
    return grid, CV.patch_params(kind), CV.place_bilinear(grid, 600, 5)


def _c2():
    return S.config_c2(n=300, seed=3)


_CASES = {"patch-latlon": lambda: _patch("latlon"), "patch-cartesian": lambda: _patch("cartesian"), "c2": _c2}
_cache = {}


def _case(name):
    """(LocateRef, bergs, {mode: [(found, i, j, branch, moves)]}): each search runs once, the tests share the results"""
    if name not in _cache:
        grid, p, b = _CASES[name]()
        ref = LR.LocateRef(grid, p)
        res = {}
        for mode in (LR.SEARCH, LR.SCAN):
            rows = []
            for x, y in zip(b["lon"], b["lat"]):
                rows.append(ref.locate(x, y, mode) + (ref.moves,))
            res[mode] = rows
        _cache[name] = (ref, b, res)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("mode", [LR.SEARCH, LR.SCAN])
def test_both_modes_return_the_cell_the_berg_was_placed_in(name, mode):
    ref, b, res = _case(name)
    rows = res[mode]
    assert all(r[0] for r in rows), [k for k, r in enumerate(rows) if not r[0]][:10]
    got_i, got_j = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    bad = np.nonzero((got_i != b["ine"]) | (got_j != b["jne"]))[0]
    assert len(bad) == 0, [(int(k), int(got_i[k]), int(got_j[k]), int(b["ine"][k]), int(b["jne"][k])) for k in bad[:10]]
    if mode == LR.SEARCH:
        moves = np.array([r[4] for r in rows if r[3] != LR.CORNER])
        branches = [r[3] for r in rows]
        print("%s: stagnation %d, exhausted %d, walk mean / max moves %.0f / %d" % (name, branches.count(LR.STAGNATION), branches.count(LR.EXHAUSTED),
                                                                                     moves.mean(), moves.max()))


def test_a_patch_latlon_berg_ends_in_the_stagnation_branch():
    """the tall band and the sheared disc bend the cost field enough for the 9-point descent to stall next to the cell: the
    find_better_min / find_cell_loc block (FW:5797-5824) is on the path of the device tests, not only the plain walk"""
    _, _, res = _case("patch-latlon")
    assert sum(r[3] == LR.STAGNATION for r in res[LR.SEARCH]) >= 1


def test_no_input_reaches_the_exhausted_branch():
    """find_cell behind a walk that used all of its (iec - isc) + (jec - jsc) moves (FW:5828): none of these inputs gets there;
    DESIGN 7.3 says so, and this is where to look when that changes"""
    for name in sorted(_CASES):
        _, _, res = _case(name)
        assert not any(r[3] == LR.EXHAUSTED for r in res[LR.SEARCH]), name


@pytest.mark.parametrize("mode", [LR.SEARCH, LR.SCAN])
def test_c2_one_period_east(mode):
    """the same bergs with 360 added to every longitude: dcost, the guess's miss and is_point_in_cell all go through
    apply_modulo_around_point, and the cells are the same"""
    ref, b, _ = _case("c2")
    for k, (x, y) in enumerate(zip(b["lon"] + 360.0, b["lat"])):
        found, i, j, _ = ref.locate(x, y, mode)
        assert found and (i, j) == (int(b["ine"][k]), int(b["jne"][k])), (k, x, y, i, j)


@pytest.mark.parametrize("name", ["patch-latlon", "patch-cartesian"])
@pytest.mark.parametrize("mode", [LR.SEARCH, LR.SCAN])
def test_a_point_outside_the_grid_is_not_found(name, mode):
    ref, _, _ = _case(name)
    d = ref.d
    lon, lat = ref.lon, ref.lat
    west = (lon[20, 0] - 3.0 * (lon[20, 1] - lon[20, 0]), lat[20, 20])
    north = (lon[20, 20], lat[-1, 20] + 3.0 * (lat[-1, 20] - lat[-2, 20]))
    halo = (0.5 * (lon[20, 0] + lon[20, 1]), 0.5 * (lat[20, 0] + lat[21, 0]))     # inside the data domain, outside the computational one
    assert d.isc - d.isd >= 1
    for x, y in (west, north, halo):
        assert ref.locate(x, y, mode)[:3] == (False, -999, -999), (x, y)


@pytest.mark.parametrize("name", ["patch-latlon", "patch-cartesian"])
def test_scan_returns_the_first_containing_cell_on_a_shared_edge(name):
    """a point exactly on a corner or an edge lies in more than one cell for is_point_in_cell on some of these (the crude bounds are
    closed); mode 2 returns the first of them in the order j outer, i inner, the same as a brute-force loop over every cell"""
    ref, _, _ = _case(name)
    d = ref.d
    pts = []
    for (i, j) in ((8, 8), (30, 21), (17, 30), (40, 12), (25, 31)):     # plain, sheared, tall band, plain, sheared + tall
        x, y = float(ref.lon[j - d.jsd, i - d.isd]), float(ref.lat[j - d.jsd, i - d.isd])
        xe, ye = float(ref.lon[j - d.jsd, i + 1 - d.isd]), float(ref.lat[j + 1 - d.jsd, i - d.isd])
        pts += [(x, y), (0.5 * (x + xe), y) if ref.lat[j - d.jsd, i + 1 - d.isd] == y else (x, y), (x, 0.5 * (y + ye)) if ref.lon[j + 1 - d.jsd, i - d.isd] == x else (x, y)]
    shared = 0
    for x, y in pts:
        holds = [(i, j) for j in range(d.jsc, d.jec + 1) for i in range(d.isc, d.iec + 1) if ref.in_cell(x, y, i, j)]
        shared += len(holds) > 1
        found, i, j, _ = ref.locate(x, y, LR.SCAN)
        if holds:
            assert found and (i, j) == holds[0], (x, y, (i, j), holds)
        else:
            assert not found
    print("%s: %d of %d edge points lie in more than one cell" % (name, shared, len(pts)))
