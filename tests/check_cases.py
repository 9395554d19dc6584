"""Populations with planted offenders for the tests of kid_check_bergs (tests/test_check_cpu.py, tests/test_check_gpu.py): the box of
tests/halo_bergs.py (16 x 12 cells of 5 km, one berg per lattice point, distinct start keys and ids), every 7th row dead, and on
its first 257 rows the duplicates and the position faults the issue lists, each with the number it must give.  The numbers are
worked out here by hand from what is planted, never from a run.  Test infrastructure: never imported by icebergs_amd/."""
import numpy as np

import halo_bergs as HB
from icebergs_amd import synthetic as S

N = 257
SHAPES = (1, 63, 64, 65, 257)
LAND = (2, 2)                                   # the masked cell of box_grid(mask=True): the lattice starts in cell (3, 3)


def box_grid(mask=False):
    g = HB.whole_grid()
    if mask:
        d = g["desc"]
        g["static"]["msk"][LAND[1] - d.jsd, LAND[0] - d.isd] = 0.0
    return g


def box_params(mts=False):
    p = HB.params(False)
    if mts:
        p.mts, p.old_interp_flds_order = 1, 0    # FW:1483: old_interp_flds_order is false whenever mts is on
    return p


def box_bergs(n=N):
    """the first n rows of the box's population in reference order (247 bergs; beyond them a second draw of the same lattice with
    another seed, its ids moved up: other positions, hence other start keys), rows 6, 13, 20, ... dead"""
    _, b = HB.population()
    _, more = HB.population(seed=HB.SEED + 1)
    more["id"] = more["id"] + 100000
    b = {k: np.concatenate([v, more[k]])[:n].copy() for k, v in b.items()}
    assert len(b["id"]) == n and len(np.unique(b["id"])) == n
    b["alive"][6::7] = 0
    return b


def live_rows(b):
    return [int(k) for k in np.nonzero(b["alive"] != 0)[0]]


def cell_centre(i, j):
    return (i - 0.5) * HB.RES, (j - 0.5) * HB.RES


EVERYTHING = None   # copy_row: every member but the id


def copy_row(b, dst, src, fields=EVERYTHING, with_id=False):
    for k, v in b.items():
        if isinstance(v, np.ndarray) and (fields is None or k in fields) and (k != "id" or with_id) and k != "alive":
            v[dst] = v[src]


KEYS = ("start_year", "start_day", "start_mass", "start_lon", "start_lat")


def plant_duplicates(b, d):
    """plants on the 257-row box (in place) and returns the numbers they must give.  Rows are taken from the live ones; a planted
    row keeps its id unless said otherwise.
      A   2 rows with equal keys, in different cells                                     1 pair
      B   3 rows with equal keys; the second a copy of the first in every member         3 pairs, 1 identical berg, 1 identical in its cell
      C   65 rows with equal keys on rows of three waves (0..63, 64..127, 128..191), 33 in cell (3, 3) and 32 in (4, 3)
                                                                                         2080 pairs, 32 + 31 identicals
      F   a copy in every member but axn_fast                                            1 pair; an identical berg without mts only
      Z   (-0.0, a), (+0.0, a) in (start_lon, start_lat), same cell, and a row (-0.0, b) 1 pair, 1 identical
      NaN 2 rows with equal keys and a NaN start_mass                                    nothing
      I   2 rows with one id and different keys                                          1 duplicate id
      a dead row, a halo copy (halo_berg = 1, cell iec + 1) and a leaver (halo_berg = 0, cell isc - 1), each repeating a live row's
      keys and id: nothing but '# in halo' = 1 for the leaver"""
    live = live_rows(b)
    dead = [k for k in range(len(b["alive"])) if b["alive"][k] == 0]
    assert len(b["alive"]) == N and len(live) >= 200
    free = list(live)

    def take(pred=lambda k: True):
        k = next(q for q in free if pred(q))
        free.remove(k)
        return k

    # C first: it wants rows of three waves
    c_rows = [take(lambda k, w=w: 64 * w <= k < 64 * (w + 1)) for w in (0, 1, 2) for _ in range(22 if w < 2 else 21)]
    assert len(c_rows) == 65 and len({k // 64 for k in c_rows}) == 3
    for q, k in enumerate(c_rows):
        copy_row(b, k, c_rows[0], KEYS)
        b["ine"][k], b["jne"][k] = (3, 3) if q % 2 == 0 else (4, 3)
    a0, a1 = take(), take(lambda k: k > 200)
    assert (b["ine"][a0], b["jne"][a0]) != (b["ine"][a1], b["jne"][a1])
    copy_row(b, a1, a0, KEYS)
    b0, b1, b2 = take(), take(), take(lambda k: k > 200)
    copy_row(b, b1, b0)
    copy_row(b, b2, b0, KEYS)
    assert (b["ine"][b0], b["jne"][b0]) != (b["ine"][b2], b["jne"][b2])
    f0, f1 = take(), take()
    copy_row(b, f1, f0)
    b["axn_fast"][f0], b["axn_fast"][f1] = 0.25, 0.5
    z0, z1, z2 = take(), take(), take()
    for k in (z1, z2):
        copy_row(b, k, z0, KEYS)
    b["ine"][z1], b["jne"][z1] = b["ine"][z0], b["jne"][z0]
    b["start_lon"][z0], b["start_lon"][z1], b["start_lon"][z2] = -0.0, 0.0, -0.0
    b["start_lat"][z2] = b["start_lat"][z0] + 1.0
    n0, n1 = take(), take()
    copy_row(b, n1, n0, KEYS)
    b["ine"][n1], b["jne"][n1] = b["ine"][n0], b["jne"][n0]
    b["start_mass"][n0] = b["start_mass"][n1] = np.nan
    i0, i1 = take(), take()
    b["id"][i1] = b["id"][i0]
    src = take()
    copy_row(b, dead[3], src, with_id=True)
    halo, leaver = take(), take()
    for k, cell_i, flag in ((halo, d.iec + 1, 1.0), (leaver, d.isc - 1, 0.0)):
        copy_row(b, k, src, KEYS, with_id=True)
        b["id"][k] = b["id"][src]
        b["ine"][k], b["halo_berg"][k] = cell_i, flag
    want = {"n_same_id": 1 + 3 + 2080 + 1 + 1, "n_same_berg": 1 + 1, "n_same_berg_mts": 1, "n_identical": 0 + 1 + (32 + 31) + 1 + 1,
            "n_dup_ids": 1, "n_in_halo": 1,
            "first_same_id": int(min(b["id"][k] for k in c_rows + [a0, a1, b0, b1, b2, f0, f1, z0, z1])), "first_dup_id": int(b["id"][i0]),
            "rows_same_id": sorted(c_rows + [a0, a1, b0, b1, b2, f0, f1, z0, z1]), "rows_dup_id": [i0, i1]}
    return want


# rows of the position plants: the first and last lane of the first wave, the first lane of the second, the last row
XI_ROWS, YJ_ROW, NAN_ROW, LAND_ROW, HALO_ROW = (0, 63, 64, 256), 100, 130, 200, 150


def move_to_cell_centre(b, k, i, j):
    """lon, lat at the centre of cell (i, j) of the box: xi = yj = 0.5 exactly, in the reference's arithmetic and in any other that
    divides 0 by the cell size exactly (FW:6287-6291 on a regular Cartesian grid)"""
    b["lon"][k], b["lat"][k] = cell_centre(i, j)
    b["ine"][k], b["jne"][k] = i, j
    b["xi"][k] = b["yj"][k] = 0.5


def plant_positions(b, d):
    """on a 257-row state whose xi, yj are what pos_within_cell gives (in place): xi one ulp off in XI_ROWS, yj in YJ_ROW, a NaN xi
    in NAN_ROW; LAND_ROW at the centre of the masked cell and HALO_ROW at the centre of a halo cell, both with the xi = yj = 0.5
    that belongs there, so that only n_land and n_in_halo see them.  Returns the numbers they must give."""
    for k in XI_ROWS + (YJ_ROW, NAN_ROW, LAND_ROW, HALO_ROW):
        assert b["alive"][k] != 0
    ulps = []
    for k in XI_ROWS:
        x = b["xi"][k]
        b["xi"][k] = np.nextafter(x, 2.0)
        ulps.append(float(b["xi"][k] - x))
    y = b["yj"][YJ_ROW]
    b["yj"][YJ_ROW] = np.nextafter(y, -2.0)
    b["xi"][NAN_ROW] = np.nan
    move_to_cell_centre(b, LAND_ROW, *LAND)
    move_to_cell_centre(b, HALO_ROW, d.iec + 1, 4)
    b["halo_berg"][HALO_ROW] = 0.0
    return {"n_xiyj": len(XI_ROWS) + 2, "n_land": 1, "n_in_halo": 1, "max_dxi": max(ulps), "max_dyj": float(y - b["yj"][YJ_ROW]),
            "first_xiyj": int(min(b["id"][k] for k in XI_ROWS + (YJ_ROW, NAN_ROW))), "first_land": int(b["id"][LAND_ROW]),
            "rows_xiyj": sorted(XI_ROWS + (YJ_ROW, NAN_ROW)), "rows_land": [LAND_ROW]}


def empty_like(n):
    return S.empty_bergs(n)
