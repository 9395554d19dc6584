"""The reference's debug-mode invariants restated on the host, from the Fortran (icebergs_framework.F90, FW):

    check_position                   FW:6576-6603    count_out_of_order   FW:4039-4089
    check_for_duplicates             FW:4118-4158    sameid  FW:4381      sameberg  FW:4397
    check_for_duplicate_ids_in_list  FW:7382-7452

What tests/test_check_cpu.py and tests/test_check_gpu.py hold kid_check_bergs against.  Bergs are the dicts of numpy arrays of
icebergs_amd.synthetic (one array per member, `alive`, `id`).  The pair loops of FW:4130-4149 are loops here, with sameid and
sameberg by value: Fortran's `.ne.` is numpy's `!=` on float64 -- a NaN differs from everything, -0.0 equals +0.0.  The position
check goes through the oracle's ko_pos_within_cell, as tests/locate_ref.py does.  The cross-PE routine is written as its
definition: the ids seen on more than one rank.

`# identicals` is icnt3 on sorted lists (what the reference prints under parallel_reprod), with equality by value: the number of
bergs that follow, in their cell's list, a berg equal to them in the five start keys.  (The reference's own test there is
inorder(a, b) .and. inorder(b, a), which lets a NaN key pass as equal; kid_check_bergs documents equality by value throughout.)
Test infrastructure: never imported by icebergs_amd/."""
import numpy as np

KEYS = ("start_year", "start_day", "start_mass", "start_lon", "start_lat")                      # FW:4387-4391
MEMBERS = ("lon", "lat", "mass", "uvel", "vvel", "thickness", "width", "length", "axn", "ayn", "bxn", "byn",
           "uvel_old", "vvel_old", "lon_old", "lat_old")                                          # FW:4404-4419
MEMBERS_MTS = ("axn_fast", "ayn_fast", "bxn_fast", "byn_fast")                                    # FW:4422-4425


def nrows(b):
    return len(b["alive"])


def on_domain(b, d):
    """live rows whose cell is on the computational domain: the bergs the reference's loops over list(isc:iec, jsc:jec) visit"""
    return (b["alive"] != 0) & (b["ine"] >= d.isc) & (b["ine"] <= d.iec) & (b["jne"] >= d.jsc) & (b["jne"] <= d.jec)


def sameid(b, k1, k2):
    for f in KEYS:
        if b[f][k1] != b[f][k2]:
            return False
    return True


def sameberg(b, k1, k2, mts=False):
    if not sameid(b, k1, k2):
        return False
    for f in MEMBERS + (MEMBERS_MTS if mts else ()):
        if b[f][k1] != b[f][k2]:
            return False
    return True


def traversal(b, d):
    """the rows in the order of the reference's double loop: cells j outer, i inner; inside a cell in row order (the order inside
    a list changes no count below)"""
    rows = np.nonzero(on_domain(b, d))[0]
    cell = (b["jne"][rows].astype(np.int64) - d.jsc) * (d.iec - d.isc + 1) + (b["ine"][rows] - d.isc)
    return rows[np.argsort(cell, kind="stable")]


def check_for_duplicates(b, d, mts=False):
    """(icnt_id, icnt_same) of FW:4130-4149: every pair of bergs of the computational domain once"""
    order = traversal(b, d)
    icnt_id = icnt_same = 0
    for a in range(len(order)):
        k1 = order[a]
        for c in range(a + 1, len(order)):
            k2 = order[c]
            if sameid(b, k1, k2):
                icnt_id += 1
                if sameberg(b, k1, k2, mts):
                    icnt_same += 1
    return icnt_id, icnt_same


def count_out_of_order(b, d):
    """(icnt2, icnt3): '# in halo' as kid_check_report.n_in_halo defines it (live, halo_berg < 0.5, cell outside the computational
    domain) and '# identicals' on sorted lists"""
    live = b["alive"] != 0
    outside = (b["ine"] < d.isc) | (b["ine"] > d.iec) | (b["jne"] < d.jsc) | (b["jne"] > d.jec)
    icnt2 = int(np.count_nonzero(live & (b["halo_berg"] < 0.5) & outside))
    order = traversal(b, d)
    icnt3 = 0
    start = 0
    while start < len(order):                      # one cell's list at a time
        end = start
        while end < len(order) and b["ine"][order[end]] == b["ine"][order[start]] and b["jne"][order[end]] == b["jne"][order[start]]:
            end += 1
        members = list(order[start:end])
        # in a sorted list bergs with equal keys are neighbours: each one after the first of its kind is counted once
        firsts = []
        for k in members:
            if any(sameid(b, k, f) for f in firsts):
                icnt3 += 1
            else:
                firsts.append(k)
        start = end
    return icnt2, icnt3


def duplicate_ids(ids):
    """FW:7405-7423: sort, count the neighbours that are equal"""
    s = np.sort(np.asarray(ids, dtype=np.int64))
    return int(np.count_nonzero(s[1:] == s[:-1]))


def duplicate_ids_across(lists):
    """FW:7424-7450 as its definition: the ids that more than one rank holds (a rank's own repeats count once)"""
    seen = {}
    for rank, ids in enumerate(lists):
        for v in set(int(x) for x in ids):
            seen.setdefault(v, set()).add(rank)
    return sum(1 for ranks in seen.values() if len(ranks) > 1)


def check_duplicates_parallel(lists):
    """what TileExchange.check_duplicates returns: (duplicates on a rank, summed; ids owned by more than one rank)"""
    return sum(duplicate_ids(ids) for ids in lists), duplicate_ids_across(lists)


class PositionRef:
    """check_position on every live row: the oracle's pos_within_cell against the stored xi, yj; the land mask"""

    def __init__(self, grid, params):
        import locate_ref
        self.loc = locate_ref.LocateRef(grid, params)
        self.d = grid["desc"]
        self.msk = np.asarray(grid["static"]["msk"], dtype=np.float64)

    def recompute(self, b, k):
        d = self.d
        i, j = int(b["ine"][k]), int(b["jne"][k])
        if i - 1 < d.isd or i > d.ied or j - 1 < d.jsd or j > d.jed:       # FW:6251-6262: outside the data domain
            return -999.0, -999.0
        return self.loc.pos_within_cell(b["lon"][k], b["lat"][k], i, j)

    def check(self, b):
        """n_rows, n_xiyj, n_land, max_dxi, max_dyj and the offending rows of both kinds"""
        d = self.d
        out = {"n_rows": 0, "n_xiyj": 0, "n_land": 0, "max_dxi": 0.0, "max_dyj": 0.0, "rows_xiyj": [], "rows_land": []}
        for k in np.nonzero(b["alive"] != 0)[0]:
            out["n_rows"] += 1
            xi, yj = self.recompute(b, k)
            sxi, syj = float(b["xi"][k]), float(b["yj"][k])
            if xi != sxi or yj != syj:
                out["n_xiyj"] += 1
                out["rows_xiyj"].append(int(k))
            for name, a, c in (("max_dxi", sxi, xi), ("max_dyj", syj, yj)):
                if np.isfinite(a) and np.isfinite(c):
                    out[name] = max(out[name], abs(a - c))
            i, j = int(b["ine"][k]), int(b["jne"][k])
            if d.isd <= i <= d.ied and d.jsd <= j <= d.jed and self.msk[j - d.jsd, i - d.isd] == 0.0:
                out["n_land"] += 1
                out["rows_land"].append(int(k))
        return out


def report(b, d, mts=False, position=None):
    """the members of kid_check_report that do not name a row, from the routines above"""
    icnt2, icnt3 = count_out_of_order(b, d)
    icnt_id, icnt_same = check_for_duplicates(b, d, mts)
    r = {"n_in_halo": icnt2, "n_identical": icnt3, "n_same_id": icnt_id, "n_same_berg": icnt_same,
         "n_dup_ids": duplicate_ids(b["id"][on_domain(b, d)])}
    if position is not None:
        p = position.check(b)
        r.update({k: p[k] for k in ("n_rows", "n_xiyj", "n_land", "max_dxi", "max_dyj")})
    return r
