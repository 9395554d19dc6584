"""A berg's cell from its position, restated on the host: what read_restart_bergs does with ignore_ij_restart
(icebergs_fms2io.F90:876-891).  Line references are to icebergs_framework.F90 (FW).

    find_cell_by_search  FW:5710-5842    dcost          FW:5845-5858    find_better_min  FW:5862-5893
    find_cell_loc        FW:5896-5924    find_cell      FW:6011-6041

The point-in-cell test, the in-cell position and the periodic shift are the oracle library's (ko_is_point_in_cell,
ko_pos_within_cell, ko_apply_modulo_around_point), called through oracle_lib.Oracle as tests/test_migration_cpu.py does; the
search itself is plain Python on IEEE doubles, one rounded operation per operator, as the reference's expressions are.
locate() returns the cell and the branch that ended the search.  Test infrastructure: never imported by icebergs_amd/."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
from oracle_lib import Oracle  # noqa: E402

SEARCH, SCAN = 1, 2                      # find_cell_by_search, find_cell (use_slow_find)
FOUND, LOST, GROUNDED = 0, 1, 2          # the status words of kid_locate_bergs
# how a search ended: at the first corner (FW:5749), by a move of the walk (FW:5792), in the stagnation block (FW:5797-5824),
# with the moves used up (find_cell, FW:5828); for find_cell itself: by the structured-grid guess (FW:6025-6031) or the scan
CORNER, WALK, STAGNATION, EXHAUSTED, GUESS, SCANNED = "corner", "walk", "stagnation", "exhausted", "guess", "scan"


class LocateRef:
    def __init__(self, grid, params):
        self.o = Oracle(grid, params)
        self.lib, self.kg, self.p = self.o.lib, self.o.kg, params
        self.d = d = grid["desc"]
        self.Lx = float(d.Lx)
        st = grid["static"]
        self.lon, self.lat = (np.ascontiguousarray(st[k], dtype=np.float64) for k in ("lon", "lat"))        # corners (grd%lon, grd%lat)
        self.lonc, self.latc = (np.ascontiguousarray(st[k], dtype=np.float64) for k in ("lonc", "latc"))    # centres
        self.area = np.ascontiguousarray(st["area"], dtype=np.float64)
        self.moves = 0          # moves of the last walk
        # dcost is called a thousand times per berg: the centres as Python floats, the extents as Python ints
        self._lonc, self._latc, self._isd, self._jsd = self.lonc.tolist(), self.latc.tolist(), int(d.isd), int(d.jsd)
        self._mod = self.lib.ko_apply_modulo_around_point
        # ylo, yhi of every cell of the computational domain, for the scan below
        a, b, c, e = self.lat[:-1, :-1], self.lat[:-1, 1:], self.lat[1:, 1:], self.lat[1:, :-1]
        ylo = np.minimum(np.minimum(a, b), np.minimum(c, e))
        yhi = np.maximum(np.maximum(a, b), np.maximum(c, e))
        js, is_ = d.jsc - d.jsd - 1, d.isc - d.isd - 1
        nj, ni = d.jec - d.jsc + 1, d.iec - d.isc + 1
        self._ylo, self._yhi = ylo[js:js + nj, is_:is_ + ni], yhi[js:js + nj, is_:is_ + ni]

    # ---- the oracle's pieces ----
    def in_cell(self, x, y, i, j):
        return bool(self.lib.ko_is_point_in_cell(C.byref(self.kg), float(x), float(y), int(i), int(j)))

    def pos_within_cell(self, x, y, i, j):
        xi, yj, err = C.c_double(), C.c_double(), C.c_int(0)
        self.lib.ko_pos_within_cell(C.byref(self.kg), C.byref(self.p), float(x), float(y), int(i), int(j), C.byref(xi), C.byref(yj), C.byref(err))
        return xi.value, yj.value

    def mod(self, x, y):
        return self.lib.ko_apply_modulo_around_point(float(x), float(y), self.Lx)

    # ---- FW:5845-5858 ----
    def dcost(self, x, y, i, j):
        x2, y2 = self._lonc[j - self._jsd][i - self._isd], self._latc[j - self._jsd][i - self._isd]
        x1m = self._mod(x, x2, self.Lx)
        return (x2 - x1m) * (x2 - x1m) + (y2 - y) * (y2 - y)

    # ---- FW:5862-5893 ----
    def find_better_min(self, x, y, w, oi, oj):
        d = self.d
        xs, xe, ys, ye = max(d.isc, oi - w), min(d.iec, oi + w), max(d.jsc, oj - w), min(d.jec, oj + w)
        better, dmin = False, self.dcost(x, y, oi, oj)
        for j in range(ys, ye + 1):
            for i in range(xs, xe + 1):
                dc = self.dcost(x, y, i, j)
                if dc < dmin:
                    better, dmin, oi, oj = True, dc, i, j
        return better, oi, oj

    # ---- FW:5896-5924 ----
    def find_cell_loc(self, x, y, w, oi, oj):
        d = self.d
        xs, xe, ys, ye = max(d.isc, oi - w), min(d.iec, oi + w), max(d.jsc, oj - w), min(d.jec, oj + w)
        for j in range(ys, ye + 1):
            for i in range(xs, xe + 1):
                if self.in_cell(x, y, i, j):
                    return True, i, j
        return False, oi, oj

    # ---- FW:6011-6041 ----
    def scan(self, x, y):
        """the loop of FW:6034-6039: j outer, i inner, the first hit.  Cells whose latitude range does not hold y are skipped
        without a call: is_point_in_cell returns false for them at FW:6120-6122 (the same min / max of the same four values)."""
        d = self.d
        jj, ii = np.nonzero((y >= self._ylo) & (y <= self._yhi))     # row-major: the scan order
        for j, i in zip(jj + d.jsc, ii + d.isc):
            if self.in_cell(x, y, i, j):
                return True, int(i), int(j)
        return False, -999, -999

    def find_cell(self, x, y):
        d = self.d
        with np.errstate(all="ignore"):
            gi = np.floor((np.float64(x) - self.lon[0, 0]) / (self.lon[1, 1] - self.lon[0, 0])) + (d.isd + 1)
            gj = np.floor((np.float64(y) - self.lat[0, 0]) / (self.lat[1, 1] - self.lat[0, 0])) + (d.jsd + 1)
        if gi > d.isc - 1 and gi < d.iec + 1 and gj > d.jsc - 1 and gj < d.jec + 1:
            if self.in_cell(x, y, int(gi), int(gj)):
                return True, int(gi), int(gj), GUESS
        return self.scan(x, y) + (SCANNED,)

    # ---- FW:5710-5842 ----
    def find_cell_by_search(self, x, y):
        d = self.d
        is_, ie, js, je = d.isc, d.iec, d.jsc, d.jec
        self.moves = 0
        corners = ((is_ + 1, js + 1), (ie - 1, js + 1), (ie - 1, je - 1), (is_ + 1, je - 1))
        dc = [self.dcost(x, y, i, j) for i, j in corners]
        dmin = min(dc)
        i, j = corners[dc.index(dmin)]            # ties go to the first listed
        if self.in_cell(x, y, i, j):
            return True, i, j, CORNER
        # d0 .. d8 of FW:5757-5765 and the order their ties resolve in, FW:5769-5777
        nine = ((0, 0), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1))
        order = (0, 2, 4, 6, 8, 1, 3, 5, 7)
        for _ in range((ie - is_) + (je - js)):
            io, jo = i, j
            dd = [self.dcost(x, y, io + a, jo + b) for a, b in nine]
            dmin = min(dd)
            di, dj = next(nine[q] for q in order if dd[q] == dmin)
            i, j = min(ie, max(is_, io + di)), min(je, max(js, jo + dj))
            self.moves += 1
            if self.in_cell(x, y, i, j):
                return True, i, j, WALK
            if i == io and j == jo:
                better, i, j = self.find_better_min(x, y, 3, i, j)
                if not better:
                    found, i, j = self.find_cell_loc(x, y, 1, i, j)
                    if not found:
                        found, i, j = self.find_cell_loc(x, y, 3, i, j)
                    i, j = min(ie, max(is_, i)), min(je, max(js, j))
                    if self.in_cell(x, y, i, j):
                        found = True
                    return found, i, j, STAGNATION
        found, i, j, _ = self.find_cell(x, y)
        return found, i, j, EXHAUSTED

    def locate(self, x, y, mode):
        """(found, ine, jne, branch); ine = jne = -999 when the reference's path finds no cell"""
        found, i, j, branch = self.find_cell_by_search(x, y) if mode == SEARCH else self.find_cell(x, y)
        return (True, i, j, branch) if found else (False, -999, -999, branch)

    def locate_all(self, lon, lat, mode):
        """arrays ine, jne, xi, yj, status and the list of branches, for kid_locate_bergs' results"""
        n = len(lon)
        ine, jne = np.full(n, -999, dtype=np.int32), np.full(n, -999, dtype=np.int32)
        xi, yj, status, branches = np.zeros(n), np.zeros(n), np.full(n, LOST, dtype=np.int32), []
        d = self.d
        for k in range(n):
            found, i, j, br = self.locate(lon[k], lat[k], mode)
            branches.append(br)
            if found:
                ine[k], jne[k] = i, j
                xi[k], yj[k] = self.pos_within_cell(lon[k], lat[k], i, j)
                status[k] = GROUNDED if self.area[j - d.jsd, i - d.isd] == 0.0 else FOUND
        return ine, jne, xi, yj, status, branches
