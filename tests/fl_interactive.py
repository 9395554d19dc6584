"""Footloose calving among interacting bergs (tests/test_fl_interactive_cpu.py, tests/test_fl_interactive_gpu.py): the
undivided box of tests/halo_bergs.py with its current and its touching discs, a wind and warm water so that the discs melt and
calve, the footloose parameters of the footloose profile (children as new bergs, displaced), and the step of this switch pair
composed from phases the oracle has -- with the promotion pass, adjust_fl_berg_interactivity (IB:2765-2841), restated in numpy.
Test infrastructure.

The population is HB.population(seed 8) in arrays of 1 200 rows -- the contact search takes every second disc -- with fl_k of the
rows taken uniform in [0, 6e4) from default_rng(108).  Measured with the oracle alone, 40 steps (test_fl_interactive_cpu.py holds
the floors; dead rows are nobody's partner in the promotion pass, as a berg that has left is in no list of the reference):

    search    children  promotions  promoted child in contact (pairs)  children at -1 at the end  smallest |r_dist/crit_dist - 1|
    3 x 3        366        119              2 315                              245                      7.8e-05
    contact      182         36                254                              141                      2.2e-04
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import halo_bergs as HB                   # noqa: E402
from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402

CAP = 1200
NSTEPS = HB.NSTEPS
CHECK_AT = HB.CHECK_AT
SEED, FLK_SEED = HB.SEED, 108
MARGIN = 1.0e-6        # no decision of the promotion pass closer to its threshold than this (relative, squared distances)


def grid():
    g = HB.whole_grid()
    f = g["forcing"]
    f["ua"][:] = -25.8
    f["sst"][:] = 2.0
    f["sss"][:] = 34.0
    return g


def params(contact, old_order=False, fl_bits=False):
    """the footloose parameters of the footloose profile (new bergs, displaced) on the springs of the halo-berg box; melt on.
    fl_bits: the other fl_style -- the calved ice goes to footloose bits, and a child is made from a berg's bits once they weigh
    3e10 kg (a tenth of the profile's threshold, so that these discs get there within 40 steps)"""
    _, p, _ = S.config_c3(n=1, fl_style="fl_bits" if fl_bits else "new_bergs", displace=True)
    if fl_bits:
        p.new_berg_from_fl_bits_mass_thres = 3.0e10
    q = HB.params(contact)
    p.dt, p.lat_ref, p.use_f_plane = HB.DT, 0.0, 0
    p.interactive_icebergs_on, p.iceberg_bonds_on, p.mts = 1, 0, 0
    p.spring_coef = q.spring_coef
    p.scale_damping_by_pmag, p.critical_interaction_damping_on, p.tang_crit_int_damp_on = 0, 1, 0
    if contact:
        p.contact_distance, p.contact_spring_coef = 2.0e3, 5.0e-7
        p.contact_cells_lon = p.contact_cells_lat = 1
    else:
        p.contact_distance, p.contact_spring_coef = 0.0, p.spring_coef
    p.old_interp_flds_order = 1 if old_order else 0
    return p


def is_contact(p):
    return HB.is_contact(p)


def population(contact):
    """(grid, bergs): arrays of CAP rows, b["_n"] live"""
    _, b0 = HB.population(SEED)
    n0 = len(b0["lon"])
    sel = np.arange(0, n0, 2) if contact else np.arange(n0)
    b = S.empty_bergs(CAP)
    b["alive"][:] = 0
    m = len(sel)
    for k, v in b0.items():
        if isinstance(v, np.ndarray):
            b[k][:m] = v[sel]
    b["fl_k"][:m] = np.random.default_rng(FLK_SEED).uniform(0.0, 6.0e4, m)
    b["_n"] = m
    return grid(), b


# ---- the box on a lat-lon patch: the promotion pass with grid_is_latlon (IB:2816-2822) ----
LATLON_CENTRE = (300.0, -70.0)
LATLON_SEED, LATLON_KEEP, LATLON_CHILDREN = 208, 0.5, 0.4


def latlon_grid(p):
    """a single tile of HB's 16 x 12 cells, 5 km tall and 5 km wide at the box's centre"""
    import latlon_bonded as LB
    dlat = HB.RES / (p.Rearth * np.pi / 180.0)
    return LB.latlon_patch(p, LATLON_CENTRE[0], LATLON_CENTRE[1], (0.5 * HB.NI * HB.NTX + 0.5, 0.5 * HB.NJ * HB.NTY + 0.5),
                           ni=HB.NI * HB.NTX, nj=HB.NJ * HB.NTY, dlat=dlat)


def latlon_state(contact):
    """(grid, params, bergs): the halo-berg box's discs mapped by tests/latlon_bonded.py's map (metres from the box's centre to
    degrees), thinned to about LATLON_KEEP of them so that some stand alone, LATLON_CHILDREN of the rest waiting at fl_k = -1;
    rows in reference order.  Chosen with np_adjust alone: both searches promote some and hold some back, and no decision is
    closer to its threshold than MARGIN (tests/test_fl_interactive_cpu.py)."""
    import latlon_bonded as LB
    p = params(contact)
    g = latlon_grid(p)
    _, b0 = HB.population(SEED)
    rng = np.random.default_rng(LATLON_SEED)
    keep = np.nonzero(rng.random(len(b0["lon"])) < LATLON_KEEP)[0]
    b = {k: (v[keep].copy() if isinstance(v, np.ndarray) else v) for k, v in b0.items()}
    x, y = b["lon"] - 0.5 * HB.NI * HB.NTX * HB.RES, b["lat"] - 0.5 * HB.NJ * HB.NTY * HB.RES
    b["lon"][:], b["lat"][:] = LB.to_degrees(p, LATLON_CENTRE[0], LATLON_CENTRE[1], x, y)
    for f in ("lon_old", "start_lon"):
        b[f][:] = b["lon"]
    for f in ("lat_old", "start_lat"):
        b[f][:] = b["lat"]
    LB.locate(g, b)
    b["fl_k"][:] = np.where(rng.random(len(keep)) < LATLON_CHILDREN, -1.0, rng.uniform(0.0, 6.0e4, len(keep)))
    return g, p, S.sort_reference_order(b)


# ---- adjust_fl_berg_interactivity, IB:2765-2841 ----
def np_adjust(p, desc, b, n, margins=None):
    """the rows whose fl_k the pass sets to -2, in row order; b["fl_k"] is changed.  The pass writes a berg's own fl_k only and
    reads nobody else's, so every decision is taken on the state before the pass.  margins: gets |r_dist / crit_dist - 1| of every
    pair a decision could have looked at (the reference stops at a berg's first contact)."""
    nc_x, nc_y = int(p.contact_cells_lon), int(p.contact_cells_lat)
    radial = nc_x == 1 and nc_y == 1
    pi_180 = p.pi / 180.0
    if p.hexagonal_icebergs:
        rdenom = 1.0 / (2.0 * np.sqrt(3.0))
    elif p.iceberg_bonds_on:
        rdenom = 1.0 / 4.0
    else:
        rdenom = 1.0 / p.pi
    live = b["alive"][:n] != 0
    ine, jne, ids = b["ine"][:n], b["jne"][:n], b["id"][:n]
    lon, lat = b["lon"][:n], b["lat"][:n]
    area = b["length"][:n] * b["width"][:n]
    promoted = []
    for k in np.nonzero(live & (b["fl_k"][:n] == -1.0))[0]:
        j0, j1 = max(jne[k] - nc_y, desc.jsd + 1), min(jne[k] + nc_y, desc.jed)
        i0, i1 = max(ine[k] - nc_x, desc.isd + 1), min(ine[k] + nc_x, desc.ied)
        o = np.nonzero(live & (jne >= j0) & (jne <= j1) & (ine >= i0) & (ine <= i1) & (ids != ids[k]))[0]
        dlon, dlat = lon[o] - lon[k], lat[o] - lat[k]
        if radial:
            R1, R2 = np.sqrt(area[k] * rdenom), np.sqrt(area[o] * rdenom)
            crit = np.maximum(R1 + R2, p.contact_distance) ** 2
        else:
            crit = np.full(len(o), p.contact_distance ** 2)
        if desc.grid_is_latlon:
            lat_ref = 0.5 * (lat[k] + lat[o])
            dx_dlon, dy_dlat = pi_180 * p.Rearth * np.cos(lat_ref * pi_180), pi_180 * p.Rearth
            r = (dlon * dx_dlon) ** 2 + (dlat * dy_dlat) ** 2
        else:
            r = dlon ** 2 + dlat ** 2
        if margins is not None and len(o):
            with np.errstate(divide="ignore", invalid="ignore"):
                margins.append(float(np.min(np.abs(r / crit - 1.0))))
        if not (r < crit).any():
            promoted.append(int(k))
    b["fl_k"][promoted] = -2.0
    return promoted


def contact_pairs_of_promoted(p, b, n):
    """ordered pairs (promoted child, another live berg that takes part in contact) within max(R1 + R2, contact_distance)"""
    live = b["alive"][:n] != 0
    a = np.nonzero(live & (b["fl_k"][:n] == -2.0))[0]
    o = np.nonzero(live & (b["fl_k"][:n] != -1.0))[0]
    if not len(a):
        return 0
    R = np.sqrt(b["length"][:n] * b["width"][:n] / p.pi)
    d2 = (b["lon"][a][:, None] - b["lon"][o][None, :]) ** 2 + (b["lat"][a][:, None] - b["lat"][o][None, :]) ** 2
    reach = np.maximum(R[a][:, None] + R[o][None, :], p.contact_distance)
    return int(((d2 < reach * reach) & (a[:, None] != o[None, :])).sum())


# ---- the composed step ----
def oracle_lib():
    return HB._oracle_lib()


class Composed:
    """icebergs_run (IB:5409-5512) for footloose with interactive_icebergs_on from the oracle's phases.  promote=False leaves the
    promotion pass out; relabel=True marks every child interactive (fl_k = -2) at birth, which is what the -1 guard prevents."""

    def __init__(self, grid_, p, b, promote=True, relabel=False):
        self.ol = oracle_lib()
        self.o, self.b, self.p = self.ol.Oracle(grid_, p), b, p
        self.desc = grid_["desc"]
        self.contact = is_contact(p)
        self.promote, self.relabel = promote, relabel
        self.visited, self.fl_step = False, 0
        self.margins = []

    def _args(self):
        return C.byref(self.o.kg), C.byref(self.o.params), C.byref(self.o.soa(self.b))

    def evolve(self):
        self.o.lib.ko_evolve_icebergs_interactive(*self._args(), None, self.ol._dp(self.o.scalars))

    def calve(self):
        lib = self.o.lib
        s = self.o.soa(self.b)
        lib.ko_set_fl_step(self.fl_step)
        lib.ko_footloose_calving(C.byref(self.o.kg), C.byref(self.o.params), C.byref(s), len(self.b["lon"]), self.ol._dp(self.o.acc), self.ol._dp(self.o.scalars))
        self.fl_step = int(lib.ko_get_fl_step())
        n0, self.b["_n"] = self.b["_n"], int(s.n)
        if self.relabel:
            self.b["fl_k"][n0:self.b["_n"]] = -2.0
        return self.b["_n"] - n0

    def step(self):
        """one step; returns (children born, rows promoted)"""
        lib, dp = self.o.lib, self.ol._dp
        self.o.acc[:] = 0.0
        if self.contact and not self.visited:
            lib.ko_set_conglom_ids(*self._args(), None)                    # IB:5415-5416
        self.visited = True
        if not self.p.old_interp_flds_order:
            lib.ko_interp_gridded_fields_to_bergs(*self._args())           # IB:5423
        self.evolve()                                                      # IB:5433
        born = self.calve()                                                # IB:5453
        if self.contact:
            lib.ko_set_conglom_ids(*self._args(), None)                    # IB:5470
        if not self.p.old_interp_flds_order:
            lib.ko_interp_gridded_fields_to_bergs(*self._args())           # IB:5473
        promoted = np_adjust(self.p, self.desc, self.b, self.b["_n"], self.margins) if self.promote else []   # IB:5486
        lib.ko_thermodynamics(*self._args(), dp(self.o.acc), dp(self.o.scalars))                             # IB:5505
        lib.ko_create_gridded_icebergs_fields(*self._args(), dp(self.o.acc), dp(self.o.out))                 # IB:5512
        self.o.scalars[T.SCALAR_NAMES["nbergs_alive"]] = float((self.b["alive"][:self.b["_n"]] != 0).sum())
        return born, promoted

    def snapshot(self):
        """(bergs, acc, out, scalars) as tests/parity.py::compare reads them"""
        return S.copy_bergs(self.b), self.o.acc.copy(), self.o.out.copy(), self.o.scalars.copy()


_RUNS = {}


def composed_run(contact, old_order=False, promote=True, relabel=False, steps=NSTEPS, fl_bits=False):
    """the composed oracle run, once per variant and shared: {step: snapshot} at CHECK_AT, {step: snapshot before the evolve} at
    CHECK_AT, the promotions of every step, and what the population has to show"""
    key = (contact, old_order, promote, relabel, steps, fl_bits)
    if key in _RUNS:
        return _RUNS[key]
    g, b = population(contact)
    p = params(contact, old_order, fl_bits)
    c = Composed(g, p, b, promote=promote, relabel=relabel)
    stats = {"children": 0, "promotions": 0, "pairs": 0, "held_back": [], "promoted_ids": {}, "finite": True}
    snaps, before = {}, {}
    for step in range(1, steps + 1):
        stats["pairs"] += contact_pairs_of_promoted(p, b, b["_n"])
        if step in CHECK_AT:
            before[step] = S.copy_bergs(b)
        born, promoted = c.step()
        n = b["_n"]
        stats["children"] += born
        stats["promotions"] += len(promoted)
        stats["promoted_ids"][step] = b["id"][promoted].copy()
        stats["held_back"].append(int(((b["alive"][:n] != 0) & (b["fl_k"][:n] == -1.0)).sum()))
        stats["finite"] = stats["finite"] and bool(np.isfinite(b["uvel"][:n]).all() and np.isfinite(b["vvel"][:n]).all())
        if step in CHECK_AT:
            snaps[step] = c.snapshot()
    stats["margin"] = min(c.margins) if c.margins else np.inf
    _RUNS[key] = (snaps, before, stats, p, g)
    return _RUNS[key]


def fl_sets(b, n=None):
    """(live ids, ids of live rows with fl_k = -1, with fl_k = -2), sorted"""
    n = int(b.get("_n", len(b["lon"]))) if n is None else n
    live = b["alive"][:n] != 0
    k = b["fl_k"][:n]
    return np.sort(b["id"][:n][live]), np.sort(b["id"][:n][live & (k == -1.0)]), np.sort(b["id"][:n][live & (k == -2.0)])
