"""Interacting bergs under RK4 (tests/test_rk_interactive_cpu.py, tests/test_rk_interactive_gpu.py): the cases, the
loader of the checker (tests/rk_interactive_ref.c: evolve_icebergs with Runge_not_Verlet and interactive_icebergs_on, the oracle's
stage driver around the oracle's accel_sts_ia), and icebergs_run composed from the oracle's phases in the sequence of
ko_run_step_interactive with that evolve in its place.  Test infrastructure.

Cases:
  (a) box(contact)     the undivided box of tests/halo_bergs.py, 247 discs, both contact searches, 40 steps of 600 s
  (b) collision()      icebergs_amd.reference_tests.collision("KID"): 16 elements in two bonded conglomerates driven against each
                       other, scale_damping_by_pmag, coastal_drift.  COLLISION_STEPS = 550: measured with the checker alone, a pair of
                       elements of different conglomerates is within R1 + R2 before each of the steps 495 .. 537, so the twentieth
                       step of contact is step 514 and 550 is the first multiple of 50 behind it (test_rk_interactive_cpu.py)
  (c) polar()          two bonded bergs of tests/latlon_bonded.py on the Stern springs at 89.01 N, under the single-time-step scheme
  (d) shapes(n)        n rows cut from the box's population: every 7th row dead, one static, one with fl_k = -1
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

NSTEPS, CHECK_AT = HB.NSTEPS, HB.CHECK_AT
COLLISION_STEPS = 550
POLAR_STEPS = 20
SHAPES = (1, 63, 64, 65, 257)
SO_PATH = os.path.join(ROOT, "tests", "_build", "librk_interactive_ref.so")
COUNTS = ("cell_changes", "bounces", "tangent_steps", "berg_steps")


# ---- the checker ----
_LIB = None


def oracle_lib():
    ol = HB._oracle_lib()
    return ol


def checker():
    """the checker library; __graft_entry__.build() compiles it (a missing library is an error, never a skip)"""
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            import __graft_entry__ as G
            G.build_rk_checker()
        import oracle_lib as OL
        lib = C.CDLL(SO_PATH)
        lib.tko_evolve_icebergs_interactive_rk.restype = None
        lib.tko_evolve_icebergs_interactive_rk.argtypes = [C.POINTER(OL.KoGrid), C.POINTER(T.Params), C.POINTER(T.BergSoA), C.c_void_p, C.POINTER(C.c_double)]
        lib.tko_set_traversal.restype = None
        lib.tko_set_traversal.argtypes = [C.c_int, C.c_int64]
        lib.tko_reset_counts.restype = None
        lib.tko_get_counts.restype = None
        lib.tko_get_counts.argtypes = [C.POINTER(C.c_int64)]
        _LIB = lib
    return _LIB


def counts():
    out = (C.c_int64 * len(COUNTS))()
    checker().tko_get_counts(out)
    return dict(zip(COUNTS, (int(v) for v in out)))


def _oracle_phases(lib):
    import oracle_lib as OL
    args = [C.POINTER(OL.KoGrid), C.POINTER(T.Params), C.POINTER(T.BergSoA), C.c_void_p]
    lib.ko_orig_bond_length.restype = None
    lib.ko_orig_bond_length.argtypes = args
    lib.ko_find_orientations.restype = None
    lib.ko_find_orientations.argtypes = args + [C.POINTER(C.c_double)]
    lib.ko_set_orientation.restype = None
    lib.ko_set_orientation.argtypes = [C.POINTER(C.c_double)]


# ---- the cases ----
def box_params(contact, old_order=True, rk=True, interactive=True):
    p = HB.params(contact)
    p.Runge_not_Verlet = 1 if rk else 0
    p.old_interp_flds_order = 1 if old_order else 0
    p.interactive_icebergs_on = 1 if interactive else 0
    return p


def box(contact, old_order=True, rk=True, interactive=True):
    """(grid, params, bergs, bonds = None, steps)"""
    grid, b = HB.population()
    return grid, box_params(contact, old_order, rk, interactive), b, None, NSTEPS


def collision(rk=True):
    from icebergs_amd import reference_tests as RT
    c = RT.collision("KID")
    p = c["params"]
    S.set_diag_all(p)
    p.Runge_not_Verlet = 1 if rk else 0
    return c["grid"], p, c["bergs"], c["bonds"], COLLISION_STEPS


def polar(rk=True):
    import latlon_bonded as LB
    kw = dict(dem=False, mts=False, contact=True, spring_coef=1.0e-5, dt=60.0, two_bergs=True, hexagonal=False, nx=4, ny=6)
    grid, p, b, bd, _ = LB.build(kw, 1.0, 89.01, (23, 30), None, "c4", POLAR_STEPS)
    p.Runge_not_Verlet = 1 if rk else 0
    return grid, p, b, bd, POLAR_STEPS


def shapes(n, contact=False):
    """n rows of the box's population (where n is larger the population over again, with ids of its own and 400 m to the east of
    the originals); every 7th row dead, row 2 static, row 4 with fl_k = -1"""
    grid, b0 = HB.population()
    n0 = len(b0["lon"])
    rows = np.arange(n) % n0
    b = {k: (np.ascontiguousarray(v[rows]) if isinstance(v, np.ndarray) else v) for k, v in b0.items()}
    b["id"] = (b0["id"][rows] + (np.arange(n) // n0) * 100000).astype(np.int64)
    if n > n0:                                   # the second copy a little aside of the first, inside the same cells where it can
        extra = np.arange(n) >= n0
        b["lon"][extra] += 400.0
        b["xi"][extra] += 400.0 / HB.RES
        over = b["xi"] >= 1.0
        b["xi"][over] -= 1.0
        b["ine"][over] += 1
        b["lon_old"][:] = b["lon"]
        b["start_lon"][extra] += 400.0
        b = S.sort_reference_order(b)
    b["alive"][6::7] = 0
    if n > 2:
        b["static_berg"][2] = 1.0
    if n > 4:
        b["fl_k"][4] = -1.0
    return grid, box_params(contact), b, None, 1


# ---- what a case has to show ----
def radius_of(p, area):
    if p.hexagonal_icebergs:
        return np.sqrt(area / (2.0 * np.sqrt(3.0)))
    if p.iceberg_bonds_on:
        return 0.5 * np.sqrt(area)
    return np.sqrt(area / p.pi)


def pairs_in_reach(p, desc, b, groups=None):
    """unordered pairs of live bergs that take part in contact closer than max(R1 + R2, contact_distance), measured as
    calculate_force measures (IB:611-660); groups: only pairs whose members differ in it (the conglomerates)"""
    n = int(b.get("_n", len(b["lon"])))
    a = np.nonzero((b["alive"][:n] != 0) & (b["fl_k"][:n] != -1.0))[0]
    lon, lat = b["lon_old"][a], b["lat_old"][a]
    R = radius_of(p, b["length"][a] * b["width"][a])
    dlon, dlat = lon[:, None] - lon[None, :], lat[:, None] - lat[None, :]
    if desc.grid_is_latlon:
        pi_180 = p.pi / 180.0
        rx = dlon * (pi_180 * p.Rearth * np.cos(0.5 * (lat[:, None] + lat[None, :]) * pi_180))
        ry = dlat * (pi_180 * p.Rearth)
    else:
        rx, ry = dlon, dlat
    r = np.sqrt(rx * rx + ry * ry)
    crit = np.maximum(R[:, None] + R[None, :], p.contact_distance)
    close = (r < crit) & (r > 0.0)
    if groups is not None:
        grp = groups[a]
        close &= grp[:, None] != grp[None, :]
    return int(close.sum()) // 2


# ---- the composed step ----
class Composed:
    """icebergs_run (IB:5409-5512) for interacting bergs under the single-time-step scheme from the oracle's phases, in the sequence
    of ko_run_step_interactive; evolve: the checker under RK4, the oracle's own ko_evolve_icebergs_interactive under Verlet"""

    def __init__(self, grid, p, b, bonds=None):
        self.ol = oracle_lib()
        self.o, self.b, self.p, self.bonds = self.ol.Oracle(grid, p), b, p, bonds
        _oracle_phases(self.o.lib)
        self.contact = HB.is_contact(p)
        self.visited = False
        self.n = len(b["lon"])

    def _args(self):
        bd = C.byref(self.o.bond_soa(self.bonds, self.n)) if self.bonds is not None else None
        return C.byref(self.o.kg), C.byref(self.o.params), C.byref(self.o.soa(self.b)), bd

    def evolve(self):
        dp = self.ol._dp
        if self.p.Runge_not_Verlet:
            bd = self._args()[3]
            checker().tko_evolve_icebergs_interactive_rk(C.byref(self.o.kg), C.byref(self.o.params), C.byref(self.o.soa(self.b)),
                                                         C.cast(bd, C.c_void_p) if bd is not None else None, dp(self.o.scalars))
        else:
            self.o.lib.ko_evolve_icebergs_interactive(*self._args(), dp(self.o.scalars))

    def gridded(self):
        lib, dp, p = self.o.lib, self.ol._dp, self.p
        orient = None
        if p.hexagonal_icebergs and p.iceberg_bonds_on and p.rotate_icebergs_for_mass_spreading and self.bonds is not None:
            orient = np.zeros(max(self.n, 1))
            lib.ko_find_orientations(*self._args(), dp(orient))
            lib.ko_set_orientation(dp(orient))
        lib.ko_create_gridded_icebergs_fields(*self._args()[:3], dp(self.o.acc), dp(self.o.out))
        lib.ko_set_orientation(None)

    def step(self):
        lib, dp, p = self.o.lib, self.ol._dp, self.p
        self.o.acc[:] = 0.0
        if not self.visited:
            if self.contact:
                lib.ko_set_conglom_ids(*self._args())                          # IB:5415-5416
            if p.iceberg_bonds_on and self.bonds is not None:
                lib.ko_orig_bond_length(*self._args())                         # IB:5418
        self.visited = True
        if not p.old_interp_flds_order:
            lib.ko_interp_gridded_fields_to_bergs(*self._args()[:3])           # IB:5423
        if not p.static_icebergs:
            self.evolve()                                                      # IB:5433
        if self.contact:
            lib.ko_set_conglom_ids(*self._args())                              # IB:5470-5471
        if not p.old_interp_flds_order:
            lib.ko_interp_gridded_fields_to_bergs(*self._args()[:3])           # IB:5473
        lib.ko_thermodynamics(*self._args()[:3], dp(self.o.acc), dp(self.o.scalars))   # IB:5505
        self.gridded()                                                         # IB:5512
        self.o.scalars[T.SCALAR_NAMES["nbergs_alive"]] = float((self.b["alive"] != 0).sum())

    def snapshot(self):
        """(bergs, acc, out, scalars) as tests/parity.py::compare reads them"""
        return S.copy_bergs(self.b), self.o.acc.copy(), self.o.out.copy(), self.o.scalars.copy()


_RUNS = {}


def composed_run(name, case, check_at, groups=None):
    """the composed run of `case` = (grid, params, bergs, bonds, steps), once per name and shared (nobody changes it):
    ({step: snapshot} at check_at, stats) -- stats: the checker's branch counts over the run, the pairs in reach summed over the
    steps (measured before each step), the first step with a pair in reach, contact_steps[s - 1]: how many of the steps 1 .. s had
    one, whether every velocity stayed finite"""
    if name in _RUNS:
        return _RUNS[name]
    grid, p, b, bonds, steps = case
    b = S.copy_bergs(b)
    bonds = S.copy_bonds(bonds) if bonds is not None else None
    c = Composed(grid, p, b, bonds)
    if p.Runge_not_Verlet:
        checker().tko_set_traversal(0, 0)
        checker().tko_reset_counts()
    stats = {"pairs": 0, "first_contact": None, "contact_steps": [], "finite": True}
    snaps = {}
    for step in range(1, steps + 1):
        if p.interactive_icebergs_on:
            n_pairs = pairs_in_reach(p, grid["desc"], b, groups)
            stats["pairs"] += n_pairs
            if n_pairs and stats["first_contact"] is None:
                stats["first_contact"] = step
            stats["contact_steps"].append((stats["contact_steps"][-1] if stats["contact_steps"] else 0) + (1 if n_pairs else 0))
        c.step()
        stats["finite"] = stats["finite"] and bool(np.isfinite(b["uvel"]).all() and np.isfinite(b["vvel"]).all())
        if step in check_at:
            snaps[step] = c.snapshot()
    if p.Runge_not_Verlet:
        stats.update(counts())
    _RUNS[name] = (snaps, stats)
    return _RUNS[name]


def box_run(contact, old_order=True, rk=True, interactive=True):
    return composed_run(("box", contact, old_order, rk, interactive), box(contact, old_order, rk, interactive), CHECK_AT)


def collision_groups(b):
    """the two conglomerates of the initial state: mirrored about y = 10 km"""
    return (b["lat"] > 10.0e3).astype(np.int64)


def collision_run(rk=True, steps=COLLISION_STEPS):
    grid, p, b, bd, _ = collision(rk)
    return composed_run(("collision", rk, steps), (grid, p, b, bd, steps), (steps,), groups=collision_groups(b))


def polar_run(rk=True):
    return composed_run(("polar", rk), polar(rk), (POLAR_STEPS,))


def shapes_run(n, contact=False):
    return composed_run(("shapes", n, contact), shapes(n, contact), (1,))
