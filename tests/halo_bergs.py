"""Geometry, population and reference runs of the halo-berg tests (tests/test_halo_bergs_cpu.py,
tests/test_halo_bergs_gpu.py): a Cartesian box of 16 x 12 cells of 5 km cut into 2 x 2 tiles of 8 x 6, a few hundred touching
discs in a rotating current that carries them across both tile edges and round the centre corner, the numpy restatement of the
strip selection of update_halo_icebergs (FW:1896, 1911, 1981, 1995), and the oracle behind the tile interface of
icebergs_amd.decomposed with halo rows.  Test infrastructure."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402

H = S.HALO
NTX = NTY = 2
NI, NJ, RES = 8, 6, 5000.0               # cells per tile, cell size
NSTEPS, DT = 40, 600.0                    # 40 steps of 600 s: a berg at 0.3 m/s crosses 1.4 cells
RADIUS = 1500.0
SEED = 8                                  # chosen with the undivided oracle alone (whole_oracle: contacts across edges, diagonal ones, migrations)
CHECK_AT = (1, 20, 40)
FIELDS = ("lon", "lat", "uvel", "vvel", "uvel_prev", "vvel_prev", "axn", "ayn", "bxn", "byn", "xi", "yj", "mass", "thickness", "width", "length",
          "lon_old", "lat_old", "uvel_old", "vvel_old", "start_lon", "start_lat", "start_mass", "mass_scaling")
WIRE = ["lon", "lat", "uvel", "vvel", "uvel_prev", "vvel_prev", "xi", "yj", "start_lon", "start_lat", "start_year", "start_day", "start_mass", "mass",
        "thickness", "width", "length", "fl_k", "mass_scaling", "mass_of_bits", "mass_of_fl_bits", "mass_of_fl_bergy_bits", "heat_density", "ine", "jne",
        "axn", "ayn", "bxn", "byn", "halo_berg", "static_berg"]          # reals 1..31 of pack_berg_into_buffer2, then the id in two, then od


# ---- geometry ----
def whole_grid():
    g = S.cartesian_grid(ni=NI * NTX, nj=NJ * NTY, gridres=RES)
    st, f = g["static"], g["forcing"]
    xc, yc = 0.5 * NI * NTX * RES, 0.5 * NJ * NTY * RES
    w = 1.5e-5                                           # a solid rotation about the centre corner plus a weak shear and drift
    f["uo"][:] = -w * (st["lat"] - yc) + 0.04 + 0.03 * np.sin(st["lat"] / 9000.0)
    f["vo"][:] = w * (st["lon"] - xc) + 0.03
    f["sst"][:] = -1.0
    f["sss"][:] = 34.0
    return g


def tile_grid(tx, ty, whole=None, ni=NI, nj=NJ):
    """the tile's arrays are slices of the whole grid's, its data domain included: the same bits (ni, nj: other tile shapes, for
    a 2 x 1 layout of the same box)"""
    whole = whole_grid() if whole is None else whole
    g = S.cartesian_grid(ni=ni, nj=nj, gridres=RES)
    js, is_ = ty * nj, tx * ni
    for group in ("static", "forcing"):
        for k, v in whole[group].items():
            g[group][k] = np.ascontiguousarray(v[js:js + nj + 2 * H, is_:is_ + ni + 2 * H])
    return g


def params(contact):
    """unbonded interacting bergs under the single-time-step Verlet scheme: Stern et al.'s 3 x 3 search, or the contact-distance
    variant with set_conglom_ids.  Melt is off: with melt on the reference's own moment for the copies would differ."""
    p = S.set_diag_all(S.default_params())
    p.dt, p.lat_ref, p.use_f_plane = DT, 0.0, 0
    p.Runge_not_Verlet, p.old_interp_flds_order, p.use_new_predictive_corrective = 0, 1, 1
    p.interactive_icebergs_on, p.iceberg_bonds_on, p.mts = 1, 0, 0
    p.spring_coef = 1.0e-6                                # dt * sqrt(k) = 0.6: the explicit spring is stable
    p.scale_damping_by_pmag, p.critical_interaction_damping_on, p.tang_crit_int_damp_on = 0, 1, 0
    p.set_melt_rates_to_zero = 1
    if contact:
        p.contact_distance, p.contact_spring_coef = 3.1e3, 5.0e-7
        p.contact_cells_lon = p.contact_cells_lat = 1    # ceil(3.1e3 / 5e3)
    else:
        p.contact_distance, p.contact_spring_coef = 0.0, p.spring_coef
    return p


def population(seed=SEED):
    """discs of 1.5 km radius (no bonds: R = sqrt(L W / pi)) on a jittered lattice of 2.9 km, moving with the current"""
    whole = whole_grid()
    rng = np.random.default_rng(seed)
    sp = 2900.0
    xs, ys = np.meshgrid(np.arange(12500.0, 67500.0, sp), np.arange(12500.0, 47500.0, sp))
    x = (xs + rng.uniform(-350.0, 350.0, xs.shape)).reshape(-1)
    y = (ys + rng.uniform(-350.0, 350.0, ys.shape)).reshape(-1)
    n = len(x)
    b = S.empty_bergs(n)
    b["lon"][:], b["lat"][:] = x, y
    b["ine"][:] = np.floor(x / RES).astype(np.int32) + 1
    b["jne"][:] = np.floor(y / RES).astype(np.int32) + 1
    b["xi"][:] = x / RES - (b["ine"] - 1)
    b["yj"][:] = y / RES - (b["jne"] - 1)
    side = np.sqrt(np.pi) * RADIUS * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, n))
    b["width"][:], b["length"][:] = side, side
    b["thickness"][:] = 200.0 * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, n))
    b["mass"][:] = b["thickness"] * S.RHO_BERGS * side * side
    b["start_mass"][:] = b["mass"]
    b["mass_scaling"][:] = 1.0
    xc, yc, w = 0.5 * NI * NTX * RES, 0.5 * NJ * NTY * RES, 1.5e-5
    b["uvel"][:] = -w * (y - yc) + 0.04
    b["vvel"][:] = w * (x - xc) + 0.03
    for f in ("uvel_old", "uvel_prev"):
        b[f][:] = b["uvel"]
    for f in ("vvel_old", "vvel_prev"):
        b[f][:] = b["vvel"]
    b["lon_old"][:], b["lat_old"][:] = x, y
    b["start_lon"][:], b["start_lat"][:] = x, y            # distinct: the `inorder` sort inside a cell is total
    b["start_year"][:] = 1
    b["start_day"][:] = 1.0e-6 * np.arange(n)
    return whole, S.sort_reference_order(b)


def split_bergs(b, tx, ty, cap, ni=NI, nj=NJ):
    """the live bergs of `b` (whole-grid cell indices) on tile (tx, ty) with the tile's own indices, in arrays of `cap` rows"""
    sel = (b["alive"] != 0) & ((b["ine"] - 1) // ni == tx) & ((b["jne"] - 1) // nj == ty)
    m = int(sel.sum())
    big = S.empty_bergs(cap)
    for k, v in b.items():
        if isinstance(v, np.ndarray):
            big[k][:m] = v[sel]
    big["ine"][:m] -= tx * ni
    big["jne"][:m] -= ty * nj
    big["_n"] = m
    return big


def trim(b):
    m = b["_n"]
    return {k: (v[:m].copy() if isinstance(v, np.ndarray) else v) for k, v in b.items() if k != "_n"}


# ---- the strip selection of update_halo_icebergs restated with numpy ----
def np_halo_select(ine, jne, alive, axis, w, nic, njc, halo=H):
    """(rows for the east / north neighbour, rows for the west / south one), in row order.  Axis 0: cells of rows 1..njc, hi strip
    columns nic-w+2..nic, lo strip 1..w (FW:1896, 1911); axis 1: columns of the whole data domain, hi strip rows njc-w+2..njc, lo
    strip 1..w (FW:1981, 1995).  Live rows only."""
    live = alive != 0
    if axis == 0:
        band, c, c1 = (jne >= 1) & (jne <= njc), ine, nic
    else:
        band, c, c1 = (ine >= 1 - halo) & (ine <= nic + halo), jne, njc
    hi = live & band & (c >= c1 - w + 2) & (c <= c1)
    lo = live & band & (c >= 1) & (c <= w)
    return np.nonzero(hi)[0], np.nonzero(lo)[0]


def np_records(b, rows, halo=None):
    """the 34 reals of pack_berg_into_buffer2 (FW:3268-3301) for `rows`; halo: what goes where halo_berg goes"""
    r = np.zeros((len(rows), 34))
    for q, name in enumerate(WIRE):
        r[:, q] = b[name][rows]
    if halo is not None:
        r[:, 29] = halo
    ids = b["id"][rows].astype(np.int64)
    r[:, 31] = (ids >> 32).astype(np.int32)
    r[:, 32] = (ids & 0xffffffff).astype(np.uint32).astype(np.int32)
    r[:, 33] = b["od"][rows]
    return r


def record_ids(r):
    return (np.rint(r[:, 31]).astype(np.int64) << 32) | (np.rint(r[:, 32]).astype(np.int64) & 0xffffffff)


# ---- the oracle ----
def _oracle_lib():
    import oracle_lib
    oracle_lib.build()
    lib = oracle_lib.load()
    args = [C.POINTER(oracle_lib.KoGrid), C.POINTER(T.Params), C.POINTER(T.BergSoA), C.c_void_p]
    lib.ko_evolve_icebergs_interactive.restype = None
    lib.ko_evolve_icebergs_interactive.argtypes = args + [C.POINTER(C.c_double)]
    lib.ko_set_conglom_ids.restype = None
    lib.ko_set_conglom_ids.argtypes = args
    lib.ko_calculate_mass_on_ocean.restype = None
    lib.ko_calculate_mass_on_ocean.argtypes = [C.POINTER(oracle_lib.KoGrid), C.POINTER(T.Params), C.POINTER(T.BergSoA), C.POINTER(C.c_double)]
    return oracle_lib


def is_contact(p):
    return p.contact_distance > 0.0 or p.contact_spring_coef != p.spring_coef


class OracleTile:
    """the oracle behind the tile interface of icebergs_amd.decomposed, for interacting bergs: the phases of a step, the migration
    calls of tests/test_decomposed.py and halo bergs -- the numpy selection above on the sending side, ko_unpack_bergs on the
    receiving one.  The oracle would step a halo row like any other and drop it only because it ends up outside the computational
    domain (and walk off its cell tables around a row on the rim of the data domain): here a halo row is pinned (static_berg = 1)
    while it is resident and taken out after the evolve, which is the contract of DESIGN 7.6."""
    NPL = 36

    def __init__(self, grid, p, bergs, with_halo_bergs=True):
        self.ol = _oracle_lib()
        self.o, self.b, self.params = self.ol.Oracle(grid, p), bergs, p
        d = grid["desc"]
        self.nic, self.njc = d.iec - d.isc + 1, d.jec - d.jsc + 1
        self.with_halo_bergs = with_halo_bergs
        self.halo_ids = []         # what arrived as halo rows, per update

    def _args(self):
        return C.byref(self.o.kg), C.byref(self.o.params), C.byref(self.o.soa(self.b))

    def zero_accumulators(self):
        self.o.acc[:] = 0.0

    def interp(self):
        self.o.lib.ko_interp_gridded_fields_to_bergs(*self._args())

    def set_conglom_ids(self):
        self.o.lib.ko_set_conglom_ids(*self._args(), None)

    def evolve(self):
        self.o.lib.ko_evolve_icebergs_interactive(*self._args(), None, self.ol._dp(self.o.scalars))
        m = self.b["_n"]
        halo = self.b["halo_berg"][:m] >= 0.5
        if halo.any():                                   # retired: they sit behind every owned row (nothing arrives between update and evolve)
            first = int(np.argmax(halo))
            assert halo[first:].all()
            self.b["_n"] = first

    def thermodynamics(self):
        self.o.lib.ko_thermodynamics(*self._args(), self.ol._dp(self.o.acc), self.ol._dp(self.o.scalars))

    def calculate_mass_on_ocean(self):
        self.o.lib.ko_calculate_mass_on_ocean(*self._args(), self.ol._dp(self.o.acc))

    def gather(self):
        self.o.step_gather()

    def pack_pair(self, axis):
        return self.o.send_bergs(self.b, 2 * axis), self.o.send_bergs(self.b, 2 * axis + 1)

    def unpack_pair(self, from_lo, from_hi):
        for recs in (from_lo, from_hi):
            m0 = self.b["_n"]
            assert self.o.unpack_bergs(self.b, recs) == 0
            m1 = self.b["_n"]
            halo = self.b["halo_berg"][m0:m1] >= 0.5
            self.b["static_berg"][m0:m1][halo] = 1.0
            if halo.any():
                self.halo_ids.append(self.b["id"][m0:m1][halo].copy())

    def pack_halo_bergs_pair(self, axis, width=0, sides=(True, True)):
        empty = np.empty((0, 34))
        if not self.with_halo_bergs:
            return empty, empty
        m = self.b["_n"]
        hi, lo = np_halo_select(self.b["ine"][:m], self.b["jne"][:m], self.b["alive"][:m], axis, width or H, self.nic, self.njc)
        recs = [np_records(self.b, rows, halo=1.0) for rows in (hi, lo)]
        for r, rows in zip(recs, (hi, lo)):             # a halo row sent on (axis 1) is pinned here; the record carries the berg's own static_berg
            r[:, 30] = np.where(self.b["halo_berg"][:m][rows] >= 0.5, 0.0, r[:, 30])
        return tuple(r if on else empty for r, on in zip(recs, sides))

    def halo_buffer_count(self, axis, width=1):
        return self.NPL * self.njc * width if axis == 0 else self.NPL * width * (self.nic + 2 * width)

    def pack_halo_pair(self, axis, width=1, sides=(True, True)):
        import test_halo_planes_cpu as HC
        hi, lo = HC.np_pack_halo_pair(self.o.acc, axis, width, self.NPL, self.nic, self.njc)
        return (hi if sides[0] else None), (lo if sides[1] else None)

    def unpack_halo_pair(self, axis, from_lo, from_hi, width=1):
        import test_halo_planes_cpu as HC
        HC.np_unpack_halo_pair(self.o.acc, axis, width, self.NPL, self.nic, self.njc, from_lo, from_hi)

    def live(self):
        m = self.b["_n"]
        a = (self.b["alive"][:m] != 0) & (self.b["halo_berg"][:m] < 0.5)
        return {k: self.b[k][:m][a].copy() for k in FIELDS + ("id", "ine", "jne")}


def tile_of(ine, jne):
    return (ine - 1) // NI, (jne - 1) // NJ


def _contact_pairs(b, reach):
    """pairs (berg, berg of another tile) closer than `reach`; how many of them sit on diagonal tiles"""
    a = np.nonzero(b["alive"] != 0)[0]
    x, y = b["lon"][a], b["lat"][a]
    tx, ty = tile_of(b["ine"][a], b["jne"][a])
    d2 = (x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2
    close = (d2 < reach * reach) & (d2 > 0.0)
    other = (tx[:, None] != tx[None, :]) | (ty[:, None] != ty[None, :])
    diag = (tx[:, None] != tx[None, :]) & (ty[:, None] != ty[None, :])
    return int((close & other).sum()), int((close & diag).sum())


_WHOLE = {}


def whole_oracle(contact):
    """the undivided oracle run, computed once per search and shared: {step: live bergs} at CHECK_AT, the five gathered outputs
    there, and what the population has to show -- contacts across tile edges, diagonal ones, migrations, nobody leaving the box"""
    if contact in _WHOLE:
        return _WHOLE[contact]
    ol = _oracle_lib()
    whole, b = population()
    p = params(contact)
    o = ol.Oracle(whole, p)
    n = len(b["lon"])
    b["_n"] = n
    t = OracleTile.__new__(OracleTile)
    t.ol, t.o, t.b, t.params = ol, o, b, p
    reach = max(2.0 * RADIUS * 1.05, p.contact_distance)
    stats = {"pairs": 0, "diag": 0, "migrations": 0, "left": 0}
    snaps, outs = {}, {}
    for step in range(1, NSTEPS + 1):
        pr, dg = _contact_pairs(b, reach)
        stats["pairs"] += pr
        stats["diag"] += dg
        before = tile_of(b["ine"].copy(), b["jne"].copy())
        t.zero_accumulators()
        if contact:
            t.set_conglom_ids()
        t.evolve()
        t.thermodynamics()
        t.calculate_mass_on_ocean()
        t.gather()
        after = tile_of(b["ine"], b["jne"])
        alive = b["alive"] != 0
        stats["migrations"] += int((alive & ((before[0] != after[0]) | (before[1] != after[1]))).sum())
        stats["left"] = n - int(alive.sum())
        if step in CHECK_AT:
            snaps[step] = t.live()
            outs[step] = o.out[:, H:H + NJ * NTY, H:H + NI * NTX].copy()
    _WHOLE[contact] = (snaps, outs, stats)
    return _WHOLE[contact]


def compare(got, want):
    """{field: largest deviation relative to the field's maximum} over the bergs of `want`, matched by id; the ids must agree"""
    assert len(np.unique(got["id"])) == len(got["id"]), "a berg is owned twice"
    o1, o2 = np.argsort(want["id"]), np.argsort(got["id"])
    assert np.array_equal(want["id"][o1], got["id"][o2]), "survivors differ"
    dev = {}
    for f in FIELDS:
        x, y = want[f][o1], got[f][o2]
        scale = float(np.abs(x).max())
        dev[f] = float(np.abs(x - y).max()) / scale if scale > 0.0 else float(np.abs(y).max())
    return dev


def join(parts):
    return {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
