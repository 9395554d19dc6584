"""Geometry, population and reference runs of the north-fold tests (tests/test_north_fold_cpu.py,
tests/test_north_fold_gpu.py): a fold that can be unfolded.

  The folded grid F has NI x NJ cells of 5 km (grid_is_latlon = 0, grid_is_regular = 0).  Its left half, columns 1 .. NI/2, is
  an ordinary Cartesian block; its right half is the same kind of block turned by 180 degrees and set on top of the left one:
  corner (i, j) with i >= NI/2 lies at x = (NI - i) dx, y = (2 NJ - j) dy and carries cos = -1, sin = 0 (a 180 degree turn
  keeps the corner order counter-clockwise).  Corner column NI/2 takes the left half's values, so cell column NI/2 + 1 is
  twisted (the pivot); it and column NI/2 are land.  The rows of the data domain above NJ are filled by the fold: cell fields
  from cell (NI+1-i, NJ+1-k), corner fields from corner (NI-i, NJ-k), cos and grid-oriented vector components with their sign
  turned.

  The unfolded grid U has NI/2 x 2 NJ cells, plain Cartesian with the same flags: cell (i, j) of F with i > NI/2 is cell
  (NI+1-i, 2 NJ+1-j) of U, and all of F's arrays are U's analytic fields taken through this map.  A run on F with the fold is
  the undivided run on U, which needs no fold, no halo update and no migration: the oracle runs it as it stands.  The 9-point
  sum pairs its terms in another index order in the turned half, so the two agree to rounding, not to the bit.

  Bergs: N_BERGS non-interacting bergs of the ten calving classes in columns 3 .. 5 of U, drifting north at 0.1 to 0.3 m/s.
  SEED was chosen with the oracle on U alone (whole_oracle): with Verlet 48 bergs cross the line y = NJ dy and at least 100 sit
  in the two rows either side of it at every step, with RK4 49 and 101; none comes within two cells of the pivot columns or of the
  box's outer edges, none leaves the box or melts away.  whole_oracle asserts these conditions on every run.

Test infrastructure."""
import ctypes as C
import math
import os
import queue
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from icebergs_amd import synthetic as S   # noqa: E402
from icebergs_amd import types as T       # noqa: E402
import test_halo_planes_cpu as HC         # noqa: E402  (OracleTile with the numpy halo update, assemble, deviations)

H = S.HALO
NI, NJ, RES = 16, 6, 5000.0
HALF = NI // 2
NSTEPS, DT = 40, 600.0
N_BERGS, SEED = 300, 5
CHECK_AT = (1, 20, 40)
LAYOUTS = (1, 2, 4)                        # ntx of the ntx x 1 layouts: tiles of 16, 8 and 4 columns
A0 = T.ENUMS["KID_A_MASS_ON_OCEAN"]
FIELDS = ("lon", "lat", "uvel", "vvel", "axn", "ayn", "bxn", "byn", "xi", "yj", "mass", "thickness", "width", "length",
          "mass_of_bits", "heat_density", "start_mass", "mass_scaling")
W_INE, W_JNE = 23, 24     # 0-based words of the wire record (pack_berg_into_buffer2, FW:3268-3301)


# ---- the fold of the on-ocean planes restated with numpy ----
def np_fold_halo(strip, w, npl, nic, swap_slots):
    """what the rows njc+1 .. njc+w, columns 1-w .. nic+w of a tile hold after the fold update, from the strip its mirror partner
    packed for the north (rows njc-w+1 .. njc, columns 1-w .. nic+w of the partner; element order plane, row, column), as
    (npl, w, nic + 2 w) with the first row njc+1.  Written from the rule of the message layer for a centred scalar on a folded
    north edge, halo(i, nj+k) = field(ni+1-i, nj+1-k) -- on tiles of one width the partner's local column is nic+1-i -- and
    from the exchange of the nine slots IB:6117-6120."""
    field = np.asarray(strip).reshape(npl, w, nic + 2 * w)      # field[:, r, c]: partner row njc-w+1+r, partner column 1-w+c
    halo = np.empty_like(field)
    for k in range(1, w + 1):                                   # my row njc+k <- partner row njc+1-k ...
        src_row = w - k                                         # ... whose place in the strip is (njc+1-k) - (njc-w+1)
        for c in range(nic + 2 * w):                            # my column i = 1-w+c <- partner column nic+1-i
            i = 1 - w + c
            halo[:, k - 1, c] = field[:, src_row, (nic + 1 - i) - (1 - w)]
    if swap_slots:
        for g in range(npl // 9):                               # var_on_ocean(i, j, 9) <-> (.., 1), 8 <-> 2, 7 <-> 3, 6 <-> 4
            for a, b in ((9, 1), (8, 2), (7, 3), (6, 4)):
                tmp = halo[9 * g + a - 1].copy()
                halo[9 * g + a - 1] = halo[9 * g + b - 1]
                halo[9 * g + b - 1] = tmp
    return halo


def np_unpack_halo_fold(acc, w, npl, nic, njc, from_fold, swap_slots):
    acc[A0:A0 + npl, H + njc:H + njc + w, H - w:H + nic + w] = np_fold_halo(from_fold, w, npl, nic, swap_slots)


# ---- geometry: everything of F is U's analytic field taken through the map ----
def _corner_map(i, j):
    """corner (i, j) of F's data domain -> (x, y) in U's frame and the sign of cos there"""
    over = j > NJ                                    # beyond the fold: corner (NI-i, NJ-k), k = j - NJ
    ii, jj = np.where(over, NI - i, i), np.where(over, 2 * NJ - j, j)
    left = ii <= HALF                                # (corner column NI/2 takes the left half's values)
    x = RES * np.where(left, ii, NI - ii)
    y = RES * np.where(left, jj, 2 * NJ - jj)
    sgn = np.where(left, 1.0, -1.0) * np.where(over, -1.0, 1.0)
    return x, y, sgn


def _cell_map(i, j):
    """cell (i, j) of F's data domain -> the cell (iu, ju) of U it is"""
    over = j > NJ                                    # beyond the fold: cell (NI+1-i, NJ+1-k)
    ii, jj = np.where(over, NI + 1 - i, i), np.where(over, 2 * NJ + 1 - j, j)
    left = ii <= HALF
    return np.where(left, ii, NI + 1 - ii), np.where(left, jj, 2 * NJ + 1 - jj)


def _corner_fields(x, y):
    """U's analytic corner fields (geographic components): a gale from the south and sea ice moving north carry the bergs
    north, with some shear.  The ocean is at rest: ustar_iceberg takes the grid-oriented ocean velocity at the corner (i, j)
    from the geographic spread velocity of cell (i, j) (IB:3470-3474), which depends on the frame and on which corner the index
    names, so with a current the turned half of F would not be U's for that one output, fold or no fold."""
    return {"uo": 0.0 * x, "vo": 0.0 * x,
            "ua": 0.8 * np.cos(y / 11000.0), "va": 8.0 + 1.0 * np.sin(x / 6000.0),
            "ui": 0.05 * np.sin(x / 8000.0), "vi": 0.3 + 0.05 * np.cos(y / 10000.0)}


def _cell_fields(xc, yc):
    return {"ssh": 0.002 * np.sin(xc / 9000.0) * np.cos(yc / 13000.0), "sst": 1.0 + 0.8 * np.sin(xc / 8000.0) * np.cos(yc / 12000.0),
            "sss": 34.0 + 0.0 * xc, "cn": 0.3 + 0.1 * np.sin(yc / 15000.0), "hi": 0.5 + 0.2 * np.cos(xc / 10000.0)}


def _fill(grid, x, y, sgn, iu, ju):
    st, f = grid["static"], grid["forcing"]
    one = np.ones_like(x)
    xc, yc = RES * (iu - 0.5), RES * (ju - 0.5)
    st["lon"], st["lat"], st["lonc"], st["latc"] = x * one, y * one, xc * one, yc * one
    st["dx"], st["dy"], st["area"], st["ocean_depth"] = RES * one, RES * one, RES * RES * one, 1000.0 * one
    st["cos"], st["sin"] = sgn * one, 0.0 * one
    st["msk"] = np.where(iu == HALF, 0.0, 1.0) * one
    for k in f:
        f[k] = 0.0 * one
    for k, v in _corner_fields(x, y).items():
        f[k] = sgn * v * one                         # grid-oriented: turned where the grid is
    for k, v in _cell_fields(xc, yc).items():
        f[k] = v * one
    for group in (st, f):
        for k in group:
            group[k] = np.ascontiguousarray(group[k], dtype=np.float64)
    return grid


def _ij(d):
    i, j = S._ij(d)
    one = S.zeros(d) + 1.0
    return (i * one).astype(np.int64), (j * one).astype(np.int64)


def unfolded_grid():
    g = S.cartesian_grid(ni=HALF, nj=2 * NJ, gridres=RES)
    g["desc"].grid_is_regular = 0
    i, j = _ij(g["desc"])
    return _fill(g, RES * i, RES * j, np.ones(i.shape), i, j)


def folded_grid():
    g = S.cartesian_grid(ni=NI, nj=NJ, gridres=RES)
    g["desc"].grid_is_regular = 0
    i, j = _ij(g["desc"])
    x, y, sgn = _corner_map(i, j)
    iu, ju = _cell_map(i, j)
    return _fill(g, x, y, sgn, iu, ju)


def tile_grid(tx, ntx, whole=None):
    """tile tx of the ntx x 1 layout of F: slices of the whole grid's arrays, the data domain with its fold rows included"""
    whole = folded_grid() if whole is None else whole
    nic = NI // ntx
    g = S.cartesian_grid(ni=nic, nj=NJ, gridres=RES)
    g["desc"].grid_is_regular = 0
    for group in ("static", "forcing"):
        for k, v in whole[group].items():
            g[group][k] = np.ascontiguousarray(v[:, tx * nic:tx * nic + nic + 2 * H])
    return g


def params(rk):
    """non-interacting bergs, melt on, add_weight_to_ocean, the rectangular (old) spreading, every diagnostic; no Coriolis term
    (an f-plane at the equator), so that the drift stays in its three columns"""
    p = S.set_diag_all(S.default_params())
    p.dt, p.lat_ref, p.use_f_plane = DT, 0.0, 1
    if not rk:
        p.Runge_not_Verlet, p.use_new_predictive_corrective, p.old_interp_flds_order = 0, 1, 0
    assert p.add_weight_to_ocean and not p.hexagonal_icebergs and not p.set_melt_rates_to_zero
    return p


def population(seed=SEED):
    """bergs on U (U's cell indices), moving with the current"""
    rng = np.random.default_rng(seed)
    n = N_BERGS
    x, y = rng.uniform(12000.0, 23000.0, n), rng.uniform(11000.0, 39000.0, n)
    b = S.empty_bergs(n)
    b["lon"][:], b["lat"][:] = x, y
    b["ine"][:] = np.floor(x / RES).astype(np.int32) + 1
    b["jne"][:] = np.floor(y / RES).astype(np.int32) + 1
    b["xi"][:] = x / RES - (b["ine"] - 1)
    b["yj"][:] = y / RES - (b["jne"] - 1)
    S._fill_classes(b, rng.integers(0, 10, size=n), jitter=rng.uniform(0.9, 1.1, n))
    b["uvel"][:], b["vvel"][:] = 0.01, 0.30
    for f in ("uvel_old", "uvel_prev"):
        b[f][:] = b["uvel"]
    for f in ("vvel_old", "vvel_prev"):
        b[f][:] = b["vvel"]
    b["lon_old"][:], b["lat_old"][:] = x, y
    b["start_lon"][:], b["start_lat"][:] = x, y
    b["start_year"][:] = 1
    b["start_day"][:] = 1.0e-6 * np.arange(n)
    return S.sort_reference_order(b)


def to_folded(b):
    """the bergs of U with F's cell indices: a berg above the fold line sits in the turned half, its in-cell position counted
    from the opposite corner"""
    f = S.copy_bergs(b)
    over = b["jne"] > NJ
    f["ine"] = np.where(over, NI + 1 - b["ine"], b["ine"]).astype(np.int32)
    f["jne"] = np.where(over, 2 * NJ + 1 - b["jne"], b["jne"]).astype(np.int32)
    f["xi"] = np.where(over, 1.0 - b["xi"], b["xi"])
    f["yj"] = np.where(over, 1.0 - b["yj"], b["yj"])
    return f


def split_bergs(bf, tx, ntx, cap):
    return HC.split_bergs(bf, tx, 0, NI // ntx, NJ, cap=cap)


def trim(b):
    m = b["_n"]
    return {k: (v[:m].copy() if isinstance(v, np.ndarray) else v) for k, v in b.items() if k != "_n"}


def out_to_unfolded(out_f):
    """(5, NJ, NI) of F's computational domain -> (5, 2 NJ, NI/2) of U's"""
    return np.concatenate([out_f[:, :, :HALF], out_f[:, ::-1, ::-1][:, :, :HALF]], axis=1)


def live_unfolded(b, tx, ntx, n=None):
    """the live bergs of a tile of F with their in-cell position counted as U counts it"""
    n = int(b.get("_n", len(b["lon"]))) if n is None else n
    a = (b["alive"][:n] != 0)
    out = {k: b[k][:n][a].copy() for k in FIELDS + ("id",)}
    turned = b["ine"][:n][a] + tx * (NI // ntx) > HALF
    out["xi"] = np.where(turned, 1.0 - out["xi"], out["xi"])
    out["yj"] = np.where(turned, 1.0 - out["yj"], out["yj"])
    return out


def compare(got, want):
    """{field: largest deviation relative to the field's maximum} over the bergs of `want`, matched by id; the same survivors,
    every id owned once"""
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


def total_mass(b):
    """sum of berg mass with every kind of bits, times mass_scaling, over the live bergs"""
    a = b["alive"] != 0
    return math.fsum((b["mass"][a] + b["mass_of_bits"][a] + b["mass_of_fl_bits"][a] + b["mass_of_fl_bergy_bits"][a]) * b["mass_scaling"][a])


# ---- the oracle ----
def _oracle_lib():
    import oracle_lib
    oracle_lib.build()
    lib = oracle_lib.load()
    lib.ko_calculate_mass_on_ocean.restype = None
    lib.ko_calculate_mass_on_ocean.argtypes = [C.POINTER(oracle_lib.KoGrid), C.POINTER(T.Params), C.POINTER(T.BergSoA), C.POINTER(C.c_double)]
    return oracle_lib


class OracleTile(HC.OracleTile):
    """the oracle behind the tile interface with the numpy fold above"""

    def __init__(self, grid, p, bergs):
        _oracle_lib()
        super().__init__(grid, p, bergs)
        self.fold_calls = 0

    def comp_domain(self):
        d = self.o.grid["desc"]
        return d.isc, d.iec, d.jsc, d.jec

    def unpack_halo_fold(self, from_fold, width=1, swap_slots=True):
        self.fold_calls += 1
        np_unpack_halo_fold(self.o.acc, width, self.NPL, self.nic, self.njc, from_fold, swap_slots)

    def fold_halo_self(self, width=1, swap_slots=True):
        hi, _ = HC.np_pack_halo_pair(self.o.acc, 1, width, self.NPL, self.nic, self.njc)
        self.unpack_halo_fold(hi, width, swap_slots)


_WHOLE = {}


def whole_oracle(rk):
    """the undivided oracle run on U, computed once per scheme and shared: {step: live bergs} and the five outputs at CHECK_AT, what
    the population shows, and the oracle's own relative gap between sum(spread_mass area) and the bergs' mass.  Asserts the
    conditions the seed was chosen for."""
    if rk in _WHOLE:
        return _WHOLE[rk]
    ol = _oracle_lib()
    g, b, p = unfolded_grid(), population(), params(rk)
    o = ol.Oracle(g, p)
    n = len(b["lon"])
    snaps, outs, gaps = {}, {}, {}
    crossed, near_min = 0, n
    area = g["static"]["area"][H:H + 2 * NJ, H:H + HALF]
    k_mass = T.ENUMS["KID_O_SPREAD_MASS"]
    for step in range(1, NSTEPS + 1):
        above = b["lat"] > NJ * RES
        o.run_step(b, 1)
        alive = b["alive"] != 0
        crossed += int((alive & (above != (b["lat"] > NJ * RES))).sum())
        near_min = min(near_min, int((alive & (b["jne"] >= NJ) & (b["jne"] <= NJ + 1)).sum()))
        inside = (b["ine"] >= 3) & (b["ine"] <= HALF - 3) & (b["jne"] >= 3) & (b["jne"] <= 2 * NJ - 2)
        assert inside[alive].all(), "a berg came within two cells of the pivot column or of the outer edges (step %d)" % step
        assert (alive | inside).all(), "a berg left the box"
        m = total_mass(b)
        gaps[step] = abs(math.fsum((o.out[k_mass, H:H + 2 * NJ, H:H + HALF] * area).reshape(-1)) - m) / m     # at every step
        if step in CHECK_AT:
            snaps[step] = live_unfolded(dict(b, _n=n), 0, 1)      # (U's indices: nothing is turned)
            snaps[step]["xi"], snaps[step]["yj"] = b["xi"][alive].copy(), b["yj"][alive].copy()
            outs[step] = o.out[:, H:H + 2 * NJ, H:H + HALF].copy()
    stats = {"crossed": crossed, "near_min": near_min, "alive": int((b["alive"] != 0).sum())}
    assert crossed >= 20 and near_min >= 10, stats
    _WHOLE[rk] = (snaps, outs, stats, gaps)
    return _WHOLE[rk]


# ---- ranks as threads of one process: what TileExchange needs of torch.distributed ----
class _Work:
    def __init__(self, fn):
        self.fn = fn

    def wait(self):
        self.fn()


class ThreadDist:
    """one object per rank; messages are copies in per-pair queues, matched in the order they were posted (as the ranks of
    one gloo pair are).  One rank computes at a time: a rank holds the shared lock except while it waits for a message (the
    oracle library keeps some state in globals)."""
    TIMEOUT = 120.0   # a safety net only: a message that never comes fails the test instead of hanging it

    class P2POp:
        def __init__(self, op, tensor, peer):
            self.op, self.tensor, self.peer = op, tensor, peer

    def __init__(self, rank, world, boxes, lock):
        self.rank, self.world, self.boxes, self.lock = rank, world, boxes, lock

    @classmethod
    def make(cls, world):
        boxes = {(s, d): queue.Queue() for s in range(world) for d in range(world)}
        lock = threading.Lock()
        return [cls(r, world, boxes, lock) for r in range(world)]

    def _take(self, tensor, peer):
        self.lock.release()
        try:
            got = self.boxes[(peer, self.rank)].get(timeout=self.TIMEOUT)
        finally:
            self.lock.acquire()
        tensor.copy_(got)

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def isend(self, tensor, peer):
        self.boxes[(self.rank, peer)].put(tensor.clone())
        return _Work(lambda: None)

    def irecv(self, tensor, peer):
        return _Work(lambda: self._take(tensor, peer))

    def batch_isend_irecv(self, ops):
        return [op.op(op.tensor, op.peer) for op in ops]


def run_ranks(world, fn):
    """fn(rank, dist) on one thread per rank; returns the results in rank order, the first exception re-raised"""
    dists = ThreadDist.make(world)
    res, err = [None] * world, []

    def body(r):
        with dists[r].lock:
            try:
                res[r] = fn(r, dists[r])
            except BaseException as e:   # noqa: BLE001
                err.append(e)
    if world == 1:
        body(0)
    else:
        threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    if err:
        raise err[0]
    return res


def step_tiles(ntx, make_tile, nsteps, fold_north=True, check_at=CHECK_AT, after_step=None, snapshot=None):
    """ntx x 1 tiles of F through TileExchange.step, ranks as threads.  make_tile(tx) -> tile; snapshot(tile, tx) -> whatever the
    caller wants kept at the steps of check_at; after_step(tile, tx, ex, step) is called after every step.  Returns per rank
    ({step: snapshot}, sent, received)."""
    from icebergs_amd.decomposed import TileExchange

    def rank_body(r, dist):
        tile = make_tile(r)
        ex = TileExchange(ntx, 1, dist, fold_north=fold_north)
        snaps = {}
        for step in range(1, nsteps + 1):
            ex.step(tile)
            if after_step is not None:
                after_step(tile, r, ex, step)
            if step in check_at:
                snaps[step] = snapshot(tile, r)
        return snaps, ex.sent, ex.received, tile
    return run_ranks(ntx, rank_body)
