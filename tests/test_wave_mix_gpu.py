"""Lanes that disagree inside one wave.  The per-berg kernels choose a code path for all 64 lanes from what any one lane holds:
interp_flds skips the interpolated rotation when no lane sits in a rotated cell (all_unrot), accel skips the sea-ice drag when no
lane has ice (any_ice) and the division of the wave-radiation factor when no lane is short (cr_q).  "Each lane's value is the same
either way" is a claim about arithmetic; the row-order tests run on config 2, where every cell is unrotated, there is no sea ice
and no berg is short, so no wave there ever disagrees.

Here 64 * 6 + 37 bergs on the curvilinear lat-lon patch (tests/curvilinear.py; the wind three times config 2's, so that a berg a
few metres long is shorter than a quarter of the wave length) come in six groups of 64:
    0 unrotated cell, open water, long      1 rotated, open water, long      2 unrotated, under ice, long
    3 unrotated, open water, short          4 rotated, under ice, short      5 rotated, under ice, long
and 37 more of the first kind.  Fourteen bergs of group 0 sit on the knife edge of cr_q: at the centre of cells whose corners carry
the same wind (8, 0) over a resting ocean, with L = 5.12 (1 + k 2^-52), k = 0 .. 13, so that cr_num is 0 to a few ulp above cr_den.
Order A hands the groups over one after the other (every full wave homogeneous: wave 0 takes all three short cuts), order B deals
them round-robin (every full wave holds all six kinds).  Four steps without re-binning, RK4 and Verlet: the per-berg fields matched
by id are bit for bit the same in A and B, and both runs are within the parity tolerances of the oracle.

The CPU test at the top shows, from the grid's corner cos / sin, the cells' hi and the lengths alone, that order B does mix the kinds
in every full wave and order A does not."""
import numpy as np
import pytest

from icebergs_amd import synthetic as S
import curvilinear as CV
import parity as P

NG, NW = 6, 64
N = NG * NW + 37
NSTEPS = 4
NKNIFE = 14
KNIFE_CELLS = [(i, j) for j in (7, 8, 9) for i in (39, 40, 41, 42, 43)][:NKNIFE]
KNIFE_WIND = 8.0
#        rotated, ice,   short
GROUPS = [(False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True), (True, True, False)]
PER_BERG = P.TRAJ_FIELDS + P.SIZE_FIELDS + P.ENV_FIELDS + ["ine", "jne"]
_case = {}


def grid():
    if "grid" not in _case:
        g = CV.patch_grid("latlon")
        d, f = g["desc"], g["forcing"]
        f["ua"] *= 3.0; f["va"] *= 3.0
        for (i, j) in KNIFE_CELLS:   # the four corners of every knife-edge cell: one wind, an ocean at rest
            for (ii, jj) in ((i - 1, j - 1), (i, j - 1), (i, j), (i - 1, j)):
                f["ua"][jj - d.jsd, ii - d.isd] = KNIFE_WIND
                for k in ("va", "uo", "vo"):
                    f[k][jj - d.jsd, ii - d.isd] = 0.0
        _case["grid"] = g
    return _case["grid"]


def _bilinear(a, ii, jj, xi, yj):
    return (a[jj, ii] * xi + a[jj, ii - 1] * (1.0 - xi)) * yj + (a[jj - 1, ii] * xi + a[jj - 1, ii - 1] * (1.0 - xi)) * (1.0 - yj)


def wmod_estimate(g, b):
    """|ua - uo|^2 where the berg sits, from the corner values in the grid's frame (a rotation keeps the length of a vector; the
    interpolated cos / sin shorten it by less than a percent here)"""
    d, f = g["desc"], g["forcing"]
    jj, ii = b["jne"] - d.jsd, b["ine"] - d.isd
    du = _bilinear(f["ua"] - f["uo"], ii, jj, b["xi"], b["yj"])
    dv = _bilinear(f["va"] - f["vo"], ii, jj, b["xi"], b["yj"])
    return du * du + dv * dv


def kinds(g, b):
    """(rotated, ice, short, sure) per berg: rotated as the packets' flag word says it (cos = 1, sin = 0 at the four corners or not),
    ice from the cell's hi, short / long with a factor 2 of margin around L = 0.25 * 0.32 * |ua - uo|^2 (sure: outside that margin)"""
    d = g["desc"]
    rot = (CV.flags_of(g, b) & 4) == 0
    ice = g["forcing"]["hi"][b["jne"] - d.jsd, b["ine"] - d.isd] > 0.0
    ltop = 0.25 * 0.32 * wmod_estimate(g, b)
    short = b["length"] < 0.5 * ltop
    sure = short | (b["length"] > 2.0 * ltop)
    return rot, ice, short, sure


def _cells_of(g, rotated, ice):
    d, st, f = g["desc"], g["static"], g["forcing"]
    flags = CV.cell_flags(g)
    out = []
    for j in range(CV.J_RANGE[0], 27):   # south of the tall band
        for i in range(CV.I_RANGE[0], CV.I_RANGE[1] + 1):
            jj, ii = j - d.jsd, i - d.isd
            wet = st["msk"][jj - 1:jj + 2, ii - 1:ii + 2].min() > 0.5
            hi = f["hi"][jj - 1:jj + 2, ii - 1:ii + 2]
            is_ice = hi.min() > 0.0 if ice else hi.max() == 0.0          # the cell and its neighbours alike: a berg may cross an edge
            fl = flags[jj - 1:jj + 2, ii - 1:ii + 2]
            is_rot = ((fl & 4) == 0).all() if rotated else ((fl & 4) != 0).all()
            if wet and is_ice and is_rot and (i, j) not in KNIFE_CELLS:
                out.append((i, j))
    return out


def population():
    """the bergs in group order (order A) and the group of every row"""
    if "a" in _case:
        return _case["a"], _case["group"]
    g = grid()
    d, st = g["desc"], g["static"]
    rng = np.random.Generator(np.random.PCG64(5))
    b = S.empty_bergs(N)
    group = np.concatenate([np.repeat(np.arange(NG), NW), np.zeros(N - NG * NW, dtype=np.int64)])
    xi, yj = rng.uniform(0.1, 0.9, N), rng.uniform(0.1, 0.9, N)
    S._fill_classes(b, rng.integers(0, 10, size=N))
    for q, (rotated, ice, short) in enumerate(GROUPS):
        cells = _cells_of(g, rotated, ice)
        assert len(cells) >= 4, (q, len(cells))
        cells = [cells[k] for k in rng.permutation(len(cells))[:8]]
        rows = np.flatnonzero(group == q)
        for n, r in enumerate(rows):
            b["ine"][r], b["jne"][r] = cells[n % len(cells)]
    knife = np.flatnonzero(group == 0)[:NKNIFE]
    for k, r in enumerate(knife):
        b["ine"][r], b["jne"][r] = KNIFE_CELLS[k]
        xi[r] = yj[r] = 0.5
    jj, ii = b["jne"] - d.jsd, b["ine"] - d.isd
    for name in ("lon", "lat"):
        b[name][:] = _bilinear(st[name], ii, jj, xi, yj)
    b["xi"][:], b["yj"][:] = xi, yj
    # the short bergs: 0.3 of a quarter of the wave length where they sit; the knife edge: L = 5.12 (1 + k 2^-52)
    ltop = 0.25 * 0.32 * wmod_estimate(g, b)
    L = b["length"].copy()
    for q, (_, _, short) in enumerate(GROUPS):
        if short:
            rows = group == q
            L[rows] = 0.3 * ltop[rows]
    L[knife] = (0.25 * (0.32 * (KNIFE_WIND * KNIFE_WIND))) * (1.0 + np.arange(NKNIFE) * 2.0 ** -52)
    small = L != b["length"]
    W = np.where(small, L / 1.5, b["width"]); Tk = np.where(small, np.minimum(W, 2.0), b["thickness"])
    b["length"][:], b["width"][:], b["thickness"][:] = L, W, Tk
    b["mass"][:] = np.where(small, S.RHO_BERGS * Tk * W * L, b["mass"])
    b["mass_scaling"][small] = 1.0
    b["start_mass"][:] = b["mass"]
    b["start_lon"][:], b["start_lat"][:] = b["lon"], b["lat"]
    b["start_year"][:] = 0
    b["start_day"][:] = 1.0e-6 * np.arange(N)
    b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"]
    _case["a"], _case["group"], _case["knife"] = b, group, knife
    return b, group


def _take(b, rows):
    return {k: (np.ascontiguousarray(v[rows]) if hasattr(v, "dtype") else v) for k, v in b.items()}


def order_b():
    """round-robin over the six groups; the 37 extra rows stay behind them"""
    full = NG * NW
    return np.concatenate([np.arange(full).reshape(NG, NW).T.ravel(), np.arange(full, N)])


def test_order_b_mixes_every_kind_in_every_wave_and_order_a_does_not():
    g = grid()
    a, group = population()
    rot, ice, short, sure = kinds(g, a)
    knife = _case["knife"]
    assert sure[np.setdiff1d(np.arange(N), knife)].all()          # short or long by a factor of two, the knife edge apart
    for q, (r, i, s) in enumerate(GROUPS):
        rows = np.setdiff1d(np.flatnonzero(group[:NG * NW] == q), knife)
        assert (rot[rows] == r).all() and (ice[rows] == i).all() and (short[rows] == s).all(), q
    # the knife edge, with the wind's square at its nominal 64: unrotated rectangular cells in open water, cr_num from 0 to a few ulp
    # above cr_den
    assert (CV.flags_of(g, _take(a, knife)) == 7).all() and not ice[knife].any() and not rot[knife].any()
    wm = KNIFE_WIND * KNIFE_WIND
    lcut, ltop = 0.125 * (0.32 * wm), 0.25 * (0.32 * wm)
    num, den = a["length"][knife] - lcut, (ltop - lcut) + 1.0e-30
    assert (num >= den).all() and num[0] == den and ((num - den) / den <= 32 * 2.0 ** -52).all() and len(np.unique(num)) >= 8
    for name, rows in (("A", np.arange(N)), ("B", order_b())):
        for w in range(NG):
            lanes = rows[w * NW:(w + 1) * NW]
            lanes = lanes[~np.isin(lanes, knife)]
            mixed = [bool(v[lanes].any() and not v[lanes].all()) for v in (rot, ice, short)]
            assert mixed == ([False] * 3 if name == "A" else [True] * 3), (name, w, mixed)
    # order A, wave 0 takes all three short cuts (with the knife-edge lanes in it, none of them short)
    assert not rot[:NW].any() and not ice[:NW].any() and not short[:NW].any()
    assert sorted(order_b().tolist()) == list(range(N))
    assert np.array_equal(np.sort(a["id"]), np.arange(1, N + 1))


def _params(verlet):
    p = CV.patch_params("latlon")
    if verlet:
        p.Runge_not_Verlet = 0
    return p


def _lib_run(g, p, b):
    from icebergs_amd.framework import Icebergs
    ib = Icebergs(g, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.set_resort_interval(0)
        ib.run(NSTEPS)
        acc, out, scal = ib.fetch()
        return ib.download_bergs(), acc.copy(), out.copy(), scal.copy()
    finally:
        ib.close()


def _by_id(b):
    live = np.flatnonzero(b["alive"] != 0)
    o = live[np.argsort(b["id"][live], kind="stable")]
    return {f: b[f][o] for f in PER_BERG + ["id"]}


@pytest.mark.gpu
@pytest.mark.parametrize("verlet", [False, True])
def test_a_bergs_bits_do_not_depend_on_its_wave_mates(oracle, verlet):
    g, p = grid(), _params(verlet)
    a, _ = population()
    b = _take(a, order_b())
    ref = P.run_oracle(g, p, S.sort_reference_order(S.copy_bergs(a)), NSTEPS)
    runs = {}
    for name, bergs in (("A", a), ("B", b)):
        got = _lib_run(g, p, bergs)
        if name == "A":
            assert np.array_equal(got[0]["id"][:N], a["id"])       # no re-binning: the rows stay where they were handed over
        rep = P.compare(ref, got, "wave mix/%s/order %s" % ("verlet" if verlet else "rk4", name), params=p)
        print(name, {f: "%.1e" % rep[f] for f in P.TRAJ_FIELDS + ["mass"]})
        runs[name] = _by_id(got[0])
    assert len(runs["A"]["id"]) >= N - 8                            # (a short berg may melt away; nearly all are still there)
    for f in PER_BERG + ["id"]:
        bad = np.flatnonzero(runs["A"][f] != runs["B"][f])
        assert bad.size == 0, (f, runs["A"]["id"][bad][:8], runs["A"][f][bad][:4], runs["B"][f][bad][:4])
