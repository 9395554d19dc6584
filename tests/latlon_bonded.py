"""Bonded, DEM, MTS and interacting bergs on lat-lon grids ("Bonded bergs on lat-lon grids"; tests/test_latlon_bonded_cpu.py,
tests/test_latlon_bonded_gpu.py): the element patterns of synthetic.config_c4 mapped onto synthetic.latlon_grid, so that the
lat-lon branches of the pair metric (cos of the pair's mean latitude times Rearth), of the Coriolis parameter, of the Verlet
position and velocity maps (metres to degrees, the tangent plane above 89 degrees) and of the depth interpolation under the
sub-steps (calc_xiyj off a regular Cartesian grid, the polar form above 89.999) are run by both sides of a comparison.
Test infrastructure: builders and rules, no HIP.

Construction of a case: config_c4's parameters and metre pattern; a grid of 45 x 45 cells of 0.05 degrees of latitude and
0.05 / cos(lat_c) degrees of longitude (about 5.5 km both ways at the conglomerate); the pattern's centre (the middle of its
bounding box) goes to (lon_c, lat_c), an element at (x, y) metres from it to lat = lat_c + y / (Rearth pi/180),
lon = lon_c + x / (Rearth pi/180 cos lat); cells and in-cell coordinates from the grid; rows in reference order; bonds from the
METRE pattern in that row order (a bond lists its partner by id, a berg's bonds by increasing partner row).  The sub-step stays
config 4's 18 s (dt / mts_sub_steps = 1800 / 100): a longer one destroys every bond.

A position is stored in degrees: one ulp of a latitude near 70 is 1.6e-9 m, of a longitude near 300 is 6e-9 m x cos, under
springs of 1e9 N/m.  The comparison is therefore much worse conditioned than on the Cartesian grid, and the tolerance of a field
is not a constant but max(compare_mts's, 10 x the oracle's own spread under one-ulp changes of the initial positions) -- spread()
and tolerances() below; the CPU tests hold every case to a cap on that spread and to a control four orders above it.
"""
import numpy as np

from icebergs_amd import synthetic as S
import parity as P

NI = NJ = 45
DLAT = 0.05
SPREAD_RUNS = 8          # oracle runs with every initial lon / lat one ulp up or down, default_rng(100 + s)
SPREAD_FACTOR = 10.0     # the spread comes from ONE perturbation of the initial state; the device rounds differently on every sub-step
SPREAD_CAP = 100.0       # 10 x spread <= 100 x today's tolerance, or the case is too ill-conditioned to test anything
CONTROL_REL = 1.0e-5     # the controls: a metric wrong by this much
STRONG = (1.0e7, 1.0e7)  # fracture thresholds (Pa) nothing in these runs comes near

_TWO = dict(two_bergs=True, hexagonal=False, nx=4, ny=6)
_FAR = (150.0e3, 150.0e3)   # config 4's way of having no seamount: 100 km from the elements (metres of the pattern)

# name: (config_c4 keywords, lon_c, lat_c, cell of the grid that holds (lon_c, lat_c), seamount offset from the centre in metres or
# None, forcing, steps).  HEX_FRACTURE's thresholds and seamount were searched on the oracle (test_latlon_bonded_cpu.py holds the conditions).
CASES = {
    "two_bergs_70S": (dict(frac=STRONG, **_TWO), 300.0, -70.0, (23, 23), None, "c4", 5),
    "hex_grounded_60S": (dict(frac=STRONG), 300.0, -60.0, (23, 23), (7.5e3, 7.5e3), "c4", 6),
    "hex_fracture": (dict(frac=(5.0e4, 2.5e4)), 300.0, -60.0, (23, 23), (7.0e3, 7.0e3), "c4", 6),
    "mts_kid_70S": (dict(dem=False, explicit_inner=False, spring_coef=1.0e-5, sub_steps=20), 300.0, -70.0, (23, 23), None, "c4", 6),
    "sts_two_bergs_70S": (dict(dem=False, mts=False, contact=True, spring_coef=1.0e-5, dt=60.0, **_TWO), 300.0, -70.0, (23, 23), None, "c4", 40),
    "polar_89N": (dict(frac=STRONG, **_TWO), 1.0, 89.01, (23, 30), None, "c4", 2),
    "c2_forcing_60S": (dict(frac=STRONG, **_TWO), 300.0, -60.0, (23, 23), None, "c2", 4),
    # four elements on the Stern springs (the DEM bonds at this latitude are beyond the cap on the spread) in cells 6 degrees wide
    # whose depth stencil reaches the row of centres at 89.9995; the seamount makes od depend on the form of the map
    "polar_depth": (dict(dem=False, explicit_inner=False, spring_coef=1.0e-5, sub_steps=20, hexagonal=False, nx=2, ny=2), 1.0, 89.9495, (23, 40),
                    (1.0e3, 1.0e3), "c4", 2, dict(dlon=6.0)),
}
EXCLUDED = {}            # name: reason -- none: every case of the list passes the admissibility conditions
NAMES = tuple(CASES)


def _seamount(grid, p, lon_b, lat_b, bump_depth=50.0, cw=5.0e3):
    """config 4's Gaussian seamount (1000 m of water, bump_depth over the top, 5 km wide) around (lon_b, lat_b), distances in metres"""
    st = grid["static"]
    rad = np.pi / 180.0
    dx = (st["lonc"] - lon_b) * (p.Rearth * rad) * np.cos(st["latc"] * rad)
    dy = (st["latc"] - lat_b) * (p.Rearth * rad)
    st["ocean_depth"][:] = 1000.0 - (1000.0 - bump_depth) * np.exp(-(dx * dx + dy * dy) / (2.0 * cw * cw))


def to_degrees(p, lon_c, lat_c, x, y):
    """an element (x, y) metres from the centre: (lon, lat)"""
    m = p.Rearth * np.pi / 180.0
    lat = lat_c + y / m
    return lon_c + x / (m * np.cos(lat * np.pi / 180.0)), lat


def locate(grid, b):
    """ine, jne, xi, yj of every row from the (rectangular) cells of a synthetic.latlon_grid, as place_bergs has them"""
    d, st = grid["desc"], grid["static"]
    lon1d, lat1d = st["lon"][0], st["lat"][:, 0]
    ine = (np.searchsorted(lon1d, b["lon"], side="right") + d.isd).astype(np.int32)   # lon(ine - 1) <= lon < lon(ine)
    jne = (np.searchsorted(lat1d, b["lat"], side="right") + d.jsd).astype(np.int32)
    assert np.all((ine >= d.isc) & (ine <= d.iec) & (jne >= d.jsc) & (jne <= d.jec)), "an element lies outside the computational domain"
    lon0, lon1 = lon1d[ine - 1 - d.isd], lon1d[ine - d.isd]
    lat0, lat1 = lat1d[jne - 1 - d.jsd], lat1d[jne - d.jsd]
    b["ine"][:], b["jne"][:] = ine, jne
    b["xi"][:] = (b["lon"] - lon0) / (lon1 - lon0)
    b["yj"][:] = (b["lat"] - lat0) / (lat1 - lat0)


def latlon_patch(p, lon_c, lat_c, cell, ni=NI, nj=NJ, dlat=DLAT, dlon=None):
    """the grid: (lon_c, lat_c) is the middle of cell `cell`"""
    dlon = dlat / np.cos(lat_c * np.pi / 180.0) if dlon is None else dlon
    return S.latlon_grid(ni=ni, nj=nj, lon0=lon_c - dlon * (cell[0] - 0.5), dlon=dlon, lat0=lat_c - dlat * (cell[1] - 0.5), dlat=dlat,
                         Rearth=p.Rearth)


def build(kw, lon_c, lat_c, cell, bump, forcing, nsteps, grid_kw=None):
    kw, grid_kw = dict(kw), dict(grid_kw or {})
    kw.setdefault("sub_steps", 100)
    kw.setdefault("bump", _FAR)
    _, p, b, _ = S.config_c4(**kw)
    S.set_diag_all(p)
    radius = kw.get("radius", 1500.0)
    grid = latlon_patch(p, lon_c, lat_c, cell, **grid_kw)
    assert p.Rearth == 6.36e6                     # latlon_grid's own: one Rearth on both sides
    x, y = b["lon"].copy(), b["lat"].copy()       # the metre pattern
    x -= 0.5 * (x.min() + x.max())
    y -= 0.5 * (y.min() + y.max())
    b["lon"][:], b["lat"][:] = to_degrees(p, lon_c, lat_c, x, y)
    for f in ("lon_old", "start_lon"):
        b[f][:] = b["lon"]
    for f in ("lat_old", "start_lat"):
        b[f][:] = b["lat"]
    locate(grid, b)
    b["n_bonds"][:] = 0
    b["_x"], b["_y"] = x, y                       # sorted with the rows
    b = S.sort_reference_order(b)
    x, y = b.pop("_x"), b.pop("_y")
    n = len(x)
    bd = S.bond_neighbours({"lon": x, "lat": y, "id": b["id"], "n_bonds": b["n_bonds"]}, n, 2.0 * radius * 1.05, p.max_bonds)
    f = grid["forcing"]
    if forcing == "c2":                           # gradients for interp_flds under MTS, melt from the SST
        S.c2_forcing(grid)
    else:                                         # config 4's uniform flow
        f["uo"][:], f["vo"][:], f["sst"][:], f["sss"][:] = 0.1, 0.1, -1.0, 34.0
    grid["static"]["ocean_depth"][:] = 1000.0
    if bump is not None:
        _seamount(grid, p, *to_degrees(p, lon_c, lat_c, bump[0], bump[1]))
    return grid, p, b, bd, nsteps


def case(name):
    """(grid, params, bergs, bonds, nsteps)"""
    return build(*CASES[name])


# ---- the oracle's own spread, and the tolerances it gives ----
def run_oracle(c, rearth_params=1.0, rearth_grid=1.0, perturb=None):
    """the oracle on case `c`; perturb: seed of the one-ulp signs; rearth_*: the controls (a factor on params.Rearth, on the
    Rearth the grid's dx / dy / area were made with)"""
    grid, p, b, bd, nsteps = c
    if rearth_params != 1.0:
        p = S.params_copy(p)
        p.Rearth = p.Rearth * rearth_params
    if rearth_grid != 1.0:
        grid = {"desc": grid["desc"], "forcing": grid["forcing"], "static": dict(grid["static"])}
        for k, power in (("dx", 1), ("dy", 1), ("area", 2)):
            grid["static"][k] = grid["static"][k] * rearth_grid ** power
    if perturb is not None:
        b = S.copy_bergs(b)
        rng = np.random.default_rng(100 + perturb)
        for f, g in (("lon", "lon_old"), ("lat", "lat_old")):
            up = rng.integers(0, 2, len(b[f])).astype(bool)
            b[f][:] = np.where(up, np.nextafter(b[f], np.inf), np.nextafter(b[f], -np.inf))
            b[g][:] = b[f]
    return P.run_oracle_mts(grid, p, b, bd, nsteps)


_CACHE = {}


def measured(name):
    """per case, computed once and shared (nobody changes it): the case, its oracle run, spread, exactness over the nine runs"""
    if name not in _CACHE:
        c = case(name)
        ref, refbd = run_oracle(c)
        worst, same = {}, {k: True for k in P.MTS_EXACT}
        for s in range(SPREAD_RUNS):
            got, gotbd = run_oracle(c, perturb=s)
            rep, exact = P.mts_errors(ref, refbd, got, gotbd, wrap_lon=True)
            for k, v in rep.items():
                worst[k] = max(worst.get(k, 0.0), v)
            for k in same:
                same[k] = same[k] and exact[k]
        _CACHE[name] = {"case": c, "ref": ref, "refbd": refbd, "spread": worst, "exact": same}
    return _CACHE[name]


def spread(name):
    """({key of parity.mts_errors: largest rel err of the eight perturbed oracle runs against the unperturbed one},
    {what must be identical: whether it was in all nine})"""
    m = measured(name)
    return m["spread"], m["exact"]


def tolerances(name):
    """{key: max(compare_mts's tolerance, 10 x spread)}: integers, bond sets, broken-bond sets and event counters stay exact"""
    base = P.mts_tolerances()
    sp, _ = spread(name)
    return {k: max(t, SPREAD_FACTOR * sp[k]) for k, t in base.items()}


def over_cap(name):
    """{key: 10 x spread / today's tolerance} of the keys beyond SPREAD_CAP (none: the case is admissible on this count)"""
    base = P.mts_tolerances()
    sp, _ = spread(name)
    return {k: SPREAD_FACTOR * sp[k] / t for k, t in base.items() if SPREAD_FACTOR * sp[k] > SPREAD_CAP * t}


def control(name, which):
    """how far a metric wrong by CONTROL_REL lies beyond the tolerances: {key: err / tolerance}.  which = "params": params.Rearth
    (the pair metric, the position and velocity maps) with the grid's dx / dy / area as they are -- Rearth on one side only;
    which = "both": those scaled too."""
    m = measured(name)
    got, gotbd = run_oracle(m["case"], rearth_params=1.0 + CONTROL_REL, rearth_grid=1.0 + (CONTROL_REL if which == "both" else 0.0))
    rep, _ = P.mts_errors(m["ref"], m["refbd"], got, gotbd, wrap_lon=True)
    tol = tolerances(name)
    return {k: rep[k] / tol[k] for k in tol}


def depth_stencil_top(grid, p, b):
    """the highest latitude among the four cell centres that quad_interp_depth (FW:7163-7252) hands to its map, per row: above
    89.999 on a lat-lon grid it takes the polar form"""
    d, st = grid["desc"], grid["static"]
    mind = 0 if p.rev_mind else 1
    j, yj = b["jne"].astype(np.int64), b["yj"]
    je = np.where(j % 2 == mind, np.where(yj >= 0.5, j + 2, j), j + 1)
    return st["latc"][je - d.jsd, b["ine"] - d.isd]


def pair_metres(p, lon1, lat1, lon2, lat2):
    """the reference's distance of a pair: cos of the MEAN latitude (IB:444-459)"""
    rad = p.pi / 180.0
    return np.hypot((lon1 - lon2) * rad * p.Rearth * np.cos(0.5 * (lat1 + lat2) * rad), (lat1 - lat2) * rad * p.Rearth)


def table_line(name):
    sp, _ = spread(name)
    tol = tolerances(name)
    base = P.mts_tolerances()
    worst = max(base, key=lambda k: sp[k] / base[k])
    cp, cb = control(name, "params"), control(name, "both")
    return ("%-18s spread lon %.1e uvel %.1e ang_accel %.1e | tol lon %.1e uvel %.1e axn %.1e ang_accel %.1e | worst 10 x spread / today's: %s %.2g | "
            "control (params) lon %.1e uvel %.1e x tol, (both) lon %.1e uvel %.1e x tol" % (
                name, sp["lon"], sp["uvel"], sp["ang_accel"], tol["lon"], tol["uvel"], tol["axn"], tol["ang_accel"], worst,
                SPREAD_FACTOR * sp[worst] / base[worst], cp["lon"], cp["uvel"], cb["lon"], cb["uvel"]))
