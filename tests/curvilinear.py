"""Curvilinear, rotated test grids: a 48x40 patch that holds the four classes of cell the hot build's packets tell apart
(flag word +-(1 + 2 [sides along the axes] + 4 [cos = 1, sin = 0 at the four corners]), pack_packets_kernel) next to each
other, in the manner of the displaced-pole patch of a tripolar ocean grid:

  * a disc of rotated velocity components (grd%cos / grd%sin differ from 1 / 0 at the corners inside it);
  * an overlapping disc of sheared corners (general convex quadrilaterals: calc_xiyj's quadratic branch, FW:6439-6534);
  * outside a disc exactly cos == 1.0, sin == 0.0 and corner coordinates constant along columns and rows;
  * sea ice over a third disc only, a non-zero sea-surface height, a block of land inside the sheared-and-rotated lens and,
    on the lat-lon variant, a band of rows 1.6 degrees tall (lat_terms_cell leaves its Taylor series at 1.15 degrees).

The discs' borders cross the grid rows, so a wave of 64 consecutive bergs (reference order: rows outer, columns inner) holds
cells of several classes.  All of it is data for both sides of a comparison: the oracle and the library read the same arrays.
"""
import numpy as np

from icebergs_amd import synthetic as S

NI, NJ = 48, 40
ROT_DISC = (17.0, 19.0, 13.0)      # centre i, centre j, radius (in corner indices)
SHEAR_DISC = (30.0, 21.0, 13.0)
ICE_DISC = (24.0, 27.0, 11.0)
TALL_ROWS = (29, 32)               # cell rows 1.6 degrees tall (lat-lon variant)
LAND = (23, 25, 19, 21)            # i0, i1, j0, j1: inside both discs
I_RANGE, J_RANGE = (5, 44), (5, 36)   # cells that receive bergs
REARTH = 6.36e6


def _disc(i, j, disc):
    """1 at the centre, exactly 0.0 on and outside the rim"""
    ic, jc, r = disc
    return np.maximum(0.0, 1.0 - ((i - ic) ** 2 + (j - jc) ** 2) / (r * r))


def _metrics(grid, latlon):
    """lonc / latc (corner means), dx / dy (lengths of the cell's north and east sides) and area (shoelace) from the corners;
    the first column and row, which have no south-west neighbour, keep their neighbour's value."""
    st = grid["static"]
    lon, lat = st["lon"], st["lat"]
    rad = np.pi / 180.0

    def sw(a):   # a(i-1, j-1), a(i, j-1), a(i, j), a(i-1, j) on the cells that have all four corners
        return a[:-1, :-1], a[:-1, 1:], a[1:, 1:], a[1:, :-1]
    x0, x1, x2, x3 = sw(lon)
    y0, y1, y2, y3 = sw(lat)
    lonc, latc = 0.25 * ((x0 + x1) + (x2 + x3)), 0.25 * ((y0 + y1) + (y2 + y3))
    if latlon:
        mx = REARTH * rad * np.cos(latc * rad)
        my = REARTH * rad
        dx = REARTH * rad * np.cos(y2 * rad) * (x2 - x3)
    else:
        mx = my = 1.0
        dx = x2 - x3
    dy = my * (y2 - y1)
    area = 0.5 * np.abs((x2 - x0) * (y3 - y1) - (x3 - x1) * (y2 - y0)) * mx * my
    for name, v in (("lonc", lonc), ("latc", latc), ("dx", dx), ("dy", dy), ("area", area)):
        st[name][1:, 1:] = v
        st[name][0, 1:] = v[0]
        st[name][:, 0] = st[name][:, 1]
    # (the centres of the first column and row lie one cell further out, not on their neighbours)
    st["lonc"][:, 0] = st["lonc"][:, 1] - (st["lonc"][:, 2] - st["lonc"][:, 1])
    st["latc"][0] = st["latc"][1] - (st["latc"][2] - st["latc"][1])


def patch_grid(kind="latlon", rotate=True, shear=True):
    """kind = "latlon": lon0 = 10, dlon = 0.5, lat0 = 58, dlat = 0.3 (grid_is_latlon, not regular), config-2 forcing;
    kind = "cartesian": 1 km cells, grid_is_latlon = 0, grid_is_regular = 0 (calc_xiyj with no trigonometric function on a
    berg's path under the f-plane of config 1), config-1 forcing."""
    latlon = kind == "latlon"
    if latlon:
        grid = S.latlon_grid(ni=NI, nj=NJ, lon0=10.0, dlon=0.5, lat0=58.0, dlat=0.3, Rearth=REARTH)
        ex, ey = 0.5, 0.3
    else:
        assert kind == "cartesian", kind
        grid = S.cartesian_grid(NI, NJ, 1000.0, Lx=-1.0)
        grid["desc"].grid_is_regular = 0
        ex, ey = 1000.0, 1000.0
    d, st, f = grid["desc"], grid["static"], grid["forcing"]
    i, j = S._ij(d)
    one = S.zeros(d) + 1.0
    i, j = i * one, j * one
    if latlon:   # the tall band: cell rows TALL_ROWS are 1.6 degrees high
        st["lat"] = st["lat"] + 1.3 * np.clip(j - (TALL_ROWS[0] - 1), 0.0, TALL_ROWS[1] - TALL_ROWS[0] + 1.0)
    if shear:
        w = _disc(i, j, SHEAR_DISC)
        st["lon"] = st["lon"] + np.where(w > 0.0, 0.12 * ex * w * np.sin(2.0 * np.pi * j / 13.0 + 0.4), 0.0)
        st["lat"] = st["lat"] + np.where(w > 0.0, 0.10 * ey * w * np.cos(2.0 * np.pi * i / 11.0 + 0.3), 0.0)
    if rotate:
        w = _disc(i, j, ROT_DISC)
        ang = 0.6 * w * np.cos(2.0 * np.pi * i / 17.0)
        st["cos"] = np.where(w > 0.0, np.cos(ang), 1.0)
        st["sin"] = np.where(w > 0.0, np.sin(ang), 0.0)
    _metrics(grid, latlon)
    st["msk"][(i >= LAND[0]) & (i <= LAND[1]) & (j >= LAND[2]) & (j <= LAND[3])] = 0.0
    if latlon:
        S.c2_forcing(grid)
        f["ssh"][:] = 0.3 * np.sin(2.0 * np.pi * i / 15.0) * np.cos(2.0 * np.pi * j / 12.0)
    else:
        S.c1_forcing(grid)
    w = _disc(i, j, ICE_DISC)   # sea ice over part of the domain: exactly none outside the disc
    f["hi"][:] = 1.2 * w
    f["cn"][:] = 0.9 * w
    f["ui"][:] = 0.05 * w * np.sin(2.0 * np.pi * j / 9.0)
    f["vi"][:] = -0.04 * w
    land = st["msk"] < 0.5   # the scrub of icebergs.F90:5364-5372
    for k in ("ua", "va", "uo", "vo", "ui", "vi", "sst", "sss", "cn", "hi"):
        f[k][land] = 0.0
    return grid


def patch_params(kind="latlon"):
    p = S.default_params()
    if kind == "latlon":
        p.dt = 1800.0
    else:
        p.dt, p.lat_ref, p.use_f_plane = 150.0, -70.0, 1   # (48 steps of config 1's 600 s would carry bergs off the 48 km domain)
    return p


def frame_grid(kind, theta):
    """The sheared patch grid with ONE angle at every corner and a level sea surface: the velocity components are stored in
    the frame turned by theta, u_g = cos u - sin v, v_g = sin u + cos v (the inverse of icebergs.F90:4964-4965), so what a berg
    feels does not depend on theta.  theta = 0 leaves cos = 1, sin = 0: the unrotated classes."""
    grid = patch_grid(kind, rotate=False)
    st, f = grid["static"], grid["forcing"]
    c, s = np.cos(theta), np.sin(theta)
    st["cos"][:], st["sin"][:] = c, s
    f["ssh"][:] = 0.0
    for a, b in (("uo", "vo"), ("ui", "vi"), ("ua", "va")):
        u, v = f[a].copy(), f[b].copy()
        f[a][:] = c * u - s * v
        f[b][:] = s * u + c * v
    return grid


def _corners(grid):
    """the four corners of every cell that has them, as arrays over [1:, 1:]: (x00, x10, x11, x01), (y...)"""
    lon, lat = grid["static"]["lon"], grid["static"]["lat"]
    return ((lon[:-1, :-1], lon[:-1, 1:], lon[1:, 1:], lon[1:, :-1]), (lat[:-1, :-1], lat[:-1, 1:], lat[1:, 1:], lat[1:, :-1]))


def cell_flags(grid):
    """|flag word| of every cell as pack_static_kernel / pack_packets_kernel form it: 1 + 2 rect + 4 unrotated (0 in the first
    row and column, which have no south-west corner)."""
    st = grid["static"]
    (x0, x1, x2, x3), (y0, y1, y2, y3) = _corners(grid)
    rect = (x3 == x0) & (x2 == x1) & (y1 == y0) & (y2 == y3)
    c, s = st["cos"], st["sin"]
    unrot = np.ones_like(rect)
    for a in (c[:-1, :-1], c[:-1, 1:], c[1:, 1:], c[1:, :-1]):
        unrot &= a == 1.0
    for a in (s[:-1, :-1], s[:-1, 1:], s[1:, 1:], s[1:, :-1]):
        unrot &= a == 0.0
    flags = np.zeros(st["lon"].shape, dtype=np.int32)
    flags[1:, 1:] = 1 + 2 * rect + 4 * unrot
    return flags


def convex_nonpolar(grid):
    """pack_static_kernel's admission test: the corners form a strictly convex quadrilateral and none is at the pole"""
    (x0, x1, x2, x3), (y0, y1, y2, y3) = _corners(grid)
    k0 = (x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1)
    k1 = (x2 - x1) * (y3 - y2) - (y2 - y1) * (x3 - x2)
    k2 = (x3 - x2) * (y0 - y3) - (y3 - y2) * (x0 - x3)
    k3 = (x0 - x3) * (y1 - y0) - (y0 - y3) * (x1 - x0)
    ok = ((k0 > 0) & (k1 > 0) & (k2 > 0) & (k3 > 0)) | ((k0 < 0) & (k1 < 0) & (k2 < 0) & (k3 < 0))
    if grid["desc"].grid_is_latlon:
        ok &= np.maximum(np.maximum(y0, y1), np.maximum(y2, y3)) < 89.999
    out = np.zeros(grid["static"]["lon"].shape, dtype=bool)
    out[1:, 1:] = ok
    return out


def flags_of(grid, b):
    d = grid["desc"]
    return cell_flags(grid)[b["jne"] - d.jsd, b["ine"] - d.isd]


def place_bilinear(grid, n, seed, i_range=I_RANGE, j_range=J_RANGE):
    """n bergs in wet cells of i_range x j_range: (xi, yj) uniform in [0.02, 0.98], lon / lat through the bilinear map of the
    cell's four corners (FW:7071-7088 without old_bug_bilin), the rest as synthetic.place_bergs fills it; reference order."""
    d, st = grid["desc"], grid["static"]
    rng = np.random.Generator(np.random.PCG64(seed))
    b = S.empty_bergs(n)
    ine = rng.integers(i_range[0], i_range[1] + 1, size=n)
    jne = rng.integers(j_range[0], j_range[1] + 1, size=n)
    for _ in range(64):
        bad = st["msk"][jne - d.jsd, ine - d.isd] < 0.5
        if not bad.any():
            break
        ine[bad] = rng.integers(i_range[0], i_range[1] + 1, size=int(bad.sum()))
        jne[bad] = rng.integers(j_range[0], j_range[1] + 1, size=int(bad.sum()))
    xi = rng.uniform(0.02, 0.98, size=n)
    yj = rng.uniform(0.02, 0.98, size=n)
    jj, ii = jne - d.jsd, ine - d.isd
    for name in ("lon", "lat"):
        a = st[name]
        b[name][:] = (a[jj, ii] * xi + a[jj, ii - 1] * (1.0 - xi)) * yj + (a[jj - 1, ii] * xi + a[jj - 1, ii - 1] * (1.0 - xi)) * (1.0 - yj)
    b["xi"][:], b["yj"][:] = xi, yj
    b["ine"][:], b["jne"][:] = ine, jne
    S._fill_classes(b, rng.integers(0, 10, size=n))
    b["start_lon"][:], b["start_lat"][:] = b["lon"], b["lat"]
    b["start_year"][:] = 0
    b["start_day"][:] = 1.0e-6 * np.arange(n)
    b["lon_old"][:], b["lat_old"][:] = b["lon"], b["lat"]
    return S.sort_reference_order(b)


def mixed_groups(flags, bit, size=64):
    """how many groups of `size` consecutive bergs hold cells with and without `bit` in their flag"""
    n = len(flags) // size * size
    has = (flags[:n] & bit).astype(bool).reshape(-1, size)
    return int((has.any(axis=1) & ~has.all(axis=1)).sum())


def by_id(b, fields):
    """the live bergs' fields in order of id (the library re-bins its rows)"""
    n = int(b.get("_n", len(b["lon"])))
    live = np.nonzero(b["alive"][:n] != 0)[0]
    o = live[np.argsort(b["id"][live], kind="stable")]
    return {f: b[f][o] for f in list(fields) + ["id", "ine", "jne"]}
