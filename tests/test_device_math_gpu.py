"""The trimmed device arithmetic of the per-berg path, every form alone against a high-precision reference.

icebergs_amd/csrc/libkid_math_probe.so (tests/device_math_probe.hip, built by build() with the library's flags) applies each form of
kid_device.hpp and kid_thermo.hpp elementwise.  The bounds asserted are the claims of the source comments read as hard numbers
(device_math_sets.BOUND) or derivations written where they are used; none is a value measured from the code under test.  Every
test prints its measured worst cases (pytest -s); DESIGN.md section 4 keeps the table.

Documented deviations from IEEE, asserted as such (DESIGN section 4 lists the call sites and why none of them can reach one with
a result the reference would have kept finite):
  * kid_rcp(+-0), kid_rcp(+-inf), and with them a * Rcp, kid_div and kid_div_r at such a divisor, are NaN (IEEE: inf and 0): the
    Newton residual fma(-b, r, 1) of (0, inf) is NaN; kid_div and kid_div_r of an infinite numerator are NaN as well (their residual
    fma(-b, q, a) is inf - inf), a * Rcp is IEEE's inf;
  * a divisor below 2^-1022 (a denormal) or above 2^1022 is outside the iteration's domain (the seed or the result is a denormal);
  * kid_sqrt_nn(x) for 0 < x < 1e-300 is not the root but a number in [0, 2.25e-150];
  * kid_sqrt and kid_sqrt_nn below 1e-300: the residual x - g^2 is a denormal there, bound 1 + 2^-1023 / x ulp (derived below)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import device_math_sets as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "icebergs_amd", "csrc", "libkid_math_probe.so")

U = {n: k for k, n in enumerate(["rcp", "sqrt", "sqrt_nn", "rsqrt", "pow08", "rpow5", "powr02", "powr08", "root4", "cube", "seed_rcp", "seed_rsq",
                                 "seed_rpow5", "sin15", "sin"])}
B = {n: k for k, n in enumerate(["mul_rcp", "div", "div_r", "mul_rpow5"])}
L = {n: k for k, n in enumerate(["cell", "cell_noref", "near", "sincos"])}
PI, REARTH = 3.14159265358979323846, 6360000.0
PI_180, R180_PI = PI / 180., 180. / PI
INF, NAN = np.inf, np.nan
TINY = np.finfo(np.float64).tiny   # 2^-1022, the smallest normal number
DEN = 5e-324


class Probe:
    def __init__(self):
        import torch
        assert os.path.exists(PROBE), "libkid_math_probe.so is not built (build() makes it)"
        self.torch = torch
        self.lib = C.CDLL(PROBE)
        vp, ll = C.c_void_p, C.c_longlong
        self.lib.kid_probe_unary.argtypes = [C.c_int, vp, vp, ll]
        self.lib.kid_probe_binary.argtypes = [C.c_int, vp, vp, vp, ll]
        self.lib.kid_probe_lat.argtypes = [C.c_int, C.c_double, C.c_double, vp, vp, vp, vp, vp, ll]

    def _dev(self, x):
        return self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda:0")

    def unary(self, op, x):
        x = np.atleast_1d(np.asarray(x, dtype=np.float64))
        dx = self._dev(x); out = self.torch.empty_like(dx)
        self.torch.cuda.synchronize()
        assert self.lib.kid_probe_unary(U[op], dx.data_ptr(), out.data_ptr(), x.size) == 0
        return out.cpu().numpy()

    def binary(self, op, a, b):
        a, b = np.broadcast_arrays(np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64)))
        da, db = self._dev(a), self._dev(b); out = self.torch.empty_like(da)
        self.torch.cuda.synchronize()
        assert self.lib.kid_probe_binary(B[op], da.data_ptr(), db.data_ptr(), out.data_ptr(), a.size) == 0
        return out.cpu().numpy()

    def lat(self, op, lat, latc):
        lat, latc = np.broadcast_arrays(np.atleast_1d(np.asarray(lat, dtype=np.float64)), np.atleast_1d(np.asarray(latc, dtype=np.float64)))
        dl, dc = self._dev(lat), self._dev(latc)
        s, c, x = self.torch.empty_like(dl), self.torch.empty_like(dl), self.torch.empty_like(dl)
        self.torch.cuda.synchronize()
        assert self.lib.kid_probe_lat(L[op], PI, REARTH, dl.data_ptr(), dc.data_ptr(), s.data_ptr(), c.data_ptr(), x.data_ptr(), lat.size) == 0
        return s.cpu().numpy(), c.cpu().numpy(), x.cpu().numpy()


@pytest.fixture(scope="module")
def probe():
    return Probe()


def report(name, err, *cols, unit="ulp"):
    w, at = D.worst(err, *cols)
    print("MEASURED %-28s worst %.4g %s at %s" % (name, w, unit, " ".join("%r" % v for v in at)))
    return w


def is_nan(v):
    return bool(np.isnan(v))


# ---- reciprocal and quotient ------------------------------------------------------------------------------------------------------
def test_reciprocal_and_quotients_hold_their_ulp_claims(probe):
    b = D.divisors(); a = D.numerators(b.size)
    one = np.ones_like(b)
    seed = probe.unary("seed_rcp", b)
    ref_r = D.ref_ld(lambda p, q: p / q, one, b)
    ref_q = D.ref_ld(lambda p, q: p / q, a, b)
    w_seed = report("v_rcp_f64 seed", D.rel_err(seed, ref_r), b, unit="relative")
    assert w_seed <= D.BAND_RCP
    r = probe.unary("rcp", b)
    assert report("kid_rcp", D.ulp_err(r, ref_r), b) <= D.BOUND["kid_rcp"]
    assert report("a * kid_rcp(b)", D.ulp_err(probe.binary("mul_rcp", a, b), ref_q), a, b) <= D.BOUND["mul_rcp"]
    q = probe.binary("div", a, b)
    assert report("kid_div", D.ulp_err(q, ref_q), a, b) <= D.BOUND["kid_div"]
    assert D.same_bits(probe.binary("div_r", a, b), q).all()


def test_reciprocal_and_quotient_edges(probe):
    """Every edge on its own.  Where the forms keep to IEEE the IEEE value is asserted; where they do not, the documented deviation."""
    big = 2.0 ** 1022 * (1 + 2.0 ** -52)
    bs = np.array([0.0, -0.0, INF, -INF, NAN, TINY, -TINY, 2.0 ** -1022, big, DEN, 2.0 ** -1030, 2.0 ** -1023])
    r = probe.unary("rcp", bs)
    for a in (0.0, 1.0, INF):
        print("EDGE a=%r" % a, {"mul_rcp": probe.binary("mul_rcp", a, bs).tolist(), "div": probe.binary("div", a, bs).tolist()})
    print("EDGE kid_rcp", dict(zip(bs.tolist(), r.tolist())))
    # documented deviation: a zero or infinite divisor gives NaN in all four forms (IEEE: inf, 0), whatever the numerator
    for k in range(4):
        assert is_nan(r[k]), (bs[k], r[k])
        for a in (0.0, 1.0, -3.5, INF):
            for op in ("mul_rcp", "div", "div_r"):
                assert is_nan(probe.binary(op, a, bs[k])[0]), (op, a, bs[k])
    # NaN propagates, as in IEEE
    assert is_nan(r[4]) and is_nan(probe.binary("div", 1.0, NAN)[0]) and is_nan(probe.binary("div", NAN, 2.0)[0])
    # the smallest normal divisor: IEEE's 2^1022 exactly (a power of two: the residual is 0), and quotients with it
    assert r[5] == 2.0 ** 1022 and r[6] == -2.0 ** 1022 and r[7] == 2.0 ** 1022
    assert probe.binary("div", 0.0, TINY)[0] == 0.0 and probe.binary("mul_rcp", 0.0, TINY)[0] == 0.0
    assert probe.binary("div", 3.0, TINY)[0] == 3.0 * 2.0 ** 1022   # IEEE's quotient, a finite double
    assert probe.binary("div", 0.75, TINY)[0] == 0.75 * 2.0 ** 1022
    # a = 0 over an in-domain divisor: IEEE's 0 with IEEE's sign
    for bv in (3.0, -3.0, 1e-200, 1e200):
        for op in ("mul_rcp", "div", "div_r"):
            z = probe.binary(op, 0.0, bv)[0]
            assert z == 0.0 and np.signbit(z) == (bv < 0), (op, bv, z)
            # an infinite numerator: a * Rcp is IEEE's inf; kid_div's residual fma(-b, inf, inf) is NaN (documented deviation)
            qi = probe.binary(op, INF, bv)[0]
            assert (qi == (INF if bv > 0 else -INF)) if op == "mul_rcp" else is_nan(qi), (op, bv, qi)
    # at the ends of the exponent range, each as DESIGN section 4 documents it
    assert bs[8] == big and r[8] == 1.0 / big and r[8] == np.nextafter(TINY, 0.0)      # 2^1022 (1 + 2^-52): IEEE's denormal
    assert bs[11] == 2.0 ** -1023 and r[11] == 2.0 ** 1023                              # a denormal divisor whose reciprocal is finite: IEEE's
    assert is_nan(r[9]) and is_nan(r[10])                                               # 5e-324, 2^-1030: NaN (IEEE: inf), the seed is inf
    for op in ("mul_rcp", "div", "div_r"):
        assert is_nan(probe.binary(op, 1.0, DEN)[0]) and is_nan(probe.binary(op, 1.0, 2.0 ** -1030)[0]), op
        assert probe.binary(op, 1.0, 2.0 ** -1023)[0] == 2.0 ** 1023 and probe.binary(op, 1.0, big)[0] == 1.0 / big, op


def test_quotient_of_a_not_below_b_is_not_below_one(probe):
    """accel's cr_q takes 1 without dividing in waves where every lane has cr_num >= cr_den and min(max(0, kid_div(..)), 1) elsewhere:
    a lane's value is the same either way only if kid_div(a, b) >= 1 whenever a >= b > 0.  It is: the last fma rounds q + (a - b q) r,
    which is within 2^-100 relative of a / b >= 1, and everything above 1 - 2^-54 rounds to 1 or more."""
    b = D.log_uniform(1e-30, 1e30, 4000, 71)
    b = np.concatenate([b, D.patterns(-60, 60, 4)])
    for k in range(0, 9):
        a = b.copy()
        for _ in range(k):
            a = np.nextafter(a, INF)
        q = probe.binary("div", a, b)
        assert (q >= 1.0).all(), (k, a[q < 1.0][:4], b[q < 1.0][:4])
        if k == 0:
            assert (q == 1.0).all()
        a2 = b * (1.0 + k * 2.0 ** -52)
        assert (probe.binary("div", a2, b) >= 1.0).all(), k
    # the expression as accel forms it: the denominator carries the 1e-30 of the reference
    den = b + 1e-30
    assert (probe.binary("div", den, den) == 1.0).all()


# ---- square roots -----------------------------------------------------------------------------------------------------------------
def test_square_roots_hold_their_ulp_claims(probe):
    x = D.sqrt_args()
    ref = D.ref_ld(np.sqrt, x)
    ref_rs = D.ref_ld(lambda v: 1 / np.sqrt(v), x)
    assert report("v_rsq_f64 seed", D.rel_err(probe.unary("seed_rsq", x), ref_rs), x, unit="relative") <= D.BAND_RSQ
    g = probe.unary("sqrt", x)
    assert report("kid_sqrt", D.ulp_err(g, ref), x) <= D.BOUND["kid_sqrt"]
    assert D.same_bits(probe.unary("sqrt_nn", x), g).all()
    xr = D.rsqrt_args()
    assert report("kid_rsqrt", D.ulp_err(probe.unary("rsqrt", xr), D.ref_ld(lambda v: 1 / np.sqrt(v), xr)), xr) <= D.BOUND["kid_rsqrt"]


def test_square_root_edges_and_domain(probe):
    """kid_sqrt: +-0, negative, NaN and +inf as sqrt() treats them; 1e-300, its neighbours, 1e300 and the largest double within the
    1 ulp claim.  Below 1e-300 the residual x - g^2 (~x 2^-44) is a denormal and is rounded to a multiple of 2^-1074: an absolute error
    <= 2^-1075, times h ~ 1 / (2 sqrt x), relative to sqrt x that is 2^-1076 / x, i.e. <= 2^-1023 / x ulps on top of the claim's 1 --
    the bound asserted there, for denormal arguments too (it passes 1.03 ulp at 2^-1018 and 2 ulp at 2^-1023).
    kid_sqrt_nn below 1e-300 is no root at all: with y = rsq(1e-300), g0 = x y < 1e-150, r = 0.5 - g0 y / 2 in (0, 0.5], g1 = g0 (1 + r)
    <= 1.5 g0, h1 <= 0.75 y, and the result g1 + (x - g1^2) h1 lies in [0, 2.25e-150] -- asserted, with the root's monotone zero at 0."""
    v = probe.unary("sqrt", [0.0, -0.0, -1.0, -DEN, -INF, NAN, INF])
    print("EDGE kid_sqrt", v.tolist())
    assert v[0] == 0.0 and not np.signbit(v[0])
    assert v[1] == 0.0 and np.signbit(v[1])
    assert is_nan(v[2]) and is_nan(v[3]) and is_nan(v[4]) and is_nan(v[5])
    assert v[6] == INF
    xs = np.array([1e-300, np.nextafter(1e-300, 1.0), 1e300, np.nextafter(1e300, 0.0), np.nextafter(1e300, INF), np.finfo(np.float64).max])
    for f in ("sqrt", "sqrt_nn"):
        assert (D.ulp_err(probe.unary(f, xs), D.ref_ld(np.sqrt, xs)) <= 1.0).all(), f
    nn = probe.unary("sqrt_nn", [0.0, INF])
    assert nn[0] == 0.0
    assert is_nan(nn[1])   # documented deviation (sqrt: +inf); a sum of squares of speeds is infinite only if a velocity is
    # below the documented floor, binade by binade
    es = np.arange(-1074, -995)
    lo = np.concatenate([np.ldexp(1.0, es), np.ldexp(1.5, es[1:]), [np.nextafter(1e-300, 0.0), DEN, TINY, np.nextafter(TINY, 0.0)]])
    ref = D.ref_ld(np.sqrt, lo)
    g = probe.unary("sqrt", lo)
    err = D.ulp_err(g, ref)
    first_bad = lo[err > 1.0].max() if (err > 1.0).any() else 0.0
    print("MEASURED kid_sqrt below 1e-300: worst %.3f ulp; largest argument with more than 1 ulp: %r" % (np.nanmax(err), first_bad))
    assert np.isfinite(g).all()
    assert (err <= 1.0 + 2.0 ** -1023 / lo).all(), (lo[err > 1.0 + 2.0 ** -1023 / lo], err[err > 1.0 + 2.0 ** -1023 / lo])
    below = np.concatenate([lo[lo < 1e-300], D.log_uniform(1e-320, 0.999e-300, 500, 81)])
    gn = probe.unary("sqrt_nn", below)
    print("MEASURED kid_sqrt_nn below 1e-300: range [%r, %r]" % (gn.min(), gn.max()))
    assert np.isfinite(gn).all() and (gn >= 0.0).all() and (gn <= 2.25e-150 * (1 + 1e-6)).all()
    # the floor of the wind's unit vector: kid_rsqrt(max(wmod, 1e-300)) is finite and within its claim at the floor
    rs = probe.unary("rsqrt", [1e-300])
    assert D.ulp_err(rs, D.ref_ld(lambda t: 1 / np.sqrt(t), np.array([1e-300])))[0] <= 1.0


# ---- the melt laws' powers --------------------------------------------------------------------------------------------------------
def _mp_pow(y):
    import mpmath as mp
    return lambda v: mp.power(v, mp.mpf(y) if not isinstance(y, tuple) else mp.mpf(y[0]) / y[1])


def slow_rel_bound(x, y, extra=0.0):
    """exp(y log x) with ocml's log and exp (1 ulp each): t = y log x carries <= 1.5 ulp, |t| 1.5 2^-52 absolute, which exp turns into the
    same relative error, plus exp's own ulp: (1.5 |t| + 1) 2^-52; `extra` ulps for a division or a product behind it."""
    with np.errstate(all="ignore"):
        return (1.5 * np.abs(y * np.log(x)) + 1.0 + extra) * 2.0 ** -52


def test_fifth_root_forms_hold_their_claims(probe):
    x = D.rpow5_args()
    ref_r = D.ref_mp(_mp_pow((-1, 5)), x)
    ref_08 = D.ref_mp(_mp_pow((4, 5)), x)
    assert report("f32 exp2/log seed of x^-0.2", D.rel_err(probe.unary("seed_rpow5", x), ref_r), x, unit="relative") <= D.BAND_RPOW5
    assert report("kid_mul_rpow5(1, x)", D.ulp_err(probe.unary("rpow5", x), ref_r), x) <= D.BOUND["kid_rpow5"]
    assert report("kid_pow08", D.ulp_err(probe.unary("pow08", x), ref_08), x) <= D.BOUND["kid_pow08"]
    a = np.abs(D.numerators(x.size))
    import mpmath as mp
    ref_a = D.ref_mp(lambda p, q: p * mp.power(q, mp.mpf(-1) / 5), a, x)
    assert report("kid_mul_rpow5(a, x)", D.ulp_err(probe.binary("mul_rpow5", a, x), ref_a), a, x) <= D.BOUND["mul_rpow5"]


def test_powr_holds_its_relative_claim(probe):
    """the reference raises to the doubles 0.2 and 0.8, the exponents the device is handed, not to 1/5 and 4/5"""
    import mpmath as mp
    for y, op in ((0.2, "powr02"), (0.8, "powr08")):
        x = D.powr_args(y)
        x = x[np.abs(y * np.log(x)) < 8.0]
        ref = D.ref_mp(lambda v, y=y: mp.power(v, mp.mpf(y)), x)
        assert report("kid_powr(x, %.1f)" % y, D.rel_err(probe.unary(op, x), ref), x, unit="relative") <= D.POWR_REL
    assert probe.unary("powr02", [0.0])[0] == 0.0 and probe.unary("powr08", [0.0])[0] == 0.0


def test_fifth_root_edges_and_hand_over(probe):
    import mpmath as mp
    u = 2.0 ** -53
    fast_rel = {"rpow5": 2 * D.BOUND["kid_rpow5"] * u, "pow08": 2 * D.BOUND["kid_pow08"] * u}   # an error of k ulp is <= 2 k u relative
    for edge in (1e-30, 1e30):
        xs = np.array([np.nextafter(edge, 0.0), edge, np.nextafter(edge, INF)])
        fast = (xs > 1e-30) & (xs < 1e30)
        assert fast.sum() == 1   # the hand-over sits between two of the three
        for op, frac, y, extra in (("rpow5", (-1, 5), 0.2, 1.0), ("pow08", (4, 5), 0.8, 0.0)):
            ref = D.ref_mp(_mp_pow(frac), xs)
            got = probe.unary(op, xs)
            rel = D.rel_err(got, ref)
            bound = np.where(fast, fast_rel[op], slow_rel_bound(xs, y, extra))
            print("EDGE %s at %r: relative errors %s, bounds %s" % (op, edge, rel.tolist(), bound.tolist()))
            assert (rel <= bound).all(), (op, edge, rel, bound)
            # the jump across the hand-over: no more than the two bounds and the function's own step over one ulp of x
            for k in (0, 1):
                jump = abs(got[k + 1] - got[k]) / abs(got[k])
                assert jump <= bound[k] + bound[k + 1] + 2.0 ** -52, (op, edge, k, jump)
    # outside the fast range: the slow path within its derived bound
    xo = np.concatenate([D.log_uniform(1e-300, 1e-30, 1000, 91), D.log_uniform(1e30, 1e300, 1000, 92), [DEN, 2.0 ** -1060, TINY]])
    for op, frac, y, extra in (("rpow5", (-1, 5), 0.2, 1.0), ("pow08", (4, 5), 0.8, 0.0)):
        rel = D.rel_err(probe.unary(op, xo), D.ref_mp(_mp_pow(frac), xo))
        report("%s outside (1e-30, 1e30)" % op, rel / slow_rel_bound(xo, y, extra), xo, unit="of its bound")
        assert (rel <= slow_rel_bound(xo, y, extra)).all(), op
    # 0, inf, NaN as pow treats them
    p8 = probe.unary("pow08", [0.0, INF, NAN]); r5 = probe.unary("rpow5", [0.0, INF, NAN])
    print("EDGE pow08", p8.tolist(), "rpow5", r5.tolist())
    assert p8[0] == 0.0 and p8[1] == INF and is_nan(p8[2])
    assert r5[0] == INF and r5[1] == 0.0 and is_nan(r5[2])
    assert probe.binary("mul_rpow5", 0.0, 2.0)[0] == 0.0 and probe.binary("mul_rpow5", 3.0, INF)[0] == 0.0


# ---- x^3, x^(1/4) and the sine series ---------------------------------------------------------------------------------------------
def test_root4_cube_and_sine_series(probe):
    import mpmath as mp
    x = D.cube_args()
    assert report("kid_root4", D.ulp_err(probe.unary("root4", x), D.ref_mp(_mp_pow((1, 4)), x)), x) <= D.BOUND["kid_root4"]
    w_cube = report("kid_cube", D.ulp_err(probe.unary("cube", x), D.ref_mp(lambda v: v * v * v, x)), x)
    t = D.small_args()
    ref = D.ref_mp(mp.sin, t)
    got = probe.unary("sin15", t)
    w_sin = report("sine series, |x| < 0.25", D.ulp_err(got, ref), t)
    dev = probe.unary("sin", t)
    diff = np.abs(got - dev) / np.spacing(np.abs(ref[0]))
    report("sine series against device sin()", diff, t)
    print("MEASURED sine series: %d of %d values differ from device sin()" % (int((diff > 0).sum()), t.size))
    assert probe.unary("sin15", [0.0])[0] == 0.0
    assert w_cube <= D.BOUND["kid_cube"]
    assert w_sin <= D.BOUND["sin15"]


# ---- the latitude series ----------------------------------------------------------------------------------------------------------
LAT_C = [0.0, 45.0, -45.0, 89.0, -89.0, 89.99, -89.99, 90.0, -90.0]


def _dev_d(lat, latc):
    return (lat - latc) * PI_180   # the device's own d: the same two IEEE operations


def _around_threshold(latc, thr, sign):
    """latitudes whose d is the last below thr in magnitude, and the first not below it (one ulp of lat apart)"""
    lat = latc + sign * thr / PI_180
    step = sign * np.inf
    while abs(_dev_d(lat, latc)) >= thr:
        lat = np.nextafter(lat, latc)
    while abs(_dev_d(np.nextafter(lat, step), latc)) < thr:
        lat = np.nextafter(lat, step)
    return lat, np.nextafter(lat, step)


def _lat_refs(lat):
    import mpmath as mp
    ang = lat * PI_180   # the double the device's sincos path forms
    return D.ref_mp(mp.sin, ang), D.ref_mp(mp.cos, ang)


@pytest.mark.parametrize("form,thr,nper", [("cell", 0.02, 2200), ("near", 2e-3, 2200)])
def test_latitude_series(probe, form, thr, nper):
    """sin / cos of lat = lat_c + d from the tabulated (sin, cos)(lat_c) and a Taylor series in d.  Reference: sin and cos, at 50 digits,
    of the double lat * pi_180.  Bound on the absolute error of s and c, 1e-15: three roundings of ~1.1e-16 (the table entry, cd, the
    final fma), up to ~3.3e-16 from the rounding of the angle and of d, truncation below 1e-17.  c > 0 for every |lat| < 90; dxdl =
    (180 / pi) / (Rearth c) within 1e-15 / c relative (c's absolute error over c, the few ulps of the product and reciprocal inside)."""
    rng = np.random.default_rng(101)
    lats, latcs = [], []
    for lc in LAT_C:
        d = np.concatenate([rng.uniform(-thr, thr, nper - 200), np.linspace(-thr, thr, 197) * 0.999999, [0.0, 1e-18, -1e-18]])
        la = lc + d / PI_180
        if 89.0 <= abs(lc) < 90.0:   # the last 39 doubles below the pole, from a tabulated latitude short of it: c stays positive
            pole = [np.copysign(90.0, lc)]
            for _ in range(39):
                pole.append(np.nextafter(pole[-1], 0.0))
            la = np.concatenate([la, pole[1:]])
        la = la[np.abs(_dev_d(la, lc)) < thr]
        lats.append(la); latcs.append(np.full(la.size, lc))
    lat, latc = np.concatenate(lats), np.concatenate(latcs)
    s, c, x = probe.lat(form, lat, latc)
    (rs, rc) = _lat_refs(lat)
    es, ec = np.abs((s - rs[0]) - rs[1]), np.abs((c - rc[0]) - rc[1])
    w_s = report("lat_terms_%s sin, |d| < %g" % (form, thr), es, lat, latc, unit="absolute")
    w_c = report("lat_terms_%s cos" % form, ec, lat, latc, unit="absolute")
    inside = np.abs(lat) < 90.0
    cexact = rc[0].astype(np.longdouble) + rc[1].astype(np.longdouble)
    with np.errstate(all="ignore"):
        xref = np.longdouble(R180_PI) / (np.longdouble(REARTH) * cexact)
        ex = np.abs((x.astype(np.longdouble) - xref) / xref).astype(np.float64) * np.abs(rc[0])
    w_x = report("lat_terms_%s dxdl, relative error times c" % form, np.where(inside, ex, 0.0), lat, latc, unit="")
    assert w_s <= 1e-15 and w_c <= 1e-15
    assert (c[inside] > 0.0).all(), (lat[inside][c[inside] <= 0.0], latc[inside][c[inside] <= 0.0])
    assert (ex[inside] <= 1e-15).all()
    # the series differs from the device's sincos by no more than the two bounds together -- and is not the sincos path
    s0, c0, _ = probe.lat("sincos", lat, latc)
    report("lat_terms_%s against device sincos (sin)" % form, np.abs(s - s0), lat, latc, unit="absolute")
    report("lat_terms_%s against device sincos (cos)" % form, np.abs(c - c0), lat, latc, unit="absolute")


@pytest.mark.parametrize("form,thr", [("cell", 0.02), ("near", 2e-3)])
def test_latitude_series_thresholds(probe, form, thr):
    """d at the threshold, one ulp of the latitude inside and outside it, on both sides of every tabulated latitude: inside, the series
    within its bound; outside, the bits of the device's sincos.  have_ref = false: sincos whatever d is."""
    import mpmath as mp
    for lc in LAT_C:
        for sign in (1.0, -1.0):
            lin, lout = _around_threshold(lc, thr, sign)
            assert abs(_dev_d(lin, lc)) < thr <= abs(_dev_d(lout, lc))
            lat = np.array([lin, lout]); latc = np.array([lc, lc])
            s, c, x = probe.lat(form, lat, latc)
            s0, c0, x0 = probe.lat("sincos", lat, latc)
            (rs, rc) = _lat_refs(lat)
            assert abs((s[0] - rs[0][0]) - rs[1][0]) <= 1e-15 and abs((c[0] - rc[0][0]) - rc[1][0]) <= 1e-15, (form, lc, sign)
            assert D.same_bits(s[1:], s0[1:]).all() and D.same_bits(c[1:], c0[1:]).all() and D.same_bits(x[1:], x0[1:]).all(), (form, lc, sign)
    if form == "cell":
        lat = np.array([lc + d for lc in LAT_C for d in (0.0, 0.3, -0.3, 1e-9)]); latc = np.repeat(LAT_C, 4)
        s, c, x = probe.lat("cell_noref", lat, latc)
        s0, c0, x0 = probe.lat("sincos", lat, latc)
        assert D.same_bits(s, s0).all() and D.same_bits(c, c0).all() and D.same_bits(x, x0).all()


# ---- the host restatement fed the device's seeds ----------------------------------------------------------------------------------
def test_host_restatement_reproduces_the_device_bit_for_bit(probe, tmp_path):
    """tests/device_math_host.cpp compiled as a shared object (no sanitizer) and fed the seeds the device returned reproduces the
    device's results bit for bit, edges included: what ties the CPU sweep of tests/test_device_math_cpu.py to the device code."""
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    so = str(tmp_path / "libdevice_math_host.so")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, os.path.join(ROOT, "tests", "device_math_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    host = C.CDLL(so)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    host.hm_apply.argtypes = [C.c_int, dp, dp, dp, dp, C.c_longlong]

    def apply(op, a, x, seed):
        a, x, seed = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, x, seed))
        out = np.empty_like(x)
        assert host.hm_apply(op, a, x, seed, out, x.size) == 0
        return out

    edges = np.array([0.0, -0.0, INF, -INF, NAN, TINY, DEN, 2.0 ** 1022 * (1 + 2.0 ** -52), 1e-300, 1e300, np.finfo(np.float64).max, -1.0])
    b = np.concatenate([D.divisors(), edges]); a = np.concatenate([D.numerators(b.size - edges.size), np.resize([0.0, 1.0, INF, -2.5], edges.size)])
    seed = probe.unary("seed_rcp", b)
    for hop, dop, un in ((0, "rcp", True), (1, "mul_rcp", False), (2, "div", False), (3, "div_r", False)):
        dev = probe.unary(dop, b) if un else probe.binary(dop, a, b)
        same = D.same_bits(apply(hop, a, b, seed), dev)
        assert same.all(), (dop, a[~same][:4], b[~same][:4])
    x = np.concatenate([D.sqrt_args(), edges, D.log_uniform(1e-320, 1e-300, 200, 111)])
    seed = probe.unary("seed_rsq", x)
    for hop, dop in ((4, "sqrt"), (6, "rsqrt")):
        same = D.same_bits(apply(hop, x, x, seed), probe.unary(dop, x))
        assert same.all(), (dop, x[~same][:6])
    seed_nn = probe.unary("seed_rsq", np.fmax(x, D.SQRT_NN_FLOOR))
    same = D.same_bits(apply(5, x, x, seed_nn), probe.unary("sqrt_nn", x))
    assert same.all(), ("sqrt_nn", x[~same][:6])
    xp = D.rpow5_args()
    seed = probe.unary("seed_rpow5", xp)
    for hop, dop in ((7, "rpow5"), (8, "pow08")):
        same = D.same_bits(apply(hop, xp, xp, seed), probe.unary(dop, xp))
        assert same.all(), (dop, xp[~same][:6])
