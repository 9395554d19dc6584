"""The bonded pair force of the DEM sub-steps, calculate_force_dem (icebergs.F90:959-1242, "IB" below), restated in mpmath at 50
digits from the same double inputs, for tests/test_dem_pair_gpu.py (the device's pair_const / pair_force_dem through
tests/dem_pair_probe.hip) and tests/test_dem_pair_cpu.py (the oracle's calculate_force_dem through ko_dem_pair).

Every intermediate value is carried as a triple (v, S, C):
  v  the exact value (50 digits);
  S  its condition scale, S >= |v|: the sum of the absolute values of the terms that are added or subtracted to form it, carried
     through the computation -- what an error in the last place of an operand is relative to;
  C  the number of unit roundoffs u = 2^-53 the computed value may be off by, in units of S:  |computed - v| <= C u S.
The rules (first order in u; the second-order terms are below 1e-13 of the bound for C < 1000), for operands a, b that satisfy
the invariant, with c_op the bound of the operation's own rounding in u (1 for an IEEE +, -, *, /, sqrt):
  input x        (x, |x|, 0)
  a +- b         S = max(|v|, sum of the S of the operands with C > 0),  C = max(Ca, Cb) + 1
                 [err <= Ca u Sa + Cb u Sb + u |v|; an exact operand carries no error, so its size does not enter];
                 free when one operand is an exact zero, and exact operands that cancel give an exact zero
  a * b          S = Sa Sb,  C = Ca + Cb + 1;  free (no rounding) when one operand is an exact power of two; an exact zero
                 times anything is an exact zero
  a / b          S = Sa Sb / b^2,  C = Ca + Cb + c_div     [err(a)/|b| + |a| err(b)/b^2]
  1 / b          S = Sb / b^2,  C = Cb + c_rcp
  sqrt(a)        S = Sa / sqrt(a),  C = Ca / 2 + c_sqrt    [err(a) / (2 sqrt(a)); Sa >= a makes S >= |v|]
  a^3            S = Sa^3,  C = 3 Ca + c_cube
  sin a, cos a   S = max(|v|, Sa if Ca > 0),  C = Ca + c_sin   [|d sin| <= 1]
  |a|, -a        unchanged
A branch (R1 < R2, tmagp > 0, the fracture tests) is taken on the exact values; inputs at a branch point are the edge cases
of the tests, asserted one by one with their exact outcome.

c_op by arithmetic model (1 ulp <= 2 u relative):
  "ieee"   the oracle: +, -, *, /, sqrt correctly rounded (1); glibc sin, cos, pow(x, 3.) within 1 ulp (2).
  "device" the shipped forms, as DESIGN section 4 bounds them: kid_rcp <= 1 ulp (2), then the product with it 1 more (the
           1.5 ulp of `a * Rcp`); kid_div <= 0.6 ulp (1.2); kid_sqrt <= 1 ulp (2); kid_cube <= 1 ulp (2); ocml sin, cos
           <= 1 ulp (2); plain sqrt and / (the radii, the damping coefficient) correctly rounded (1).
The expression tree is the source's: IB's for "ieee", pair_const / pair_geom / pair_finish of kid_mts.inc for "device" (the same
operations in the same order, with `x * kid_rcp(y)` where IB divides)."""
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 50
U = 2.0 ** -53
OUTPUTS = ("len", "tg1", "tg2", "relrot", "nstress", "sstress", "Fx", "Fy", "Fdx", "Fdy", "Tq", "Tdq", "To_q", "half_delta", "L", "Thick")
# the coefficients a sensitivity control perturbs (perturb={name: factor})
COEFFICIENTS = ("dem_spring_coef", "two_one_plus_poisson", "twelve", "two_thirds", "dem_damping_coef", "half_L_lever")
HEXDENOM = 1.0 / (2.0 * np.sqrt(3.0))   # the double of IB:987


class V:
    __slots__ = ("v", "s", "c")

    def __init__(self, v, s=None, c=0.0):
        self.v = mp.mpf(v)
        self.s = abs(float(v)) if s is None else float(s)
        self.c = float(c)


def _pow2(x):
    if x.c != 0.0 or x.v == 0:
        return False
    m, _ = mp.frexp(abs(x.v))
    return m == mp.mpf(0.5)


def _zero(x):
    return x.c == 0.0 and x.v == 0


def add(a, b, sign=1):
    if _zero(b):   # adding an exact zero rounds nothing
        return a
    if _zero(a):
        return b if sign > 0 else neg(b)
    v = a.v + b.v if sign > 0 else a.v - b.v
    if v == 0 and a.c == 0.0 and b.c == 0.0:   # x - x of exact operands
        return V(0.0)
    s = (a.s if a.c > 0 else 0.0) + (b.s if b.c > 0 else 0.0)
    return V(v, max(s, abs(float(v))), max(a.c, b.c) + 1.0)


def sub(a, b):
    return add(a, b, -1)


def mul(a, b):
    if _zero(a) or _zero(b):   # an exact zero times anything finite
        return V(0.0)
    free = _pow2(a) or _pow2(b)
    return V(a.v * b.v, a.s * b.s, a.c + b.c + (0.0 if free else 1.0))


def div(a, b, cost=1.0):
    return V(a.v / b.v, a.s * b.s / float(b.v * b.v), a.c + b.c + cost)


def rcp(b, cost):
    return V(1 / b.v, b.s / float(b.v * b.v), b.c + cost)


def sqrt(a, cost=1.0):
    v = mp.sqrt(a.v)
    return V(v, a.s / float(v) if v > 0 else 0.0, 0.5 * a.c + cost)


def cube(a, cost):
    return V(a.v ** 3, a.s ** 3, 3.0 * a.c + cost)


def trig(fn, a, cost):
    v = fn(a.v)
    return V(v, max(abs(float(v)), a.s if a.c > 0 else 0.0), a.c + cost)


def neg(a):
    return V(-a.v, a.s, a.c)


def fabs(a):
    return V(abs(a.v), a.s, a.c)


def const(x):
    return V(float(x))


MODELS = {"ieee": dict(rcp=None, div=1.0, sqrt=1.0, cube=2.0, sin=2.0),
          "device": dict(rcp=2.0, div=1.2, sqrt=2.0, cube=2.0, sin=2.0)}


def pair_one(P, latlon, x, model="device", perturb=None):
    """One pair.  P: dict of the doubles and switches read of kid_params and of the derived constants (constant_area,
    constant_radius, dem_K_damp); x: dict of the pair's doubles (two-element sequences for the per-berg ones, berg 0 evaluates).
    Returns ({output: V}, status, broke)."""
    m = MODELS[model]
    pf = {k: 1.0 for k in COEFFICIENTS}
    pf.update(perturb or {})

    def coef(name, val):   # a coefficient of the force law, perturbed in a sensitivity control
        return V(mp.mpf(float(val)) * mp.mpf(pf[name]))

    def over(a, b, rb):   # IB's a / b: the device multiplies by a kid_rcp it keeps
        return div(a, b) if m["rcp"] is None else mul(a, rb)

    def keep(b):
        return None if m["rcp"] is None else rcp(b, m["rcp"])
    k_spring = coef("dem_spring_coef", P["dem_spring_coef"])
    interacting = x["id"][0] != x["id"][1] and x["fl_k"][0] != -1 and x["fl_k"][1] != -1   # IB:995
    Tk, To = const(x["thickness"][0]), const(x["thickness"][1])
    if P["constant_interaction_LW"]:   # IB:997-1005
        ca, rho = const(P["constant_area"]), const(P["rho_bergs"])
        M1, M2 = mul(mul(ca, Tk), rho), mul(mul(ca, To), rho)
        R1 = const(P["constant_radius"]); R2 = R1; Rmin = R1; l0 = mul(const(2.0), R1); T_Rmin = To
    else:   # IB:1008-1032
        M1, M2 = const(x["mass"][0]), const(x["mass"][1])
        A1, A2 = mul(const(x["length"][0]), const(x["width"][0])), mul(const(x["length"][1]), const(x["width"][1]))
        if P["hexagonal_icebergs"]:
            R1, R2 = sqrt(mul(A1, const(HEXDENOM))), sqrt(mul(A2, const(HEXDENOM)))
        else:
            R1, R2 = mul(const(0.5), sqrt(A1)), mul(const(0.5), sqrt(A2))
        if R1.v < R2.v:
            Rmin, T_Rmin = R1, Tk
        else:
            Rmin, T_Rmin = R2, To
        l0 = add(R1, R2)
    # IB:1039-1044, convert_from_grid_to_meters IB:444-459
    latK, latO = const(x["lat"][0]), const(x["lat"][1])
    if latlon:
        pi_180 = div(const(P["pi"]), const(180.0))
        lat_ref = mul(const(0.5), add(latK, latO))
        dx_dlon = mul(mul(pi_180, const(P["Rearth"])), trig(mp.cos, mul(lat_ref, pi_180), m["sin"]))
        dy_dlat = mul(pi_180, const(P["Rearth"]))
    else:
        dx_dlon, dy_dlat = const(1.0), const(1.0)
    rx = mul(sub(const(x["lon"][0]), const(x["lon"][1])), dx_dlon)
    ry = mul(sub(latK, latO), dy_dlat)
    length = sqrt(add(mul(rx, rx), mul(ry, ry)), m["sqrt"])
    out = {"len": length}
    zero_len = length.v == 0
    if not interacting or zero_len:
        return out, (1 if not interacting else 2), False
    rlen = keep(length)
    n1, n2 = over(rx, length, rlen), over(ry, length, rlen)   # IB:1048
    half_delta = mul(const(0.5), sub(l0, length))   # IB:1050
    RR1, RR2 = sub(R1, half_delta), sub(R2, half_delta)   # IB:1053-1055
    RR1x, RR1y, RR2x, RR2y = mul(RR1, n1), mul(RR1, n2), mul(RR2, n1), mul(RR2, n2)
    Lw = mul(const(2.0), add(Rmin, over(mul(sub(Rmin, half_delta), fabs(sub(R1, R2))), length, rlen)))   # IB:1058
    Thick = add(T_Rmin, over(mul(sub(Rmin, half_delta), fabs(sub(Tk, To))), length, rlen))   # IB:1061
    rl0 = keep(l0)
    Fn = over(mul(mul(mul(mul(k_spring, Thick), const(2.0)), half_delta), Lw), l0, rl0)   # IB:1070
    Fn_y = mul(Fn, n2); Fn_x = mul(Fn, n1)
    ur, vr = sub(const(x["u"][0]), const(x["u"][1])), sub(const(x["v"][0]), const(x["v"][1]))   # IB:1073
    wk, wo = const(x["w"][0]), const(x["w"][1])
    t1, t2, dt = const(x["t1"]), const(x["t2"]), const(x["dt"])
    tmag = add(mul(t1, t1), mul(t2, t2))   # IB:1077-1089
    tdn = add(mul(t1, n1), mul(t2, n2))
    tp1, tp2 = sub(t1, mul(tdn, n1)), sub(t2, mul(tdn, n2))
    tmagp = add(mul(tp1, tp1), mul(tp2, tp2))
    if tmagp.v > 0:
        t_rat = sqrt(div(tmag, tmagp, m["div"]), m["sqrt"])
        tp1, tp2 = mul(t_rat, tp1), mul(t_rat, tp2)
    else:
        tp1, tp2 = const(0.0), const(0.0)
    rotu = add(mul(RR1y, wk), mul(RR2y, wo))   # IB:1093-1098
    rotv = neg(add(mul(RR1x, wk), mul(RR2x, wo)))
    ur2, vr2 = add(ur, rotu), add(vr, rotv)
    up = add(mul(ur2, n1), mul(vr2, n2)); vp = mul(up, n2); up = mul(up, n1)
    tg1, tg2 = add(tp1, mul(sub(ur2, up), dt)), add(tp2, mul(sub(vr2, vp), dt))   # IB:1105
    shear_den = mul(mul(l0, const(2.0)), add(const(1.0), const(P["poisson"])))
    if pf["two_one_plus_poisson"] != 1.0:
        shear_den = V(shear_den.v * mp.mpf(pf["two_one_plus_poisson"]), shear_den.s, shear_den.c)
    ss = over(mul(mul(neg(Lw), Thick), k_spring), shear_den, keep(shear_den))   # IB:1109-1111
    if P["ignore_tangential_force"]:
        ss = const(0.0)
    Fs_x, Fs_y = mul(ss, tg1), mul(ss, tg2)
    sstress = div(sqrt(add(mul(Fs_x, Fs_x), mul(Fs_y, Fs_y)), m["sqrt"]), mul(Lw, Thick), m["div"])   # IB:1112
    Ts = neg(sub(mul(RR1x, Fs_y), mul(RR1y, Fs_x)))   # IB:1115
    dw = sub(wk, wo)
    relrot = add(const(x["relrot0"]), mul(dw, dt))   # IB:1117
    arg = sub(const(x["rot"][0]), const(x["rot"][1]))
    if not P["orig_dem_moment_of_inertia"]:   # IB:1120-1125
        theta = trig(mp.sin, arg, m["sin"])
        twelve_l0 = mul(coef("twelve", 12.0), l0)
        Tr = over(mul(mul(mul(neg(k_spring), cube(Lw, m["cube"])), Thick), theta), twelve_l0, keep(twelve_l0))
    else:   # IB:1129-1132
        theta = arg
        two_thirds = coef("two_thirds", 2.0 / 3.0)
        Tr = mul(mul(mul(mul(neg(over(k_spring, l0, rl0)), two_thirds), cube(mul(const(0.5), Lw), m["cube"])), Thick), theta)
    lever = mul(mul(theta, const(0.5)), Lw)
    if pf["half_L_lever"] != 1.0:
        lever = V(lever.v * mp.mpf(pf["half_L_lever"]), lever.s, lever.c)
    nstress = mul(over(k_spring, l0, rl0), add(mul(const(-2.0), half_delta), fabs(lever)))   # IB:1136
    dc = mul(coef("dem_damping_coef", P["dem_damping_coef"]),
             sqrt(div(mul(mul(const(P["dem_K_damp"]), M1), M2), add(M1, M2))))   # IB:1164, 1208
    Fdx, Fdy = mul(neg(dc), ur), mul(neg(dc), vr)
    broke = bool(P["break_bonds_on_sub_steps"] and P["fracture_criterion_stress"] and
                 (nstress.v > mp.mpf(float(P["frac_thres_n"])) or sstress.v > mp.mpf(float(P["frac_thres_t"]))))   # IB:1140-1143
    pull = nstress.v < 0
    zero = const(0.0)
    if broke:   # IB:1162-1197
        Fx, Fy = (Fn_x, Fn_y) if pull else (zero, zero)
        if not pull:
            Fdx, Fdy = zero, zero
        Tq, Tdq, To_q = zero, zero, zero
    else:   # IB:1208-1222
        Fx, Fy = add(Fn_x, Fs_x), add(Fn_y, Fs_y)
        Tq, Tdq, To_q = add(Ts, Tr), mul(neg(dc), dw), sub(Ts, Tr)
    status = 3 if (not broke and P["break_bonds_on_sub_steps"] and not P["fracture_criterion_stress"]) else 0   # IB:1200
    out.update(tg1=tg1, tg2=tg2, relrot=relrot, nstress=nstress, sstress=sstress, Fx=Fx, Fy=Fy, Fdx=Fdx, Fdy=Fdy, Tq=Tq, Tdq=Tdq,
               To_q=To_q, half_delta=half_delta, L=Lw, Thick=Thick)
    return out, status, broke


# ---------------------------------------------------------------------------------------------------------------------------
# parameters and inputs
# ---------------------------------------------------------------------------------------------------------------------------
def derived(p):
    """constant_area, constant_radius, dem_K_damp as the library and the oracle derive them (FW:1436, 1453-1463, 1301)"""
    area = p.constant_length * p.constant_width
    if p.hexagonal_icebergs:
        radius = float(np.sqrt(area / (2.0 * np.sqrt(3.0))))
    elif p.iceberg_bonds_on:
        radius = float(0.5 * np.sqrt(area))
    else:
        radius = float(np.sqrt(area / p.pi))
    return area, radius, 2.0 * p.dem_spring_coef / (3.0 * (1.0 - p.poisson * p.poisson))


def params_dict(p):
    area, radius, kd = derived(p)
    d = {k: getattr(p, k) for k in ("dem_spring_coef", "poisson", "dem_damping_coef", "rho_bergs", "pi", "Rearth", "frac_thres_n", "frac_thres_t",
                                    "constant_interaction_LW", "hexagonal_icebergs", "ignore_tangential_force", "orig_dem_moment_of_inertia",
                                    "break_bonds_on_sub_steps", "fracture_criterion_stress")}
    d.update(constant_area=area, constant_radius=radius, dem_K_damp=kd)
    return d


def base_params(**kw):
    """the DEM namelist of config 4 (icebergs_amd.synthetic.config_c4) as far as the pair force reads it; fracture off"""
    from icebergs_amd import synthetic as S
    p = S.default_params()
    p.mts, p.dem, p.iceberg_bonds_on = 1, 1, 1
    p.hexagonal_icebergs, p.constant_interaction_LW = 1, 1
    p.poisson, p.dem_damping_coef, p.dem_spring_coef = 0.3, 1.0, 5.0e6
    area = (3.0 * np.sqrt(3.0) / 2.0) * ((4.0 / 3.0) * 1500.0 ** 2)
    p.constant_length = p.constant_width = float(np.sqrt(area))
    p.break_bonds_on_sub_steps, p.fracture_criterion_stress, p.frac_thres_n, p.frac_thres_t = 0, 1, 1850.0, 1000.0
    p.use_broken_bonds_for_substep_contact = 1
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


PER_BERG = ("fl_k", "thickness", "mass", "length", "width", "lon", "lat", "u", "v", "w", "rot")
PER_PAIR = ("t1", "t2", "relrot0", "dt")


def empty_inputs(n):
    x = {f: np.zeros((n, 2)) for f in PER_BERG}
    x.update({f: np.zeros(n) for f in PER_PAIR})
    x["id"] = np.stack([np.arange(1, 2 * n, 2, dtype=np.int64), np.arange(2, 2 * n + 1, 2, dtype=np.int64)], axis=1)
    return x


def geometry(p, latlon, rng, n, strain, radii="equal", thick="equal", lat_max=85.0):
    """n pairs of elements of radius ~1500 m, the second at distance l0 (1 - strain) of the first in a uniformly random direction
    (strain > 0: compression).  l0 is formed as the routine forms it, so that strain = 0 leaves |l0 - len| at rounding size."""
    x = empty_inputs(n)
    hexa = bool(p.hexagonal_icebergs)
    r = np.full((n, 2), 1500.0)
    if radii != "equal":
        r[:, 0] *= rng.uniform(0.6, 1.0, n) if radii == "less" else (rng.uniform(1.0, 1.6, n) if radii == "greater" else rng.uniform(0.6, 1.6, n))
        if radii == "mixed":
            r[::3, 0] = r[::3, 1]
    area = r * r / HEXDENOM if hexa else (2.0 * r) ** 2
    x["length"][:] = np.sqrt(area) * 1.25
    x["width"][:] = area / x["length"]
    x["thickness"][:] = 200.0
    if thick != "equal":
        x["thickness"][:] = rng.uniform(120.0, 320.0, (n, 2))
    x["mass"][:] = x["thickness"] * p.rho_bergs * x["length"] * x["width"]
    if p.constant_interaction_LW:
        l0 = np.full(n, 2.0 * derived(p)[1])
    else:
        A = x["length"] * x["width"]
        R = np.sqrt(A * HEXDENOM) if hexa else 0.5 * np.sqrt(A)
        l0 = R[:, 0] + R[:, 1]
    ln = l0 * (1.0 - strain)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    if latlon:
        x["lon"][:, 0] = rng.uniform(-280.0, 80.0, n)
        x["lat"][:, 0] = rng.uniform(-lat_max, lat_max, n)
        x["lat"][::7, 0] = np.sign(x["lat"][::7, 0]) * rng.uniform(lat_max - 1.0, lat_max, len(x["lat"][::7, 0]))
        dy = (p.pi / 180.0) * p.Rearth
        x["lat"][:, 1] = x["lat"][:, 0] - ln * np.sin(phi) / dy
        dx = dy * np.cos(0.5 * (x["lat"][:, 0] + x["lat"][:, 1]) * (p.pi / 180.0))
        x["lon"][:, 1] = x["lon"][:, 0] - ln * np.cos(phi) / dx
    else:
        x["lon"][:, 0] = rng.uniform(2.0e4, 2.0e5, n)
        x["lat"][:, 0] = rng.uniform(2.0e4, 2.0e5, n)
        x["lon"][:, 1] = x["lon"][:, 0] - ln * np.cos(phi)
        x["lat"][:, 1] = x["lat"][:, 0] - ln * np.sin(phi)
    x["_phi"] = phi
    x["dt"][:] = 9.0   # dt / mts_sub_steps of config 4
    return x


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


N_FAMILY = 600   # pairs per family (the reference takes ~1.5 ms per pair)


@functools.lru_cache(maxsize=None)
def families():
    """[(name, params, latlon, inputs, coefficients it must see, outputs that show them)]: the mechanism families first (each leaves
    one term of the force non-zero), then the mixtures."""
    fam = []
    n = N_FAMILY
    zero = np.zeros(n)

    def tangent(x, mag):   # a vector of size `mag` at a random angle of 20..160 degrees to the pair's axis (either side)
        a = x["_phi"] + np.sign(rng.uniform(-1, 1, n)) * rng.uniform(np.pi / 9, 8 * np.pi / 9, n)
        return mag * np.cos(a), mag * np.sin(a)
    for sgn, name in ((1.0, "normal_compression"), (-1.0, "normal_tension")):
        rng = np.random.default_rng(101 if sgn > 0 else 102)
        p = base_params()
        fam.append((name, p, 0, geometry(p, 0, rng, n, sgn * log_uniform(rng, 1e-6, 1e-1, n)), ("dem_spring_coef",), ("Fx", "Fy", "nstress")))
    rng = np.random.default_rng(103)
    p = base_params(dem_damping_coef=0.0)
    x = geometry(p, 0, rng, n, zero)
    x["t1"], x["t2"] = tangent(x, log_uniform(rng, 1e-3, 10.0, n))
    fam.append(("stored_tangential", p, 0, x, ("dem_spring_coef", "two_one_plus_poisson"), ("Fx", "Fy", "sstress", "Tq", "To_q")))
    rng = np.random.default_rng(104)
    x = geometry(p, 0, rng, n, zero)
    du, dv = tangent(x, log_uniform(rng, 1e-4, 1.0, n))
    x["u"][:, 0] = rng.uniform(-0.5, 0.5, n); x["v"][:, 0] = rng.uniform(-0.5, 0.5, n)
    x["u"][:, 1] = x["u"][:, 0] - du; x["v"][:, 1] = x["v"][:, 0] - dv
    fam.append(("tangential_velocity", p, 0, x, ("two_one_plus_poisson",), ("Fx", "Fy", "sstress", "Tq", "To_q")))
    rng = np.random.default_rng(105)
    x = geometry(p, 0, rng, n, zero)
    x["w"][:] = rng.uniform(-1e-3, 1e-3, (n, 2))
    x["relrot0"][:] = rng.uniform(-0.1, 0.1, n)
    fam.append(("rotation_velocity", p, 0, x, ("two_one_plus_poisson",), ("Fx", "Fy", "sstress", "Tq", "To_q")))
    for orig, name, cf in ((0, "bending_wang", "twelve"), (1, "bending_original", "two_thirds")):
        rng = np.random.default_rng(106 + orig)
        p = base_params(orig_dem_moment_of_inertia=orig)
        x = geometry(p, 0, rng, n, zero)
        x["rot"][:, 0] = rng.uniform(-3.0, 3.0, n)
        arg = np.where(np.arange(n) % 3 == 0, rng.uniform(-3.0, 3.0, n), rng.uniform(-1.0, 1.0, n) * log_uniform(rng, 1e-6, 0.25, n))
        x["rot"][:, 1] = x["rot"][:, 0] - arg
        fam.append((name, p, 0, x, ("dem_spring_coef", cf, "half_L_lever"), ("Tq", "To_q", "nstress")))
    rng = np.random.default_rng(108)
    p = base_params()
    x = geometry(p, 0, rng, n, zero)
    x["u"][:] = rng.uniform(-0.5, 0.5, (n, 2)); x["v"][:] = rng.uniform(-0.5, 0.5, (n, 2)); x["w"][:] = rng.uniform(-1e-3, 1e-3, (n, 2))
    x["dt"][:] = 0.0
    fam.append(("damping", p, 0, x, ("dem_damping_coef",), ("Fdx", "Fdy", "Tdq")))
    # mixtures: everything at once
    seed = 200
    for lw in (1, 0):
        for hexa in (1, 0):
            for latlon in (0, 1):
                for ignore in ((0, 1) if (lw, hexa, latlon) == (0, 1, 0) else (0,)):
                    seed += 1
                    rng = np.random.default_rng(seed)
                    p = base_params(constant_interaction_LW=lw, hexagonal_icebergs=hexa, ignore_tangential_force=ignore,
                                    orig_dem_moment_of_inertia=seed & 1, max_bonds=6 if hexa else 4)
                    strain = np.sign(rng.uniform(-1, 1, n)) * log_uniform(rng, 1e-6, 1e-1, n)
                    x = geometry(p, latlon, rng, n, strain, radii="mixed", thick="mixed")
                    x["t1"], x["t2"] = tangent(x, log_uniform(rng, 1e-3, 10.0, n))
                    x["u"][:] = rng.uniform(-0.5, 0.5, (n, 2)); x["v"][:] = rng.uniform(-0.5, 0.5, (n, 2))
                    x["w"][:] = rng.uniform(-1e-3, 1e-3, (n, 2)); x["relrot0"][:] = rng.uniform(-0.1, 0.1, n)
                    x["rot"][:] = rng.uniform(-0.3, 0.3, (n, 2))
                    fam.append(("mix_lw%d_hex%d_%s%s" % (lw, hexa, "latlon" if latlon else "cart", "_notang" if ignore else ""), p, latlon, x, (), ()))
    for f in fam:
        f[3].pop("_phi", None)
    return fam


def pair_inputs(x, e):
    d = {f: (float(x[f][e, 0]), float(x[f][e, 1])) for f in PER_BERG}
    d.update({f: float(x[f][e]) for f in PER_PAIR})
    d["id"] = (int(x["id"][e, 0]), int(x["id"][e, 1]))
    return d


def reference(p, latlon, x, model, perturb=None):
    """{output: (exact values as mpf, bound of |computed - exact| as floats = C u S, C as floats)}, status, broke for all the pairs"""
    P = params_dict(p)
    n = len(x["dt"])
    ex = {o: [mp.mpf(0)] * n for o in OUTPUTS}
    bound = {o: np.zeros(n) for o in OUTPUTS}
    cc = {o: np.zeros(n) for o in OUTPUTS}
    status, broke = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for e in range(n):
        out, status[e], b = pair_one(P, latlon, pair_inputs(x, e), model, perturb)
        broke[e] = 1 if b else 0
        for o, val in out.items():
            ex[o][e] = val.v
            bound[o][e] = val.c * U * val.s
            cc[o][e] = val.c
    return ex, bound, cc, status, broke


@functools.lru_cache(maxsize=None)
def family_reference(index, model, perturb=None):
    name, p, latlon, x, _, _ = families()[index]
    return reference(p, latlon, x, model, dict(perturb) if perturb else None)


def ratios(got, ex, bound):
    """|got - exact| / bound per element; 0 where both vanish, inf where the bound is 0 and the value is not the exact one"""
    r = np.zeros(len(got))
    for e in range(len(got)):
        d = abs(float(mp.mpf(float(got[e])) - ex[e]))
        r[e] = (d / bound[e]) if bound[e] > 0 else (0.0 if d == 0.0 else np.inf)
    return r


# The constants C of |computed - exact| <= C u S that the rules above give, per output: the largest over the namelist switches of
# the families on a Cartesian grid, then on a lat-lon grid (the cosine of the mid latitude and pi/180 join every length).  What the
# tests assert is each element's own C (it depends on the switches and on which operands are exact, never on the values), which is
# never more than this; DESIGN section 4 quotes the table.  test_dem_pair_cpu.py::test_derived_constants_are_the_table holds it to the
# rules.  Reading one line of it, Fx on a Cartesian grid with the device's forms: len = kid_sqrt(rx^2 + ry^2) is 4 (two exact
# differences squared and added: 1 + 1 + 1 + 1 = 4, halved by the root, + 2 for kid_sqrt), rlen 6, n1 = rx rlen 8, half_delta 5,
# L and Thick 16 to 18 (Rmin - half_delta, |R1 - R2| of two rooted areas, rlen, three products, two sums), then the five products of
# Fn = k Thick 2 half_delta L rl0 and the one with n1: 63; Fs = ss tg with tg at 46.6 (the projection of the stored displacement
# on the new tangent, rescaled by kid_sqrt(kid_div(tmag, tmagp))) and ss at 43: 91.6; their sum 92.6.
DERIVED_C = {
    "device": {"len": (4.0, 13.0), "tg1": (46.6, 118.6), "tg2": (46.6, 112.6), "relrot": (3.0, 3.0), "nstress": (30.0, 46.0), "sstress": (130.8, 274.8),
               "Fx": (92.6, 200.6), "Fy": (92.6, 194.6), "Fdx": (8.0, 8.0), "Fdy": (8.0, 8.0), "Tq": (109.6, 238.6), "Tdq": (8.0, 8.0),
               "To_q": (109.6, 238.6), "half_delta": (5.0, 14.0), "L": (18.0, 36.0), "Thick": (16.0, 34.0)},
    "ieee": {"len": (3.0, 12.0), "tg1": (33.5, 105.5), "tg2": (33.5, 99.5), "relrot": (3.0, 3.0), "nstress": (24.0, 40.0), "sstress": (98.5, 242.5),
             "Fx": (69.5, 177.5), "Fy": (69.5, 171.5), "Fdx": (8.0, 8.0), "Fdy": (8.0, 8.0), "Tq": (82.5, 211.5), "Tdq": (8.0, 8.0),
             "To_q": (82.5, 211.5)},
}


def check_family(index, got, status, broke, model, label, perturb=None):
    """The assertion of the two tests: every output of every pair of family `index` within its derived bound of the exact value.
    Returns {output: (largest C, worst |got - exact| / bound)}; prints them first."""
    name, p, latlon, x, _, _ = families()[index]
    ex, bound, cc, st_ref, br_ref = family_reference(index, model)
    assert np.array_equal(status, st_ref) and np.array_equal(broke, br_ref), "%s %s: status / broke differ from the reference" % (label, name)
    rep = {}
    for o in OUTPUTS:
        if o not in got:
            continue
        r = ratios(got[o], ex[o], bound[o])
        rep[o] = (float(cc[o].max()), float(r.max()))
    print("%s %-26s %s" % (label, name, "  ".join("%s %.0f (%.3f)" % (o, c, r) for o, (c, r) in rep.items())))
    for o, (c, r) in rep.items():
        assert c <= DERIVED_C[model][o][1 if latlon else 0] + 0.05, "%s %s: C of %s is %.1f, the table says less" % (label, name, o, c)
        assert r <= 1.0, "%s %s: %s is %.3f of its derived bound (C = %.1f) away from the exact value" % (label, name, o, r, c)
    return rep


def check_sensitivity(index, got, model, label):
    """The control of a mechanism family: against the same reference with one coefficient of the mechanism off by 1e-9 relative,
    the outputs that carry the mechanism must VIOLATE the bound (a family that cannot see its own coefficient is not testing it)."""
    name, p, latlon, x, coefs, outs = families()[index]
    _, bound, _, _, _ = family_reference(index, model)
    rep = {}
    for cf in coefs:
        ex, _, _, _, _ = family_reference(index, model, ((cf, 1.0 + 1.0e-9),))
        seen = {o: float(ratios(got[o], ex[o], bound[o]).max()) for o in outs}
        # (twelve and two_thirds sit in the torque only, the lever in nstress only, the shear modulus not in nstress)
        sees = {"twelve": ("Tq", "To_q"), "two_thirds": ("Tq", "To_q"), "half_L_lever": ("nstress",),
                "two_one_plus_poisson": tuple(o for o in outs if o != "nstress")}.get(cf, outs)
        rep[cf] = {o: seen[o] for o in sees}
        print("%s %-20s %-22s off by 1e-9: %s" % (label, name, cf, "  ".join("%s %.3g" % (o, v) for o, v in rep[cf].items())))
        for o, v in rep[cf].items():
            assert v > 10.0, "%s %s: %s does not see %s (worst ratio %.3g of the bound)" % (label, name, o, cf, v)
    return rep


# ---------------------------------------------------------------------------------------------------------------------------
# edges: each with its exact outcome.  evaluate(p, latlon, x) -> {"status", "broke", every output it has}: the device through the
# probe, or the oracle through ko_dem_pair (kind = "oracle": what the reference's FATALs leave is visible as error_count, and the
# routine returns there without the forces, as IB does)
# ---------------------------------------------------------------------------------------------------------------------------
def edge_pair(p, rot=(0.0, 0.0), strain=0.01, axis=False, seed=7):
    rng = np.random.default_rng(seed)
    x = geometry(p, 0, rng, 1, np.array([strain]))
    x.pop("_phi")
    if axis:   # the partner due west at the same y, 2048 m away: the difference, its root and the unit vector n = (1, 0) are exact in
        x["lat"][0, 1] = x["lat"][0, 0]   # any of the forms (a reciprocal of a power of two is), so "t parallel to n" is a statement
        x["lon"][0, 1] = x["lon"][0, 0] - 2048.0   # about doubles, not about a rounding
        assert x["lon"][0, 0] - x["lon"][0, 1] == 2048.0
    x["rot"][0] = rot
    return x


def check_edges(evaluate, kind):
    from icebergs_amd import synthetic as S
    FORCES = ("Fx", "Fy", "Fdx", "Fdy", "Tq", "Tdq", "To_q")

    def one(r, o):
        return float(r[o][0])
    # same id, a footloose child on either side: not an interacting pair (IB:995)
    p = base_params()
    for what in ("same_id", "fl_k0", "fl_k1"):
        x = edge_pair(p)
        if what == "same_id":
            x["id"][0, 1] = x["id"][0, 0]
        else:
            x["fl_k"][0, int(what[-1])] = -1.0
        r = evaluate(p, 0, x)
        assert r["status"][0] == 1 and r["broke"][0] == 0, (what, r["status"], r["broke"])
    # zero separation (the FATAL of IB:1046)
    x = edge_pair(p)
    x["lon"][0, 1], x["lat"][0, 1] = x["lon"][0, 0], x["lat"][0, 0]
    r = evaluate(p, 0, x)
    assert r["status"][0] == 2 and one(r, "len") == 0.0 and r["broke"][0] == 0, (r["status"], r["len"])
    # tmagp == 0 (IB:1084-1089): no stored displacement, and a stored displacement along the pair's axis -- nothing tangential
    for t in (0.0, 0.37):
        x = edge_pair(p, axis=True)
        x["t1"][0] = t
        r = evaluate(p, 0, x)
        assert r["status"][0] == 0 and one(r, "tg1") == 0.0 and one(r, "tg2") == 0.0 and one(r, "sstress") == 0.0, (t, r["tg1"], r["tg2"], r["sstress"])
        assert one(r, "Fy") == 0.0 and one(r, "Tq") == 0.0 and one(r, "To_q") == 0.0 and one(r, "Fx") != 0.0, (t, r["Fy"], r["Tq"])
    # the fracture tests are `>` (IB:1143): a stress exactly at its threshold holds, one ulp above it breaks
    x = edge_pair(p, rot=(0.02, -0.01), strain=-0.002)
    x["t1"][0], x["t2"][0] = 0.11, -0.07
    x["u"][0], x["v"][0], x["w"][0] = (0.3, 0.1), (-0.2, 0.05), (1e-4, -2e-4)
    whole = evaluate(p, 0, x)
    ns, ss = one(whole, "nstress"), one(whole, "sstress")
    assert whole["status"][0] == 0 and ns > 0.0 and ss > 0.0
    q = base_params(break_bonds_on_sub_steps=1, frac_thres_n=ns, frac_thres_t=ss)
    r = evaluate(q, 0, x)
    assert r["broke"][0] == 0 and r["status"][0] == 0 and all(one(r, o) == one(whole, o) for o in FORCES), "at the thresholds"
    for tn, tt in ((np.nextafter(ns, -np.inf), ss), (ns, np.nextafter(ss, -np.inf))):
        q = base_params(break_bonds_on_sub_steps=1, frac_thres_n=float(tn), frac_thres_t=float(tt))
        r = evaluate(q, 0, x)
        # broken with nstress >= 0: nothing is left of the bond (IB:1172-1179)
        assert r["broke"][0] == 1 and r["status"][0] == 0 and all(one(r, o) == 0.0 for o in FORCES), ("one ulp above", tn, tt, {o: one(r, o) for o in FORCES})
        assert one(r, "nstress") == ns and one(r, "sstress") == ss and one(r, "tg1") == one(whole, "tg1")
    # broken in shear under compression (nstress < 0): the normal force and the damping stay, shear and torques go (IB:1162-1175)
    x = edge_pair(p, strain=0.003)
    x["t1"][0], x["t2"][0] = 0.4, 0.9
    x["u"][0], x["v"][0], x["w"][0] = (0.3, 0.1), (-0.2, 0.05), (1e-4, -2e-4)
    whole = evaluate(p, 0, x)
    normal = evaluate(base_params(ignore_tangential_force=1), 0, x)   # Fx = Fn_x + 0 there
    assert one(whole, "nstress") < 0.0 and one(whole, "sstress") > 0.0 and one(normal, "Fx") != one(whole, "Fx")
    q = base_params(break_bonds_on_sub_steps=1, frac_thres_n=1850.0, frac_thres_t=float(np.nextafter(one(whole, "sstress"), -np.inf)))
    r = evaluate(q, 0, x)
    assert r["broke"][0] == 1 and r["status"][0] == 0
    assert one(r, "Fx") == one(normal, "Fx") and one(r, "Fy") == one(normal, "Fy"), "the normal force stays"
    assert one(r, "Fdx") == one(whole, "Fdx") and one(r, "Fdy") == one(whole, "Fdy") and one(r, "Fdx") != 0.0, "the damping stays"
    assert one(r, "Tq") == 0.0 and one(r, "Tdq") == 0.0 and one(r, "To_q") == 0.0, "no torque"
    # fracture on the sub-steps without the stress criterion (the FATAL of IB:1200)
    q = base_params(break_bonds_on_sub_steps=1, fracture_criterion_stress=0)
    r = evaluate(q, 0, x)
    assert r["status"][0] == 3 and r["broke"][0] == 0
    assert all(one(r, o) == one(whole, o) for o in ("len", "tg1", "tg2", "relrot", "nstress", "sstress"))
    if kind == "device":   # the forces are still returned
        assert all(one(r, o) == one(whole, o) for o in FORCES)
    else:                  # the routine stops there, as IB does
        assert all(one(r, o) == 0.0 for o in FORCES)
