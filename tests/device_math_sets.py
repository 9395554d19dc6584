"""Input sets, references and the error metric shared by tests/test_device_math_gpu.py and tests/test_device_math_cpu.py.

Every set is fixed-seed and holds about 2e4 values (313 waves and a partial one): a log-uniform sweep of the form's stated domain
and, at every binade of a coarse exponent sweep, the mantissa patterns at which an iteration's rounding goes wrong first -- all
ones, a single bit, 1 plus or minus a few ulp.

A reference is a pair (hi, lo) of float64 arrays: hi the correctly rounded exact result, lo the rest, good to 2^-10 ulp or better.
np.longdouble (x87: 64-bit significand, correctly rounded +, -, *, /, sqrt) serves reciprocal, quotient and square root; powers,
sine and cosine come from mpmath at 50 digits.  The error in ulps is |got - exact| / spacing of the doubles at hi."""
import numpy as np

N = 20000

# What the hardware's first guesses are allowed (relative error): v_rcp_f64 and v_rsq_f64 are specified to 2^29 ulp of a double,
# 2^-23 (the CDNA ISA guide; the source comments say "~2^-26" and "~23 bits"); the single-precision exp2/log seed of the fifth-root
# forms 3e-6, the figure the comment's 50-digit check of the two Newton steps assumed.
BAND_RCP = 2.0 ** -23
BAND_RSQ = 2.0 ** -23
BAND_RPOW5 = 3e-6

# The bounds: the claims of the source comments (kid_device.hpp, kid_thermo.hpp) read as hard numbers, in ulps.
#
# kid_pow08 = x * r and kid_mul_rpow5 = a * r with r = kid_rpow5_newton(x) are the exception.  The comment used to say "within ~1 ulp
# of pow" of both; that holds for r itself and cannot hold for a product with it, so the claim was replaced by this derivation (u =
# 2^-53; an error of rho * u relative is at most rho ulps, the spacing of the doubles at v being between u |v| and 2 u |v|):
#   * the last Newton step is r + r (0.2 e) with e = fma(-x, r^5, 1).  r^5 is formed by three rounded products r2 = r r, r4 = r2 r2,
#     r5 = r4 r, relative error <= (2 + 1 + 1) u, and x r^5 is within 1e-10 of 1: e carries an absolute error <= 4 u (its own
#     rounding is relative to |e| < 1e-10 and does not count), so r (1 + 0.2 e) is off by <= 0.8 u relative; what the step before
#     left (the seed's 3e-6 squared twice, ~1e-22) does not count either;
#   * the final fma rounds once: r is within 0.8 + 0.5 = 1.3 ulp by this count (the table's 1 ulp is the claim that is asserted);
#     relative to the exact root that is <= 0.8 u + 1 u = 1.8 u;
#   * the product x * r (a * r) keeps the 1.8 u, at most 1.8 ulps of the product, and rounds once more: <= 2.3 ulp.
BOUND = {"kid_rcp": 1.0, "mul_rcp": 1.5, "kid_div": 0.6, "kid_sqrt": 1.0, "kid_rsqrt": 1.0, "kid_rpow5": 1.0, "kid_pow08": 2.3,
         "mul_rpow5": 2.3, "kid_root4": 1.0, "kid_cube": 1.0, "sin15": 1.0}
POWR_REL = 2e-15      # kid_powr: exp(y log x), relative, on |y log x| < 8
SQRT_NN_FLOOR = 1e-300


def log_uniform(lo, hi, n, seed):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def patterns(e_lo, e_hi, step):
    """Mantissa patterns at the binades 2^e, e = e_lo, e_lo + step, ... <= e_hi (all normal doubles)."""
    out = []
    for e in range(e_lo, e_hi + 1, step):
        one = np.ldexp(1.0, e)
        vals = [one, np.nextafter(np.ldexp(1.0, e + 1), 0.0)]                       # 1.000..0, 1.111..1
        vals += [one * (1.0 + 2.0 ** -k) for k in (1, 2, 3, 8, 21, 26, 27, 40, 51, 52)]   # a single bit
        up = dn = one
        for _ in range(4):                                                         # 1 +- a few ulp
            up = np.nextafter(up, np.inf); dn = np.nextafter(dn, 0.0)
            vals += [up, dn]
        out += vals
    return np.array(out, dtype=np.float64)


def make_set(lo, hi, seed, e_step=8):
    """About N values in [lo, hi]: the patterns of every e_step-th binade inside, the rest log-uniform."""
    e_lo, e_hi = int(np.ceil(np.log2(lo))) + 1, int(np.floor(np.log2(hi))) - 1
    pat = patterns(e_lo, e_hi, e_step)
    pat = pat[(pat >= lo) & (pat <= hi)]
    return np.concatenate([pat, log_uniform(lo, hi, max(N - pat.size, 1000), seed)])


# ---- the sets -------------------------------------------------------------------------------------------------------------------
# Divisors: 2^-900 .. 2^900, so that with numerators in 1e-6 .. 1e6 the quotient, the residual a - b q and the correction all stay
# normal numbers; the ends of the exponent range are edges with asserts of their own.
def divisors():
    x = make_set(2.0 ** -900, 2.0 ** 900, 11, e_step=16)
    sign = np.where(np.random.default_rng(12).random(x.size) < 0.25, -1.0, 1.0)
    return x * sign


def numerators(n):
    a = log_uniform(1e-6, 1e6, n, 13)
    a[::7] = patterns(-3, 3, 1)[np.arange(a[::7].size) % patterns(-3, 3, 1).size]
    return a * np.where(np.random.default_rng(14).random(n) < 0.25, -1.0, 1.0)


def sqrt_args():       # kid_sqrt, kid_sqrt_nn: the documented domain, 1e-300 and up
    return make_set(1e-300, 1.7e308, 21, e_step=16)


def rsqrt_args():
    return make_set(1e-300, 1e300, 22, e_step=16)


def rpow5_args():      # the fast range of the fifth-root forms
    x = make_set(1e-30, 1e30, 31, e_step=2)
    return x[(x > 1e-30) & (x < 1e30)]


def powr_args(y):      # |y log x| < 8
    lim = np.exp(7.999 / y)
    return make_set(1.0 / lim, lim, 41, e_step=1)


def small_args():      # the sine series: |x| < 0.25
    x = make_set(1e-20, 0.2499999, 51, e_step=1)
    x = x[np.abs(x) < 0.25]
    return np.concatenate([x, -x[::3], [0.0, np.nextafter(0.25, 0.0), -np.nextafter(0.25, 0.0)]])


def cube_args():
    return make_set(1e-90, 1e90, 61, e_step=4)


# ---- references -----------------------------------------------------------------------------------------------------------------
def split_ld(v):
    """(hi, lo) of a longdouble array."""
    hi = v.astype(np.float64)
    return hi, (v - hi.astype(np.longdouble)).astype(np.float64)


def ref_ld(fn, *args):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not the x87 extended format here"
    with np.errstate(all="ignore"):
        return split_ld(fn(*[np.asarray(a, dtype=np.float64).astype(np.longdouble) for a in args]))


def ref_mp(fn, *args):
    """(hi, lo) of fn applied elementwise with mpmath at 50 digits; fn takes and returns mpf."""
    import mpmath as mp
    with mp.workdps(50):
        hi = np.empty(len(args[0])); lo = np.empty(len(args[0]))
        for k, vs in enumerate(zip(*args)):
            e = fn(*[mp.mpf(float(v)) for v in vs])
            h = float(e)
            hi[k] = h; lo[k] = float(e - mp.mpf(h))
    return hi, lo


def ulp_err(got, ref):
    """|got - exact| / spacing of the doubles at the correctly rounded exact result."""
    hi, lo = ref
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.abs((got - hi) - lo) / np.spacing(np.abs(hi))


def rel_err(got, ref):
    hi, lo = ref
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo) / np.abs(hi)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def worst(err, *cols):
    """(largest error, the inputs there) for the printed table."""
    k = int(np.nanargmax(err))
    return float(err[k]), tuple(float(c[k]) for c in cols)


def write_host_sets(path):
    """The file tests/device_math_host.cpp reads: five arrays, each an int64 count and that many doubles."""
    b = np.abs(divisors())
    sets = [b, np.abs(numerators(b.size)), sqrt_args(), rsqrt_args(), rpow5_args()]
    with open(path, "wb") as f:
        for s in sets:
            s = np.ascontiguousarray(s, dtype=np.float64)
            np.array([s.size], dtype=np.int64).tofile(f)
            s.tofile(f)
