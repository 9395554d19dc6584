// device_math_host.cpp -- the Newton and Goldschmidt iterations of icebergs_amd/csrc/kid_device.hpp and kid_thermo.hpp restated in
// plain C++17 with the hardware seed as an argument: the same fused multiply-adds and rounded products in the same order.
// Compile with -ffp-contract=off (a contracted product would be another operation than the device performs).
//
//   * as a shared object (tests/test_device_math_gpu.py, through ctypes): fed the seeds the device returned, the hm_* functions
//     must reproduce the device's results bit for bit -- fma and multiply are IEEE on both sides;
//   * as a program (tests/test_device_math_cpu.py, under AddressSanitizer and UndefinedBehaviorSanitizer): reads the input sets of
//     tests/device_math_sets.py from a file and, for seeds exact * (1 + delta) with delta swept over the band the GPU test allows
//     the hardware, prints the worst error of every form against long double and fails where a bound is missed: the bounds belong
//     to the iterations, not to one chip's seeds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
double rcp_it(double b, double r) {
  double e = std::fma(-b, r, 1.0);
  r = std::fma(r, e, r);
  e = std::fma(-b, r, 1.0);
  return std::fma(r, e, r);
}
double div_it(double a, double b, double r0) {
  const double r = rcp_it(b, r0);
  const double q = a * r;
  return std::fma(std::fma(-b, q, a), r, q);
}
double sqrt_core(double x, double y) {
  double g = x * y, h = 0.5 * y;
  const double r = std::fma(-h, g, 0.5);
  g = std::fma(g, r, g); h = std::fma(h, r, h);
  return std::fma(std::fma(-g, g, x), h, g);
}
double sqrt_it(double x, double y) {
  const double g = sqrt_core(x, y);
  const double inf = std::numeric_limits<double>::infinity();   // x > 0 and finite: the iteration; +-0, +inf: x; negative, NaN: NaN
  return (x > 0. && x < inf) ? g : ((x == 0. || x == inf) ? x : std::numeric_limits<double>::quiet_NaN());
}
double rsqrt_it(double x, double y) {
  double e = std::fma(-x * y, y, 1.0);
  y = std::fma(y, 0.5 * e, y);
  e = std::fma(-x * y, y, 1.0);
  return std::fma(y, 0.5 * e, y);
}
double rpow5_it(double x, double r) {
  for (int it = 0; it < 2; ++it) {
    const double r2 = r * r, r4 = r2 * r2;
    const double e = std::fma(-x, r4 * r, 1.0);
    r = std::fma(r, 0.2 * e, r);
  }
  return r;
}
}  // namespace

// op: 0 kid_rcp (1.0 * Rcp), 1 a * kid_rcp(b), 2 kid_div, 3 kid_div_r, 4 kid_sqrt, 5 kid_sqrt_nn (seed: of max(x, 1e-300)), 6 kid_rsqrt,
// 7 kid_rpow5_newton, 8 x * kid_rpow5_newton(x).  a: numerator (binary forms), x: divisor / argument, seed: the hardware's first guess.
extern "C" int hm_apply(int op, const double *a, const double *x, const double *seed, double *out, long long n) {
  if (op < 0 || op > 8 || n < 0) return -1;
  for (long long k = 0; k < n; ++k) {
    const double s = seed[k], v = x[k];
    switch (op) {
      case 0: out[k] = 1.0 * rcp_it(v, s); break;
      case 1: out[k] = a[k] * rcp_it(v, s); break;
      case 2: out[k] = div_it(a[k], v, s); break;
      case 3: { const double r = rcp_it(v, s), q = a[k] * r; out[k] = std::fma(std::fma(-v, q, a[k]), r, q); break; }
      case 4: out[k] = sqrt_it(v, s); break;
      case 5: out[k] = sqrt_core(v, s); break;
      case 6: out[k] = rsqrt_it(v, s); break;
      case 7: out[k] = rpow5_it(v, s); break;
      default: out[k] = v * rpow5_it(v, s); break;
    }
  }
  return 0;
}

namespace {
typedef long double ld;
double ulps(double got, ld exact) {
  const double d = (double)exact;   // correctly rounded
  const double sp = std::nextafter(std::fabs(d), std::numeric_limits<double>::infinity()) - std::fabs(d);
  return (double)(std::fabs((ld)got - exact) / (ld)sp);
}
struct Worst { double u = 0., x = 0., a = 0., delta = 0.; };
void note(Worst &w, double u, double x, double a, double delta) { if (!(u <= w.u)) { w.u = u; w.x = x; w.a = a; w.delta = delta; } }

bool read_set(FILE *f, std::vector<double> &v) {
  int64_t n = 0;
  if (std::fread(&n, sizeof n, 1, f) != 1 || n < 0 || n > (1 << 22)) return false;
  v.resize((size_t)n);
  return n == 0 || std::fread(v.data(), sizeof(double), (size_t)n, f) == (size_t)n;
}
}  // namespace

// usage: device_math_host SETS BAND_RCP BAND_RSQ BAND_RPOW5
// SETS holds five arrays, each an int64 count and that many doubles: divisors b, numerators a (as many as b), arguments of the
// square roots, arguments of 1/sqrt, arguments of the fifth-root forms -- all positive, finite and inside the forms' domains.
int main(int argc, char **argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: %s SETS BAND_RCP BAND_RSQ BAND_RPOW5\n", argv[0]); return 2; }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  std::vector<double> b, a, xs, xr, xp;
  const bool ok_read = read_set(f, b) && read_set(f, a) && read_set(f, xs) && read_set(f, xr) && read_set(f, xp) && a.size() == b.size();
  std::fclose(f);
  if (!ok_read) { std::fprintf(stderr, "bad input file\n"); return 2; }
  const double band_rcp = std::stod(argv[2]), band_rsq = std::stod(argv[3]), band_p5 = std::stod(argv[4]);
  const double frac[] = {-1., -0.75, -0.5, -0.125, -1. / 1024., 0., 1. / 1024., 0.125, 0.5, 0.75, 1.};
  Worst w_rcp, w_mul, w_div, w_sqrt, w_rsqrt, w_p5, w_p08;
  long long bits_div_r = 0, bits_sqrt_nn = 0, div_below_one = 0;
  for (double fr : frac) {
    for (size_t k = 0; k < b.size(); ++k) {
      const double d = fr * band_rcp, bv = b[k], av = a[k];
      const double seed = (double)(((ld)1 / (ld)bv) * ((ld)1 + (ld)d));
      const double r = rcp_it(bv, seed);
      note(w_rcp, ulps(r, (ld)1 / (ld)bv), bv, 1., d);
      note(w_mul, ulps(av * r, (ld)av / (ld)bv), bv, av, d);
      const double q = div_it(av, bv, seed);
      note(w_div, ulps(q, (ld)av / (ld)bv), bv, av, d);
      double q2; { const double qq = av * r; q2 = std::fma(std::fma(-bv, qq, av), r, qq); }
      if (std::memcmp(&q, &q2, sizeof q) != 0) ++bits_div_r;
      // the quotient of a >= b > 0 is never below 1, whatever the seed inside the band: accel's wave-uniform short cut of cr_q leans on it
      for (int j = 0; j <= 8; ++j) {
        double num = bv;
        for (int t = 0; t < j; ++t) num = std::nextafter(num, std::numeric_limits<double>::infinity());
        if (std::isfinite(num) && div_it(num, bv, seed) < 1.0) ++div_below_one;
      }
    }
    for (size_t k = 0; k < xs.size(); ++k) {
      const double d = fr * band_rsq, x = xs[k];
      const double seed = (double)(((ld)1 / sqrtl((ld)x)) * ((ld)1 + (ld)d));
      const double g = sqrt_it(x, seed);
      note(w_sqrt, ulps(g, sqrtl((ld)x)), x, 0., d);
      const double g2 = sqrt_core(x, seed);   // x >= 1e-300: max(x, 1e-300) = x, the same seed
      if (x >= 1e-300 && std::memcmp(&g, &g2, sizeof g) != 0) ++bits_sqrt_nn;
    }
    for (size_t k = 0; k < xr.size(); ++k) {
      const double d = fr * band_rsq, x = xr[k];
      const ld ex = (ld)1 / sqrtl((ld)x);
      note(w_rsqrt, ulps(rsqrt_it(x, (double)(ex * ((ld)1 + (ld)d))), ex), x, 0., d);
    }
    for (size_t k = 0; k < xp.size(); ++k) {
      const double d = fr * band_p5, x = xp[k];
      const ld ex = powl((ld)x, (ld)-0.2L);
      const double seed = (double)(float)(double)(ex * ((ld)1 + (ld)d));   // a single-precision seed, as on the device
      const double r = rpow5_it(x, seed);
      note(w_p5, ulps(r, ex), x, 0., d);
      note(w_p08, ulps(x * r, powl((ld)x, (ld)0.8L)), x, 0., d);
    }
  }
  struct Row { const char *name; const Worst *w; double bound; } rows[] = {
      {"kid_rcp", &w_rcp, 1.0}, {"mul_rcp", &w_mul, 1.5}, {"kid_div", &w_div, 0.6}, {"kid_sqrt", &w_sqrt, 1.0},
      {"kid_rsqrt", &w_rsqrt, 1.0}, {"kid_rpow5", &w_p5, 1.0}, {"kid_pow08", &w_p08, 2.3}};
  bool ok = true;
  for (const Row &r : rows) {
    std::printf("WORST %s %.6f bound %.2f at x=%a a=%a delta=%.3e\n", r.name, r.w->u, r.bound, r.w->x, r.w->a, r.w->delta);
    if (!(r.w->u <= r.bound)) ok = false;
  }
  std::printf("BITS kid_div_r %lld kid_sqrt_nn %lld DIV_BELOW_ONE %lld\n", bits_div_r, bits_sqrt_nn, div_below_one);
  if (bits_div_r != 0 || bits_sqrt_nn != 0 || div_below_one != 0) ok = false;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
