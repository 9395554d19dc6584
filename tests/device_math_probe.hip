// device_math_probe.hip -- test-only library (libkid_math_probe.so): every trimmed arithmetic form of the per-berg path applied
// elementwise to fp64 arrays, one lane per element, so that tests/test_device_math_gpu.py can hold each of them to a
// high-precision reference in isolation.  Built with exactly the library's flags (-ffp-contract=off among them): the instruction
// sequence of a form here is the one the library's kernels inline.  Never loaded by icebergs_amd/lib.py.
#include "../include/kid.h"
#include "../icebergs_amd/csrc/kid_device.hpp"
#include "../icebergs_amd/csrc/kid_thermo.hpp"

#ifdef KID_EXACT_MATH
#error "the probe is for the shipped forms: build it without -DKID_EXACT_MATH"
#endif

namespace {
using namespace kid;

// the single-precision seed of kid_rpow5_newton, as that function forms it
__device__ __forceinline__ double rpow5_seed(double x) { return (double)__builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf((float)x)); }

enum { U_RCP = 0, U_SQRT, U_SQRT_NN, U_RSQRT, U_POW08, U_RPOW5, U_POWR02, U_POWR08, U_ROOT4, U_CUBE, U_SEED_RCP, U_SEED_RSQ, U_SEED_RPOW5,
       U_SIN15, U_SIN, U_COUNT };
enum { B_MUL_RCP = 0, B_DIV, B_DIV_R, B_MUL_RPOW5, B_COUNT };
enum { L_CELL = 0, L_CELL_NOREF, L_NEAR, L_SINCOS, L_COUNT };

__global__ void __launch_bounds__(256) unary_kernel(int op, const double *__restrict__ x, double *__restrict__ out, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + (long long)threadIdx.x;
  if (k >= n) return;
  const double v = x[k];
  double r;
  switch (op) {
    case U_RCP: r = 1.0 * kid_rcp(v); break;
    case U_SQRT: r = kid_sqrt(v); break;
    case U_SQRT_NN: r = kid_sqrt_nn(v); break;
    case U_RSQRT: r = kid_rsqrt(v); break;
    case U_POW08: r = kid_pow08(v); break;
    case U_RPOW5: r = kid_mul_rpow5(1.0, v); break;
    case U_POWR02: r = kid_powr(v, 0.2); break;
    case U_POWR08: r = kid_powr(v, 0.8); break;
    case U_ROOT4: r = kid_root4(v); break;
    case U_CUBE: r = kid_cube(v); break;
    case U_SEED_RCP: r = __builtin_amdgcn_rcp(v); break;
    case U_SEED_RSQ: r = __builtin_amdgcn_rsq(v); break;
    case U_SEED_RPOW5: r = rpow5_seed(v); break;
    case U_SIN15: r = kid_sin_series15(v); break;
    default: r = sin(v); break;
  }
  out[k] = r;
}

__global__ void __launch_bounds__(256) binary_kernel(int op, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + (long long)threadIdx.x;
  if (k >= n) return;
  const double u = a[k], v = b[k];
  double r;
  switch (op) {
    case B_MUL_RCP: r = u * kid_rcp(v); break;
    case B_DIV: r = kid_div(u, v); break;
    case B_DIV_R: r = kid_div_r(u, v, kid_rcp(v)); break;
    default: r = kid_mul_rpow5(u, v); break;
  }
  out[k] = r;
}

// (lat, lat_c) -> s, c, dxdl.  sin / cos of the tabulated latitude come from the device's sincos of lat_c * pi_180, as
// pack_static_kernel fills DevGrid::latref and the RK4 stages carry (s1, c1) of stage 1.
__global__ void __launch_bounds__(256) lat_kernel(int op, DevGrid g, double pi, double Rearth, const double *__restrict__ lat, const double *__restrict__ latc,
                                                  double *__restrict__ s, double *__restrict__ c, double *__restrict__ dxdl, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + (long long)threadIdx.x;
  if (k >= n) return;
  kid_params p = {};   // the latitude terms read pi, Rearth and use_f_plane
  p.pi = pi; p.Rearth = Rearth; p.use_f_plane = 0;
  const double la = lat[k], lc = latc[k];
  double s_c, c_c;
  sincos(lc * g.pi_180, &s_c, &c_c);
  LatTerms t;
  switch (op) {
    case L_CELL: t = lat_terms_cell<0>(g, p, la, 0., lc, s_c, c_c, true); break;
    case L_CELL_NOREF: t = lat_terms_cell<0>(g, p, la, 0., lc, s_c, c_c, false); break;
    case L_NEAR: t = lat_terms_near<0>(g, p, la, 0., lc, s_c, c_c); break;
    default: t = lat_terms<0>(g, p, la, 0.); break;
  }
  s[k] = t.s; c[k] = t.c; dxdl[k] = 1.0 * t.dxdl;
}

int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}
unsigned blocks(long long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// x, a, b, out, ...: device pointers to n doubles each.  Returns the hipError_t of the launch (0: done), -1 for a bad argument.
extern "C" int kid_probe_unary(int op, const double *x, double *out, long long n) {
  if (op < 0 || op >= U_COUNT || n <= 0 || n > (1ll << 30) || !x || !out) return -1;
  hipLaunchKernelGGL(unary_kernel, dim3(blocks(n)), dim3(256), 0, 0, op, x, out, n);
  return finish();
}
extern "C" int kid_probe_binary(int op, const double *a, const double *b, double *out, long long n) {
  if (op < 0 || op >= B_COUNT || n <= 0 || n > (1ll << 30) || !a || !b || !out) return -1;
  hipLaunchKernelGGL(binary_kernel, dim3(blocks(n)), dim3(256), 0, 0, op, a, b, out, n);
  return finish();
}
extern "C" int kid_probe_lat(int op, double pi, double Rearth, const double *lat, const double *latc, double *s, double *c, double *dxdl, long long n) {
  if (op < 0 || op >= L_COUNT || n <= 0 || n > (1ll << 30) || !lat || !latc || !s || !c || !dxdl) return -1;
  DevGrid g = {};
  g.latlon = 1; g.pi_180 = pi / 180.; g.r180_pi = 180. / pi;   // as refresh_tables forms them
  hipLaunchKernelGGL(lat_kernel, dim3(blocks(n)), dim3(256), 0, 0, op, g, pi, Rearth, lat, latc, s, c, dxdl, n);
  return finish();
}
