// dem_pair_probe.hip -- test-only library (libkid_dem_probe.so): the bonded pair force of the DEM sub-steps (pair_const, then
// pair_force_dem of kid_mts.inc, unchanged) evaluated for independent pairs, one lane per pair, so that tests/test_dem_pair_gpu.py
// can hold every output of it to a 50-digit reference element by element.  Built with exactly the library's flags
// (-ffp-contract=off among them) and from the library's own source of the pair functions: the instruction sequence here is the
// one bond_pass_kernel and mts_substeps_kernel inline.  Never loaded by icebergs_amd/lib.py.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "../include/kid.h"
#include "../icebergs_amd/csrc/kid_device.hpp"
#include "../icebergs_amd/csrc/kid_thermo.hpp"
#include "../icebergs_amd/csrc/kid_footloose.hpp"
#include "../icebergs_amd/csrc/kid_berg_kernel.hpp"

#ifdef KID_EXACT_MATH
#error "the probe is for the shipped forms: build it without -DKID_EXACT_MATH"
#endif

using namespace kid;

namespace {
#include "../icebergs_amd/csrc/kid_mts.inc"

enum { O_LEN = 0, O_TG1, O_TG2, O_RELROT, O_NSTRESS, O_SSTRESS, O_FX, O_FY, O_FDX, O_FDY, O_TQ, O_TDQ, O_TOQ, O_HALF_DELTA, O_L, O_THICK, O_COUNT };

// lane e: the pair (row 2e evaluates, row 2e+1 is its partner).  rec: 6 doubles per row {lon, lat, u, v, w, rot} (DemRec);
// out: O_COUNT planes of n doubles.
__global__ void __launch_bounds__(256) dem_pair_kernel(const DevGrid g, const kid_params p, const BergPtrs b, const MtsDev m, const double *__restrict__ rec,
                                                       const double *__restrict__ t1, const double *__restrict__ t2, const double *__restrict__ relrot0,
                                                       const double *__restrict__ dt, int32_t *__restrict__ status, int32_t *__restrict__ broke,
                                                       double *__restrict__ out, long long n) {
  const long long e = (long long)blockIdx.x * 256ll + (long long)threadIdx.x;
  if (e >= n) return;
  const long long k = 2 * e, o = 2 * e + 1;
  const DemRec K{rec[6 * k + 0], rec[6 * k + 1], rec[6 * k + 2], rec[6 * k + 3], rec[6 * k + 4], rec[6 * k + 5]};
  const DemRec O{rec[6 * o + 0], rec[6 * o + 1], rec[6 * o + 2], rec[6 * o + 3], rec[6 * o + 4], rec[6 * o + 5]};
  const PairConst c = pair_const(p, b, m, k, o);
  const PairOut r = pair_force_dem(g, p, m, c, K, O, t1[e], t2[e], relrot0[e], dt[e]);
  const PairMid q = pair_geom(g, p, m, c, K, O, t1[e], t2[e], relrot0[e], dt[e]);   // (the same values again: for the three it does not hand on)
  status[e] = r.status; broke[e] = r.broke ? 1 : 0;
  out[O_LEN * n + e] = r.len; out[O_TG1 * n + e] = r.tg1; out[O_TG2 * n + e] = r.tg2; out[O_RELROT * n + e] = r.relrot;
  out[O_NSTRESS * n + e] = r.nstress; out[O_SSTRESS * n + e] = r.sstress;
  out[O_FX * n + e] = r.Fx; out[O_FY * n + e] = r.Fy; out[O_FDX * n + e] = r.Fdx; out[O_FDY * n + e] = r.Fdy;
  out[O_TQ * n + e] = r.Tq; out[O_TDQ * n + e] = r.Tdq; out[O_TOQ * n + e] = r.To_q;
  out[O_HALF_DELTA * n + e] = q.half_delta; out[O_L * n + e] = q.L; out[O_THICK * n + e] = q.Thick;
}
}  // namespace

// Every pointer is a device pointer: id .. width hold 2n rows, rec 2n x 6 doubles, t1 .. dt n doubles, status and broke n int32,
// out 16 x n doubles (plane j at out + j n, in the order of the enum above).  Returns the hipError_t of the launch (0: done),
// -1 for a bad argument.
extern "C" int kid_probe_dem_pair(const kid_params *params, int latlon, double constant_area, double constant_radius, double dem_K_damp,
                                  const int64_t *id, const double *fl_k, const double *thickness, const double *mass, const double *length, const double *width,
                                  const double *rec, const double *t1, const double *t2, const double *relrot0, const double *dt,
                                  int32_t *status, int32_t *broke, double *out, long long n) {
  if (!params || n <= 0 || n > (1ll << 24) || !id || !fl_k || !thickness || !mass || !length || !width || !rec || !t1 || !t2 || !relrot0 || !dt ||
      !status || !broke || !out) return -1;
  DevGrid g = {};
  g.latlon = latlon ? 1 : 0;
  BergPtrs b = {};
  b.id = const_cast<int64_t *>(id);
  b.f[KID_B_FL_K] = const_cast<double *>(fl_k); b.f[KID_B_THICKNESS] = const_cast<double *>(thickness); b.f[KID_B_MASS] = const_cast<double *>(mass);
  b.f[KID_B_LENGTH] = const_cast<double *>(length); b.f[KID_B_WIDTH] = const_cast<double *>(width);
  MtsDev m = {};
  m.constant_area = constant_area; m.constant_radius = constant_radius; m.dem_K_damp = dem_K_damp;
  hipLaunchKernelGGL(dem_pair_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, g, *params, b, m, rec, t1, t2, relrot0, dt, status, broke, out, n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}
extern "C" int kid_probe_dem_pair_outputs(void) { return O_COUNT; }
