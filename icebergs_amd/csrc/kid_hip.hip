// kid_hip.hip -- kernels and C ABI of libkid_hip.so (gfx950 / MI355X).  See include/kid.h.
//
// Data layout in HBM
//   bergs   : structure of arrays, one contiguous fp64/int32 array of `capacity` elements per field of the
//             reference's `type iceberg` (FW:290-359), in reference traversal order (cell-major).
//   grid    : the 11 static + 11 forcing planes as the host passes them, plus three packed record arrays
//             (VelRec/TrcRec/GeoRec, kid_device.hpp) rebuilt by a prepass kernel whenever the forcing changes.
//   accum   : KID_NACC planes of ni*nj fp64 + KID_NSCALAR scalars in ONE block (one RCCL all-reduce per step),
//             followed by KID_NOUT derived planes.
// Kernels
//   pack_static / pack_forcing : per cell, builds the records and hoists the SSH-slope stencils (IB:4903-4926).
//   berg_kernel<RK,OLD,PH>     : one lane per berg; PH selects interp / evolve / thermodynamics / spreading, so
//                                the reference's phase-by-phase call sites and the fused per-step launch share
//                                one body.  HBM-streaming on the SoA, grid served from L2 / Infinity Cache.
//   gather_kernel              : per cell, the 9-point gather of sum_up_spread_fields (IB:6126-6138) + ustar.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string.h>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <unordered_map>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "../../include/kid.h"
#include "kid_device.hpp"
#include "kid_thermo.hpp"
#include "kid_footloose.hpp"
#include "kid_berg_kernel.hpp"
#include "kid_rows_plan.hpp"
#include "kid_fl_contact.hpp"
#include "kid_reserve_plan.hpp"

using namespace kid;

// the plain hot build of the fused RK4 step: its own translation unit in the product build (kid_hot_plain.hip, another machine
// scheduler), included here in a one-file build
#ifdef KID_HOT_PLAIN_SEPARATE
namespace kid { void launch_hot_plain(bool store_env, bool rebin, unsigned nblocks, void *stream, const DevGrid *gtab, const kid_params *pp, const void *bp, long long n,
                                      double *acc, size_t ncell, const void *flags, const void *redo); }
#else
#include "kid_hot_plain.inc"
#endif

namespace {

// -------------------------------------------------------------------------------------------------------
// grid prepass kernels
// -------------------------------------------------------------------------------------------------------
struct GridPlanes { const double *st[KID_NGRID_STATIC]; const double *fo[KID_NFORCING]; };

__global__ void __launch_bounds__(256) pack_static_kernel(GridPlanes gp, GeoRec *geo, double *hotok, double *latref, double pi_180, int ni, int nj, int latlon, double Lx) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ni * nj) return;
  GeoRec r;
  r.lon = gp.st[KID_G_LON][c]; r.lat = gp.st[KID_G_LAT][c]; r.area = gp.st[KID_G_AREA][c]; r.msk = gp.st[KID_G_MSK][c];
  geo[c] = r;
  if (latref) { double s_, c_; sincos(r.lat * pi_180, &s_, &c_); latref[2 * c] = s_; latref[2 * c + 1] = c_; }   // DevGrid::latref
  // DevGrid::hotok: may the hot build step a berg of this cell?  Its in-cell test is "(xi, yj) inside the unit square",
  // which is the reference's point-in-cell test (FW:6076-6160) exactly when the four corners form a strictly convex
  // quadrilateral (the bilinear map of calc_xiyj is then one-to-one onto it); polar cells (FW:6359) and cells whose
  // packet would reach outside the data domain are left to the general build.
  const int il = c % ni, jl = c / ni;
  double ok = 0.;
  if (il >= 1 && jl >= 1 && il + 1 < ni && jl + 1 < nj) {
    const double *lon = gp.st[KID_G_LON], *lat = gp.st[KID_G_LAT];
    const double x0 = lon[c - ni - 1], y0 = lat[c - ni - 1];
    const double x1 = mod_around(lon[c - ni], x0, Lx), y1 = lat[c - ni];
    const double x2 = mod_around(lon[c], x0, Lx), y2 = lat[c];
    const double x3 = mod_around(lon[c - 1], x0, Lx), y3 = lat[c - 1];
    const double k0 = (x1 - x0) * (y2 - y1) - (y1 - y0) * (x2 - x1), k1 = (x2 - x1) * (y3 - y2) - (y2 - y1) * (x3 - x2);
    const double k2 = (x3 - x2) * (y0 - y3) - (y3 - y2) * (x0 - x3), k3 = (x0 - x3) * (y1 - y0) - (y0 - y3) * (x1 - x0);
    const bool convex = (k0 > 0. && k1 > 0. && k2 > 0. && k3 > 0.) || (k0 < 0. && k1 < 0. && k2 < 0. && k3 < 0.);
    const bool polar = latlon && dmax(dmax(y0, y1), dmax(y2, y3)) >= 89.999;
    // 2: moreover its sides lie along the axes as calc_xiyj sees the corners (beta = delta = gamma = kappa = 0 there: its
    // linear branch, with xi = dx / alpha), the cell of every regular lat-lon grid -- the hot build takes that branch directly
    const double *lo = gp.st[KID_G_LON];
    const bool rect = lo[c - 1] == lo[c - ni - 1] && lo[c] == lo[c - ni] && lat[c - ni] == lat[c - ni - 1] && lat[c] == lat[c - 1];
    if (convex && !polar) ok = rect ? 2. : 1.;
  }
  hotok[c] = ok;
}

// The cell packets of the hot build (kid_device.hpp, PK_*).  A wave takes one row of cells at a time, lane q copying
// elements q and q + 64 of a cell from where packet_source() says they live -- resolved once per lane, as in the hot
// build's own staging before the packets were gathered -- for KID_PKT_CELLS_PER_WAVE consecutive cells, eight loads in
// flight.  (One lane per (cell, element) with the index arithmetic done per lane was ~150 instructions per element: 0.65 ms
// for the 2000 x 1000 grid of config 3, compute-bound; this is the bandwidth of 576 B written per cell.)  Cells on the rim
// of the data domain have no complete neighbourhood and are never hot (hotok = 0): only that flag is written for them.
// Runs after pack_forcing_kernel (it reads the neighbours' records).
enum { KID_PKT_CELLS_PER_WAVE = 32 };
__global__ void __launch_bounds__(256) pack_packets_kernel(const DevGrid g, double *__restrict__ pkt) {
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  const int j = (int)blockIdx.y;
  const int i0 = ((int)blockIdx.x * 4 + wave) * KID_PKT_CELLS_PER_WAVE;
  if (i0 >= g.ni) return;
  const bool second = lane < PK_SIZE - 64;
  const PacketSrc s0 = packet_source(g, lane), s1 = packet_source(g, second ? 64 + lane : 0);
  const bool row_inside = j >= 1 && j < g.nj - 1;
  const int i1 = min(i0 + KID_PKT_CELLS_PER_WAVE, g.ni);
  for (int ib = i0; ib < i1; ib += 8) {
    double a[8], a2[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = ib + u;
      const bool interior = row_inside && i >= 1 && i < g.ni - 1 && i < i1;
      const long long c = interior ? (long long)j * g.ni + i : (long long)g.ni + 1;   // (a cell whose whole neighbourhood exists)
      a[u] = *reinterpret_cast<const double *>(s0.base + c * s0.stride);
      a2[u] = *reinterpret_cast<const double *>(s1.base + c * s1.stride);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = ib + u;
      if (i >= i1) continue;
      const bool interior = row_inside && i >= 1 && i < g.ni - 1;
      // the packet's flag word (PkCell::flags): +-(1 + 2 [sides along the axes] + 4 [unrotated: cos = 1, sin = 0 at the four
      // corners]), positive where the hot build may step a berg of the cell (DevGrid::hotok, and no NaN among the
      // sea-surface-slope stencil values: IB:4869-4870 stays with the general build); 0 on the rim of the data domain
      const bool is_cos = lane < PK_CORNER && (lane & 7) == 0, is_sin = lane < PK_CORNER && (lane & 7) == 1;
      const bool rotated = __ballot((is_cos && a[u] != 1.) || (is_sin && a[u] != 0.)) != 0ull;
      const bool nan_stencil = __ballot(lane >= PK_DDX && lane < PK_AREA && a[u] != a[u]) != 0ull;
      double *o = pkt + ((long long)j * g.ni + i) * PK_GSTRIDE;
      o[lane] = interior ? a[u] : 0.;
      if (second) {
        double v = interior ? a2[u] : 0.;
        if (64 + lane == PK_HOTOK) v = interior ? ((v != 0. && !nan_stencil) ? 1. : -1.) * (1. + (v == 2. ? 2. : 0.) + (rotated ? 0. : 4.)) : 0.;
        o[64 + lane] = v;
      }
    }
  }
}

// Optional extras fused into the per-cell prepass (kid_step_prepare): keep a copy of the ssh plane, zero the cell's
// entries of the first `zero_planes` accumulator planes, zero two redo counters -- one launch instead of five.
struct PrepExtras { double *ssh_copy; double *acc; int zero_planes; int *cnt0, *cnt1; };
__global__ void __launch_bounds__(256) pack_forcing_kernel(GridPlanes gp, VelRec *vel, TrcRec *trc, int ni, int nj, PrepExtras ex) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ni * nj) return;
  if (ex.ssh_copy) ex.ssh_copy[c] = gp.fo[KID_F_SSH][c];
  if (ex.acc) {
    const size_t ncell = (size_t)ni * (size_t)nj;
    for (int q = 0; q < ex.zero_planes; ++q) ex.acc[(size_t)q * ncell + (size_t)c] = 0.;
  }
  if (c == 0) { if (ex.cnt0) *ex.cnt0 = 0; if (ex.cnt1) *ex.cnt1 = 0; }
  const int il = c % ni, jl = c / ni;
  VelRec v;
  v.cosr = gp.st[KID_G_COS][c]; v.sinr = gp.st[KID_G_SIN][c];
  v.uo = gp.fo[KID_F_UO][c]; v.vo = gp.fo[KID_F_VO][c]; v.ui = gp.fo[KID_F_UI][c]; v.vi = gp.fo[KID_F_VI][c];
  v.ua = gp.fo[KID_F_UA][c]; v.va = gp.fo[KID_F_VA][c];
  vel[c] = v;
  const double *dx = gp.st[KID_G_DX], *dy = gp.st[KID_G_DY], *msk = gp.st[KID_G_MSK], *ssh = gp.fo[KID_F_SSH];
  TrcRec t;
  t.sst = gp.fo[KID_F_SST][c]; t.sss = gp.fo[KID_F_SSS][c]; t.cn = gp.fo[KID_F_CN][c]; t.hi = gp.fo[KID_F_HI][c];
  t.od = gp.st[KID_G_OCEAN_DEPTH][c] + ssh[c];  // IB:4897
  t.msk = msk[c];
  t.ddx = 0.; t.ddy = 0.;
  if (il + 1 < ni && jl >= 1) {  // ddx_ssh(i,j) IB:4903-4913
    const double dxp = 0.5 * (dx[c + 1] + dx[c + 1 - ni]);
    const double dx0 = 0.5 * (dx[c] + dx[c - ni]);
    t.ddx = 2. * (ssh[c + 1] - ssh[c]) / (dx0 + dxp) * msk[c + 1] * msk[c];
  }
  if (jl + 1 < nj && il >= 1) {  // ddy_ssh(i,j) IB:4916-4926
    const double dyp = 0.5 * (dy[c + ni] + dy[c + ni - 1]);
    const double dy0 = 0.5 * (dy[c] + dy[c - 1]);
    t.ddy = 2. * (ssh[c + ni] - ssh[c]) / (dy0 + dyp) * msk[c + ni] * msk[c];
  }
  trc[c] = t;
}

// footloose_calving (IB:2503-2734): streaming pass, one lane per berg that existed when the pass started
__global__ void __launch_bounds__(256) footloose_kernel(const DevGrid g, const kid_params *__restrict__ pp, const BergPtrs *__restrict__ bt,
                                                        const FlChildCtx cx, double *__restrict__ acc, const size_t ncell) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q >= cx.n) return;
  const BergPtrs &b = *bt;
  if (b.i[KID_BI_ALIVE][q] == 0) return;
  footloose_one(g, *pp, b, cx, q, acc, ncell, acc - KID_NSCALAR);
}

// the device-side tables are rewritten by stream-ordered one-lane kernels (the new contents travel as kernel arguments):
// no host synchronisation, unlike a copy from pageable memory
__global__ void set_berg_table_kernel(const BergPtrs src, BergPtrs *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_rebin_table_kernel(const RebinTab src, RebinTab *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_params_kernel(const kid_params src, kid_params *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }
__global__ void set_time_kernel(int32_t year, double yearday, kid_params *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) { dst->current_year = year; dst->current_yearday = yearday; } }
__global__ void set_grid_kernel(const DevGrid src, DevGrid *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }

#include "kid_mts.inc"
#include "kid_fl_interact.inc"

// -------------------------------------------------------------------------------------------------------
// IB:6077-6150 sum_up_spread_fields + IB:3449-3488, per cell of the computational domain
// -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gather_kernel(const DevGrid g, const kid_params p, double *__restrict__ acc,
                                                     double *__restrict__ out, const size_t ncell, double *__restrict__ totals,
                                                     const double *__restrict__ spread_mass_old, const double *__restrict__ spread_mass_tmp) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < KID_NSCALAR) {  // fold this step's increments into the running totals kept on `bergs` (IB:3130, 3295)
    totals[t] += (acc - KID_NSCALAR)[t];   // (the step's scalar increments sit in front of plane 0)
    (acc - KID_NSCALAR)[t] = 0.;
  }
  const int nic = g.iec - g.isc + 1, njc = g.jec - g.jsc + 1;
  if (t >= nic * njc) return;
  const int i = g.isc + t % nic, j = g.jsc + t / nic;
  const int c = g.idx(i, j), ni = g.ni;
  const double a = g.geo[c].area, m = g.geo[c].msk;
  const int dm = p.diag_mask;
  const bool wrap = p.periodic_reentry != 0 && g.Lx > 0.;
  auto nine = [&](int base) {
    const double *v = acc + (size_t)base * ncell;
    // periodic_reentry: the neighbour column across the zonal seam (mpp_update_domains of var_on_ocean, IB:6103)
    const int wm = (wrap && i == g.isc) ? nic : 0, wp = (wrap && i == g.iec) ? -nic : 0;
#define KID_V(di, dj, s) v[(size_t)((s) - 1) * ncell + (size_t)(c + (di) + ((di) < 0 ? wm : ((di) > 0 ? wp : 0)) + (dj) * ni)]
    double dmda = KID_V(0, 0, 5) + (((KID_V(-1, -1, 9) + KID_V(1, 1, 1)) + (KID_V(1, -1, 7) + KID_V(-1, 1, 3)))
                                   + ((KID_V(-1, 0, 6) + KID_V(1, 0, 4)) + (KID_V(0, -1, 8) + KID_V(0, 1, 2))));
#undef KID_V
    if (a > 0) dmda = dmda / a * m;
    return dmda;
  };
  double su = 0., sv = 0., sa = 0.;
  if ((dm & KID_DIAG_SPREAD_UVEL) || p.pass_fields_to_ocean_model) su = nine(KID_A_UVEL_ON_OCEAN);
  if ((dm & KID_DIAG_SPREAD_VVEL) || p.pass_fields_to_ocean_model) sv = nine(KID_A_VVEL_ON_OCEAN);
  if ((dm & KID_DIAG_SPREAD_AREA) || p.pass_fields_to_ocean_model) sa = dmin(nine(KID_A_AREA_ON_OCEAN), 1.0);
  const double sm = nine(KID_A_MASS_ON_OCEAN);
  out[(size_t)KID_O_SPREAD_MASS * ncell + c] = sm;
  out[(size_t)KID_O_SPREAD_AREA * ncell + c] = sa;
  out[(size_t)KID_O_SPREAD_UVEL * ncell + c] = su;
  out[(size_t)KID_O_SPREAD_VVEL * ncell + c] = sv;
  if ((dm & KID_DIAG_U_ICEBERG) || (dm & KID_DIAG_V_ICEBERG)) {  // IB:3450-3462
    const double mass = acc[(size_t)KID_A_MASS * ncell + c];
    if (dm & KID_DIAG_U_ICEBERG) acc[(size_t)KID_A_U_ICEBERG * ncell + c] = (mass > 0.) ? acc[(size_t)KID_A_U_ICEBERG * ncell + c] / mass : 0.;
    if (dm & KID_DIAG_V_ICEBERG) acc[(size_t)KID_A_V_ICEBERG * ncell + c] = (mass > 0.) ? acc[(size_t)KID_A_V_ICEBERG * ncell + c] / mass : 0.;
  }
  double ustar_h = 0.;
  if ((dm & KID_DIAG_USTAR_ICEBERG) || p.pass_fields_to_ocean_model) {  // IB:3466-3474
    const double du = su - g.vel[c].uo, dv = sv - g.vel[c].vo;
    const double dvo = sqrt(du * du + dv * dv);
    const double ustar = sqrt(p.cdrag_icebergs * (dvo * dvo + p.utide_icebergs * p.utide_icebergs));
    ustar_h = dmax(p.ustar_icebergs_bg, ustar);
    if (sa == 0.0) ustar_h = 0.;
  }
  out[(size_t)KID_O_USTAR_ICEBERG * ncell + c] = ustar_h;
  if (spread_mass_old)  // find_melt_using_spread_mass: the melt flux is what the gridded mass lost over the step, IB:3436-3445
    acc[(size_t)KID_A_FLOATING_MELT * ncell + c] = (a > 0.0) ? dmax((spread_mass_old[c] - (spread_mass_tmp ? spread_mass_tmp[c] : sm)) / p.dt, 0.0) : 0.0;
  if (p.apply_thickness_cutoff_to_gridded_melt && (p.melt_cutoff >= 0.) && (sa > 0.)) {  // IB:3477-3488 (comp. domain)
    const double ave_thickness = sm / (sa * p.rho_bergs);
    const double ave_draft = ave_thickness * (p.rho_bergs / RHO_SEAWATER);
    if ((g.ocean_depth[c] - ave_draft) < p.melt_cutoff) {
      acc[(size_t)KID_A_FLOATING_MELT * ncell + c] = 0.0; acc[(size_t)KID_A_CALVING_HFLX * ncell + c] = 0.0;
    }
  }
}

// sum_up_spread_fields(.., 'mass') alone (IB:6126-6138) into a plane of its own: grd%spread_mass_old, IB:5495-5497
__global__ void __launch_bounds__(256) mass_gather_kernel(const DevGrid g, const double *__restrict__ acc, double *__restrict__ plane, const size_t ncell, const bool wrap) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nic = g.iec - g.isc + 1, njc = g.jec - g.jsc + 1;
  if (t >= nic * njc) return;
  const int i = g.isc + t % nic, j = g.jsc + t / nic;
  const int c = g.idx(i, j), ni = g.ni;
  const double a = g.geo[c].area, m = g.geo[c].msk;
  const double *v = acc + (size_t)KID_A_MASS_ON_OCEAN * ncell;
  const int wm = (wrap && i == g.isc) ? nic : 0, wp = (wrap && i == g.iec) ? -nic : 0;
#define KID_V(di, dj, s) v[(size_t)((s) - 1) * ncell + (size_t)(c + (di) + ((di) < 0 ? wm : ((di) > 0 ? wp : 0)) + (dj) * ni)]
  double dmda = KID_V(0, 0, 5) + (((KID_V(-1, -1, 9) + KID_V(1, 1, 1)) + (KID_V(1, -1, 7) + KID_V(-1, 1, 3)))
                                 + ((KID_V(-1, 0, 6) + KID_V(1, 0, 4)) + (KID_V(0, -1, 8) + KID_V(0, 1, 2))));
#undef KID_V
  if (a > 0) dmda = dmda / a * m;
  plane[c] = dmda;
}


}  // namespace

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
#include "kid_handle.hpp"

// Halo rows (kid_halo_bergs.inc) are force sources for one kid_evolve_icebergs and nothing else: between the unpack that
// brought them and the evolve that retires them, whatever would melt, spread, count, move or write them out is refused.
static int halo_rows_refuse(kid_handle *h, const char *what) {
  if (!h->halo_rows_live) return KID_OK;
  h->err = std::string(what) + ": halo rows are resident (copies of the neighbours' bergs, kid_unpack_immigrants); the next kid_evolve_icebergs retires them";
  return KID_EINVAL;
}

static DevGrid dev_grid(const kid_handle *h) {
  DevGrid g;
  g.isd = h->gd.isd; g.ied = h->gd.ied; g.jsd = h->gd.jsd; g.jed = h->gd.jed;
  g.isc = h->gd.isc; g.iec = h->gd.iec; g.jsc = h->gd.jsc; g.jec = h->gd.jec;
  g.ni = h->ni; g.nj = h->nj; g.latlon = h->gd.grid_is_latlon; g.regular = h->gd.grid_is_regular; g.Lx = h->gd.Lx;
  g.vel = h->forc_parity ? h->d_vel2 : h->d_vel; g.trc = h->forc_parity ? h->d_trc2 : h->d_trc; g.geo = h->d_geo; g.hotok = h->d_hotok; g.latref = h->d_latref;
  g.pkt = h->d_pkt[h->forc_parity ? 1 : 0];
  g.dx = h->d_static[KID_G_DX]; g.dy = h->d_static[KID_G_DY]; g.ocean_depth = h->d_static[KID_G_OCEAN_DEPTH];
  g.ssh = h->d_forcing[KID_F_SSH];
  g.sin_lat_ref = sin((h->params.pi / 180.) * h->params.lat_ref);
  g.pi_180 = h->params.pi / 180.; g.r180_pi = 180. / h->params.pi; g.dydl = (180. / h->params.pi) / h->params.Rearth;
  g.rho_ratio = h->params.rho_bergs / RHO_SEAWATER;
  g.fl_e1 = exp(0.25 * h->params.pi);
  return g;
}
// area/Uvel/Vvel_on_ocean (27 planes) are intermediates of spread_area / spread_uvel / spread_vvel / ustar_iceberg
// (IB:3419-3474), which the reference evaluates only for `id_*>0` or pass_fields_to_ocean_model: when nobody reads them
// they are neither scattered nor zeroed nor exchanged (the reference fills them regardless and drops them)
static bool footprint_needed(const kid_params &p) {
  const int diag = KID_DIAG_SPREAD_UVEL | KID_DIAG_SPREAD_VVEL | KID_DIAG_SPREAD_AREA | KID_DIAG_USTAR_ICEBERG;
  return p.pass_fields_to_ocean_model || (p.diag_mask & diag);
}
static int nacc_active(const kid_handle *h) {
  const int diag_planes = KID_DIAG_MELT_BY_CLASS | KID_DIAG_FL_PARENT_MELT | KID_DIAG_FL_CHILD_MELT | KID_DIAG_MELT_BUOY |
                          KID_DIAG_MELT_EROS | KID_DIAG_MELT_CONV | KID_DIAG_MELT_BUOY_FL | KID_DIAG_MELT_EROS_FL |
                          KID_DIAG_MELT_CONV_FL | KID_DIAG_VIRTUAL_AREA | KID_DIAG_MASS | KID_DIAG_U_ICEBERG | KID_DIAG_V_ICEBERG;
  if (h->params.diag_mask & diag_planes) return KID_NACC;
  return footprint_needed(h->params) ? KID_NACC_CORE : KID_A_MASS_ON_OCEAN + 9;
}
static int check_params(kid_handle *h, const kid_params *p) {
  if (p->dem && !p->mts) { h->err = "dem needs mts=T (the DEM forces live on the MTS sub-steps)"; return KID_EINVAL; }
  if (p->mts) {
    if (p->Runge_not_Verlet) { h->err = "Runge_not_Verlet must be false to use MTS or DEM (FW:1485-1490)"; return KID_EINVAL; }
    if (p->old_interp_flds_order) { h->err = "old_interp_flds_order is false whenever mts/dem is on (FW:1483)"; return KID_EINVAL; }
    if (p->mts_sub_steps < 1) { h->err = "mts_sub_steps must be >= 1 (pass the value ice_bergs_framework_init derives, FW:1296-1301)"; return KID_EINVAL; }
    if (p->dem && !p->explicit_inner_mts) { h->err = "dem forces explicit_inner_mts=T (FW:1433)"; return KID_EINVAL; }
    if (p->dem && !p->iceberg_bonds_on) { h->err = "dem needs iceberg_bonds_on"; return KID_EINVAL; }
    if (p->max_bonds < 1 || p->max_bonds > KID_MAX_BONDS) { h->err = "max_bonds out of range"; return KID_EINVAL; }
    if (p->use_broken_bonds_for_substep_contact && !(p->break_bonds_on_sub_steps && p->dem && p->iceberg_bonds_on)) {
      h->err = "use_broken_bonds_for_substep_contact requires break_bonds_on_sub_steps, dem and iceberg_bonds_on (FW:1438-1447)"; return KID_EINVAL; }
    if (p->footloose) { h->err = "footloose together with mts is not implemented"; return KID_EUNSUPPORTED; }
  } else if (p->interactive_icebergs_on || p->iceberg_bonds_on) {
    if (p->Runge_not_Verlet) { h->err = "interacting / bonded bergs under the single-time-step scheme are implemented for Verlet only (Runge_not_Verlet=F)"; return KID_EUNSUPPORTED; }
    // footloose children among interacting bergs: kid_fl_interact.inc.  With bonds a bonded edge element that would calve is the
    // reference's own FATAL (IB:2566-2569, 2585)
    if (p->footloose && p->iceberg_bonds_on) { h->err = "footloose together with iceberg_bonds_on: bonded footloose calving (edge elements that calve, IB:2566-2585) is not implemented"; return KID_EUNSUPPORTED; }
    if (p->iceberg_bonds_on && !p->interactive_icebergs_on) { h->err = "iceberg_bonds_on without interactive_icebergs_on is not implemented"; return KID_EUNSUPPORTED; }
    if (p->max_bonds < 1 || p->max_bonds > KID_MAX_BONDS) { h->err = "max_bonds out of range"; return KID_EINVAL; }
  }
  if (p->tidal_drift > 0.) { h->err = "tidal_drift needs FMS's random stream: not supported"; return KID_EUNSUPPORTED; }
  // time_average_weight=T is accepted: the spreading it moves into the integrator stages (IB:7264, 7395, 7433, 7490, 7620)
  // fills mass/area/Uvel/Vvel_on_ocean, but calculate_mass_on_ocean zeroes those planes again (IB:4984-4987) without
  // refilling them (IB:4997), and nothing reads them in between: the reference's spread_mass is identically zero in
  // this mode.  So the stage spreading is not launched and the spreading phase skips the berg (berg_kernel, PH_SPREAD).
  if (p->find_melt_using_spread_mass && (p->mts || p->interactive_icebergs_on || p->footloose)) {
    h->err = "find_melt_using_spread_mass is implemented for the plain evolve loop only (no bonds, interactions or footloose)";
    return KID_EUNSUPPORTED;
  }
  if (p->Runge_not_Verlet && p->footloose) { h->err = "Runge_not_Verlet must be false to use footloose (FW:1485-1490)"; return KID_EINVAL; }
  if (p->footloose && !p->use_operator_splitting) { h->err = "use_operator_splitting must be true to use footloose (FW:1476)"; return KID_EINVAL; }
  return KID_OK;
}

extern "C" {

// The build's arithmetic and measurement switches are part of its identity: a library built with -DKID_EXPERIMENTS (KID_EXP_*
// measurement macros, possibly wrong answers) or -DKID_EXACT_MATH (IEEE division/sqrt/pow everywhere) says so.
#ifndef KID_BUILD_ID
#define KID_BUILD_ID "unknown"
#endif
// "src <id>": the first 12 hex digits of the SHA-1 of the library's sources (csrc/Makefile): profiles name the build they measured
const char *kid_version(void) {
  return "kid_hip 0.3 (gfx950) src " KID_BUILD_ID
#ifdef KID_EXACT_MATH
         " exact-math"
#endif
#ifdef KID_EXPERIMENTS
         " EXPERIMENTS"
#endif
      ;
}
int64_t kid_sizeof(int which) {
  switch (which) { case 0: return (int64_t)sizeof(kid_params); case 1: return (int64_t)sizeof(kid_grid_desc);
                   case 2: return (int64_t)sizeof(kid_berg_soa); case 3: return (int64_t)sizeof(kid_bond_soa);
                   case 4: return (int64_t)sizeof(kid_forcing_in);
                   case 5: return (int64_t)sizeof(kid_calving_params); case 6: return (int64_t)sizeof(kid_calving_in); default: return -1; }
}
#ifdef KID_EXP_TIMING
// measurement build only: the segment clock of the per-berg kernels (kid_device.hpp, KID_TICK); out[0] = waves, out[1+n] = cycles of segment n
int kid_exp_timing(unsigned long long *out, int reset) {
  if (out) {
    std::vector<unsigned long long> all((size_t)KID_TPROF_WAVES * 16);
    if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(kid_tprof), all.size() * sizeof(unsigned long long)) != hipSuccess) return KID_EHIP;
    for (int q = 0; q < 16; ++q) out[q] = 0ull;
    for (size_t r = 0; r < (size_t)KID_TPROF_WAVES; ++r) for (int q = 0; q < 16; ++q) out[q] += all[r * 16 + q];
  }
  if (reset) {
    void *sym = nullptr;
    if (hipGetSymbolAddress(&sym, HIP_SYMBOL(kid_tprof)) != hipSuccess || hipMemset(sym, 0, (size_t)KID_TPROF_WAVES * 16 * sizeof(unsigned long long)) != hipSuccess) return KID_EHIP;
  }
  return KID_OK;
}
#endif
// kid_destroy reports a failed free through kid_last_error(NULL), to the thread that called it: the handle is gone by then
static thread_local std::string destroy_err;
const char *kid_last_error(const kid_handle *h) { return h ? h->err.c_str() : destroy_err.empty() ? "null handle" : destroy_err.c_str(); }

int kid_create(const kid_grid_desc *grid, const kid_params *params, int64_t capacity, int device, kid_handle **out) {
  if (!grid || !params || !out || capacity <= 0) return KID_EINVAL;
  if (capacity > (int64_t(1) << 29)) return KID_EINVAL;   // the per-berg kernel addresses a row by a 32-bit byte offset (2^29 rows of 8 bytes; 240 GB of berg state)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KID_ENODEV;
  if (device < 0 || device >= ndev) return KID_ENODEV;
  kid_handle *h = new kid_handle();
  *out = h;  // returned even on failure so that kid_last_error() can be read; caller still destroys it
  h->device = device;
  KID_HIP(h, hipSetDevice(device));
  h->gd = *grid;
  h->ni = grid->ied - grid->isd + 1; h->nj = grid->jed - grid->jsd + 1;
  if (h->ni < 5 || h->nj < 5 || grid->isc - grid->isd < 2 || grid->ied - grid->iec < 2 || grid->jsc - grid->jsd < 2 || grid->jed - grid->jec < 2) {
    h->err = "grid needs a halo of at least 2 cells"; return KID_EINVAL;
  }
  h->ncell = (size_t)h->ni * (size_t)h->nj;
  int rc = check_params(h, params);
  if (rc) return rc;
  h->params = *params;
  h->flags.footprint = footprint_needed(h->params) ? 1 : 0;
  h->capacity = capacity;
  if (getenv("KID_MTS_NO_GRAPH")) h->use_graph = false;  // A/B switch for measurements
  h->dbg.stable_resort = getenv("KID_STABLE_RESORT") != nullptr; h->dbg.no_plain_build = getenv("KID_NO_PLAIN_BUILD") != nullptr;
  h->dbg.fl_unfused = getenv("KID_FL_UNFUSED") != nullptr; h->dbg.new_order_unfused = getenv("KID_NEW_ORDER_UNFUSED") != nullptr;
  h->dbg.rebin_eager = getenv("KID_REBIN_EAGER") != nullptr; h->dbg.chksum_timing = getenv("KID_CHKSUM_TIMING") != nullptr;
  h->dbg.mts_always_label = getenv("KID_MTS_ALWAYS_LABEL") != nullptr; h->dbg.mts_no_fused = getenv("KID_MTS_NO_FUSED") != nullptr;
  if (const char *e = getenv("KID_MTS_FUSED_BLOCKS_CAP")) h->dbg.mts_fused_blocks_cap = atoi(e);
  if (const char *e = getenv("KID_MTS_POLL_LIMIT")) h->dbg.mts_poll_limit = atoi(e);
  KID_HIP(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  const size_t cap = (size_t)capacity;
  for (auto &plane : h->d_static) KID_HIP(h, h->mem.dev(plane, h->ncell, 0));
  for (auto &plane : h->d_forcing) KID_HIP(h, h->mem.dev(plane, h->ncell, 0));
  for (VelRec **q : {&h->d_vel, &h->d_vel2}) KID_HIP(h, h->mem.dev(*q, h->ncell));   // (the second set: forcing records of the odd steps)
  for (TrcRec **q : {&h->d_trc, &h->d_trc2}) KID_HIP(h, h->mem.dev(*q, h->ncell));
  KID_HIP(h, h->mem.dev(h->d_geo, h->ncell));
  KID_HIP(h, h->mem.dev(h->d_hotok, h->ncell, 0));
  if (grid->grid_is_latlon) KID_HIP(h, h->mem.dev(h->d_latref, 2 * h->ncell));   // DevGrid::latref
  KID_HIP(h, h->mem.dev(h->d_acc_own, (size_t)KID_NACC * h->ncell + KID_NSCALAR, 0));
  h->d_acc = h->d_acc_own + KID_NSCALAR;
  KID_HIP(h, h->mem.dev(h->d_out, (size_t)KID_NOUT * h->ncell, 0));
  KID_HIP(h, h->mem.dev(h->d_totals, KID_NSCALAR, 0));
  for (auto &field : h->bp.f) KID_HIP(h, h->mem.dev(field, cap, 0));
  for (auto &field : h->bp.i) KID_HIP(h, h->mem.dev(field, cap, 0));
  KID_HIP(h, h->mem.dev(h->bp.id, cap, 0));
  KID_HIP(h, h->mem.dev(h->d_bp, 1));
  KID_HIP(h, h->mem.dev(h->d_rb, 1));
  KID_HIP(h, h->mem.dev(h->d_params, 1));
  for (DevGrid **q : {&h->d_grid, &h->d_grid2}) KID_HIP(h, h->mem.dev(*q, 1));
  for (auto &pkt : h->d_pkt) KID_HIP(h, h->mem.dev(pkt, h->ncell * PK_GSTRIDE, 0));
  KID_HIP(h, h->mem.dev(h->d_lane, cap, 0));
  KID_HIP(h, h->mem.dev(h->d_count, 4));
  KID_HIP(h, h->mem.dev(h->d_iceberg_counter, h->ncell, 0));
  KID_HIP(h, h->mem.dev(h->d_fl_cursor, 1));
  for (int **q : {&h->d_redo_list, &h->d_redo_list2}) KID_HIP(h, h->mem.dev(*q, cap));
  KID_HIP(h, h->mem.dev(h->d_redo_count2, 4, 0));
  for (int part = 0; part < 2; ++part) for (int par = 0; par < 2; ++par) h->d_redo_cnt[part][par] = h->d_redo_count2 + (2 * part + par);
  for (hipEvent_t *e : {&h->evC, &h->evP, &h->evF[0], &h->evF[1], &h->evG[0], &h->evG[1]}) KID_HIP(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (hipEvent_t *e : {&h->ev0, &h->ev1, &h->ev2, &h->ev3}) KID_HIP(h, hipEventCreate(e));
  // The zero-fills above are on the handle's own stream.  kid_set_stream may name another one before the first upload,
  // and that stream does not order itself behind this one: wait here, or a fill could land after the upload (seen once,
  // with null-stream fills, as a zeroed `ine` array of a 1-berg population).
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_destroy(kid_handle *h) {
  if (!h) return KID_EINVAL;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  if (h->sub_graph_exec) (void)hipGraphExecDestroy(h->sub_graph_exec);
  for (hipEvent_t e : {h->evR, h->evC, h->evP, h->evF[0], h->evF[1], h->evG[0], h->evG[1], h->ev0, h->ev1, h->ev2, h->ev3}) if (e) (void)hipEventDestroy(e);
  for (auto &pe : h->pending) { (void)hipEventDestroy(pe.first); (void)hipEventDestroy(pe.second); }
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  const int e_rp = h->rp_mem.free_all(), e_mem = h->mem.free_all();
  const hipError_t e = (hipError_t)(e_rp ? e_rp : e_mem);
  delete h;
  if (e == hipSuccess) return KID_OK;
  destroy_err = std::string("kid_destroy: freeing the handle's memory: ") + hipGetErrorString(e);
  return KID_EHIP;
}

int kid_memory_in_use(int64_t *device_bytes, int64_t *pinned_bytes) {
  if (device_bytes) *device_bytes = kid::mem_in_use(kid::MEM_DEVICE).load();
  if (pinned_bytes) *pinned_bytes = kid::mem_in_use(kid::MEM_PINNED).load();
  return KID_OK;
}

int kid_set_params(kid_handle *h, const kid_params *params) {
  if (!h || !params) return KID_EINVAL;
  int rc = check_params(h, params);
  if (rc) return rc;
  if (!h->tables_dirty && h->d_params) {
    // A model clock that advances (bergs%current_year / current_yearday, every step of a real run) is not a reason to
    // rebuild the device tables -- which waits for the side stream, i.e. puts the slow lane's general build back between
    // two hot builds.  The two words are written in place by a stream-ordered one-lane kernel; the launches that may
    // still be in flight on the side stream (fused step without footloose) never read them.
    kid_params a = h->params, b = *params;
    a.current_year = b.current_year = 0; a.current_yearday = b.current_yearday = 0.;
    if (std::memcmp(&a, &b, sizeof(kid_params)) == 0) {
      h->params = *params;
      KID_HIP(h, hipSetDevice(h->device));
      hipLaunchKernelGGL(set_time_kernel, dim3(1), dim3(64), 0, h->stream, params->current_year, params->current_yearday, h->d_params);
      KID_HIP(h, hipGetLastError());
      return KID_OK;
    }
  }
  h->params = *params;
  h->tables_dirty = true;
  h->labels_stale = true;   // (the conglomerate labelling reads dem / max_bonds / use_broken_bonds_for_substep_contact)
  h->flags.footprint = footprint_needed(h->params) ? 1 : 0;
  if (!h->params.old_interp_flds_order && !h->env_off_requested) h->flags.store_env = 1;  // the stored environment is an input again
  return KID_OK;
}
// order the main stream behind general-build launches that are still in flight on the side stream
static int join_side(kid_handle *h) {
  for (int q = 0; q < 2; ++q)
    if (h->evG_live[q]) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evG[q], 0)); }
  if (h->evC_live) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evC, 0)); }
  return KID_OK;
}
// Leave the slow-lane schedule: both lanes are complete through the last step once the side stream is joined, so every
// berg can go back to the hot build and nothing is carried over.  Needed before anything that moves rows (the lists
// hold row numbers) or that launches outside launch_berg_lanes (kid_launch.inc).
static int lanes_drain(kid_handle *h) {
  const int rc = join_side(h);
  if (rc || !h->lanes_active) return rc;
  KID_HIP(h, hipMemsetAsync(h->d_lane, 0, (size_t)h->capacity * sizeof(int), h->stream));
  // the other buffer of the in-step re-binning too: its rows beyond the population would come back with stamps of a
  // step count that starts over below
  if (h->d_lane_alt) KID_HIP(h, hipMemsetAsync(h->d_lane_alt, 0, (size_t)h->capacity * sizeof(int), h->stream));
  h->lanes_active = false; h->carry_valid = false; h->lane_step = 1;
  return KID_OK;
}
int kid_set_side_stream(kid_handle *h, void *s, int enable) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  int rc = join_side(h);
  if (rc) return rc;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  { const int rc_d = lanes_drain(h); if (rc_d) return rc_d; }
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->evG_live[0] = h->evG_live[1] = false; h->evC_live = false;
  h->side_stream = (hipStream_t)s;
  h->pipelined = enable == 1;
  h->side_mode = (s && enable == 2) ? 2 : 0;
  return KID_OK;
}
int kid_set_stream(kid_handle *h, void *s) {
  if (!h) return KID_EINVAL;
  // NULL is the device's default (null) stream -- e.g. torch's default current stream -- not "no stream": work the
  // caller orders with its own events or collectives must really be on the stream it names
  h->stream = (hipStream_t)s;
  return KID_OK;
}
// the cell hash of a berg id (ij_component_of_id FW:4227-4240) on this grid: i + iNg * (j - 1) + ij0 with local i, j
static inline int id_iNg(const kid_grid_desc &d) { return d.gni > 0 ? d.gni : d.iec - d.isc + 1; }
static inline int id_ij0(const kid_grid_desc &d) { return d.gni > 0 ? d.gi0 + d.gni * d.gj0 : 0; }
int kid_sync(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return mts_check_timeout(h);
}

// gather the cell packets of the current parity from the record arrays (after either of them has changed)
static int pack_packets(kid_handle *h) {
  const unsigned bx = (unsigned)((h->ni + 4 * KID_PKT_CELLS_PER_WAVE - 1) / (4 * KID_PKT_CELLS_PER_WAVE));
  hipLaunchKernelGGL(pack_packets_kernel, dim3(bx, (unsigned)h->nj), dim3(256), 0, h->stream, dev_grid(h), h->d_pkt[h->forc_parity ? 1 : 0]);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static int pack_static(kid_handle *h) {
  GridPlanes gp;
  for (int k = 0; k < KID_NGRID_STATIC; ++k) gp.st[k] = h->d_static[k];
  for (int k = 0; k < KID_NFORCING; ++k) gp.fo[k] = h->d_forcing[k];
  const int nb = (int)((h->ncell + 255) / 256);
  hipLaunchKernelGGL(pack_static_kernel, dim3(nb), dim3(256), 0, h->stream, gp, h->d_geo, h->d_hotok, h->d_latref, h->params.pi / 180., h->ni, h->nj, (int)h->gd.grid_is_latlon, h->gd.Lx);
  KID_HIP(h, hipGetLastError());
  return h->have_forcing ? pack_packets(h) : KID_OK;   // (the other parity's packets are rebuilt by the pack_forcing that precedes their use)
}
// src[k]: where forcing plane k currently lives on the device (the handle's own copy, or the caller's buffer)
static int pack_forcing(kid_handle *h, const double *const src[KID_NFORCING], const PrepExtras ex = PrepExtras{nullptr, nullptr, 0, nullptr, nullptr}) {
  GridPlanes gp;
  for (int k = 0; k < KID_NGRID_STATIC; ++k) gp.st[k] = h->d_static[k];
  for (int k = 0; k < KID_NFORCING; ++k) gp.fo[k] = src[k] ? src[k] : h->d_forcing[k];
  const int nb = (int)((h->ncell + 255) / 256);
  // a side stream is in use: general-build launches of the previous step may still read its records -> alternate two sets
  if (h->side_mode == 2 || h->pipelined) h->forc_parity ^= 1;
  hipLaunchKernelGGL(pack_forcing_kernel, dim3(nb), dim3(256), 0, h->stream, gp, h->forc_parity ? h->d_vel2 : h->d_vel, h->forc_parity ? h->d_trc2 : h->d_trc, h->ni, h->nj, ex);
  return pack_packets(h);
}

int kid_set_static_grid(kid_handle *h, const double *const fields[KID_NGRID_STATIC]) {
  if (!h || !fields) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  for (int k = 0; k < KID_NGRID_STATIC; ++k) {
    if (!fields[k]) { if (k == KID_G_LONC || k == KID_G_LATC) continue; h->err = "static grid field missing"; return KID_EINVAL; }
    KID_HIP(h, hipMemcpyAsync(h->d_static[k], fields[k], h->ncell * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  h->have_static = true; h->bond_ext_valid = false;
  h->have_centres = fields[KID_G_LONC] && fields[KID_G_LATC];
  int rc = pack_static(h);
  if (rc) return rc;
  const double *none[KID_NFORCING] = {};
  rc = pack_forcing(h, none);
  if (rc) return rc;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_set_forcing(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h || !fields) return KID_EINVAL;
  if (!h->have_static) { h->err = "kid_set_static_grid must be called first"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  for (int k = 0; k < KID_NFORCING; ++k) {
    if (!fields[k]) continue;  // NULL keeps the previous plane
    KID_HIP(h, hipMemcpyAsync(h->d_forcing[k], fields[k], h->ncell * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->forcing_held[k] = true;
  }
  h->have_forcing = true;
  { bool all = true; for (int k = 0; k < KID_NFORCING; ++k) all = all && (fields[k] || h->have_planes); h->have_planes = all; }
  const double *none[KID_NFORCING] = {};
  int rc = pack_forcing(h, none);
  if (rc) return rc;
  KID_HIP(h, hipStreamSynchronize(h->stream));  // the host arrays may be reused by the caller
  return KID_OK;
}

int kid_set_forcing_device(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h || !fields) return KID_EINVAL;
  if (!h->have_static) { h->err = "kid_set_static_grid must be called first"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  // The per-cell records are built straight from the caller's planes; only ssh is also kept as a plane (the
  // grounding_fraction path of the mass spreading reads it, IB:3942).
  if (fields[KID_F_SSH])
    { KID_HIP(h, hipMemcpyAsync(h->d_forcing[KID_F_SSH], fields[KID_F_SSH], h->ncell * sizeof(double), hipMemcpyDeviceToDevice, h->stream)); h->forcing_held[KID_F_SSH] = true; }
  h->have_forcing = true;
  return pack_forcing(h, fields);
}

// kid_set_forcing_device + kid_zero_accumulators (+ the reset of this step's redo counters) as ONE per-cell launch
int kid_step_prepare(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h) return KID_EINVAL;
  if (!h->have_static) { h->err = "kid_set_static_grid must be called first"; return KID_EINVAL; }
  if (!fields && !h->have_forcing) { h->err = "kid_set_forcing must be called before stepping"; return KID_EINVAL; }
  KID_HIP(h, hipSetDevice(h->device));
  const double *none[KID_NFORCING] = {};
  const double *const *src = fields ? fields : none;
  h->redo_parity ^= 1;
  if (h->side_mode == 2) {  // slow-lane schedule: the counter this prepass zeroes is the one the last carry-over launch read
    h->redo_parity = h->lane_step & 1;
    if (h->evC_live) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evC, 0)); }
  }
  PrepExtras ex;
  ex.ssh_copy = (src[KID_F_SSH] && src[KID_F_SSH] != h->d_forcing[KID_F_SSH]) ? h->d_forcing[KID_F_SSH] : nullptr;
  if (ex.ssh_copy) h->forcing_held[KID_F_SSH] = true;
  ex.acc = h->d_acc; ex.zero_planes = nacc_active(h);
  ex.cnt0 = h->d_redo_cnt[0][h->redo_parity]; ex.cnt1 = h->d_redo_cnt[1][h->redo_parity];
  h->have_forcing = true;
  const int rc = pack_forcing(h, src, ex);
  if (rc) return rc;
  h->acc_prezeroed = true; h->redo_prezeroed = true;
  return KID_OK;
}

#include "kid_ingest.inc"
}  // extern "C"
#include "kid_rows.inc"
extern "C" {

int kid_upload_bergs(kid_handle *h, const kid_berg_soa *host) {
  if (!h || !host || host->n < 0) return KID_EINVAL;
  if (host->n > h->capacity) { const int rc = auto_reserve(h, host->n, "kid_upload_bergs"); if (rc) return rc; }
  if (host->n > h->capacity) { h->err = "more bergs than capacity"; return KID_ECAPACITY; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  const size_t n = (size_t)host->n;
  for (int f = 0; f < KID_NB_F64; ++f) {
    if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(h->bp.f[f], host->f64[f], n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    else KID_HIP(h, hipMemsetAsync(h->bp.f[f], 0, n * sizeof(double), h->stream));
  }
  for (int f = 0; f < KID_NB_I32; ++f) {
    if (host->i32[f]) KID_HIP(h, hipMemcpyAsync(h->bp.i[f], host->i32[f], n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    else if (f == KID_BI_ALIVE) { if (n) hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->bp.i[f], 1, (long long)n); }
    else KID_HIP(h, hipMemsetAsync(h->bp.i[f], 0, n * sizeof(int32_t), h->stream));
  }
  if (host->id) KID_HIP(h, hipMemcpyAsync(h->bp.id, host->id, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  else KID_HIP(h, hipMemsetAsync(h->bp.id, 0, n * sizeof(int64_t), h->stream));
  // cell indices are trusted by the kernels: reject anything outside the computational domain + first halo row
  if (host->i32[KID_BI_INE] && host->i32[KID_BI_JNE]) {
    for (size_t k = 0; k < n; ++k) {
      const int i = host->i32[KID_BI_INE][k], j = host->i32[KID_BI_JNE][k];
      if (i < h->gd.isc - 1 || i > h->gd.iec + 1 || j < h->gd.jsc - 1 || j > h->gd.jec + 1) {
        h->err = "berg cell index (ine,jne) outside the computational domain"; return KID_EINVAL;
      }
    }
  } else if (n > 0) { h->err = "ine/jne are required"; return KID_EINVAL; }
  if (h->bp.orient) { h->bp.orient = nullptr; h->tables_dirty = true; }
  rows_replaced(h, host);
  h->visited = false; h->have_bonds = false;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

int kid_download_bergs(kid_handle *h, kid_berg_soa *host) {
  if (!h || !host) return KID_EINVAL;
  if (host->n < h->n) { h->err = "host SoA too small"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  const size_t n = (size_t)h->n;
  for (int f = 0; f < KID_NB_F64; ++f)
    if (host->f64[f]) KID_HIP(h, hipMemcpyAsync(host->f64[f], h->bp.f[f], n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  for (int f = 0; f < KID_NB_I32; ++f)
    if (host->i32[f]) KID_HIP(h, hipMemcpyAsync(host->i32[f], h->bp.i[f], n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (host->id) KID_HIP(h, hipMemcpyAsync(host->id, h->bp.id, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  host->n = h->n;
  return KID_OK;
}


// With .not.old_interp_flds_order the stored environment (berg%uo ... od) is an input of evolve_icebergs and thermodynamics as
// the reference calls them, one after the other; the fused step (kid_run_step / kid_step_local) interpolates it for itself
// and only writes it -- 104 B per berg-step that nothing inside the library reads back.  Switching the store off is
// therefore allowed there too; the entry points that do read it then refuse to run (launch_phase, kid_launch.inc) instead of reading values
// of some earlier step.
int kid_set_store_environment(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  h->flags.store_env = on ? 1 : 0;
  h->env_off_requested = !on;
  return KID_OK;
}

int kid_zero_accumulators(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  const size_t planes = (size_t)nacc_active(h);
  KID_HIP(h, hipMemsetAsync(h->d_acc, 0, planes * h->ncell * sizeof(double), h->stream));
  // the KID_NSCALAR words behind the planes hold this step's increments of the running totals the reference
  // keeps on `bergs` (net_heat_to_ocean, nbergs_melted, ...); the gather folds them into the totals and clears them.
  return KID_OK;
}

}  // extern "C"

extern "C" {

static int refresh_tables(kid_handle *h) {
  if (h->tables_dirty) {
    const int rc = join_side(h);  // a general-build launch on the side stream may still be reading the tables
    if (rc) return rc;
    hipLaunchKernelGGL(set_berg_table_kernel, dim3(1), dim3(64), 0, h->stream, h->bp, h->d_bp);
    hipLaunchKernelGGL(set_params_kernel, dim3(1), dim3(64), 0, h->stream, h->params, h->d_params);
    { const int par = h->forc_parity;
      h->forc_parity = 0; hipLaunchKernelGGL(set_grid_kernel, dim3(1), dim3(64), 0, h->stream, dev_grid(h), h->d_grid);
      h->forc_parity = 1; hipLaunchKernelGGL(set_grid_kernel, dim3(1), dim3(64), 0, h->stream, dev_grid(h), h->d_grid2);
      h->forc_parity = par; }
    KID_HIP(h, hipGetLastError());
    h->tables_dirty = false;
  }
  return KID_OK;
}
// ids of the children a footloose pass appended to rows [n_old, n_old + m): the per-cell counter values in the order the
// reference's loop would have met the events (kid_footloose.hpp, fl_assign_ids_*)
// second half of calve_fl_icebergs for the children of one pass (kid_footloose.hpp): positions, copied members, constants
static int fl_place_children(kid_handle *h, long long n_old, int m, unsigned step) {
  if (!h->fl_place_warm) {   // the kernel's out-of-line helpers need stack scratch, which the runtime allocates at the FIRST launch
    // (1.6 s at 1e7 bergs' worth of device memory in use): an empty launch at the first footloose pass, not at the first event
    h->fl_place_warm = true;
    hipLaunchKernelGGL(fl_place_children_kernel<BergPtrs>, dim3(1), dim3(64), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, n_old, 0, step);
    KID_HIP(h, hipGetLastError());
  }
  if (m <= 0) return KID_OK;
  hipLaunchKernelGGL(fl_place_children_kernel<BergPtrs>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, (const BergPtrs *)h->d_bp, n_old, m, step);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static int fl_assign_ids(kid_handle *h, long long n_old, int m) {
  if (m <= 0) return KID_OK;
  if (!h->d_fl_head) KID_HIP(h, h->mem.dev(h->d_fl_head, h->ncell, 0xff));   // -1: empty lists
  if (m > h->fl_ev_capacity) {
    KID_HIP(h, h->mem.drop(h->d_fl_next));
    KID_HIP(h, h->mem.drop(h->d_fl_newid));
    h->fl_ev_capacity = std::max<long long>(2ll * m, 4096);
    KID_HIP(h, h->mem.dev(h->d_fl_next, (size_t)h->fl_ev_capacity));
    KID_HIP(h, h->mem.dev(h->d_fl_newid, (size_t)h->fl_ev_capacity));
  }
  const FlIdCtx x{h->d_fl_head, h->d_fl_next, h->d_fl_newid, h->d_iceberg_counter, n_old, m, id_iNg(h->gd), id_ij0(h->gd)};
  const dim3 grid((unsigned)((m + 255) / 256)), block(256);
  const DevGrid g = dev_grid(h);
  hipLaunchKernelGGL(fl_assign_ids_push<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  hipLaunchKernelGGL(fl_assign_ids_rank<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  hipLaunchKernelGGL(fl_assign_ids_store<BergPtrs>, grid, block, 0, h->stream, g, (const BergPtrs *)h->d_bp, x);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static const char *const fl_full = "footloose calving ran out of capacity: create the handle with room for child bergs";
int kid_footloose_calving(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_footloose_calving"); if (rc_h) return rc_h; }
  if (!h->params.footloose || h->n == 0) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  int rc = repro_refuse(h);
  if (rc) return rc;
  rc = rebin_flush(h);
  if (rc) return rc;
  rc = refresh_tables(h);
  if (rc) return rc;
  h->flags.has_fl = 1;
  // auto-reserve: min_free rows behind the parents before the launch (no retry afterwards: the parents' bits are spent by then)
  rc = auto_reserve(h, h->n + h->auto_min_free, "kid_footloose_calving");
  if (rc) return rc;
  KID_HIP(h, hipMemsetAsync(h->d_fl_cursor, 0, sizeof(int), h->stream));
  const unsigned fl_step_now = h->fl_step;
  FlChildCtx cx{h->d_fl_cursor, h->d_iceberg_counter, (long long)h->n, (long long)h->capacity, h->gd.iec - h->gd.isc + 1, h->fl_step++};
  hipLaunchKernelGGL(footloose_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->d_bp, cx, h->d_acc, h->ncell);
  KID_HIP(h, hipGetLastError());
  int appended = 0;  // the population grew: the host needs the new size before the next launch
  KID_HIP(h, hipMemcpyAsync(&appended, h->d_fl_cursor, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  // the children become rows only once they are placed and have their ids: after a failure of either helper the population is
  // what it was before the call
  if (appended <= h->capacity - h->n) {
    rc = fl_place_children(h, h->n, appended, fl_step_now);
    if (!rc) rc = fl_assign_ids(h, h->n, appended);
    if (rc) return rc;
  }
  return rows_appended(h, appended, nullptr, fl_full);
}
double kid_footloose_uniform(int32_t seed, int64_t berg_id, int64_t step, int32_t draw) {   // the number a child placement uses (host side of kid_rng.h)
  return kid_fl_uniform((uint32_t)seed, berg_id, (uint32_t)step, (uint32_t)draw);
}
int kid_set_footloose_step(kid_handle *h, int64_t step) {   // restart: continue the child-placement sequence (kid_rng.h)
  if (!h || step < 0) return KID_EINVAL;
  h->fl_step = (unsigned)step;
  return KID_OK;
}
int kid_get_footloose_step(kid_handle *h, int64_t *step) {
  if (!h || !step) return KID_EINVAL;
  *step = (int64_t)h->fl_step;
  return KID_OK;
}
int kid_set_iceberg_counter(kid_handle *h, const int32_t *counter) {  // grd%iceberg_counter_grd, (isd:ied,jsd:jed)
  if (!h || !counter) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipMemcpy(h->d_iceberg_counter, counter, h->ncell * sizeof(int32_t), hipMemcpyHostToDevice));
  return KID_OK;
}
int kid_get_iceberg_counter(kid_handle *h, int32_t *counter) {
  if (!h || !counter) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  KID_HIP(h, hipMemcpy(counter, h->d_iceberg_counter, h->ncell * sizeof(int32_t), hipMemcpyDeviceToHost));
  return KID_OK;
}

static int launch_gather(kid_handle *h) {
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  const DevGrid g = dev_grid(h);
  const int ncomp = (h->gd.iec - h->gd.isc + 1) * (h->gd.jec - h->gd.jsc + 1);
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)((ncomp + 255) / 256)), dim3(256), 0, h->stream, g, h->params, h->d_acc, h->d_out, h->ncell, h->d_totals,
                     (const double *)(h->params.find_melt_using_spread_mass ? h->d_spread_mass_old : nullptr),
                     (const double *)((h->params.find_melt_using_spread_mass && h->params.Iceberg_melt_without_decay) ? h->d_spread_mass_old + h->ncell : nullptr));
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
#include "kid_mts_host.inc"
#include "kid_calving.inc"
#include "kid_repro.inc"
}  // extern "C"
#include "kid_bond_init.inc"
#include "kid_budget.inc"
#include "kid_launch.inc"
#include "kid_reserve.inc"
extern "C" {

int kid_get_accumulators(kid_handle *h, double *acc, double *out, double *scalars) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  if (acc) KID_HIP(h, hipMemcpyAsync(acc, h->d_acc, (size_t)KID_NACC * h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out) KID_HIP(h, hipMemcpyAsync(out, h->d_out, (size_t)KID_NOUT * h->ncell * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (scalars) KID_HIP(h, hipMemcpyAsync(scalars, h->d_totals, KID_NSCALAR * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if (scalars) {
    int64_t alive = 0;
    int rc = kid_num_bergs(h, nullptr, &alive);
    if (rc) return rc;
    scalars[KID_S_NBERGS_ALIVE] = (double)alive;
  }
  return KID_OK;
}
int kid_accum_device_ptr(kid_handle *h, void **dev_ptr, int64_t *count) {
  if (!h || !dev_ptr || !count) return KID_EINVAL;
  *dev_ptr = h->d_acc - KID_NSCALAR;
  *count = (int64_t)((size_t)KID_NACC * h->ncell + KID_NSCALAR);
  return KID_OK;
}
int kid_accum_live_count(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  *count = (int64_t)((size_t)nacc_active(h) * h->ncell + KID_NSCALAR);
  return KID_OK;
}
int kid_bind_accum_buffer(kid_handle *h, void *dev_ptr, int64_t count) {
  if (!h) return KID_EINVAL;
  if (!dev_ptr) { h->d_acc = h->d_acc_own + KID_NSCALAR; h->acc_prezeroed = false; return KID_OK; }
  if (count < (int64_t)((size_t)KID_NACC * h->ncell + KID_NSCALAR)) { h->err = "accumulator buffer too small"; return KID_EINVAL; }
  h->d_acc = (double *)dev_ptr + KID_NSCALAR;
  h->acc_prezeroed = false;
  return KID_OK;
}

int kid_bind_spread_mass_old(kid_handle *h, void *dev_ptr, int64_t count) {
  if (!h) return KID_EINVAL;
  if (!dev_ptr) { h->d_spread_mass_old = h->d_spread_mass_old_own; return KID_OK; }
  if (count < (int64_t)(2 * h->ncell)) { h->err = "spread_mass_old buffer too small (2 planes)"; return KID_EINVAL; }
  h->d_spread_mass_old = (double *)dev_ptr;
  return KID_OK;
}
int kid_last_redo_count(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_j = join_side(h); if (rc_j) return rc_j; }
  int c[4] = {0, 0, 0, 0};
  KID_HIP(h, hipMemcpyAsync(c, h->d_redo_count2, 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  *count = (int64_t)c[0 + h->redo_parity] + (h->pipelined ? (int64_t)c[2 + h->redo_parity] : 0);
  return KID_OK;
}
int kid_rebin_fused_count(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  *count = h->rebin_fused_count;
  return KID_OK;
}
int kid_profile_enable(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  h->profile = on != 0;
  h->berg_ms = 0.; h->all_ms = 0.; h->berg_launches = 0;
  return KID_OK;
}
int kid_profile_get(kid_handle *h, double *berg_ms, int64_t *launches, double *all_ms) {
  if (!h) return KID_EINVAL;
  // the events were only recorded while stepping (no host/device sync in the timed loop); resolve them now
  KID_HIP(h, hipSetDevice(h->device));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  for (auto &pe : h->pending) {
    float ms = 0.f;
    KID_HIP(h, hipEventElapsedTime(&ms, pe.first, pe.second));
    h->berg_ms += ms;
    (void)hipEventDestroy(pe.first); (void)hipEventDestroy(pe.second);
  }
  h->pending.clear();
  if (berg_ms) *berg_ms = h->berg_ms;
  if (launches) *launches = h->berg_launches;
  if (all_ms) *all_ms = h->all_ms;
  return KID_OK;
}

}  // extern "C"

#include "kid_locate.inc"
#include "kid_restart.inc"
#include "kid_traj.inc"
#include "kid_migrate.inc"
#include "kid_halo_bergs.inc"
#include "kid_halo.inc"
#include "kid_chksum.inc"
#include "kid_chksum_device.inc"
