// kid_cells.inc -- everything the library does per cell: the static grid and the forcing planes as the host passes them, the
// packed records and cell packets the per-berg kernels read (VelRec / TrcRec / GeoRec, PK_*: kid_device.hpp), rebuilt by a
// prepass whenever the forcing changes, the accumulator block (layout: kid_planes.hpp) and the nine-point gather of
// sum_up_spread_fields.  Included by kid_hip.hip once, after kid_handle.hpp.
//   pack_static / pack_forcing : per cell, builds the records and hoists the SSH-slope stencils (IB:4903-4926).
//   pack_packets               : per cell, gathers the neighbourhood the hot build reads into one packet.
//   gather_kernel              : per cell, the 9-point gather of sum_up_spread_fields (IB:6126-6138) + ustar.
// The rest of the library calls dev_grid, pack_forcing / forcing_given, need_static / need_forcing / forcing_held,
// nacc_active / footprint_needed, zero_planes / on_ocean_base, launch_gather and gather_mass_and_reset, and reads h->forc;
// only pack_forcing changes h->forc_parity.
#include "kid_planes.hpp"

namespace {
// ------------------------------------------- grid prepass kernels --------------------------------------
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

// (stream-ordered one-lane table writer, as set_params_kernel and its kin in kid_hip.hip)
__global__ void set_grid_kernel(const DevGrid src, DevGrid *dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = src; }

// ---------------- IB:6077-6150 sum_up_spread_fields + IB:3449-3488, per cell of the computational domain --------------
// The nine-point sum (order and slots: kid_planes.hpp) over the family of planes at v for cell c = (i, j), per area a on ocean
// cells (m).  wrap: periodic_reentry, the neighbour column across the zonal seam (mpp_update_domains of var_on_ocean, IB:6103)
__device__ __forceinline__ double nine_point(const DevGrid &g, const double *v, const size_t ncell, const int c, const int i, const bool wrap, const double a, const double m) {
  const int nic = g.iec - g.isc + 1, ni = g.ni;
  const int wm = (wrap && i == g.isc) ? nic : 0, wp = (wrap && i == g.iec) ? -nic : 0;
  double dmda = nine_point_sum([&](int di, int dj, int slot) { return v[(size_t)(slot - 1) * ncell + (size_t)(c + di + (di < 0 ? wm : (di > 0 ? wp : 0)) + dj * ni)]; });
  if (a > 0) dmda = dmda / a * m;
  return dmda;
}

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
  const int c = g.idx(i, j);
  const double a = g.geo[c].area, m = g.geo[c].msk;
  const int dm = p.diag_mask;
  const bool wrap = p.periodic_reentry != 0 && g.Lx > 0.;
  auto nine = [&](int base) { return nine_point(g, acc + (size_t)base * ncell, ncell, c, i, wrap, a, m); };
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
  const int c = g.idx(i, j);
  plane[c] = nine_point(g, acc + (size_t)KID_A_MASS_ON_OCEAN * ncell, ncell, c, i, wrap, g.geo[c].area, g.geo[c].msk);
}

}  // namespace

// ------------------------------------------------- host side -------------------------------------------
// what the kernels read of the grid, with the forcing records of set `parity` (default: the current one)
static DevGrid dev_grid(const kid_handle *h, int parity = -1) {
  const ForcingSet &fs = h->fset[parity < 0 ? h->forc_parity : parity];
  DevGrid g;
  g.isd = h->gd.isd; g.ied = h->gd.ied; g.jsd = h->gd.jsd; g.jed = h->gd.jed;
  g.isc = h->gd.isc; g.iec = h->gd.iec; g.jsc = h->gd.jsc; g.jec = h->gd.jec;
  g.ni = h->ni; g.nj = h->nj; g.latlon = h->gd.grid_is_latlon; g.regular = h->gd.grid_is_regular; g.Lx = h->gd.Lx;
  g.vel = fs.vel; g.trc = fs.trc; g.geo = h->d_geo; g.hotok = h->d_hotok; g.latref = h->d_latref;
  g.pkt = fs.pkt;
  g.dx = h->d_static[KID_G_DX]; g.dy = h->d_static[KID_G_DY]; g.ocean_depth = h->d_static[KID_G_OCEAN_DEPTH];
  g.ssh = h->d_forcing[KID_F_SSH];
  g.sin_lat_ref = sin((h->params.pi / 180.) * h->params.lat_ref);
  g.pi_180 = h->params.pi / 180.; g.r180_pi = 180. / h->params.pi; g.dydl = (180. / h->params.pi) / h->params.Rearth;
  g.rho_ratio = h->params.rho_bergs / RHO_SEAWATER;
  g.fl_e1 = exp(0.25 * h->params.pi);
  return g;
}
// which planes of the accumulator block a step keeps live: kid_planes.hpp
static bool footprint_needed(const kid_params &p) { return kid::footprint_needed(p.pass_fields_to_ocean_model, p.diag_mask); }
static int nacc_active(const kid_handle *h) { return kid::nacc_live(h->params.pass_fields_to_ocean_model, h->params.diag_mask); }
static double *on_ocean_base(const kid_handle *h) { return h->d_acc + (size_t)ON_OCEAN_ALL.first * h->ncell; }
static int zero_planes(kid_handle *h, const PlaneRange r) {
  KID_HIP(h, hipMemsetAsync(h->d_acc + (size_t)r.first * h->ncell, 0, (size_t)r.count * h->ncell * sizeof(double), h->stream));
  return KID_OK;
}
// what the handle has been given (ForcingState, kid_handle.hpp): the refusals of the entry points that need it
static int refuse(kid_handle *h, bool ok, const char *msg) { if (!ok) h->err = msg; return ok ? KID_OK : KID_EINVAL; }
static int need_static(kid_handle *h) { return refuse(h, h->forc.have_static, "kid_set_static_grid must be called first"); }
static int need_forcing(kid_handle *h) { return refuse(h, h->forc.have_forcing, "kid_set_forcing must be called before stepping"); }
static bool forcing_held(const kid_handle *h, int k) { return h->forc.held[k]; }
// the plane pointers of the prepass kernels; src[k]: where forcing plane k currently lives on the device (null, or src itself
// null: the handle's own copy)
static GridPlanes grid_planes(const kid_handle *h, const double *const *src) {
  GridPlanes gp;
  for (int k = 0; k < KID_NGRID_STATIC; ++k) gp.st[k] = h->d_static[k];
  for (int k = 0; k < KID_NFORCING; ++k) gp.fo[k] = (src && src[k]) ? src[k] : h->d_forcing[k];
  return gp;
}

// gather the cell packets of the current parity from the record arrays (after either of them has changed)
static int pack_packets(kid_handle *h) {
  const unsigned bx = (unsigned)((h->ni + 4 * KID_PKT_CELLS_PER_WAVE - 1) / (4 * KID_PKT_CELLS_PER_WAVE));
  hipLaunchKernelGGL(pack_packets_kernel, dim3(bx, (unsigned)h->nj), dim3(256), 0, h->stream, dev_grid(h), h->fset[h->forc_parity].pkt);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
static int pack_static(kid_handle *h) {
  const int nb = (int)((h->ncell + 255) / 256);
  hipLaunchKernelGGL(pack_static_kernel, dim3(nb), dim3(256), 0, h->stream, grid_planes(h, nullptr), h->d_geo, h->d_hotok, h->d_latref, h->params.pi / 180., h->ni, h->nj, (int)h->gd.grid_is_latlon, h->gd.Lx);
  KID_HIP(h, hipGetLastError());
  return h->forc.have_forcing ? pack_packets(h) : KID_OK;   // (the other parity's packets are rebuilt by the pack_forcing that precedes their use)
}
static const PrepExtras no_extras{nullptr, nullptr, 0, nullptr, nullptr};
static int pack_forcing(kid_handle *h, const double *const *src, const PrepExtras ex = no_extras) {
  const int nb = (int)((h->ncell + 255) / 256);
  // a side stream is in use: general-build launches of the previous step may still read its records -> alternate two sets
  if (h->side_mode == 2 || h->pipelined) h->forc_parity ^= 1;
  const ForcingSet &fs = h->fset[h->forc_parity];
  hipLaunchKernelGGL(pack_forcing_kernel, dim3(nb), dim3(256), 0, h->stream, grid_planes(h, src), fs.vel, fs.trc, h->ni, h->nj, ex);
  return pack_packets(h);
}
// The common tail of the entry points that bring forcing: the planes of `given` (bit k: plane k) are in d_forcing now; the
// records are rebuilt from src (as pack_forcing); sync: return only when the caller's host arrays may be reused
static int forcing_given(kid_handle *h, unsigned given, const double *const *src, bool sync, const PrepExtras ex = no_extras) {
  ForcingState &f = h->forc;
  const unsigned every = (1u << KID_NFORCING) - 1u;
  for (int k = 0; k < KID_NFORCING; ++k) f.held[k] = f.held[k] || ((given >> k) & 1u);
  f.have_planes = f.have_planes || (given & every) == every; f.have_forcing = true;
  const int rc = pack_forcing(h, src, ex);
  if (rc) return rc;
  if (sync) KID_HIP(h, hipStreamSynchronize(h->stream));
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
// the 'mass' gather of the on-ocean planes into a plane of spread_mass_old, and the planes reset (IB:5495-5497, IB:3411-3413)
static int gather_mass_and_reset(kid_handle *h, double *dst) {
  const int ncomp = (h->gd.iec - h->gd.isc + 1) * (h->gd.jec - h->gd.jsc + 1);
  hipLaunchKernelGGL(mass_gather_kernel, dim3((unsigned)((ncomp + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), (const double *)h->d_acc, dst, h->ncell,
                     h->params.periodic_reentry != 0 && h->gd.Lx > 0.);
  return zero_planes(h, ON_OCEAN_ALL);
}

extern "C" {

int kid_set_static_grid(kid_handle *h, const double *const fields[KID_NGRID_STATIC]) {
  if (!h || !fields) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  for (int k = 0; k < KID_NGRID_STATIC; ++k) {
    if (!fields[k]) { if (k == KID_G_LONC || k == KID_G_LATC) continue; h->err = "static grid field missing"; return KID_EINVAL; }
    KID_HIP(h, hipMemcpyAsync(h->d_static[k], fields[k], h->ncell * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  h->forc.have_static = true; h->bond_ext_valid = false;
  h->forc.have_centres = fields[KID_G_LONC] && fields[KID_G_LATC];
  int rc = pack_static(h);
  if (!rc) rc = pack_forcing(h, nullptr);
  if (rc) return rc;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}
int kid_set_forcing(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h || !fields) return KID_EINVAL;
  if (need_static(h)) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  unsigned given = 0u;
  for (int k = 0; k < KID_NFORCING; ++k) {
    if (!fields[k]) continue;  // NULL keeps the previous plane
    KID_HIP(h, hipMemcpyAsync(h->d_forcing[k], fields[k], h->ncell * sizeof(double), hipMemcpyHostToDevice, h->stream));
    given |= 1u << k;
  }
  return forcing_given(h, given, nullptr, true);
}
int kid_set_forcing_device(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h || !fields) return KID_EINVAL;
  if (need_static(h)) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  // The per-cell records are built straight from the caller's planes; only ssh is also kept as a plane (the
  // grounding_fraction path of the mass spreading reads it, IB:3942).
  if (fields[KID_F_SSH]) KID_HIP(h, hipMemcpyAsync(h->d_forcing[KID_F_SSH], fields[KID_F_SSH], h->ncell * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return forcing_given(h, fields[KID_F_SSH] ? 1u << KID_F_SSH : 0u, fields, false);
}
// kid_set_forcing_device + kid_zero_accumulators (+ the reset of this step's redo counters) as ONE per-cell launch
int kid_step_prepare(kid_handle *h, const double *const fields[KID_NFORCING]) {
  if (!h) return KID_EINVAL;
  if (need_static(h) || (!fields && need_forcing(h))) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  h->redo_parity ^= 1;
  if (h->side_mode == 2) {  // slow-lane schedule: the counter this prepass zeroes is the one the last carry-over launch read
    h->redo_parity = h->lane_step & 1;
    if (h->evC_live) { KID_HIP(h, hipStreamWaitEvent(h->stream, h->evC, 0)); }
  }
  PrepExtras ex;
  ex.ssh_copy = (fields && fields[KID_F_SSH] && fields[KID_F_SSH] != h->d_forcing[KID_F_SSH]) ? h->d_forcing[KID_F_SSH] : nullptr;
  ex.acc = h->d_acc; ex.zero_planes = nacc_active(h);
  ex.cnt0 = h->d_redo_cnt[0][h->redo_parity]; ex.cnt1 = h->d_redo_cnt[1][h->redo_parity];
  const int rc = forcing_given(h, ex.ssh_copy ? 1u << KID_F_SSH : 0u, fields, false, ex);
  if (rc) return rc;
  h->acc_prezeroed = true; h->redo_prezeroed = true;
  return KID_OK;
}
int kid_zero_accumulators(kid_handle *h) {
  if (!h) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  // the KID_NSCALAR words in front of the planes hold this step's increments of the running totals the reference
  // keeps on `bergs` (net_heat_to_ocean, nbergs_melted, ...); the gather folds them into the totals and clears them.
  return zero_planes(h, PlaneRange{0, nacc_active(h)});
}
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

}  // extern "C"
