// kid_locate.inc -- a berg's cell from its position: read_restart_bergs with ignore_ij_restart (IO2:876-891, 947-957).
//   find_cell_by_search  FW:5710-5842   dcost FW:5845-5858   find_better_min FW:5862-5893   find_cell_loc FW:5896-5924
//   find_cell            FW:6011-6041   (use_slow_find)
// One kernel on plain pointers, one lane per berg, fp64: the resident SoA (kid_locate_bergs) and the temporary blocks that
// kid_read_restart fills from a file (kid_set_restart_locate) go through the same code.
//   mode 1: the walk of find_cell_by_search on the cell centres (grd%lonc, grd%latc), per lane, in the reference's order of
//           comparisons; its ends are the first corner, a move into the cell, stagnation (find_better_min(3), find_cell_loc(1),
//           find_cell_loc(3)) and, with the moves used up, find_cell (FW:5828).
//   mode 2: find_cell: the structured-grid guess (FW:6025-6031), then the scan of the computational domain, j outer, i inner.
// The scan is the wave's work, not the lane's: the wave takes its lanes that need one in turn (ballot, readlane of the lane's
// x, y), all 64 lanes test 64 consecutive cells of the scan order, and the lowest set bit of the ballot is the reference's
// first hit.  A berg that the reference's path does not find is reported as not found; nothing else is tried.
// The walk reads lonc / latc one cell beyond the computational domain (FW:5757-5765 at a clamped i, j) and the first corner
// may lie there on a domain one cell wide: the host refuses a grid without a halo (locate_check).
// Textual unit of kid_hip.hip, included once.
namespace {
enum { LOC_FOUND = 0, LOC_LOST = 1, LOC_GROUNDED = 2, LOC_SKIPPED = -1 };
enum { LOC_SEARCH = 1, LOC_SCAN = 2 };
// alive: rows with alive[k] == 0 are skipped (NULL: every row).  kill: where a row that is lost or grounded is marked dead, its
// cell put back inside (isc, jsc) so that a decomposed handle does not take it for a berg waiting to be packed (NULL: the row
// keeps ine = jne = -999 or its grounded cell, and the caller reads `status`).  status: NULL or one word per row.
struct LocateIO { const double *lon, *lat; const int32_t *alive; int32_t *ine, *jne; double *xi, *yj; int32_t *status, *kill; long long n; };

__device__ __forceinline__ double loc_dcost(const DevGrid &g, const double *lonc, const double *latc, double x, double y, int i, int j) {   // FW:5845-5858
  const int c = g.idx(i, j);
  const double x2 = lonc[c], y2 = latc[c];
  const double x1m = mod_around(x, x2, g.Lx);
  return (x2 - x1m) * (x2 - x1m) + (y2 - y) * (y2 - y);
}
__device__ __forceinline__ bool loc_in_cell(const DevGrid &g, double x, double y, int i, int j) {
  return is_point_in_cell<false>(g, GlbCell{g, g.idx(i, j)}.corners(), x, y);
}
__device__ __forceinline__ int loc_clamp(int v, int lo, int hi) { return min(hi, max(lo, v)); }
// FW:5862-5893
__device__ bool loc_find_better_min(const DevGrid &g, const double *lonc, const double *latc, double x, double y, int w, int &oi, int &oj) {
  const int xs = max(g.isc, oi - w), xe = min(g.iec, oi + w), ys = max(g.jsc, oj - w), ye = min(g.jec, oj + w);
  bool better = false;
  double dmin = loc_dcost(g, lonc, latc, x, y, oi, oj);
  for (int j = ys; j <= ye; ++j)
    for (int i = xs; i <= xe; ++i) {
      const double d = loc_dcost(g, lonc, latc, x, y, i, j);
      if (d < dmin) { better = true; dmin = d; oi = i; oj = j; }
    }
  return better;
}
// FW:5896-5924
__device__ bool loc_find_cell_loc(const DevGrid &g, double x, double y, int w, int &oi, int &oj) {
  const int xs = max(g.isc, oi - w), xe = min(g.iec, oi + w), ys = max(g.jsc, oj - w), ye = min(g.jec, oj + w);
  for (int j = ys; j <= ye; ++j)
    for (int i = xs; i <= xe; ++i)
      if (loc_in_cell(g, x, y, i, j)) { oi = i; oj = j; return true; }
  return false;
}
// find_cell_by_search up to FW:5826.  Returns true when the search has ended (found says how); false when the moves ran out
// and find_cell is next (FW:5828).
__device__ bool loc_walk(const DevGrid &g, const double *lonc, const double *latc, double x, double y, int &i, int &j, bool &found) {
  const int is = g.isc, ie = g.iec, js = g.jsc, je = g.jec;
  found = false;
  {  // the nearest of the four inset corners, the first listed on a tie (FW:5730-5741)
    const double d1 = loc_dcost(g, lonc, latc, x, y, is + 1, js + 1), d2 = loc_dcost(g, lonc, latc, x, y, ie - 1, js + 1);
    const double d3 = loc_dcost(g, lonc, latc, x, y, ie - 1, je - 1), d4 = loc_dcost(g, lonc, latc, x, y, is + 1, je - 1);
    const double dmin = fmin(fmin(d1, d2), fmin(d3, d4));
    if (d1 == dmin) { i = is + 1; j = js + 1; }
    else if (d2 == dmin) { i = ie - 1; j = js + 1; }
    else if (d3 == dmin) { i = ie - 1; j = je - 1; }
    else if (d4 == dmin) { i = is + 1; j = je - 1; }
    else return true;   // a NaN position: the reference's FATAL (FW:5740); not found
  }
  if (loc_in_cell(g, x, y, i, j)) { found = true; return true; }
  const int nmove = (ie - is) + (je - js);
  for (int icnt = 0; icnt < nmove; ++icnt) {
    const int io = i, jo = j;
    const double d0 = loc_dcost(g, lonc, latc, x, y, io, jo), d1 = loc_dcost(g, lonc, latc, x, y, io, jo + 1);
    const double d2 = loc_dcost(g, lonc, latc, x, y, io - 1, jo + 1), d3 = loc_dcost(g, lonc, latc, x, y, io - 1, jo);
    const double d4 = loc_dcost(g, lonc, latc, x, y, io - 1, jo - 1), d5 = loc_dcost(g, lonc, latc, x, y, io, jo - 1);
    const double d6 = loc_dcost(g, lonc, latc, x, y, io + 1, jo - 1), d7 = loc_dcost(g, lonc, latc, x, y, io + 1, jo);
    const double d8 = loc_dcost(g, lonc, latc, x, y, io + 1, jo + 1);
    const double dmin = fmin(fmin(fmin(fmin(d0, d1), fmin(d2, d3)), fmin(fmin(d4, d5), fmin(d6, d7))), d8);
    int di = 0, dj = 0;   // FW:5769-5777: the centre, the diagonals, then the sides
    if (d0 == dmin) { di = 0; dj = 0; }
    else if (d2 == dmin) { di = -1; dj = 1; }
    else if (d4 == dmin) { di = -1; dj = -1; }
    else if (d6 == dmin) { di = 1; dj = -1; }
    else if (d8 == dmin) { di = 1; dj = 1; }
    else if (d1 == dmin) { di = 0; dj = 1; }
    else if (d3 == dmin) { di = -1; dj = 0; }
    else if (d5 == dmin) { di = 0; dj = -1; }
    else if (d7 == dmin) { di = 1; dj = 0; }
    else return true;   // FATAL in the reference (FW:5779)
    i = loc_clamp(io + di, is, ie);
    j = loc_clamp(jo + dj, js, je);
    if (loc_in_cell(g, x, y, i, j)) { found = true; return true; }
    // (.and. short-circuits in the reference's compilers: find_better_min, which moves i, j, runs on stagnation only)
    if (i == io && j == jo && !loc_find_better_min(g, lonc, latc, x, y, 3, i, j)) {   // stagnated, FW:5797-5824
      found = loc_find_cell_loc(g, x, y, 1, i, j);
      if (!found) found = loc_find_cell_loc(g, x, y, 3, i, j);
      i = loc_clamp(i, is, ie);
      j = loc_clamp(j, js, je);
      if (loc_in_cell(g, x, y, i, j)) found = true;
      return true;
    }
  }
  return false;
}
__device__ __forceinline__ double loc_readlane(double v, int src) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}
// The scan of find_cell (FW:6033-6039) for the lanes of this wave with `need`: every lane of the wave must call it.
__device__ __forceinline__ void loc_wave_scan(const DevGrid &g, bool need, double x, double y, int &oi, int &oj, bool &found) {
  const int lane = (int)__lane_id();
  const int nic = g.iec - g.isc + 1, ncomp = nic * (g.jec - g.jsc + 1);
  unsigned long long pending = __ballot(need);
  while (pending) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
    pending &= pending - 1ull;
    const double sx = loc_readlane(x, src), sy = loc_readlane(y, src);
    int hit = -1;
    for (int base = 0; base < ncomp; base += 64) {
      const int q = base + lane;
      bool in = false;
      if (q < ncomp) { const int dj = q / nic; in = loc_in_cell(g, sx, sy, g.isc + (q - dj * nic), g.jsc + dj); }
      const unsigned long long m = __ballot(in);
      if (m) { hit = base + (__ffsll((long long)m) - 1); break; }
    }
    if (lane == src) {
      if (hit >= 0) { const int dj = hit / nic; oi = g.isc + (hit - dj * nic); oj = g.jsc + dj; found = true; }
      else { oi = -999; oj = -999; found = false; }
    }
  }
}

__global__ void __launch_bounds__(256) locate_kernel(const DevGrid g, const kid_params *pp, const double *lonc, const double *latc, int mode, const LocateIO io,
                                                     unsigned long long *counts) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const bool active = k < io.n && (!io.alive || io.alive[k] != 0);   // (no early return: the scan needs every lane of the wave)
  double x = 0., y = 0.;
  int i = -999, j = -999;
  bool found = false, need_find_cell = false;
  if (active) {
    x = io.lon[k]; y = io.lat[k];
    if (mode == LOC_SEARCH) need_find_cell = !loc_walk(g, lonc, latc, x, y, i, j, found);
    else need_find_cell = true;
  }
  bool need_scan = false;
  if (need_find_cell) {   // find_cell, FW:6025-6031: the guess from the corner arrays' first diagonal step
    const GeoRec a = g.geo[g.idx(g.isd, g.jsd)], c = g.geo[g.idx(g.isd + 1, g.jsd + 1)];
    const double gi = floor((x - a.lon) / (c.lon - a.lon)) + (double)(g.isd + 1), gj = floor((y - a.lat) / (c.lat - a.lat)) + (double)(g.jsd + 1);
    need_scan = true;
    if (gi > (double)(g.isc - 1) && gi < (double)(g.iec + 1) && gj > (double)(g.jsc - 1) && gj < (double)(g.jec + 1)) {   // (false for a NaN or an index no integer holds)
      i = (int)gi; j = (int)gj;
      if (loc_in_cell(g, x, y, i, j)) { found = true; need_scan = false; }
    }
  }
  loc_wave_scan(g, need_scan, x, y, i, j, found);
  int status = LOC_SKIPPED;
  if (active) {
    status = LOC_LOST;
    if (found) {   // IO2:947-957
      double xi = 0., yj = 0.;
      int err = 0; bool bail = false;
      const GlbCell cell{g, g.idx(i, j)};
      (void)pos_within_cell<false>(g, *pp, cell, x, y, i, j, xi, yj, err, bail);
      io.xi[k] = xi; io.yj[k] = yj;
      status = cell.area() == 0. ? LOC_GROUNDED : LOC_FOUND;
    } else { i = -999; j = -999; }
    if (io.kill && status != LOC_FOUND) { io.kill[k] = 0; i = g.isc; j = g.jsc; }
    io.ine[k] = i; io.jne[k] = j;
  }
  if (io.status && k < io.n) io.status[k] = status;
  for (int s = 0; s < 3; ++s) {
    const unsigned long long m = __ballot(status == s);
    if (m && __lane_id() == 0) atomicAdd(counts + s, (unsigned long long)__popcll(m));
  }
}
}  // namespace

extern "C" {

// what the search needs of the grid: the cell centres and one halo cell around the computational domain
static int locate_check(kid_handle *h, const char *what) {
  if (need_static(h)) return KID_EINVAL;
  if (!h->forc.have_centres) { h->err = std::string(what) + ": the static grid was set without lonc / latc, which the search walks on"; return KID_EINVAL; }
  const kid_grid_desc &d = h->gd;
  // (on a domain one cell wide the inset corners isc+1, iec-1 are themselves outside it, and the first move looks one cell further)
  const int w = (d.iec - d.isc < 1 || d.jec - d.jsc < 1) ? 2 : 1;
  if (d.isc - w < d.isd || d.iec + w > d.ied || d.jsc - w < d.jsd || d.jec + w > d.jed) {
    h->err = std::string(what) + ": the search reads lonc / latc one cell beyond the computational domain (FW:5757-5765): the grid needs a halo";
    return KID_EINVAL;
  }
  return KID_OK;
}
// the launch and the read of the three counts; the caller has checked the grid and the mode
static int locate_run(kid_handle *h, int mode, const LocateIO &io, int64_t counts[3]) {
  counts[0] = counts[1] = counts[2] = 0;
  if (io.n <= 0) return KID_OK;
  { const int rc = refresh_tables(h); if (rc) return rc; }
  unsigned long long *d_cnt = nullptr, cnt[3] = {0ull, 0ull, 0ull};
  KID_HIP(h, h->mem.dev(d_cnt, 3, 0));
  hipLaunchKernelGGL(locate_kernel, dim3((unsigned)((io.n + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params,
                     (const double *)h->d_static[KID_G_LONC], (const double *)h->d_static[KID_G_LATC], mode, io, d_cnt);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  const hipError_t e2 = h->mem.drop(d_cnt);
  KID_HIP(h, e);
  KID_HIP(h, e2);
  for (int s = 0; s < 3; ++s) counts[s] = (int64_t)cnt[s];
  return KID_OK;
}

int kid_locate_bergs(kid_handle *h, int mode, int64_t counts[3]) {
  if (!h) return KID_EINVAL;
  if (mode != LOC_SEARCH && mode != LOC_SCAN) { h->err = "kid_locate_bergs: mode is 1 (find_cell_by_search) or 2 (find_cell)"; return KID_EINVAL; }
  { const int rc = locate_check(h, "kid_locate_bergs"); if (rc) return rc; }
  { const int rc = halo_rows_refuse(h, "kid_locate_bergs"); if (rc) return rc; }
  if (h->have_bonds) { h->err = "kid_locate_bergs: bergs with bonds keep their rows and a berg that is not found leaves its row: locate first, then kid_upload_bonds"; return KID_EUNSUPPORTED; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  int64_t cnt[3] = {0, 0, 0};
  const LocateIO io{h->bp.f[KID_B_LON], h->bp.f[KID_B_LAT], h->bp.i[KID_BI_ALIVE], h->bp.i[KID_BI_INE], h->bp.i[KID_BI_JNE], h->bp.f[KID_B_XI], h->bp.f[KID_B_YJ],
                    nullptr, h->bp.i[KID_BI_ALIVE], (long long)h->n};
  { const int rc = locate_run(h, mode, io, cnt); if (rc) return rc; }
  if (h->n > 0) rows_located(h);
  if (counts) for (int s = 0; s < 3; ++s) counts[s] = cnt[s];
  return KID_OK;
}

int kid_set_restart_locate(kid_handle *h, int mode) {
  if (!h) return KID_EINVAL;
  if (mode < 0 || mode > LOC_SCAN) { h->err = "kid_set_restart_locate: mode is 0 (the file's ine, jne), 1 (find_cell_by_search) or 2 (find_cell)"; return KID_EINVAL; }
  h->restart_locate = mode;
  return KID_OK;
}

// ignore_ij_restart inside kid_read_restart: ine, jne of the file's n bergs from their lon, lat (-999 where no cell of this grid
// holds them); temporary blocks sized by the file, from the handle's owner, gone on return
static int restart_locate_cells(kid_handle *h, const double *lon, const double *lat, int32_t *ine, int32_t *jne, long long n) {
  { const int rc = locate_check(h, "kid_read_restart with kid_set_restart_locate"); if (rc) return rc; }
  if (n <= 0) return KID_OK;
  double *d_f[4] = {nullptr, nullptr, nullptr, nullptr};   // lon, lat, xi, yj
  int32_t *d_i[2] = {nullptr, nullptr};
  hipError_t e = hipSuccess;
  for (auto &p : d_f) if (e == hipSuccess) e = h->mem.dev(p, (size_t)n);
  for (auto &p : d_i) if (e == hipSuccess) e = h->mem.dev(p, (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_f[0], lon, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_f[1], lat, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream);
  int rc = KID_OK;
  if (e == hipSuccess) {
    int64_t cnt[3];
    const LocateIO io{d_f[0], d_f[1], nullptr, d_i[0], d_i[1], d_f[2], d_f[3], nullptr, nullptr, n};
    rc = locate_run(h, h->restart_locate, io, cnt);
  }
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(ine, d_i[0], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(jne, d_i[1], (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess && !rc) e = hipStreamSynchronize(h->stream);
  for (auto &p : d_f) { const hipError_t e2 = h->mem.drop(p); if (e == hipSuccess) e = e2; }
  for (auto &p : d_i) { const hipError_t e2 = h->mem.drop(p); if (e == hipSuccess) e = e2; }
  if (rc) return rc;
  KID_HIP(h, e);
  return KID_OK;
}

}  // extern "C"
