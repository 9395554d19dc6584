// kid_halo_bergs.inc -- halo bergs of a domain-decomposed model (SURVEY.md 8f N4; DESIGN 7.6):
//   update_halo_icebergs   icebergs_framework.F90 (FW):1800-2131   the strips per direction, the record with halo_berg = 1
//   interactive_force      icebergs.F90:480-607   walks the lists of the neighbouring cells, which on a tile edge belong to another rank
// A halo row is a copy of a neighbour tile's berg: halo_berg = 1, alive, its cell in the halo.  It is a force source for one
// kid_evolve_icebergs and nothing else: the velocity sweep skips it, the position sweep retires it (kid_mts.inc), and while such
// rows are resident (h->halo_rows_live) every call that would melt, spread, count, move or write them out is refused.
// This file is the sending side.  The receiving side is kid_unpack_immigrants as it stands (the record is the emigrants' one).
// Scope: unbonded interacting bergs under the single-time-step Verlet scheme; everything else is refused by name.
namespace {
// axis 0: rows jsc..jec, hi strip columns iec-w+2..iec (w-1 of them), lo strip isc..isc+w-1 (FW:1896, 1911: the asymmetry is
// the reference's -- a cell (isd, j) has no south-west corner on the receiving side); axis 1: columns isd..ied, so the halo rows
// axis 0 has just brought are sent on and a diagonal neighbour's bergs arrive in two hops, hi strip rows jec-w+2..jec, lo strip
// jsc..jsc+w-1 (FW:1981, 1995).  On a narrow tile a cell can be in both strips; its bergs go both ways.
struct HaloBergSel { int axis, w, on_hi, on_lo, isc, iec, jsc, jec, isd, ied; };
__device__ __forceinline__ int halo_berg_selected(const HaloBergSel &s, const BergPtrs &b, long long k) {   // bit 0: hi, bit 1: lo
  if (b.i[KID_BI_ALIVE][k] == 0) return 0;
  const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
  const bool ew = s.axis == 0;
  const int c = ew ? i : j, c0 = ew ? s.isc : s.jsc, c1 = ew ? s.iec : s.jec;   // along the axis
  const int x = ew ? j : i, x0 = ew ? s.jsc : s.isd, x1 = ew ? s.jec : s.ied;   // across it
  if (x < x0 || x > x1) return 0;
  int sel = 0;
  if (s.on_hi && c >= c1 - s.w + 2 && c <= c1) sel |= 1;
  if (s.on_lo && c >= c0 && c <= c0 + s.w - 1) sel |= 2;
  return sel;
}
// one direction: a reservation per wave (all selected rows are counted), then the first `cap` of them are written
__device__ __forceinline__ void halo_berg_emit(bool mine, unsigned long long *cursor, double *buf, long long cap, const BergPtrs &b, long long k) {
  const long long slot = wave_reserve(mine, cursor);
  if (slot >= 0 && slot < cap) mig_write_record(buf + (size_t)slot * MIG_WIDTH, b, k, 1.);   // FW:1904
}
}  // namespace

// One lane per row, both directions of an axis in one launch (a row on a narrow tile can go both ways).  The source rows are
// only read.  Plain vector loads and stores, no LDS.
__global__ void __launch_bounds__(256) halo_berg_pack_kernel(const BergPtrs b, const HaloBergSel s, long long n, unsigned long long *cursor, const MigOut out) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const int sel = k < n ? halo_berg_selected(s, b, k) : 0;
  halo_berg_emit((sel & 1) != 0, cursor, out.buf[0], out.cap[0], b, k);
  halo_berg_emit((sel & 2) != 0, cursor + 1, out.buf[1], out.cap[1], b, k);
}

extern "C" {

static int halo_bergs_supported(kid_handle *h, const char *what) {
  const kid_params &p = h->params;
  const char *why = nullptr;
  if (p.footloose) why = "footloose: its calving pass and the children it appends are not covered on tiles";
  else if (h->have_bonds || p.iceberg_bonds_on) why = "iceberg_bonds_on: the bonded record (FW:1266-1292) is not built";
  else if (p.mts) why = "mts: transfer_mts_bergs and its wider record are not built";
  else if (p.dem) why = "dem: its wider record is not built";
  else if (p.find_melt_using_spread_mass) why = "find_melt_using_spread_mass is not covered on tiles";
  else if (p.static_icebergs) why = "static_icebergs: kid_evolve_icebergs does nothing then, so nothing would use the copies or retire them";
  else if (p.periodic_reentry) why = "periodic_reentry: a zonally periodic run (update_latlon, IB:5467) is not covered";
  else if (!p.interactive_icebergs_on) why = "interactive_icebergs_on is off: bergs that do not interact need no halo bergs";
  else if (p.Runge_not_Verlet) why = "Runge_not_Verlet: interacting bergs are stepped by the Verlet scheme only";
  if (!why) return KID_OK;
  h->err = std::string(what) + ": halo bergs cover unbonded interacting bergs under the single-time-step Verlet scheme; " + why;
  return KID_EUNSUPPORTED;
}

int kid_pack_halo_bergs_pair(kid_handle *h, int32_t axis, int32_t width, double *buf_hi, int64_t capacity_hi, int64_t *n_hi, double *buf_lo, int64_t capacity_lo, int64_t *n_lo) {
  if (!h || axis < 0 || axis > 1) return KID_EINVAL;
  double *const buf[2] = {buf_hi, buf_lo};
  const int64_t capacity[2] = {buf_hi ? capacity_hi : 0, buf_lo ? capacity_lo : 0};
  int64_t *const n[2] = {n_hi, n_lo};
  for (int q = 0; q < 2; ++q) {
    if (buf[q] && (!n[q] || capacity[q] < 0)) return KID_EINVAL;
    if (n[q]) *n[q] = 0;
  }
  { const int rc = halo_bergs_supported(h, "kid_pack_halo_bergs_pair"); if (rc) return rc; }
  const kid_grid_desc &d = h->gd;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1, halo = std::min(std::min(d.isc - d.isd, d.ied - d.iec), std::min(d.jsc - d.jsd, d.jed - d.jec));
  const int w = width == 0 ? halo : width;
  if (w < 2 || w > std::min(halo, std::min(nic, njc))) {
    h->err = "kid_pack_halo_bergs_pair: width must be 0 (the grid's halo) or 2 .. min(halo, nic, njc)"; return KID_EINVAL;
  }
  h->mig_mode = true;   // a decomposed run, as with the migration calls
  if (!buf_hi && !buf_lo) return KID_OK;   // no neighbour on either side
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  if (h->n == 0) return KID_OK;
  const HaloBergSel s{axis, w, buf_hi ? 1 : 0, buf_lo ? 1 : 0, d.isc, d.iec, d.jsc, d.jec, d.isd, d.ied};
  const unsigned nb = (unsigned)((h->n + 255) / 256);
  bool packed = false;
  return pack_staged(h, 2, buf, capacity, n, h->halo_last, "kid_pack_halo_bergs_pair: a buffer is too small (*n holds the bergs of the strip); nothing was packed",
                     [&](const MigOut &out) { hipLaunchKernelGGL(halo_berg_pack_kernel, dim3(nb), dim3(256), 0, h->stream, h->bp, s, (long long)h->n, h->d_count, out); }, packed);
}

int kid_halo_berg_count(kid_handle *h, int64_t *n) {
  if (!h || !n) return KID_EINVAL;
  *n = 0;
  if (!h->flags.has_static) return KID_OK;   // no row has ever held halo_berg != 0
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  return count_rows(h, h->bp.i[KID_BI_ALIVE], h->bp.f[KID_B_HALO_BERG], n);
}

}  // extern "C"
