// kid_halo.inc -- halo update of the on-ocean planes of a domain-decomposed model (DESIGN 7.5):
//   sum_up_spread_fields   icebergs.F90:6077-6150   mpp_update_domains(var_on_ocean, grd%domain) at IB:6106-6107,
//                                                                        then the 9-point sum IB:6126-6131
// A berg writes the nine slots of its own cell only (calculate_mass_on_ocean, IB:4984-...), so the gather of a cell on a tile's
// edge reads slots of cells that belong to the neighbouring tile.  The handle does not talk to the neighbours (as in
// kid_migrate.inc): it packs the edge strips of the live planes into two buffers per axis and unpacks the neighbours' strips
// into its halo; the caller moves the buffers.  East/west first over the computational rows, then north/south over the columns
// isc-w .. iec+w, which carry the corners the first pass has filled (the two hops of mpp_update_domains).
// The work is latency, not bytes (a 1440 x 1080 tile sends 36 x 1080 doubles east): one launch per call, one thread per
// element, plain loads and stores.
// A tile of the top row of a tripolar grid takes its mirror partner's north strip over the fold instead of a north
// neighbour's south strip: kid_unpack_halo_fold / kid_fold_halo_self (IB:6110-6122), further down.
namespace {
// one strip per side (0: hi = east / north, 1: lo = west / south): nrow x ncol cells of every plane, the first of them at
// (col0[side], row0[side]) counted from the corner of the data domain; buf[side] == nullptr: no neighbour there
struct HaloStrips { int np, nrow, ncol, ni, col0[2], row0[2]; double *buf[2]; };
// PACK: planes -> buffers; else buffers -> planes.  Element order of a buffer: plane, row, column (column fastest).
template <bool PACK>
__global__ void __launch_bounds__(256) halo_strips_kernel(double *__restrict__ planes, const size_t ncell, const HaloStrips s) {
  const int per = s.np * s.nrow * s.ncol;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * per) return;
  const int side = t >= per ? 1 : 0, e = t - side * per;
  double *buf = s.buf[side];
  if (!buf) return;
  const int c = e % s.ncol, r = (e / s.ncol) % s.nrow, pl = e / (s.ncol * s.nrow);
  double *cell = planes + (size_t)pl * ncell + (size_t)(s.row0[side] + r) * s.ni + (size_t)(s.col0[side] + c);
  if (PACK) buf[e] = *cell; else *cell = buf[e];
}
// The tripolar north fold (DESIGN 7.5): a tile of the top row takes the strip its mirror partner packed for the north (rows
// jec-w+1 .. jec, columns isc-w .. iec+w) into its own rows jec+1 .. jec+w turned by 180 degrees -- FMS's
// halo(i, nj+k) = field(ni+1-i, nj+1-k) for a centred scalar -- and with the nine slots of every group mirrored through the
// centre (1<->9, 2<->8, 3<->7, 4<->6 of IB:6117-6120; swap == 0: old_bug_rotated_weights, the slot stays).
// row_src: the strip's first row in the planes (SELF only), row_top: the row strip row 0 lands in (jec + w).
struct FoldStrip { int np, w, ncol, ni, col0, row_src, row_top, swap; const double *buf; };
// SELF: the partner is the handle itself (it owns the whole zonal width), planes to planes.  What a thread reads (rows <= jec)
// and what any thread writes (rows > jec) are disjoint, so the one launch needs no ordering between its threads.
template <bool SELF>
__global__ void __launch_bounds__(256) halo_fold_kernel(double *__restrict__ planes, const size_t ncell, const FoldStrip s) {
  const int per = s.np * s.w * s.ncol;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  const int c = e % s.ncol, r = (e / s.ncol) % s.w, pl = e / (s.ncol * s.w);
  const int to = s.swap ? pl - pl % 9 + (8 - pl % 9) : pl;
  const double v = SELF ? planes[(size_t)pl * ncell + (size_t)(s.row_src + r) * s.ni + (size_t)(s.col0 + c)] : s.buf[e];
  planes[(size_t)to * ncell + (size_t)(s.row_top - r) * s.ni + (size_t)(s.col0 + s.ncol - 1 - c)] = v;
}
}  // namespace

static int halo_planes(const kid_handle *h) { return kid::halo_plane_count(h->params.pass_fields_to_ocean_model, h->params.diag_mask); }
// the strips of one call; false: axis or width out of range
static bool halo_strips(const kid_handle *h, int axis, int w, bool pack, HaloStrips &s) {
  const kid_grid_desc &d = h->gd;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1;
  const int halo = std::min(std::min(d.isc - d.isd, d.ied - d.iec), std::min(d.jsc - d.jsd, d.jed - d.jec));
  if (axis < 0 || axis > 1 || w < 1 || w > halo || w > nic || w > njc) return false;
  s.np = halo_planes(h); s.ni = h->ni; s.buf[0] = s.buf[1] = nullptr;
  const int i0 = d.isc - d.isd, i1 = d.iec - d.isd, j0 = d.jsc - d.jsd, j1 = d.jec - d.jsd;   // the computational corners, from the data corner
  if (axis == 0) {
    s.nrow = njc; s.ncol = w; s.row0[0] = s.row0[1] = j0;
    s.col0[0] = pack ? i1 - w + 1 : i1 + 1;   // hi: sent east from iec-w+1 .. iec, received from the east into iec+1 .. iec+w
    s.col0[1] = pack ? i0 : i0 - w;           // lo: sent west from isc .. isc+w-1, received from the west into isc-w .. isc-1
  } else {
    s.nrow = w; s.ncol = nic + 2 * w; s.col0[0] = s.col0[1] = i0 - w;
    s.row0[0] = pack ? j1 - w + 1 : j1 + 1;
    s.row0[1] = pack ? j0 : j0 - w;
  }
  return true;
}
static int halo_refuse(kid_handle *h, const char *who) {
  h->err = std::string(who) + ": axis is 0 (east/west) or 1 (north/south) and 1 <= width <= min(halo, nic, njc)";
  return KID_EINVAL;
}
static int halo_stage(kid_handle *h, long long count) {   // pinned staging the device addresses directly (grows)
  if (count <= h->halo_capacity) return KID_OK;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->halo_capacity = 0;
  KID_HIP(h, h->mem.drop(h->halo_buf));
  KID_HIP(h, h->mem.pinned(h->halo_buf, (size_t)count));
  h->halo_capacity = count;
  return KID_OK;
}
template <bool PACK>
static int halo_launch(kid_handle *h, const HaloStrips &s) {
  const long long total = 2ll * s.np * s.nrow * s.ncol;
  hipLaunchKernelGGL(halo_strips_kernel<PACK>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,
                     on_ocean_base(h), h->ncell, s);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}

// the fold strip of one call: the north strip of kid_pack_halo_pair(axis 1), mirrored into the rows above jec
static bool fold_strip(const kid_handle *h, int w, FoldStrip &f) {
  HaloStrips s;
  if (!halo_strips(h, 1, w, true, s)) return false;
  f.np = s.np; f.w = w; f.ncol = s.ncol; f.ni = s.ni; f.col0 = s.col0[0]; f.row_src = s.row0[0]; f.row_top = s.row0[0] + 2 * w - 1; f.buf = nullptr;
  return true;
}
template <bool SELF>
static int fold_launch(kid_handle *h, const FoldStrip &f) {
  const long long total = (long long)f.np * f.w * f.ncol;
  hipLaunchKernelGGL(halo_fold_kernel<SELF>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream,
                     on_ocean_base(h), h->ncell, f);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}

extern "C" {

int kid_calculate_mass_on_ocean(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_calculate_mass_on_ocean"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  const int rc = zero_planes(h, ON_OCEAN_ALL);   // IB:4984-4987
  return rc ? rc : launch_berg<PH_SPREAD>(h);
}

int kid_halo_plane_count(kid_handle *h, int32_t *nplanes) {
  if (!h || !nplanes) return KID_EINVAL;
  *nplanes = halo_planes(h);
  return KID_OK;
}

int kid_halo_buffer_count(kid_handle *h, int32_t axis, int32_t width, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  HaloStrips s;
  if (!halo_strips(h, axis, width, true, s)) return halo_refuse(h, "kid_halo_buffer_count");
  *count = (int64_t)s.np * s.nrow * s.ncol;
  return KID_OK;
}

int kid_pack_halo_pair(kid_handle *h, int32_t axis, int32_t width, double *buf_hi, double *buf_lo, int32_t on_device) {
  if (!h) return KID_EINVAL;
  HaloStrips s;
  if (!halo_strips(h, axis, width, true, s)) return halo_refuse(h, "kid_pack_halo_pair");
  if (!buf_hi && !buf_lo) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = join_side(h); if (rc) return rc; }
  const long long per = (long long)s.np * s.nrow * s.ncol;
  if (on_device) { s.buf[0] = buf_hi; s.buf[1] = buf_lo; return halo_launch<true>(h, s); }
  { const int rc = halo_stage(h, 2 * per); if (rc) return rc; }
  s.buf[0] = buf_hi ? h->halo_buf : nullptr; s.buf[1] = buf_lo ? h->halo_buf + per : nullptr;
  { const int rc = halo_launch<true>(h, s); if (rc) return rc; }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  if (buf_hi) std::memcpy(buf_hi, s.buf[0], (size_t)per * sizeof(double));
  if (buf_lo) std::memcpy(buf_lo, s.buf[1], (size_t)per * sizeof(double));
  return KID_OK;
}

int kid_unpack_halo_pair(kid_handle *h, int32_t axis, int32_t width, const double *from_lo, const double *from_hi, int32_t on_device) {
  if (!h) return KID_EINVAL;
  HaloStrips s;
  if (!halo_strips(h, axis, width, false, s)) return halo_refuse(h, "kid_unpack_halo_pair");
  if (!from_lo && !from_hi) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = join_side(h); if (rc) return rc; }
  const long long per = (long long)s.np * s.nrow * s.ncol;
  if (on_device) { s.buf[0] = const_cast<double *>(from_hi); s.buf[1] = const_cast<double *>(from_lo); return halo_launch<false>(h, s); }
  { const int rc = halo_stage(h, 2 * per); if (rc) return rc; }
  KID_HIP(h, hipStreamSynchronize(h->stream));   // an earlier unpack launch may still be reading the staging buffer
  if (from_hi) std::memcpy(h->halo_buf, from_hi, (size_t)per * sizeof(double));
  if (from_lo) std::memcpy(h->halo_buf + per, from_lo, (size_t)per * sizeof(double));
  s.buf[0] = from_hi ? h->halo_buf : nullptr; s.buf[1] = from_lo ? h->halo_buf + per : nullptr;
  return halo_launch<false>(h, s);   // no wait: the caller's buffers are free already and the stream orders the gather behind it
}

int kid_unpack_halo_fold(kid_handle *h, int32_t width, const double *from_fold, int32_t swap_slots, int32_t on_device) {
  if (!h) return KID_EINVAL;
  FoldStrip f;
  if (!fold_strip(h, width, f)) return halo_refuse(h, "kid_unpack_halo_fold");
  if (!from_fold) { h->err = "kid_unpack_halo_fold: from_fold is NULL (a fold tile always has a partner)"; return KID_EINVAL; }
  { const int rc_h = halo_rows_refuse(h, "kid_unpack_halo_fold"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = join_side(h); if (rc) return rc; }
  f.swap = swap_slots ? 1 : 0;
  if (on_device) { f.buf = from_fold; return fold_launch<false>(h, f); }
  const long long per = (long long)f.np * f.w * f.ncol;
  { const int rc = halo_stage(h, 2 * per); if (rc) return rc; }   // (the size the north/south pair of the same width asks for: no regrowth between the two)
  KID_HIP(h, hipStreamSynchronize(h->stream));   // an earlier unpack launch may still be reading the staging buffer
  std::memcpy(h->halo_buf, from_fold, (size_t)per * sizeof(double));
  f.buf = h->halo_buf;
  return fold_launch<false>(h, f);   // no wait, as kid_unpack_halo_pair
}

int kid_fold_halo_self(kid_handle *h, int32_t width, int32_t swap_slots) {
  if (!h) return KID_EINVAL;
  FoldStrip f;
  if (!fold_strip(h, width, f)) return halo_refuse(h, "kid_fold_halo_self");
  { const int rc_h = halo_rows_refuse(h, "kid_fold_halo_self"); if (rc_h) return rc_h; }
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = join_side(h); if (rc) return rc; }
  f.swap = swap_slots ? 1 : 0;
  return fold_launch<true>(h, f);
}

}  // extern "C"
