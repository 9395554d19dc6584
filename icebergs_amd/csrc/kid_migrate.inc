// kid_migrate.inc -- berg migration between the handles of a domain-decomposed model (SURVEY.md 8f N4, first slice):
//   send_bergs_to_other_pes   /root/reference/src/icebergs_framework.F90:2997-3247  the selection per direction
//   pack_berg_into_buffer2    FW:3250-3379   the wire format: buffer_width reals per berg, integers as reals
//   unpack_berg_from_buffer2  FW:3455-3680   the receiving side: *_old reset, check_and_find_cell (FW:5973-6008), pos_within_cell
// The handle does not talk to the neighbours: the caller moves the buffers (mpp_send / mpp_recv in the reference, FW:3050-3107),
// so a GPU rank exchanges bergs with ranks that still run the reference.  Scope: bergs without bonds, mts and dem off
// (buffer_width = 34, FW:21); the bonded layouts (FW:1266-1292) are refused.
// Each call is one pass over the rows and one host read: the records go through a pinned staging buffer that the
// device addresses directly.
// A berg that leaves the computational domain is marked dead by the step with its post-evolve state stored (what
// send_bergs_to_other_pes would pack before thermodynamics runs, IB:5404-5413); kid_pack_emigrants collects those rows and
// moves their cell index back inside so that they are not sent twice.
// The record itself -- MIG_WIDTH words, their order, kinds and members -- is WIRE_RECORD in kid_rows_plan.hpp.
namespace {
struct MigSel { int dir[2], isc, iec, jsc, jec, has_halo; };   // dir[1] < 0: one direction; has_halo: some row may hold halo_berg != 0
struct MigOut { double *buf[2]; long long cap[2]; };
__device__ __forceinline__ int mig_selected(const MigSel &s, const BergPtrs &b, long long k) {   // 0 / 1: leaves through dir[0] / dir[1]; -1: stays
  const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
  int which = -1;
  for (int q = 0; q < 2; ++q) {
    const int d = s.dir[q];
    if (d < 0 || which >= 0) continue;
    if (d == KID_DIR_E ? i > s.iec : d == KID_DIR_W ? i < s.isc : d == KID_DIR_N ? j > s.jec : j < s.jsc) which = q;   // FW:3028, 3035, 3101, 3109
  }
  if (which >= 0 && s.has_halo && b.f[KID_B_HALO_BERG][k] >= 0.5) which = -1;              // FW:3027
  return which;
}
// pack_berg_into_buffer2 without bonds, FW:3268-3301: one record.  `halo` goes where halo_berg goes: the row's own for an
// emigrant, 1 for the copy update_halo_icebergs sends (FW:1903-1906)
template <int W> __device__ __forceinline__ double wire_word_of(const BergPtrs &b, long long k, double halo) {
  constexpr WireWord ww = WIRE_RECORD[W];
  if constexpr (W == WIRE_W_HALO_BERG) return halo;
  else if constexpr (ww.kind == WIRE_F64) return b.f[ww.field][k];
  else if constexpr (ww.kind == WIRE_ID_HI) return (double)(int32_t)(b.id[k] >> 32);                 // split_id, FW:3297-3299
  else if constexpr (ww.kind == WIRE_ID_LO) return (double)(int32_t)(b.id[k] & 0xffffffffll);
  else return (double)b.i[ww.field][k];                                                              // integers as reals
}
template <int... W> __device__ __forceinline__ void mig_write_words(double *o, const BergPtrs &b, long long k, double halo, std::integer_sequence<int, W...>) {
  ((o[W] = wire_word_of<W>(b, k, halo)), ...);
}
__device__ __forceinline__ void mig_write_record(double *o, const BergPtrs &b, long long k, double halo) {
  mig_write_words(o, b, k, halo, std::make_integer_sequence<int, MIG_WIDTH>{});
}
// the members a record carries, into row k: unpack_berg_from_buffer2's pulls (FW:3503-3541) but for the cell and the position
// inside it, which the receiving grid decides, and the id
template <int W> __device__ __forceinline__ void wire_word_into(const BergPtrs &b, long long k, const double *r) {
  constexpr WireWord ww = WIRE_RECORD[W];
  if constexpr (ww.kind == WIRE_F64 && ww.field != KID_B_XI && ww.field != KID_B_YJ) b.f[ww.field][k] = r[W];
  else if constexpr (ww.kind == WIRE_I32) b.i[ww.field][k] = (int)rint(r[W]);                        // nint, FW:3421
}
template <int... W> __device__ __forceinline__ void mig_read_words(const BergPtrs &b, long long k, const double *r, std::integer_sequence<int, W...>) {
  (wire_word_into<W>(b, k, r), ...);
}
}  // namespace

// pack_berg_into_buffer2 without bonds, FW:3268-3301, into a host-visible staging buffer: the first `cap` selected rows are
// written, all are counted; nothing is deleted yet (the host deletes only when every selected row fitted).  Two
// directions of one exchange pass (east + west, or north + south: no row is in both) can share the launch.
__global__ void __launch_bounds__(256) pack_emigrants_kernel(const BergPtrs b, const MigSel s, long long n, unsigned long long *cursor, const MigOut out) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const int which = k < n ? mig_selected(s, b, k) : -1;
  long long slot = -1;
  for (int q = 0; q < 2; ++q) {   // one reservation per wave and direction
    const long long mine = wave_reserve(which == q, cursor + q);
    if (which == q) slot = mine;
  }
  if (which < 0 || slot >= out.cap[which]) return;
  mig_write_record(out.buf[which] + (size_t)slot * MIG_WIDTH, b, k, b.f[KID_B_HALO_BERG][k]);
}
// delete_iceberg_from_list for the rows just packed (FW:3034): gone, and never selected again
__global__ void __launch_bounds__(256) consume_emigrants_kernel(const BergPtrs b, const MigSel s, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n || mig_selected(s, b, k) < 0) return;
  b.i[KID_BI_ALIVE][k] = 0; b.i[KID_BI_INE][k] = s.isc; b.i[KID_BI_JNE][k] = s.jsc;
}

// the receiving side of unpack_berg_from_buffer2 for rows [k0, k0 + m): the cell that holds (lon, lat) on THIS grid
// (check_and_find_cell FW:5973-6008: the sender's indices, then the regular-grid guess, then a scan of the data domain) and the
// position inside it (FW:3634); a berg no cell takes is the reference's FATAL 'can not find a cell to place berg in!' (FW:3660)
__global__ void __launch_bounds__(64) unpack_immigrants_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, const double *buf, long long k0, long long m, int *nerr) {
  const long long q = (long long)blockIdx.x * 64ll + threadIdx.x;
  if (q >= m) return;
  const long long k = k0 + q;
  const double *r = buf + (size_t)q * MIG_WIDTH;
  // the order of the pulls, FW:3503-3541; everything a record does not carry starts from zero
  for (int f = 0; f < KID_NB_F64; ++f) b.f[f][k] = 0.;
  for (int f = 0; f < KID_NB_I32; ++f) b.i[f][k] = 0;
  const double x = r[WIRE_W_LON], y = r[WIRE_W_LAT];
  mig_read_words(b, k, r, std::make_integer_sequence<int, MIG_WIDTH>{});
  b.id[k] = (int64_t)(((uint64_t)(uint32_t)(int32_t)rint(r[WIRE_W_ID_HI]) << 32) | (uint64_t)(uint32_t)(int32_t)rint(r[WIRE_W_ID_LO]));   // id_from_2_ints
  b.f[KID_B_UVEL_OLD][k] = r[WIRE_W_UVEL]; b.f[KID_B_VVEL_OLD][k] = r[WIRE_W_VVEL]; b.f[KID_B_LON_OLD][k] = x; b.f[KID_B_LAT_OLD][k] = y;   // FW:3573-3577
  b.i[KID_BI_ALIVE][k] = 1;
  int i = (int)rint(r[WIRE_W_INE]), j = (int)rint(r[WIRE_W_JNE]);
  auto holds = [&](int ii, int jj) { return cell_in_data_domain(g, ii, jj) && is_point_in_cell<false>(g, GlbCell{g, g.idx(ii, jj)}.corners(), x, y); };
  bool found = holds(i, j);
  if (!found) {
    const GeoRec a = g.geo[g.idx(g.isd, g.jsd)], c = g.geo[g.idx(g.isd + 1, g.jsd + 1)];
    i = (int)floor((x - a.lon) / (c.lon - a.lon)) + g.isd + 1;                                                           // FW:5993-5994
    j = (int)floor((y - a.lat) / (c.lat - a.lat)) + g.jsd + 1;
    found = holds(i, j);
  }
  if (!found)
    for (int jj = g.jsd + 1; jj <= g.jed && !found; ++jj)
      for (int ii = g.isd + 1; ii <= g.ied && !found; ++ii)
        if (holds(ii, jj)) { i = ii; j = jj; found = true; }
  // the kernels trust cell indices up to one cell outside the computational domain (as kid_upload_bergs checks); a halo row
  // (halo_berg = 1, kid_halo_bergs.inc) sits anywhere in the data domain: only the cell tables of the interacting scheme see it
  if (found && !(r[WIRE_W_HALO_BERG] >= 0.5) && (i < g.isc - 1 || i > g.iec + 1 || j < g.jsc - 1 || j > g.jec + 1)) found = false;
  if (!found) { atomicAdd(nerr, 1); b.i[KID_BI_ALIVE][k] = 0; b.i[KID_BI_INE][k] = g.isc; b.i[KID_BI_JNE][k] = g.jsc; return; }
  double xi = 0., yj = 0.;
  int err = 0; bool bail = false;
  (void)pos_within_cell<false>(g, *pp, GlbCell{g, g.idx(i, j)}, x, y, i, j, xi, yj, err, bail);
  b.i[KID_BI_INE][k] = i; b.i[KID_BI_JNE][k] = j; b.f[KID_B_XI][k] = xi; b.f[KID_B_YJ][k] = yj;
}

extern "C" {

static int mig_supported(kid_handle *h) {
  h->mig_mode = true;   // from the first migration call on, dead rows waiting to be packed survive tail drops, compaction and re-binning (layout_flags)
  if (h->have_bonds || h->params.iceberg_bonds_on || h->params.mts || h->params.dem) {
    h->err = "berg migration covers bergs without bonds (mts, dem, iceberg_bonds_on off): the bonded wire format is not built"; return KID_EUNSUPPORTED;
  }
  return KID_OK;
}

int kid_buffer_width(kid_handle *h, int32_t *width) {
  if (!h || !width) return KID_EINVAL;
  { const int rc = mig_supported(h); if (rc) return rc; }
  *width = MIG_WIDTH;
  return KID_OK;
}

static unsigned long long *mig_pinned_word(kid_handle *h) { return h->mig_word; }   // where the one host read of a call lands (two counters)
static int mig_stage(kid_handle *h, long long rows) {   // host-visible staging the device reads and writes directly (pinned, grows)
  if (!h->mig_word) KID_HIP(h, h->mem.pinned(h->mig_word, 2));
  if (rows <= h->mig_capacity) return KID_OK;
  KID_HIP(h, hipStreamSynchronize(h->stream));
  h->mig_capacity = 0;
  KID_HIP(h, h->mem.drop(h->d_mig_buf));
  const long long cap = std::max<long long>(rows, 4096);
  KID_HIP(h, h->mem.pinned(h->d_mig_buf, (size_t)cap * MIG_WIDTH));
  h->mig_capacity = cap;
  return KID_OK;
}

// One pack pass through the staging buffer, for kid_pack_emigrants* and kid_pack_halo_bergs_pair.  launch(out) enqueues the
// caller's kernel, which counts every selected row of direction q on h->d_count[q] and writes the first out.cap[q] records.
// The staging is sized from what the previous calls carried (`last`), not from the caller's capacities (a host passes its
// whole obuffer, n_slots x 272 B per direction): a pass that finds more than fit counts them all and is repeated once with
// room for the count; the source rows are only read, so nothing is lost.  One host read per pass.  *n[q] (where given) is the
// count; `packed`: the records are in buf[].  A caller's buffer smaller than its count: nothing is copied, KID_ECAPACITY.
}  // extern "C"
template <class Launch>
static int pack_staged(kid_handle *h, int nd, double *const *buf, const int64_t *capacity, int64_t *const *n, long long *last, const char *too_small, Launch launch, bool &packed) {
  packed = false;
  long long sc[2] = {0, 0}, cnt[2] = {0, 0};
  for (int q = 0; q < nd; ++q) sc[q] = std::min<long long>((long long)capacity[q], std::max<long long>(4096, 2 * last[q]));
  MigOut out{};
  bool fits = true, any = false;
  for (int attempt = 0; attempt < 2; ++attempt) {
    { const int rc = mig_stage(h, sc[0] + sc[1]); if (rc) return rc; }
    out = MigOut{{h->d_mig_buf, h->d_mig_buf + (size_t)sc[0] * MIG_WIDTH}, {sc[0], sc[1]}};
    KID_HIP(h, hipMemsetAsync(h->d_count, 0, 2 * sizeof(unsigned long long), h->stream));
    launch(out);
    KID_HIP(h, hipGetLastError());
    KID_HIP(h, hipMemcpyAsync(mig_pinned_word(h), h->d_count, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    fits = true; any = false;
    bool staged = true;
    for (int q = 0; q < nd; ++q) {
      const long long c = cnt[q] = (long long)mig_pinned_word(h)[q];
      if (n[q]) *n[q] = c;
      last[q] = c;
      fits = fits && c <= capacity[q]; any = any || c > 0; staged = staged && c <= sc[q];
      sc[q] = std::min<long long>((long long)capacity[q], std::max<long long>(sc[q], c));
    }
    if (!any || !fits || staged) break;
  }
  if (!any) return KID_OK;
  if (!fits) { h->err = too_small; return KID_ECAPACITY; }
  for (int q = 0; q < nd; ++q) if (cnt[q] > 0) std::memcpy(buf[q], out.buf[q], (size_t)cnt[q] * MIG_WIDTH * sizeof(double));
  packed = true;
  return KID_OK;
}
extern "C" {

static int pack_core(kid_handle *h, int nd, const int32_t *dir, double *const *buf, const int64_t *capacity, int64_t *const *n) {
  for (int q = 0; q < nd; ++q) {
    if (!n[q] || dir[q] < KID_DIR_E || dir[q] > KID_DIR_S || capacity[q] < 0 || (capacity[q] > 0 && !buf[q])) return KID_EINVAL;
    *n[q] = 0;
  }
  { const int rc_h = halo_rows_refuse(h, "kid_pack_emigrants"); if (rc_h) return rc_h; }
  { const int rc = mig_supported(h); if (rc) return rc; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }   // a berg the slow lane still owes a step has not left yet
  if (h->n == 0) return KID_OK;
  const MigSel s{{dir[0], nd > 1 ? dir[1] : -1}, h->gd.isc, h->gd.iec, h->gd.jsc, h->gd.jec, h->flags.has_static ? 1 : 0};
  const unsigned nb = (unsigned)((h->n + 255) / 256);
  bool packed = false;   // nothing is deleted before every record has landed
  const int rc = pack_staged(h, nd, buf, capacity, n, h->mig_last, "kid_pack_emigrants: a buffer is too small (*n holds the bergs waiting); nothing was packed",
                             [&](const MigOut &out) { hipLaunchKernelGGL(pack_emigrants_kernel, dim3(nb), dim3(256), 0, h->stream, h->bp, s, (long long)h->n, h->d_count, out); }, packed);
  if (rc || !packed) return rc;
  hipLaunchKernelGGL(consume_emigrants_kernel, dim3(nb), dim3(256), 0, h->stream, h->bp, s, (long long)h->n);   // no wait: the stream orders it
  KID_HIP(h, hipGetLastError());
  rows_killed(h);
  return KID_OK;
}


int kid_pack_emigrants(kid_handle *h, int32_t dir, double *buf, int64_t capacity, int64_t *n) {
  if (!h) return KID_EINVAL;
  return pack_core(h, 1, &dir, &buf, &capacity, &n);
}

int kid_pack_emigrants_pair(kid_handle *h, int32_t axis, double *buf_a, int64_t capacity_a, int64_t *n_a, double *buf_b, int64_t capacity_b, int64_t *n_b) {
  if (!h || axis < 0 || axis > 1) return KID_EINVAL;
  const int32_t dir[2] = {axis == 0 ? KID_DIR_E : KID_DIR_N, axis == 0 ? KID_DIR_W : KID_DIR_S};
  double *const buf[2] = {buf_a, buf_b};
  const int64_t cap[2] = {capacity_a, capacity_b};
  int64_t *const n[2] = {n_a, n_b};
  return pack_core(h, 2, dir, buf, cap, n);
}

static int unpack_core(kid_handle *h, const double *buf_a, int64_t m_a, const double *buf_b, int64_t m_b) {
  if (!h || m_a < 0 || m_b < 0 || (m_a > 0 && !buf_a) || (m_b > 0 && !buf_b)) return KID_EINVAL;
  { const int rc = mig_supported(h); if (rc) return rc; }
  const int64_t m = m_a + m_b;
  if (m == 0) return KID_OK;
  bool any_halo = false;   // copies of a neighbour's bergs (update_halo_icebergs FW:1800-2131): only the scheme kid_halo_bergs.inc covers takes them
  for (int64_t q = 0; q < m_a && !any_halo; ++q) any_halo = buf_a[(size_t)q * MIG_WIDTH + WIRE_W_HALO_BERG] >= 0.5;
  for (int64_t q = 0; q < m_b && !any_halo; ++q) any_halo = buf_b[(size_t)q * MIG_WIDTH + WIRE_W_HALO_BERG] >= 0.5;
  if (any_halo) { const int rc = halo_bergs_supported(h, "kid_unpack_immigrants"); if (rc) return rc; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  if (h->tail_valid) { int64_t slots = 0, alive = 0; const int rc = kid_num_bergs(h, &slots, &alive); if (rc) return rc; }   // drop a dead tail first (rows waiting to be packed are not part of it)
  if (h->n + m > h->capacity) {   // dead rows of earlier leavers and melted bergs pile up between re-binnings: reclaim them before refusing
    const int rc = kid_compact_bergs(h);
    if (rc) return rc;
  }
  if (h->n + m > h->capacity) { const int rc = auto_reserve(h, h->n + m, "kid_unpack_immigrants"); if (rc) return rc; }   // the remainder: grow
  if (h->n + m > h->capacity) { h->err = "kid_unpack_immigrants: out of capacity: create the handle with room for arrivals"; return KID_ECAPACITY; }
  const size_t mm = (size_t)m;
  { const int rc = mig_stage(h, m); if (rc) return rc; }
  KID_HIP(h, hipStreamSynchronize(h->stream));   // (a consume launch may still read nothing of it, but an earlier unpack kernel may)
  if (m_a > 0) std::memcpy(h->d_mig_buf, buf_a, (size_t)m_a * MIG_WIDTH * sizeof(double));   // rows in the order of the reference's two unpack loops
  if (m_b > 0) std::memcpy(h->d_mig_buf + (size_t)m_a * MIG_WIDTH, buf_b, (size_t)m_b * MIG_WIDTH * sizeof(double));
  { const int rc = refresh_tables(h); if (rc) return rc; }
  // one launch decodes the records into rows n .. n + m - 1, finds the cells and the positions inside them; one host read
  KID_HIP(h, hipMemsetAsync(h->d_count, 0, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(unpack_immigrants_kernel, dim3((unsigned)((mm + 63) / 64)), dim3(64), 0, h->stream, dev_grid(h), h->d_params, h->bp, (const double *)h->d_mig_buf,
                     (long long)h->n, (long long)mm, reinterpret_cast<int *>(h->d_count));
  KID_HIP(h, hipGetLastError());
  KID_HIP(h, hipMemcpyAsync(mig_pinned_word(h), h->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  const int nerr = (int)(*mig_pinned_word(h) & 0xffffffffull);
  // room was made above, before anything was written: this cannot come back full.  The records tell which optional fields
  // can matter from now on (kid_upload_bergs keeps the same books)
  { const int rc = rows_appended(h, m, h->d_mig_buf, "kid_unpack_immigrants: out of capacity"); if (rc) return rc; }
  if (any_halo) h->halo_rows_live = true;
  if (nerr > 0) { h->err = "kid_unpack_immigrants: can not find a cell to place berg in! (" + std::to_string(nerr) + " bergs dropped)"; return KID_EINVAL; }
  return KID_OK;
}

int kid_unpack_immigrants(kid_handle *h, const double *buf, int64_t n) { return unpack_core(h, buf, n, nullptr, 0); }

int kid_unpack_immigrants_pair(kid_handle *h, const double *buf_a, int64_t n_a, const double *buf_b, int64_t n_b) { return unpack_core(h, buf_a, n_a, buf_b, n_b); }

}  // extern "C"
