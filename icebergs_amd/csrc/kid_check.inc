// kid_check.inc -- the reference's debug-mode invariants on the resident state: kid_check_bergs and kid_sorted_ids.
//   check_position            FW:6576-6603   stored xi, yj against pos_within_cell(lon, lat, ine, jne); the land mask
//   count_out_of_order        FW:4039-4089   "# in halo" (icnt2), "# identicals" (icnt3); "# out of order" has no counterpart
//   check_for_duplicates      FW:4118-4158   pairs with sameid (FW:4381), pairs with sameberg (FW:4397)
//   check_for_duplicate_ids_in_list FW:7405-7452, the half on one PE: ids that occur more than once
// Nothing is written to a row and nothing is downloaded but the report.
//
// Position.  check_position_kernel, one lane per row, pos_within_cell<false> on GlbCell: the instance kid_locate_bergs, the
// restart read and the immigrants' unpack store from.  Counters by ballot and popcount, one atomicAdd per wave and counter;
// the largest |stored - recomputed| by a butterfly and one 64-bit atomicMax per wave on the bit pattern (non-negative doubles
// order like unsigned integers); the smallest offending id by a 64-bit atomicMin of the waves that have an offender.  The row
// that holds it comes from a second launch of the same kernel, only when a count is non-zero.
//
// Groups.  The rows that count (alive, cell on the computational domain) are selected into a list of row numbers, in row
// order (rocprim::select).  Stable LSD radix passes over it by start_lat, start_lon, start_mass, start_day, start_year put rows
// whose five keys are equal by value next to each other (check_sort_key, kid_check_plan.hpp: -0.0 taken for +0.0, every NaN
// last); check_heads_kernel compares each position with its predecessor BY VALUE, so a NaN row is a group of its own.  The
// group of a position is named by the position of its head: an inclusive maximum scan of (head ? q : 0) (rocprim::inclusive_scan).
// A scan rather than a lane that walks back to its head: the cost is one pass over the rows whatever the group sizes, and the
// head positions are what the pair kernel needs to know where a group ends.  check_pairs_kernel: the last row of a group adds
// check_pair_count(m) to "# with same id"; every row walks over the LATER rows of its group and counts those equal in the
// members of sameberg -- m(m-1)/2 compares per group of m rows, which is 0 in a healthy state (every group has one row) and
// grows with the square of the largest group in a broken one.  One more stable pass by cell on top of that order gives
// (cell, keys): its rows that equal their predecessor in cell and keys are "# identicals", the sum of (m - 1).
// Ids: one 64-bit radix sort of the ids of the rows that count, adjacent compares; kid_sorted_ids copies that array out.
// Every block is temporary, from the handle's owner, sized by h->n, and gone on return.
// Textual unit of kid_hip.hip, included once.
namespace {

enum { CK_ROWS = 0, CK_XIYJ, CK_LAND, CK_IN_HALO, CK_IDENTICAL, CK_SAME_ID, CK_SAME_BERG, CK_DUP_IDS, CK_NCOUNT };
enum { CK_F_XIYJ = 0, CK_F_LAND, CK_F_SAME_ID, CK_F_DUP_IDS, CK_NFIRST };
// the device's copy of the report: first_id and first_row start at the largest value and take minima
struct CheckDev { unsigned long long count[CK_NCOUNT]; unsigned long long max_bits[2]; long long first_id[CK_NFIRST], first_row[CK_NFIRST]; };
constexpr long long CK_NONE = 0x7fffffffffffffffll;

__device__ __forceinline__ void ck_wave_count(bool mine, unsigned long long *counter) {
  const unsigned long long m = __ballot(mine);
  if (m && __lane_id() == 0) atomicAdd(counter, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ void ck_wave_add(unsigned long long v, unsigned long long *counter) {
  v = chkd_wave_sum(v);
  if (v && __lane_id() == 0) atomicAdd(counter, v);
}
// the smallest of the lanes' values (CK_NONE: the lane has none) into *dst, one atomic per wave that has one
__device__ __forceinline__ void ck_wave_min(long long v, long long *dst) {
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) { const long long o = __shfl_xor(v, d); v = o < v ? o : v; }
  if (v != CK_NONE && __lane_id() == 0) atomicMin(dst, v);
}
__device__ __forceinline__ void ck_wave_max_bits(double v, unsigned long long *dst) {   // v >= 0, never a NaN
  v = chkd_wave_max(v);
  if (v > 0. && __lane_id() == 0) atomicMax(dst, chkd_bits(v));
}

// do_pos: the position check (needs the static grid); the "# in halo" count needs the handle's index ranges only.
// find: the second pass -- r.first_id holds the smallest offending ids, the rows that hold them go to r.first_row.
__global__ void __launch_bounds__(256) check_position_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, const long long n, const int do_pos, const int do_halo,
                                                             const int find, CheckDev *r) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const bool live = k < n && b.i[KID_BI_ALIVE][k] != 0;
  bool bad_xy = false, bad_land = false, in_halo = false;
  double dxi = 0., dyj = 0.;
  if (live) {
    const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
    if (do_pos) {
      double xi = 0., yj = 0.;
      int err = 0; bool bail = false;
      // (a cell outside the data domain: pos_within_cell returns -999, -999 before it reads a corner)
      (void)pos_within_cell<false>(g, *pp, GlbCell{g, g.idx(i, j)}, b.f[KID_B_LON][k], b.f[KID_B_LAT][k], i, j, xi, yj, err, bail);
      const double sxi = b.f[KID_B_XI][k], syj = b.f[KID_B_YJ][k];
      bad_xy = xi != sxi || yj != syj;   // FW:6592
      const double ax = fabs(sxi - xi), ay = fabs(syj - yj);
      if (ax < __builtin_inf()) dxi = ax;   // (false for a NaN and for an infinite difference: both sides finite)
      if (ay < __builtin_inf()) dyj = ay;
      if (i >= g.isd && i <= g.ied && j >= g.jsd && j <= g.jed) bad_land = g.geo[g.idx(i, j)].msk == 0.;   // FW:6598
    }
    if (do_halo) in_halo = b.f[KID_B_HALO_BERG][k] < 0.5 && (i < g.isc || i > g.iec || j < g.jsc || j > g.jec);
  }
  if (find) {
    const long long id = live ? (long long)b.id[k] : 0;
    ck_wave_min(bad_xy && id == r->first_id[CK_F_XIYJ] ? k : CK_NONE, &r->first_row[CK_F_XIYJ]);
    ck_wave_min(bad_land && id == r->first_id[CK_F_LAND] ? k : CK_NONE, &r->first_row[CK_F_LAND]);
    return;
  }
  if (do_pos) {
    ck_wave_count(live, &r->count[CK_ROWS]);
    ck_wave_count(bad_xy, &r->count[CK_XIYJ]);
    ck_wave_count(bad_land, &r->count[CK_LAND]);
    ck_wave_max_bits(dxi, &r->max_bits[0]);
    ck_wave_max_bits(dyj, &r->max_bits[1]);
    if (__ballot(bad_xy)) ck_wave_min(bad_xy ? (long long)b.id[k] : CK_NONE, &r->first_id[CK_F_XIYJ]);
    if (__ballot(bad_land)) ck_wave_min(bad_land ? (long long)b.id[k] : CK_NONE, &r->first_id[CK_F_LAND]);
  }
  if (do_halo) ck_wave_count(in_halo, &r->count[CK_IN_HALO]);
}

// the rows the order, duplicate and id checks cover: alive, cell on the computational domain
__global__ void __launch_bounds__(256) check_counted_kernel(const BergPtrs b, const long long n, const int isc, const int iec, const int jsc, const int jec, unsigned char *__restrict__ flag) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
  flag[k] = (b.i[KID_BI_ALIVE][k] != 0 && i >= isc && i <= iec && j >= jsc && j <= jec) ? 1 : 0;
}
__global__ void __launch_bounds__(256) check_key_f64_kernel(const double *__restrict__ fld, const int *__restrict__ rows, unsigned long long *__restrict__ keys, const long long m) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q < m) keys[q] = check_sort_key(fld[rows[q]]);
}
__global__ void __launch_bounds__(256) check_key_id_kernel(const int64_t *__restrict__ id, const int *__restrict__ rows, long long *__restrict__ keys, const long long m) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q < m) keys[q] = (long long)id[rows[q]];
}
__device__ __forceinline__ CheckKeys ck_keys(const BergPtrs &b, long long k) {
  return CheckKeys{b.i[KID_BI_START_YEAR][k], b.f[KID_B_START_DAY][k], b.f[KID_B_START_MASS][k], b.f[KID_B_START_LON][k], b.f[KID_B_START_LAT][k]};
}
// head[q] = q where position q starts a group of equal keys (with_cell: of equal cell and keys), 0 elsewhere -- position 0 is
// a head either way.  with_cell: the rows that are no head are the identicals and are counted here; head may be null.
__global__ void __launch_bounds__(256) check_heads_kernel(const BergPtrs b, const int *__restrict__ rows, const long long m, const int with_cell, int *__restrict__ head,
                                                          unsigned long long *__restrict__ n_identical) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  bool follows = false;
  if (q < m && q > 0) {
    const long long k = rows[q], kp = rows[q - 1];
    follows = check_same_keys(ck_keys(b, k), ck_keys(b, kp));
    if (with_cell) follows = follows && b.i[KID_BI_INE][k] == b.i[KID_BI_INE][kp] && b.i[KID_BI_JNE][k] == b.i[KID_BI_JNE][kp];
  }
  if (head && q < m) head[q] = follows ? 0 : (int)q;
  if (with_cell) ck_wave_count(follows, n_identical);
}
// hp[q]: the position of the head of q's group.  find: the second pass for the row of r->first_id[CK_F_SAME_ID].
__global__ void __launch_bounds__(256) check_pairs_kernel(const BergPtrs b, const int *__restrict__ rows, const int *__restrict__ hp, const long long m, const int mts, const int find,
                                                          CheckDev *r) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  unsigned long long pairs = 0ull, same = 0ull;
  long long lo = CK_NONE;
  if (q < m) {
    const int h0 = hp[q];
    const bool last = q + 1 == m || hp[q + 1] != h0;
    const bool grouped = !last || h0 != (int)q;   // its group has more than one row
    const long long k = rows[q];
    if (find) { if (grouped && (long long)b.id[k] == r->first_id[CK_F_SAME_ID]) lo = k; }
    else {
      if (last) pairs = check_pair_count(q - (long long)h0 + 1);
      if (grouped) lo = (long long)b.id[k];
      for (long long q2 = q + 1; q2 < m && hp[q2] == h0; ++q2)
        if (check_same_members(b.f, k, (long long)rows[q2], mts != 0)) ++same;
    }
  }
  if (find) { ck_wave_min(lo, &r->first_row[CK_F_SAME_ID]); return; }
  ck_wave_add(pairs, &r->count[CK_SAME_ID]);
  ck_wave_add(same, &r->count[CK_SAME_BERG]);
  if (__ballot(lo != CK_NONE)) ck_wave_min(lo, &r->first_id[CK_F_SAME_ID]);
}
// ids ascending, rows beside them: a position whose id is its predecessor's is a duplicate (FW:7418-7423)
__global__ void __launch_bounds__(256) check_dup_ids_kernel(const long long *__restrict__ ids, const int *__restrict__ rows, const long long m, const int find, CheckDev *r) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (find) {
    ck_wave_min(q < m && ids[q] == r->first_id[CK_F_DUP_IDS] ? (long long)rows[q] : CK_NONE, &r->first_row[CK_F_DUP_IDS]);
    return;
  }
  const bool dup = q < m && q > 0 && ids[q] == ids[q - 1];
  ck_wave_count(dup, &r->count[CK_DUP_IDS]);
  if (__ballot(dup)) ck_wave_min(dup ? ids[q] : CK_NONE, &r->first_id[CK_F_DUP_IDS]);
}

struct CheckTmp { CheckDev *rep = nullptr; unsigned char *flag = nullptr; int *rows[2] = {nullptr, nullptr}, *head = nullptr, *hp = nullptr; unsigned long long *k64[2] = {nullptr, nullptr};
                  long long *d_m = nullptr; Scratch tmp; };
static hipError_t check_tmp_free(kid_handle *h, CheckTmp &t) {
  hipError_t first = hipSuccess;
  auto note = [&first](hipError_t e) { if (first == hipSuccess) first = e; };
  for (int q = 0; q < 2; ++q) { note(h->mem.drop(t.rows[q])); note(h->mem.drop(t.k64[q])); }
  note(h->mem.drop(t.rep)); note(h->mem.drop(t.flag)); note(h->mem.drop(t.head)); note(h->mem.drop(t.hp)); note(h->mem.drop(t.d_m));
  note((hipError_t)h->mem.release(&t.tmp.p));
  t.tmp.bytes = 0;
  return first;
}
static dim3 check_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

// t.rows[0] = the rows that count, in row order; *m = how many
static int check_select(kid_handle *h, CheckTmp &t, long long *m) {
  const long long n = h->n;
  const kid_grid_desc &d = h->gd;
  *m = 0;
  if (n <= 0) return KID_OK;
  const size_t sn = (size_t)n;
  KID_HIP(h, h->mem.dev(t.flag, sn));
  for (int q = 0; q < 2; ++q) { KID_HIP(h, h->mem.dev(t.rows[q], sn)); KID_HIP(h, h->mem.dev(t.k64[q], sn)); }
  KID_HIP(h, h->mem.dev(t.d_m, 1, 0));
  hipLaunchKernelGGL(check_counted_kernel, check_grid(n), dim3(256), 0, h->stream, h->bp, n, d.isc, d.iec, d.jsc, d.jec, t.flag);
  KID_HIP(h, hipGetLastError());
  size_t bytes = 0;
  KID_HIP(h, rocprim::select(nullptr, bytes, rocprim::counting_iterator<int>(0), t.flag, t.rows[0], t.d_m, sn, h->stream));
  KID_HIP(h, h->mem.reserve(t.tmp, bytes));
  bytes = t.tmp.bytes;
  KID_HIP(h, rocprim::select(t.tmp.p, bytes, rocprim::counting_iterator<int>(0), t.flag, t.rows[0], t.d_m, sn, h->stream));
  KID_HIP(h, hipMemcpyAsync(m, t.d_m, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}
// the ids of t.rows[0][0 .. m) ascending in *ids (a view of t.k64), their rows in *rows (a view of t.rows); t.rows[0] stays
static int check_sort_ids(kid_handle *h, CheckTmp &t, long long m, const long long **ids, const int **rows) {
  long long *k[2] = {(long long *)t.k64[0], (long long *)t.k64[1]};
  size_t bytes = 0;
  KID_HIP(h, rocprim::radix_sort_pairs(nullptr, bytes, k[0], k[1], t.rows[0], t.rows[1], (size_t)m, 0, 64, h->stream));
  KID_HIP(h, h->mem.reserve(t.tmp, bytes));
  hipLaunchKernelGGL(check_key_id_kernel, check_grid(m), dim3(256), 0, h->stream, (const int64_t *)h->bp.id, (const int *)t.rows[0], k[0], m);
  KID_HIP(h, hipGetLastError());
  bytes = t.tmp.bytes;
  KID_HIP(h, rocprim::radix_sort_pairs(t.tmp.p, bytes, k[0], k[1], t.rows[0], t.rows[1], (size_t)m, 0, 64, h->stream));
  *ids = k[1]; *rows = t.rows[1];
  return KID_OK;
}

static int check_run(kid_handle *h, CheckTmp &t, uint32_t what, kid_check_report *rep) {
  const long long n = h->n;
  const kid_grid_desc &d = h->gd;
  CheckDev r{};
  for (int q = 0; q < CK_NFIRST; ++q) { r.first_id[q] = CK_NONE; r.first_row[q] = CK_NONE; }
  if (n > 0) {
    KID_HIP(h, h->mem.dev(t.rep, 1));
    KID_HIP(h, hipMemcpyAsync(t.rep, &r, sizeof(r), hipMemcpyHostToDevice, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));   // (r is read again below)
    const int do_pos = (what & KID_CHECK_POSITION) ? 1 : 0, do_halo = (what & KID_CHECK_ORDER) ? 1 : 0;
    if (do_pos) { const int rc = refresh_tables(h); if (rc) return rc; }
    if (do_pos || do_halo) {
      hipLaunchKernelGGL(check_position_kernel, check_grid(n), dim3(256), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, h->bp, n, do_pos, do_halo, 0, t.rep);
      KID_HIP(h, hipGetLastError());
    }
    long long m = 0;
    if (what & (KID_CHECK_ORDER | KID_CHECK_DUPLICATES | KID_CHECK_IDS)) { const int rc = check_select(h, t, &m); if (rc) return rc; }
    const long long *ids = nullptr; const int *id_rows = nullptr;
    if ((what & KID_CHECK_IDS) && m > 0) {   // first: it leaves t.rows[0] as it found it and the key passes below take both buffers
      { const int rc = check_sort_ids(h, t, m, &ids, &id_rows); if (rc) return rc; }
      hipLaunchKernelGGL(check_dup_ids_kernel, check_grid(m), dim3(256), 0, h->stream, ids, id_rows, m, 0, t.rep);
      KID_HIP(h, hipGetLastError());
      // (the row of the smallest duplicated id is looked up now, while the sorted ids are there: a launch that finds nothing without one)
      hipLaunchKernelGGL(check_dup_ids_kernel, check_grid(m), dim3(256), 0, h->stream, ids, id_rows, m, 1, t.rep);
      KID_HIP(h, hipGetLastError());
    }
    if ((what & (KID_CHECK_ORDER | KID_CHECK_DUPLICATES)) && m > 0) {
      const size_t sm = (size_t)m;
      const int ncomp = (d.iec - d.isc + 1) * (d.jec - d.jsc + 1);
      unsigned *k32[2] = {(unsigned *)t.k64[0], (unsigned *)t.k64[1]};
      size_t b64 = 0, b32 = 0, bsc = 0;
      KID_HIP(h, h->mem.dev(t.head, sm));
      KID_HIP(h, h->mem.dev(t.hp, sm));
      KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b64, t.k64[0], t.k64[1], t.rows[0], t.rows[1], sm, 0, 64, h->stream));
      KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b32, k32[0], k32[1], t.rows[0], t.rows[1], sm, 0, 32, h->stream));
      KID_HIP(h, rocprim::inclusive_scan(nullptr, bsc, t.head, t.hp, sm, rocprim::maximum<int>(), h->stream));
      KID_HIP(h, h->mem.reserve(t.tmp, std::max(std::max(b64, b32), bsc)));
      int cur = 0;
      const int f64_keys[4] = {KID_B_START_LAT, KID_B_START_LON, KID_B_START_MASS, KID_B_START_DAY};
      for (int pass = 0; pass < 5; ++pass) {
        if (pass < 4) hipLaunchKernelGGL(check_key_f64_kernel, check_grid(m), dim3(256), 0, h->stream, (const double *)h->bp.f[f64_keys[pass]], (const int *)t.rows[cur], t.k64[0], m);
        else hipLaunchKernelGGL(mts_key_i32_kernel, check_grid(m), dim3(256), 0, h->stream, (const int32_t *)h->bp.i[KID_BI_START_YEAR], (const int *)t.rows[cur], t.k64[0], m);
        size_t bytes = t.tmp.bytes;
        KID_HIP(h, rocprim::radix_sort_pairs(t.tmp.p, bytes, t.k64[0], t.k64[1], t.rows[cur], t.rows[cur ^ 1], sm, 0, 64, h->stream));
        cur ^= 1;
      }
      if (what & KID_CHECK_DUPLICATES) {
        hipLaunchKernelGGL(check_heads_kernel, check_grid(m), dim3(256), 0, h->stream, h->bp, (const int *)t.rows[cur], m, 0, t.head, (unsigned long long *)nullptr);
        size_t bytes = t.tmp.bytes;
        KID_HIP(h, rocprim::inclusive_scan(t.tmp.p, bytes, t.head, t.hp, sm, rocprim::maximum<int>(), h->stream));
        hipLaunchKernelGGL(check_pairs_kernel, check_grid(m), dim3(256), 0, h->stream, h->bp, (const int *)t.rows[cur], (const int *)t.hp, m, (int)(h->params.mts != 0), 0, t.rep);
        hipLaunchKernelGGL(check_pairs_kernel, check_grid(m), dim3(256), 0, h->stream, h->bp, (const int *)t.rows[cur], (const int *)t.hp, m, (int)(h->params.mts != 0), 1, t.rep);
        KID_HIP(h, hipGetLastError());
      }
      if (what & KID_CHECK_ORDER) {   // one more stable pass: (cell, keys)
        hipLaunchKernelGGL(chkd_key_cell_kernel, check_grid(m), dim3(256), 0, h->stream, (const int32_t *)h->bp.i[KID_BI_ALIVE], (const int32_t *)h->bp.i[KID_BI_INE], (const int32_t *)h->bp.i[KID_BI_JNE],
                           (const int *)t.rows[cur], k32[0], m, d.isc, d.iec, d.jsc, d.jec, (unsigned)ncomp);
        const unsigned bits = 32u - (unsigned)__builtin_clz((unsigned)ncomp);
        size_t bytes = t.tmp.bytes;
        KID_HIP(h, rocprim::radix_sort_pairs(t.tmp.p, bytes, k32[0], k32[1], t.rows[cur], t.rows[cur ^ 1], sm, 0, bits, h->stream));
        cur ^= 1;
        hipLaunchKernelGGL(check_heads_kernel, check_grid(m), dim3(256), 0, h->stream, h->bp, (const int *)t.rows[cur], m, 1, (int *)nullptr, &t.rep->count[CK_IDENTICAL]);
        KID_HIP(h, hipGetLastError());
      }
    }
    KID_HIP(h, hipMemcpyAsync(&r, t.rep, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipStreamSynchronize(h->stream));
    if (do_pos && (r.count[CK_XIYJ] || r.count[CK_LAND])) {   // the rows of the smallest offending ids
      hipLaunchKernelGGL(check_position_kernel, check_grid(n), dim3(256), 0, h->stream, dev_grid(h), (const kid_params *)h->d_params, h->bp, n, do_pos, 0, 1, t.rep);
      KID_HIP(h, hipGetLastError());
      KID_HIP(h, hipMemcpyAsync(&r, t.rep, sizeof(r), hipMemcpyDeviceToHost, h->stream));
      KID_HIP(h, hipStreamSynchronize(h->stream));
    }
  }
  *rep = kid_check_report{};
  rep->n_rows = (int64_t)r.count[CK_ROWS]; rep->n_xiyj = (int64_t)r.count[CK_XIYJ]; rep->n_land = (int64_t)r.count[CK_LAND];
  rep->n_in_halo = (int64_t)r.count[CK_IN_HALO]; rep->n_identical = (int64_t)r.count[CK_IDENTICAL]; rep->n_same_id = (int64_t)r.count[CK_SAME_ID];
  rep->n_same_berg = (int64_t)r.count[CK_SAME_BERG]; rep->n_dup_ids = (int64_t)r.count[CK_DUP_IDS];
  std::memcpy(&rep->max_dxi, &r.max_bits[0], sizeof(double));
  std::memcpy(&rep->max_dyj, &r.max_bits[1], sizeof(double));
  for (int q = 0; q < CK_NFIRST; ++q) {
    const bool any = r.first_id[q] != CK_NONE && r.first_row[q] != CK_NONE;
    rep->first_id[q] = any ? (int64_t)r.first_id[q] : -1;
    rep->first_row[q] = any ? (int64_t)r.first_row[q] : -1;
  }
  return KID_OK;
}

}  // namespace

extern "C" int kid_check_bergs(kid_handle *h, uint32_t what, kid_check_report *rep) {
  if (!h) return KID_EINVAL;
  if (!rep) { h->err = "kid_check_bergs: rep is NULL"; return KID_EINVAL; }
  if (what == 0 || (what & ~(uint32_t)KID_CHECK_ALL)) { h->err = "kid_check_bergs: what is a non-empty combination of KID_CHECK_POSITION, _ORDER, _DUPLICATES and _IDS"; return KID_EINVAL; }
  if ((what & KID_CHECK_POSITION) && need_static(h)) return KID_EINVAL;
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  CheckTmp t;
  const int rc = check_run(h, t, what, rep);
  const hipError_t e = check_tmp_free(h, t);
  if (rc) return rc;
  KID_HIP(h, e);
  return KID_OK;
}

extern "C" int kid_sorted_ids(kid_handle *h, int64_t *ids, int64_t capacity, int64_t *n) {
  if (!h) return KID_EINVAL;
  if (!n) { h->err = "kid_sorted_ids: n is NULL"; return KID_EINVAL; }
  if (ids && capacity < 0) { h->err = "kid_sorted_ids: capacity is negative"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_READ); if (rc) return rc; }
  CheckTmp t;
  long long m = 0;
  int rc = check_select(h, t, &m);
  *n = (int64_t)m;
  if (!rc && ids && m > capacity) { h->err = "kid_sorted_ids: " + std::to_string(m) + " ids, capacity " + std::to_string(capacity); rc = KID_ECAPACITY; }
  hipError_t e = hipSuccess;
  if (!rc && ids && m > 0) {
    const long long *d_ids = nullptr; const int *d_rows = nullptr;
    rc = check_sort_ids(h, t, m, &d_ids, &d_rows);
    if (!rc) e = hipMemcpyAsync(ids, d_ids, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream);
    if (!rc && e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  const hipError_t e2 = check_tmp_free(h, t);
  if (rc) return rc;
  KID_HIP(h, e);
  KID_HIP(h, e2);
  return KID_OK;
}
