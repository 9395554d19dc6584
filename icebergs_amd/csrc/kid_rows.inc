// kid_rows.inc -- the rows of the berg SoA: which are occupied, how many, and everything that moves, drops or appends them.
//   kernels      : counts, layout flags, the counting sort by cell, the permutation of every field in one launch
//   row events   : rows_replaced / rows_moved / rows_truncated / rows_appended / rows_killed -- the ONLY places that assign h->n,
//                  tail_valid, static_rows_n, rp.srows_n and uploaded_nonzero (DESIGN.md has the event x cache table); the two
//                  caches of a traversal order are filled by their owners (mts_build_order, repro_static_order) and rebin_plan
//                  carries rp.srows_n through translate_rows_kernel
//   rows_enter   : the prologue of an entry point that reads or changes rows
//   permutation  : compaction and re-binning are both "build a permutation, gather every moving field into the second set of
//                  arrays in one launch, swap" (perm_fields, rebin_apply, rebin_swap); with kid_set_bonds_follow_rows the bond
//                  tables go through the same permutation into a second set of tables (bonds_move, permute_bonds_kernel)
// Textual unit of kid_hip.hip, included once.  The HIP-free decisions (skip rule, wire record) are kid_rows_plan.hpp.
namespace {
// one reservation per wave on *cursor: the lanes with `mine` get consecutive slots in lane order (all are counted, whether or
// not the caller's buffer takes them); -1 for the others.  The pack kernels of kid_migrate.inc and kid_halo_bergs.inc.
__device__ __forceinline__ long long wave_reserve(bool mine, unsigned long long *cursor) {
  const unsigned long long m = __ballot(mine);
  if (!m) return -1;
  const int lane = (int)__lane_id();
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
  base = __shfl(base, 0);
  return mine ? (long long)base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}
__global__ void __launch_bounds__(256) count_alive_kernel(const int32_t *alive, long long n, unsigned long long *out) {
  __shared__ unsigned wsum[4];
  unsigned local = 0;
  for (long long k = (long long)blockIdx.x * 256ll + threadIdx.x; k < n; k += (long long)gridDim.x * 256ll) local += alive[k] ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) local += __shfl_xor(local, d);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)(wsum[0] + wsum[1] + wsum[2] + wsum[3]));
}
// compaction as a permutation: destination row pos[k] takes kept row k (pos: exclusive scan of the flags, so the order is kept)
__global__ void __launch_bounds__(256) compact_perm_kernel(const int32_t *keep, const unsigned *pos, unsigned *perm, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n && keep[k]) perm[pos[k]] = (unsigned)k;
}
// Rows that must survive a dead-tail drop, a compaction or a re-binning.  In a domain-decomposed run (kid_migrate.inc) a berg
// that left the tile is a DEAD row whose cell lies outside the computational domain until kid_pack_emigrants has collected
// it (evolve -> move_berg_between_cells -> send_bergs_to_other_pes is the reference's own order, IB:5433-5447); it counts as
// occupied here, keeps its cell as sort key and is never stepped (alive = 0).  Once packed, its cell is moved inside.
struct KeepSel { int isc, iec, jsc, jec; const double *halo; };
__global__ void __launch_bounds__(256) keep_flags_kernel(const int32_t *alive, const int32_t *ine, const int32_t *jne, const KeepSel s, int32_t *keep, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const int i = ine[k], j = jne[k];
  const bool waiting = (i < s.isc || i > s.iec || j < s.jsc || j > s.jec) && !(s.halo && s.halo[k] >= 0.5);   // the selection of FW:3027-3035, 3101-3109
  keep[k] = (alive[k] != 0 || waiting) ? 1 : 0;
}
__global__ void __launch_bounds__(256) alive_to_u32_kernel(const int32_t *alive, unsigned *flag, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) flag[k] = alive[k] ? 1u : 0u;
}
// cell key of every berg (dead bergs sort to the end) + identity permutation, for kid_move_berg_between_cells
__global__ void __launch_bounds__(256) cell_key_kernel(const int32_t *ine, const int32_t *jne, const int32_t *alive, int isd, int jsd, int ni,
                                                       unsigned dead_key, unsigned *key, unsigned *idx, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) {
    key[k] = alive[k] ? (unsigned)((ine[k] - isd) + (jne[k] - jsd) * ni) : dead_key;
    idx[k] = (unsigned)k;
  }
}
// Counting sort by cell for kid_move_berg_between_cells: (1) key + rank of every berg within its cell (one atomic per
// distinct cell of a wave on the cell's counter), (2) exclusive scan of the counters, (3) destination row = cell start + rank.  Three small
// launches instead of the ~20 of a comparison sort of 1e6 pairs; the order of the bergs inside a cell is the order the
// atomics arrive in (results never depend on the row order, see kid.h).
__global__ void __launch_bounds__(256) cell_rank_kernel(const int32_t *ine, const int32_t *jne, const int32_t *alive, int isd, int jsd, int ni,
                                                        unsigned dead_key, unsigned *key, unsigned *rank, unsigned *hist, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const bool in = k < n;
  const unsigned c = in ? (alive[k] ? (unsigned)((ine[k] - isd) + (jne[k] - jsd) * ni) : dead_key) : 0xffffffffu;
  // the SoA is almost sorted: the lanes of a wave hold a few distinct cells.  One atomic per distinct cell (its first lane adds
  // the number of lanes that share it), not one per berg -- ~14 lanes would otherwise queue on the same address -- and not one
  // per run of adjacent lanes either: as the order decays between two re-binnings an out-of-place berg is a run of its own and
  // splits the run it sits in (7.9 runs against 2.6 cells fifteen steps after a re-binning).  The walk of the hot build
  // (kid_berg_kernel.hpp): first lane not yet served, its cell by v_readlane, a ballot of the lanes that share it.  The atomics
  // are issued after the walk, all at once: one round trip per wave, not one per cell.
  const int lane = (int)__lane_id();
  unsigned long long rem = __ballot(in);
  int leader = lane;
  unsigned cnt = 0u, place = 0u;
  while (rem != 0ull) {  // wave-uniform: one turn per distinct cell
    const int u = (int)__ffsll((long long)rem) - 1;
    const unsigned cu = (unsigned)__builtin_amdgcn_readlane((int)c, u);
    const bool mine = in && c == cu;
    const unsigned long long bm = __ballot(mine);
    if (mine) { leader = u; cnt = (unsigned)__popcll(bm); place = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, 0u)); }
    rem &= ~bm;
  }
  unsigned base = 0u;
  if (in && lane == leader) base = atomicAdd(hist + c, cnt);
  base = __shfl(base, leader);
  if (in) { key[k] = c; rank[k] = base + place; }
}
// the identity of `origin` (cold fields, kid_rows_plan.hpp)
__global__ void __launch_bounds__(256) iota_i32_kernel(int32_t *p, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) p[k] = (int32_t)k;
}
__global__ void __launch_bounds__(256) cell_place_kernel(const unsigned *key, const unsigned *rank, const unsigned *start, unsigned *perm, unsigned *inv, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) { const unsigned pos = start[key[k]] + rank[k]; perm[pos] = (unsigned)k; inv[k] = pos; }
}
// a list of row numbers through the re-binning (slow-lane schedule: the bergs handed over by the hot build just before it)
__global__ void __launch_bounds__(256) translate_list_kernel(int *list, const int *count, const unsigned *inv) {
  const int total = *count;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) list[t] = (int)inv[list[t]];
}
// the canonical order of reproducible sums (kid_repro.inc) through the re-binning: it orders bergs, so only its row numbers change
__global__ void __launch_bounds__(256) translate_rows_kernel(int *rows, const unsigned *inv, long long n) {
  const long long q = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (q < n) rows[q] = (int)inv[rows[q]];
}
// every field of the SoA through the permutation in ONE launch: a thread owns a destination row, reads the source row
// number once and walks the fields (the loads of consecutive fields are independent).  PermTable: kid_handle.hpp.
__global__ void __launch_bounds__(256) permute_all_kernel(const PermTable t, const unsigned *perm, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const unsigned p = perm[k];
  int f = 0;
  for (; f + 4 <= t.n8; f += 4) {
    const double a = ((const double *)t.src[f])[p], b = ((const double *)t.src[f + 1])[p], c = ((const double *)t.src[f + 2])[p], d = ((const double *)t.src[f + 3])[p];
    ((double *)t.dst[f])[k] = a; ((double *)t.dst[f + 1])[k] = b; ((double *)t.dst[f + 2])[k] = c; ((double *)t.dst[f + 3])[k] = d;
  }
  for (; f < t.n8; ++f) ((double *)t.dst[f])[k] = ((const double *)t.src[f])[p];
  for (; f < t.n8 + t.n4; ++f) ((int32_t *)t.dst[f])[k] = ((const int32_t *)t.src[f])[p];
}
// the inverse of a permutation that has none yet (KID_STABLE_RESORT: the comparison sort leaves only perm)
__global__ void __launch_bounds__(256) invert_perm_kernel(const unsigned *perm, unsigned *inv, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) inv[perm[k]] = (unsigned)k;
}
// The bond tables through the permutation (kid_set_bonds_follow_rows): a thread owns destination row k < n_dst, reads its source
// row p = perm[k] once and walks the list of p in list order, slot by slot; every store of a slot is to MB_S(s, k), so the
// lanes of a wave store side by side in each of the sixteen planes, and the loads are the gather.  Partner references go
// through kid::bond_ref_moved (kid_rows_plan.hpp) with keep / alive / inv, all indexed by source row (n_src of them).  Slots past
// the list's end, the rows of a source that is not kept (the tail a re-binning leaves to be cut off) and the rows [n_dst, rows)
// get the values the tables are born with: whatever is appended there later starts with no bonds.  src and dst share the stride.
__global__ void __launch_bounds__(256) permute_bonds_kernel(const BondTables src, const BondTables dst, long long stride, int mb, const unsigned *perm,
                                                            long long n_src, long long n_dst, long long rows, const int32_t *keep, const int32_t *alive, const unsigned *inv) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= rows) return;
  long long p = 0;
  int cnt = kid::BOND_FILL_COUNT;
  if (k < n_dst) {
    p = (long long)perm[k];
    if (keep[p] != 0) cnt = min(max(src.bcount[p], 0), mb);
  }
  dst.bcount[k] = cnt;
  for (int s = 0; s < mb; ++s) {
    const size_t to = (size_t)s * (size_t)stride + (size_t)k;
    if (s < cnt) {
      const size_t from = (size_t)s * (size_t)stride + (size_t)p;
      const int32_t o = src.bother_row[from];
      const bool there = o >= 0 && (long long)o < n_src && keep[o] != 0;
      const kid::BondRef r = kid::bond_ref_moved(o, src.bother_slot[from], there && alive[o] != 0, there ? (int32_t)inv[o] : -1);
      double v[KID_NBOND_F64];
#pragma unroll
      for (int f = 0; f < KID_NBOND_F64; ++f) v[f] = src.bf[f][from];
      dst.bother_id[to] = src.bother_id[from]; dst.bbroken[to] = src.bbroken[from];
      dst.bother_row[to] = r.row; dst.bother_slot[to] = r.slot;
#pragma unroll
      for (int f = 0; f < KID_NBOND_F64; ++f) dst.bf[f][to] = v[f];
    } else {
      dst.bother_id[to] = (int64_t)kid::BOND_FILL_ID; dst.bbroken[to] = kid::BOND_FILL_BROKEN;
      dst.bother_row[to] = kid::BOND_FILL_REF; dst.bother_slot[to] = kid::BOND_FILL_REF;
#pragma unroll
      for (int f = 0; f < KID_NBOND_F64; ++f) dst.bf[f][to] = kid::BOND_FILL_F64;
    }
  }
}
__global__ void __launch_bounds__(256) fill_i32_kernel(int32_t *p, int32_t v, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k < n) p[k] = v;
}
}  // namespace
// resident halo rows (kid_halo_bergs.inc): the two-array form of count_rows
__global__ void __launch_bounds__(256) halo_berg_count_kernel(const int32_t *alive, const double *halo, long long n, unsigned long long *count) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  const unsigned long long m = __ballot(k < n && alive[k] != 0 && halo[k] >= 0.5);
  if (m && __lane_id() == 0) atomicAdd(count, (unsigned long long)__popcll(m));
}

extern "C" {

// -------------------------------------------------------------------------------------------------------
// row events: what each does to the state that depends on rows (DESIGN.md, "Row events")
// -------------------------------------------------------------------------------------------------------
// the cached traversal orders (mts_build_order, repro_static_order) hold row numbers of a population that is gone
static void rows_orders_stale(kid_handle *h) { h->static_rows_n = -1; h->rp.srows_n = -1; }
// kid_upload_bergs: `host` is the new population, already copied.  Which optional per-berg fields can matter at all (avoids
// streaming all-zero arrays through the kernels and the permutation)
static void rows_replaced(kid_handle *h, const kid_berg_soa *host) {
  const size_t n = (size_t)host->n;
  bool any_static = false, any_fl = false;
  for (int f = 0; f < KID_NB_F64; ++f) {
    bool nz = false;
    // (-0. counts as something else than zeros: a build that skips the field would leave it where another stores +0.)
    if (host->f64[f]) for (size_t k = 0; k < n && !nz; ++k) nz = host->f64[f][k] != 0. || std::signbit(host->f64[f][k]);
    h->zs.uploaded(f, nz);
    any_static = any_static || (nz && marks_has_static(f)); any_fl = any_fl || (nz && marks_has_fl(f));
  }
  h->flags.has_static = any_static ? 1 : 0;
  h->flags.has_fl = (any_fl || h->params.footloose) ? 1 : 0;
  rows_orders_stale(h);
  h->tail_valid = false; h->env_ever_stored = false; h->halo_rows_live = false;
  h->n = host->n;
}
// compaction, re-binning: rows changed places (the pointer tables follow in rebin_swap)
// dead_last: the move sorted the dead rows to the tail and nothing is launched on the rows before the host can ask for the count
static void rows_moved(kid_handle *h, bool dead_last) { rows_orders_stale(h); h->tail_valid = dead_last; }
// dead-tail drop, compaction: the population is rows [0, n) of what it was; no dead tail is left to drop
static void rows_truncated(kid_handle *h, int64_t n) { rows_orders_stale(h); h->tail_valid = false; h->n = n; }
// a per-berg launch or a pack call may have killed rows anywhere: the dead are no longer exactly the tail
static void rows_killed(kid_handle *h) { h->tail_valid = false; }
// kid_locate_bergs: every live row has a new cell and new xi, yj (whatever was uploaded there), the rows no cell took are dead
static void rows_located(kid_handle *h) {
  rows_orders_stale(h);
  rows_killed(h);
  h->zs.uploaded_nonzero[KID_B_XI] = true; h->zs.uploaded_nonzero[KID_B_YJ] = true;
}
// calving, footloose calving, immigrants: rows [n, n + m) were written.  records: the m wire records they were decoded from
// (kid_rows_plan.hpp), or NULL for rows a kernel wrote -- those may hold anything in any field.  The kernels bound their own
// writes by the capacity and count on: more rows than room leaves the handle full and is KID_ECAPACITY with `full` as message.
static int rows_appended(kid_handle *h, int64_t m, const double *records, const char *full) {
  if (m <= 0) return KID_OK;
  rows_orders_stale(h);
  h->tail_valid = false;   // live rows now stand behind whatever dead tail a re-binning left
  if (!h->params.old_interp_flds_order) h->env_ever_stored = true;   // new rows carry an interpolated environment
  if (!records) h->zs.appended_by_kernel();
  else {
    for (int64_t q = 0; q < m; ++q)
      for (int w = 0; w < MIG_WIDTH; ++w) {
        const double word = records[(size_t)q * MIG_WIDTH + w];
        if (WIRE_RECORD[w].kind != WIRE_F64 || (word == 0. && !std::signbit(word))) continue;
        const int f = WIRE_RECORD[w].field;
        h->zs.appended_word(f);
        if (marks_has_static(f)) h->flags.has_static = 1;
        if (marks_has_fl(f)) h->flags.has_fl = 1;
      }
    // the decode resets the *_old members to the current ones (FW:3573-3577)
    h->zs.uploaded_nonzero[KID_B_UVEL_OLD] |= h->zs.uploaded_nonzero[KID_B_UVEL]; h->zs.uploaded_nonzero[KID_B_VVEL_OLD] |= h->zs.uploaded_nonzero[KID_B_VVEL];
    h->zs.uploaded_nonzero[KID_B_LON_OLD] |= h->zs.uploaded_nonzero[KID_B_LON]; h->zs.uploaded_nonzero[KID_B_LAT_OLD] |= h->zs.uploaded_nonzero[KID_B_LAT];
  }
  if (m > h->capacity - h->n) {
    h->err = full;
    // auto-reserve made min_free rows of room before the launch and the launch wanted more: say how many
    if (h->auto_growth != 0.) h->err += " (the launch tried to append " + std::to_string(m) + " rows, " + std::to_string(h->capacity - h->n) + " were free: raise min_free of kid_set_auto_reserve)";
    h->n = h->capacity;
    return KID_ECAPACITY;
  }
  h->n += m;
  return KID_OK;
}

// The prologue of an entry point that looks at rows: on the handle's device, behind whatever the side stream still runs, with
// no re-binning pending.  ROWS_CHANGE also leaves the slow-lane schedule (its lists hold row numbers; new rows start in the hot lane).
// Cold fields (kid_rows_plan.hpp) are put in row order too, unless the caller says it touches none of them and keeps the rows
// that exist (COLD_LEAVE: kid_move_berg_between_cells, kid_num_bergs -- which materialises itself before it drops a tail).
enum RowsMode { ROWS_READ, ROWS_CHANGE };
enum RowsCold { COLD_READ, COLD_LEAVE };
static int rows_enter(kid_handle *h, RowsMode mode, RowsCold cold = COLD_READ) {
  KID_HIP(h, hipSetDevice(h->device));
  const int rc = mode == ROWS_CHANGE ? lanes_drain(h) : join_side(h);
  if (rc) return rc;
  return cold == COLD_LEAVE ? rebin_flush_rows(h) : rebin_flush(h);
}
// rows k < h->n with flags[k] != 0 -- and, with `halo`, halo[k] >= 0.5 too: one launch, one host read
static int count_rows(kid_handle *h, const int32_t *flags, const double *halo, int64_t *count) {
  unsigned long long cnt = 0;
  *count = 0;
  if (h->n == 0) return KID_OK;
  const long long n = h->n;
  KID_HIP(h, hipMemsetAsync(h->d_count, 0, sizeof(cnt), h->stream));
  if (halo) hipLaunchKernelGGL(halo_berg_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, flags, halo, n, h->d_count);
  else hipLaunchKernelGGL(count_alive_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, h->stream, flags, n, h->d_count);
  KID_HIP(h, hipGetLastError());
  KID_HIP(h, hipMemcpyAsync(&cnt, h->d_count, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
  KID_HIP(h, hipStreamSynchronize(h->stream));
  *count = (int64_t)cnt;
  return KID_OK;
}

// which rows are occupied, for tail drops, compaction and re-binning: `alive`, plus (decomposed runs) the rows still waiting
// to be packed for a neighbour
static int layout_flags(kid_handle *h, const int32_t **flags) {
  *flags = h->bp.i[KID_BI_ALIVE];
  if (!h->mig_mode || h->n == 0) return KID_OK;
  if (!h->d_keep) KID_HIP(h, h->mem.dev(h->d_keep, (size_t)h->capacity));
  const KeepSel ks{h->gd.isc, h->gd.iec, h->gd.jsc, h->gd.jec, h->flags.has_static ? h->bp.f[KID_B_HALO_BERG] : nullptr};
  hipLaunchKernelGGL(keep_flags_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->bp.i[KID_BI_ALIVE], h->bp.i[KID_BI_INE], h->bp.i[KID_BI_JNE], ks, h->d_keep, (long long)h->n);
  KID_HIP(h, hipGetLastError());
  *flags = h->d_keep;
  return KID_OK;
}

int kid_num_bergs(kid_handle *h, int64_t *n_slots, int64_t *n_alive) {
  if (!h) return KID_EINVAL;
  { const int rc = rows_enter(h, ROWS_READ, COLD_LEAVE); if (rc) return rc; }   // (counting looks at `alive` only)
  if (n_slots) *n_slots = h->n;
  if (n_alive) {
    int64_t cnt = 0;
    { const int rc = count_rows(h, h->bp.i[KID_BI_ALIVE], nullptr, &cnt); if (rc) return rc; }
    *n_alive = cnt;
    if (h->tail_valid && h->mig_mode && cnt < h->n) {   // decomposed run: the tail is what is neither alive nor waiting to be packed
      const int32_t *flags = nullptr;
      { const int rc = layout_flags(h, &flags); if (rc) return rc; }
      { const int rc = count_rows(h, flags, nullptr, &cnt); if (rc) return rc; }
    }
    if (h->tail_valid && cnt < h->n) {  // a re-binning left the dead at the tail: drop them now that the count is known
      { const int rc = cold_materialise(h); if (rc) return rc; }   // the rows that exist change
      rows_truncated(h, cnt);
      if (n_slots) *n_slots = h->n;
    }
  }
  return KID_OK;
}

// The skip rule of a row permutation (kid_rows_plan.hpp) on this handle's switches and flags
static bool field_never_written(const kid_handle *h, int f) {
  const kid_params &p = h->params;
  // (the interacting evolve of the single-time-step scheme writes the *_old members and the rotation like the MTS path: same answer)
  return kid::field_never_written(NeverWrittenIn{p.footloose != 0, p.mts != 0 || p.interactive_icebergs_on != 0, h->calving_on, p.periodic_reentry != 0, p.Runge_not_Verlet != 0,
                                                 h->flags.has_fl != 0, h->env_ever_stored}, f);
}
// The fp64 fields a launch enqueued now -- or a row permutation planned now -- may treat as zeros in every row, a bit per field
// (kid_rows_plan.hpp).  KID_NO_ZERO_SKIP: none
static unsigned long long known_zero_mask(const kid_handle *h) {
  if (h->dbg.no_zero_skip) return 0ull;
  return kid::known_zero_mask(h->zs, field_never_written(h, KID_B_HEAT_DENSITY), h->params.Runge_not_Verlet != 0, h->params.bergy_bit_erosion_fraction == 0.);
}
// The cold set of this handle now (kid_rows_plan.hpp).  KID_COLD_EAGER: empty
static bool rebin_fusable(const kid_handle *h);
static kid::ColdSet cold_set(const kid_handle *h) {
  const kid_params &p = h->params;
  if (h->dbg.cold_eager) return kid::ColdSet{};
  return kid::cold_set(kid::ColdIn{rebin_fusable(h), p.Runge_not_Verlet != 0, p.periodic_reentry != 0, h->flags.has_static != 0, h->flags.has_fl != 0,
                                   p.iceberg_bonds_on != 0, (p.diag_mask & KID_DIAG_MELT_BY_CLASS) != 0});
}
// only the field pointers changed: one table, not four (a launch on the side stream may still be reading it)
static int berg_table_follows(kid_handle *h) {
  if (h->tables_dirty) return refresh_tables(h);
  { const int rc = join_side(h); if (rc) return rc; }
  hipLaunchKernelGGL(set_berg_table_kernel, dim3(1), dim3(64), 0, h->stream, h->bp, h->d_bp);
  KID_HIP(h, hipGetLastError());
  return KID_OK;
}
// Put the deferred cold fields in row order: ONE launch gathers them through `origin` into the second set of arrays, which
// become the SoA's.  `origin` is filled with the identity again by the next permutation that defers.  Nothing deferred: a compare.
static int cold_materialise(kid_handle *h) {
  if (!h->cold.deferred) return KID_OK;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc = rebin_flush_rows(h); if (rc) return rc; }   // (a pending copy composes `origin` once more)
  h->cold.deferred = false;
  const kid::ColdSet cs = h->cold.set;
  h->cold.set = kid::ColdSet{};
  h->cold.materialised++;
  PermTable t{};
  for (int f = 0; f < KID_NB_F64; ++f) if ((cs.f64 >> f) & 1ull) { t.src[t.n8] = h->bp.f[f]; t.dst[t.n8] = h->bp_alt.f[f]; ++t.n8; std::swap(h->bp.f[f], h->bp_alt.f[f]); }
  if (cs.id) { t.src[t.n8] = h->bp.id; t.dst[t.n8] = h->bp_alt.id; ++t.n8; std::swap(h->bp.id, h->bp_alt.id); }
  for (int f = 0; f < KID_NB_I32; ++f) if ((cs.i32 >> f) & 1u) { t.src[t.n8 + t.n4] = h->bp.i[f]; t.dst[t.n8 + t.n4] = h->bp_alt.i[f]; ++t.n4; std::swap(h->bp.i[f], h->bp_alt.i[f]); }
  const long long n = h->n;
  if (n > 0) hipLaunchKernelGGL(permute_all_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, t, (const unsigned *)h->cold.origin, n);
  KID_HIP(h, hipGetLastError());
  return berg_table_follows(h);
}
// Do the deferred fields still lie outside everything a step of this handle touches?  Asked wherever the answer can change
// (kid_set_params, kid_set_store_environment, the head of a step, a new re-binning) and by launch_phase for the launch it is about to make
static bool cold_holds(const kid_handle *h) { return !h->cold.deferred || h->cold.set.within(cold_set(h)); }
static int cold_settle(kid_handle *h) {
  if (cold_holds(h)) return KID_OK;
  const int rc = rebin_flush_rows(h);   // (the pending copy was planned with the deferred set)
  return rc ? rc : cold_materialise(h);
}
// The second set of field arrays and the sort / scan storage of a row permutation, at the first compaction or re-binning
static int perm_storage(kid_handle *h) {
  if (h->d_key[0]) return KID_OK;
  h->stable_resort = h->dbg.stable_resort;  // a stable comparison sort keeps the row order inside a cell
  for (unsigned **q : {&h->d_key[0], &h->d_key[1], &h->d_idx[0], &h->d_idx[1]}) KID_HIP(h, h->mem.dev(*q, (size_t)h->capacity));
  size_t tmp = 0;
  KID_HIP(h, rocprim::radix_sort_pairs(nullptr, tmp, h->d_key[0], h->d_key[1], h->d_idx[0], h->d_idx[1], (size_t)h->capacity, 0u, 32u, h->stream));
  KID_HIP(h, h->mem.reserve(h->sort_tmp, tmp));
  KID_HIP(h, h->mem.dev(h->d_cell_hist, (size_t)h->ncell + 1));
  tmp = 0;
  KID_HIP(h, rocprim::exclusive_scan(nullptr, tmp, h->d_cell_hist, h->d_cell_hist, 0u, (size_t)h->ncell + 1, rocprim::plus<unsigned>(), h->stream));
  KID_HIP(h, h->mem.reserve(h->cscan_tmp, tmp));
  tmp = 0;   // compaction: the scan of the row flags
  KID_HIP(h, rocprim::exclusive_scan(nullptr, tmp, h->d_key[0], h->d_key[1], 0u, (size_t)h->capacity, rocprim::plus<unsigned>(), h->stream));
  KID_HIP(h, h->mem.reserve(h->scan_tmp, tmp));
  for (auto &field : h->bp_alt.f) KID_HIP(h, h->mem.dev(field, (size_t)h->capacity));
  for (auto &field : h->bp_alt.i) KID_HIP(h, h->mem.dev(field, (size_t)h->capacity));
  KID_HIP(h, h->mem.dev(h->bp_alt.id, (size_t)h->capacity));
  for (int32_t **q : {&h->cold.origin, &h->cold.origin_alt}) KID_HIP(h, h->mem.dev(*q, (size_t)h->capacity));   // cold fields: `origin` and its double
  return KID_OK;
}
// The plan of a permutation of n destination rows (perm: the source row of each): the fields that move.  A field that was
// uploaded as zeros and that no kernel of the configuration writes is zeros before and after, and stays where it is.
// A cold field (kid_rows_plan.hpp) stays where it is as well, whatever it holds, and `origin` moves in its place: one 4-byte
// field among the int32 ones.  Fields already deferred stay deferred -- the permutation composes `origin` again and never looks
// at cold data -- and no further field joins them before they are materialised (it would be in row order, they are not).
// defer_cold = false (compaction: it changes which rows exist, its caller has materialised): every field that is not zeros moves.
static int perm_fields(kid_handle *h, const unsigned *perm, long long n, bool defer_cold) {
  kid_handle::RebinPlan &pl = h->rplan;
  pl = kid_handle::RebinPlan{};
  PermTable &t = pl.t;
  kid::ColdSet cold = h->cold.deferred ? h->cold.set : (defer_cold ? cold_set(h) : kid::ColdSet{});
  if (!h->cold.deferred) {
    // all zeros, before and after: such a field neither moves nor is deferred (nothing to gather when the rows are read)
    for (int f = 0; f < KID_NB_F64; ++f) if (!h->zs.uploaded_nonzero[f] && field_never_written(h, f)) cold.f64 &= ~(1ull << f);
  }
  if (!h->cold.deferred && !cold.empty()) {
    hipLaunchKernelGGL(iota_i32_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->cold.origin, (long long)h->n);
    KID_HIP(h, hipGetLastError());
    h->cold.deferred = true; h->cold.set = cold;
  }
  const unsigned long long zeros = known_zero_mask(h);
  for (int f = 0; f < KID_NB_F64; ++f) {
    if (!h->zs.uploaded_nonzero[f] && field_never_written(h, f)) continue;  // all zeros, before and after
    // zeros now, though a later launch may write it (axn, ayn, mass_of_bits): it stays in the array it is in, which is the one
    // every later launch and copy uses.  A fused re-binning launch that no longer knows it as zeros copies first (rebin_take_or_flush)
    if ((zeros >> f) & 1ull) { pl.zero_skipped |= 1ull << f; continue; }
    if ((cold.f64 >> f) & 1ull) continue;
    t.src[t.n8] = h->bp.f[f]; t.dst[t.n8] = h->bp_alt.f[f]; ++t.n8; pl.moved_f[pl.nmf++] = f; pl.moved |= 1ull << f;
  }
  if (!cold.id) { t.src[t.n8] = h->bp.id; t.dst[t.n8] = h->bp_alt.id; ++t.n8; pl.moved_id = true; }
  for (int f = 0; f < KID_NB_I32; ++f) {
    if ((cold.i32 >> f) & 1u) continue;
    t.src[t.n8 + t.n4] = h->bp.i[f]; t.dst[t.n8 + t.n4] = h->bp_alt.i[f]; ++t.n4; pl.moved_i32 |= 1u << f;
  }
  if (h->cold.deferred) { t.src[t.n8 + t.n4] = h->cold.origin; t.dst[t.n8 + t.n4] = h->cold.origin_alt; ++t.n4; pl.origin_moves = true; }
  pl.perm = perm; pl.n = n;
  return KID_OK;
}
static const char *const bonds_keep_rows = "bergs with bonds keep their rows: no re-binning while bond tables exist";
// The bond tables follow a planned permutation (kid_set_bonds_follow_rows), between its plan and rebin_apply: `alive` and `keep`
// are still those of the source rows.  perm: the source row of each of the n_dst destination rows; inv: the new row of every
// kept source row.  The second set of tables is made at the first call (as the primary set is born, at the handle's stride) and
// the two change places afterwards; the device's table follows in mts_refresh, which the callers run once their rows have moved.
// Nothing that is captured or held across steps points into either set: the sub-step graph and the cooperative launch take d_bp
// and d_mts, the tables of pointers.
static int bonds_move(kid_handle *h, const unsigned *perm, long long n_src, long long n_dst, const int32_t *keep, const unsigned *inv) {
  if (!h->have_bonds || !h->mts_ready) return KID_OK;
  MtsDev &m = h->mts;
  BondTables &alt = h->bond_alt;
  const int mb = h->mb > 0 ? h->mb : 1;
  if (!alt.bcount) {
    const size_t cap = (size_t)h->capacity, nb = (size_t)mb * cap;
    KID_HIP(h, h->mem.dev(alt.bcount, cap, 0));
    KID_HIP(h, h->mem.dev(alt.bother_id, nb, 0));
    KID_HIP(h, h->mem.dev(alt.bbroken, nb, 0));
    for (int32_t **q : {&alt.bother_row, &alt.bother_slot}) KID_HIP(h, h->mem.dev(*q, nb, 0xff));
    for (auto &field : alt.bf) KID_HIP(h, h->mem.dev(field, nb, 0));
    h->bond_alt_rows = 0;
  }
  BondTables src;
  src.bcount = m.bcount; src.bother_id = m.bother_id; src.bbroken = m.bbroken; src.bother_row = m.bother_row; src.bother_slot = m.bother_slot;
  for (int f = 0; f < KID_NBOND_F64; ++f) src.bf[f] = m.bf[f];
  const long long rows = std::min<long long>(std::max(n_src, h->bond_alt_rows), h->capacity);
  if (rows > 0) {   // (a compaction may keep no row: the rows that go are still put back to what they were born with)
    hipLaunchKernelGGL(permute_bonds_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, h->stream, (const BondTables)src, (const BondTables)alt, m.stride, mb,
                       perm, n_src, n_dst, rows, keep, (const int32_t *)h->bp.i[KID_BI_ALIVE], inv);
    KID_HIP(h, hipGetLastError());
  }
  m.bcount = alt.bcount; m.bother_id = alt.bother_id; m.bbroken = alt.bbroken; m.bother_row = alt.bother_row; m.bother_slot = alt.bother_slot;
  for (int f = 0; f < KID_NBOND_F64; ++f) m.bf[f] = alt.bf[f];
  alt = src;
  h->bond_alt_rows = n_src;
  h->mts_dirty = true;
  // the bond-derived orientations are by row and are not moved: bond_orientations makes them again before the next spreading
  // of a step; until then there are none, as after kid_upload_bergs
  if (h->bp.orient) { h->bp.orient = nullptr; h->tables_dirty = true; }
  return mts_refresh(h);   // d_mts names the new set before anything else is enqueued (the berg table follows in rebin_swap)
}

// Drop the rows that are not occupied and keep the order of the rest: the permutation "kept row k goes to the number of kept
// rows before it", through the same one-launch gather and swap as a re-binning.  Every int32 field moves, `alive` included
// (in a decomposed run the rows waiting to be packed stay dead).
int kid_compact_bergs(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  if (h->n == 0) return KID_OK;
  if (h->have_bonds && !h->bonds_follow) { h->err = bonds_keep_rows; return KID_EUNSUPPORTED; }   // the bond tables are indexed by row and move only when asked to (kid_set_bonds_follow_rows)
  { const int rc = perm_storage(h); if (rc) return rc; }
  const long long n = h->n;
  const unsigned nb = (unsigned)((n + 255) / 256);
  const int32_t *live = nullptr;   // alive, or alive + waiting to be packed (decomposed runs)
  { const int rc_l = layout_flags(h, &live); if (rc_l) return rc_l; }
  unsigned *flag = h->d_key[0], *pos = h->d_key[1], *perm = h->d_idx[1];
  hipLaunchKernelGGL(alive_to_u32_kernel, dim3(nb), dim3(256), 0, h->stream, live, flag, n);
  size_t tmp = h->scan_tmp.bytes;
  KID_HIP(h, rocprim::exclusive_scan(h->scan_tmp.p, tmp, flag, pos, 0u, (size_t)n, rocprim::plus<unsigned>(), h->stream));
  hipLaunchKernelGGL(compact_perm_kernel, dim3(nb), dim3(256), 0, h->stream, live, (const unsigned *)pos, perm, n);
  KID_HIP(h, hipGetLastError());
  int64_t kept = 0;
  { const int rc = count_rows(h, live, nullptr, &kept); if (rc) return rc; }
  rows_moved(h, false);
  { const int rc = perm_fields(h, perm, kept, false); if (rc) return rc; }
  { const int rc = bonds_move(h, perm, n, kept, live, pos); if (rc) return rc; }   // pos: the new row of every kept row
  { const int rc = rebin_apply(h, false, nullptr, nullptr); if (rc) return rc; }
  rows_truncated(h, kept);
  return KID_OK;
}

// move_berg_between_cells (IB:5437, FW:1758-1797): re-bin the bergs after they moved.  With per-cell linked lists
// that is list surgery; on the SoA it is a device counting sort by cell index (j-major, i-minor: the reference's
// traversal order, IB:7106) followed by ONE launch that gathers every field into a second set of arrays, which then
// becomes the SoA.  Dead bergs sort to the end and are dropped.  The order inside a cell is arbitrary (the bonded /
// MTS path, where it matters, builds its own order every step and never re-bins); KID_STABLE_RESORT=1 in the
// environment selects a stable comparison sort instead.
// Correctness never depends on it (the kernels accept any order); speed does: the hot build shares LDS cell
// packets and atomics between the lanes of a wave that sit in the same cell.
// Is a step of this handle ONE plain hot build over the whole population (kid_step_local's default family -> launch_phase with
// evolve | thermo | spread, kid_launch.inc)?  Only then can the copy of a re-binning wait for the step: asked when the re-binning is planned,
// at the head of kid_step_local and by launch_phase itself.  The slow-lane schedule (it re-bins inside the step, with the
// copy), the two-halves schedule and reproducible sums keep the eager copy; so does a decomposed run, which packs its
// emigrants right after the re-binning.
static bool rebin_fusable(const kid_handle *h) {
  const kid_params &p = h->params;
  // (bond tables move with the copy, never later: a plain namelist with uploaded bonds is possible)
  return !h->dbg.rebin_eager && !h->have_bonds && !h->repro && !h->mig_mode && !h->pipelined && h->forc.have_forcing && p.Runge_not_Verlet && p.old_interp_flds_order &&
         !p.static_icebergs && !p.mts && !p.interactive_icebergs_on && !p.footloose && !p.find_melt_using_spread_mass && !lanes_eligible(h) && plain_namelist(h);
}
int kid_move_berg_between_cells(kid_handle *h) {
  if (!h) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_move_berg_between_cells"); if (rc_h) return rc_h; }
  // (re-binning twice in a row: the second one sorts the rows of the first.)  Cold fields stay deferred: only `origin` is composed again
  { const int rc_e = rows_enter(h, ROWS_CHANGE, COLD_LEAVE); if (rc_e) return rc_e; }
  { const int rc_c = cold_settle(h); if (rc_c) return rc_c; }
  h->steps_since_sort = 0;
  if (h->n == 0) return KID_OK;
  if (h->have_bonds && !h->bonds_follow) { h->err = bonds_keep_rows; return KID_EUNSUPPORTED; }
  // the dead sort to the tail; they are dropped the next time the host asks for the count (no synchronisation here)
  int rc = rebin_plan(h, true);
  if (rc) return rc;
  if (rebin_fusable(h)) h->rebin_pending = true;
  else {
    if (h->have_bonds) {   // (never deferred: rebin_fusable says no)
      const int32_t *live = nullptr;
      rc = layout_flags(h, &live); if (rc) return rc;
      if (h->stable_resort) {   // the comparison sort leaves no inverse; its input values, d_idx[0], are free now
        hipLaunchKernelGGL(invert_perm_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, h->stream, h->rplan.perm, h->d_idx[0], (long long)h->n);
        KID_HIP(h, hipGetLastError());
      }
      rc = bonds_move(h, h->rplan.perm, h->n, h->n, live, h->d_idx[0]); if (rc) return rc;
    }
    rc = rebin_apply(h, false, nullptr, nullptr); if (rc) return rc;
  }
  return KID_OK;
}
// the re-binning inside a step of the slow-lane schedule.  with_lane: the lane array moves with the rows and `list` (row
// numbers, *list_count of them) is translated
static int rebin_core(kid_handle *h, bool with_lane, int *list, const int *list_count) {
  const int rc = rebin_plan(h, false);
  return rc ? rc : rebin_apply(h, with_lane, list, list_count);
}
// plan: the permutation (h->rplan.perm: source row of every destination row; its inverse in d_idx[0]) and the fields that move
// dead_last: the dead rows, sorted to the tail, are still the tail when the host next asks for the count (no launch follows)
static int rebin_plan(kid_handle *h, bool dead_last) {
  const bool carry_repro = h->rp.srows_n == h->n;   // the order of reproducible sums is carried through the move (translate_rows_kernel)
  rows_moved(h, dead_last);
  const long long n = h->n;
  const unsigned nb = (unsigned)((n + 255) / 256);
  const unsigned dead_key = (unsigned)h->ncell;  // larger than any cell index
  { const int rc_s = perm_storage(h); if (rc_s) return rc_s; }
  const int32_t *live = nullptr;   // alive, or alive + waiting to be packed (decomposed runs): those keep their cell as key
  { const int rc_l = layout_flags(h, &live); if (rc_l) return rc_l; }
  const unsigned *perm = nullptr;
  if (h->stable_resort) {
    unsigned bits = 1; while ((1ull << bits) <= (unsigned long long)dead_key) ++bits;
    hipLaunchKernelGGL(cell_key_kernel, dim3(nb), dim3(256), 0, h->stream, h->bp.i[KID_BI_INE], h->bp.i[KID_BI_JNE], live,
                       h->gd.isd, h->gd.jsd, h->ni, dead_key, h->d_key[0], h->d_idx[0], n);
    size_t tmp = h->sort_tmp.bytes;
    KID_HIP(h, rocprim::radix_sort_pairs(h->sort_tmp.p, tmp, h->d_key[0], h->d_key[1], h->d_idx[0], h->d_idx[1], (size_t)n, 0u, bits, h->stream));
    perm = h->d_idx[1];
  } else {
    KID_HIP(h, hipMemsetAsync(h->d_cell_hist, 0, ((size_t)h->ncell + 1) * sizeof(unsigned), h->stream));
    hipLaunchKernelGGL(cell_rank_kernel, dim3(nb), dim3(256), 0, h->stream, h->bp.i[KID_BI_INE], h->bp.i[KID_BI_JNE], live,
                       h->gd.isd, h->gd.jsd, h->ni, dead_key, h->d_key[0], h->d_key[1], h->d_cell_hist, n);
    size_t tmp = h->cscan_tmp.bytes;
    KID_HIP(h, rocprim::exclusive_scan(h->cscan_tmp.p, tmp, h->d_cell_hist, h->d_cell_hist, 0u, (size_t)h->ncell + 1, rocprim::plus<unsigned>(), h->stream));
    hipLaunchKernelGGL(cell_place_kernel, dim3(nb), dim3(256), 0, h->stream, h->d_key[0], h->d_key[1], h->d_cell_hist, h->d_idx[1], h->d_idx[0], n);
    perm = h->d_idx[1];
    if (carry_repro) { hipLaunchKernelGGL(translate_rows_kernel, dim3(nb), dim3(256), 0, h->stream, h->rp.srows, (const unsigned *)h->d_idx[0], n); h->rp.srows_n = n; }
  }
  KID_HIP(h, hipGetLastError());
  return perm_fields(h, perm, n, true);
}
// the planned rows change places on the host: the second set of arrays becomes the SoA; the device's pointer table follows
static int rebin_swap(kid_handle *h) {
  const kid_handle::RebinPlan &pl = h->rplan;
  for (int q = 0; q < pl.nmf; ++q) std::swap(h->bp.f[pl.moved_f[q]], h->bp_alt.f[pl.moved_f[q]]);
  if (pl.moved_id) std::swap(h->bp.id, h->bp_alt.id);
  for (int f = 0; f < KID_NB_I32; ++f) if ((pl.moved_i32 >> f) & 1u) std::swap(h->bp.i[f], h->bp_alt.i[f]);
  if (pl.origin_moves) std::swap(h->cold.origin, h->cold.origin_alt);
  return berg_table_follows(h);
}
// apply: ONE launch gathers every moving field into the second set of arrays
static int rebin_apply(kid_handle *h, bool with_lane, int *list, const int *list_count) {
  PermTable t = h->rplan.t;
  const long long n = h->rplan.n;
  const unsigned nb = (unsigned)((n + 255) / 256);
  if (with_lane) {
    if (h->stable_resort) { h->err = "KID_STABLE_RESORT has no inverse permutation for the slow-lane re-binning"; return KID_EUNSUPPORTED; }
    if (!h->d_lane_alt) KID_HIP(h, h->mem.dev(h->d_lane_alt, (size_t)h->capacity, 0));
    t.src[t.n8 + t.n4] = h->d_lane; t.dst[t.n8 + t.n4] = h->d_lane_alt; ++t.n4;
  }
  if (n > 0) hipLaunchKernelGGL(permute_all_kernel, dim3(nb), dim3(256), 0, h->stream, t, h->rplan.perm, n);   // (a compaction may keep no row)
  if (with_lane) {
    std::swap(h->d_lane, h->d_lane_alt);
    if (list) hipLaunchKernelGGL(translate_list_kernel, dim3(64), dim3(256), 0, h->stream, list, list_count, h->d_idx[0]);
  }
  KID_HIP(h, hipGetLastError());
  return rebin_swap(h);
}
static int rebin_flush_rows(kid_handle *h) {
  if (!h->rebin_pending) return KID_OK;
  h->rebin_pending = false;
  KID_HIP(h, hipSetDevice(h->device));
  return rebin_apply(h, false, nullptr, nullptr);
}
static int rebin_flush(kid_handle *h) {
  const int rc = rebin_flush_rows(h);
  return rc ? rc : cold_materialise(h);
}
// The table of the re-binning instance of the plain hot build K for the pending plan.  The moved fields that build does not
// write itself are head copies (KID_RB_NX8 with the id; the int32 fields always fit); what is left over is `surplus`.
static bool rebin_table(const kid_handle *h, int K, RebinTab &tab) {
  const kid_handle::RebinPlan &pl = h->rplan;
  tab = RebinTab{};
  tab.dst = h->bp;
  for (int q = 0; q < pl.nmf; ++q) tab.dst.f[pl.moved_f[q]] = h->bp_alt.f[pl.moved_f[q]];
  if (pl.moved_id) tab.dst.id = h->bp_alt.id;
  for (int f = 0; f < KID_NB_I32; ++f) if ((pl.moved_i32 >> f) & 1u) tab.dst.i[f] = h->bp_alt.i[f];
  tab.moved = pl.moved;
  const int id_slot = pl.moved_id ? 1 : 0;
  const unsigned long long own = KID_RB_DYN | rb_thermo_fields(K);
  for (int q = 0; q < pl.nmf; ++q) {
    const int f = pl.moved_f[q];
    if ((own >> f) & 1ull) continue;
    if (tab.n8 >= KID_RB_NX8 - id_slot) { tab.surplus |= 1ull << f; continue; }
    tab.xs[tab.n8] = h->bp.f[f]; tab.xd[tab.n8] = h->bp_alt.f[f]; ++tab.n8;
  }
  if (pl.moved_id) { tab.xs[tab.n8] = h->bp.id; tab.xd[tab.n8] = h->bp_alt.id; ++tab.n8; }
  // every moving int32 field but the cell is a head copy, and so is `origin` when cold fields are deferred: the cold int32
  // fields (at least conglom_id) have left the head copies then, so the four slots still hold them
  static_assert(KID_NB_I32 - 2 <= KID_RB_NX4, "every int32 field but the cell is a head copy");
  static_assert((kid::cold_set(kid::ColdIn{true, true, true, true, true, true, true}).i32 & ~(1u << KID_BI_INE | 1u << KID_BI_JNE)) != 0u, "a cold int32 field makes room for origin");
  int n4 = 0;
  for (int f = 0; f < KID_NB_I32; ++f) if (f != KID_BI_INE && f != KID_BI_JNE && ((pl.moved_i32 >> f) & 1u)) ++n4;
  if (n4 + (pl.origin_moves ? 1 : 0) > KID_RB_NX4) return false;   // (the caller copies first)
  for (int f = 0; f < KID_NB_I32; ++f) {
    if (f == KID_BI_INE || f == KID_BI_JNE || !((pl.moved_i32 >> f) & 1u)) continue;
    tab.xs[KID_RB_NX8 + tab.n4] = h->bp.i[f]; tab.xd[KID_RB_NX8 + tab.n4] = h->bp_alt.i[f]; ++tab.n4;
  }
  if (pl.origin_moves) { tab.xs[KID_RB_NX8 + tab.n4] = h->cold.origin; tab.xd[KID_RB_NX8 + tab.n4] = h->cold.origin_alt; ++tab.n4; }
  return true;
}
int kid_set_resort_interval(kid_handle *h, int steps) {
  if (!h || steps < 0) return KID_EINVAL;
  h->resort_interval = steps;
  return KID_OK;
}
// Bond tables follow their rows through kid_compact_bergs and kid_move_berg_between_cells (1) or pin them (0, the default)
int kid_set_bonds_follow_rows(kid_handle *h, int on) {
  if (!h) return KID_EINVAL;
  if (on != 0 && on != 1) { h->err = "kid_set_bonds_follow_rows: on is 0 or 1"; return KID_EINVAL; }
  h->bonds_follow = on == 1;
  return KID_OK;
}
// bother_row and bother_slot as the kernels see them, in the layout of kid_bond_soa ([max_bonds * n], slot-major with stride n);
// -1 past a list's end whatever the device holds there.  A hook for tests, like kid_cold_state.
int kid_bond_partner_rows(kid_handle *h, int32_t *row, int32_t *slot, int64_t n) {
  if (!h || !row || !slot) return KID_EINVAL;
  if (!h->have_bonds || !h->mts_ready) { h->err = "no bonds were uploaded"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_READ, COLD_LEAVE); if (rc) return rc; }
  if (n != h->n) { h->err = "kid_bond_partner_rows: n is not the handle's row count"; return KID_EINVAL; }
  const size_t nn = (size_t)h->n, stride = (size_t)h->mts.stride;
  if (nn == 0) return KID_OK;
  std::vector<int32_t> count(nn);
  KID_HIP(h, hipMemcpyAsync(count.data(), h->mts.bcount, nn * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  for (int s = 0; s < h->mb; ++s) {
    KID_HIP(h, hipMemcpyAsync(row + (size_t)s * nn, h->mts.bother_row + (size_t)s * stride, nn * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    KID_HIP(h, hipMemcpyAsync(slot + (size_t)s * nn, h->mts.bother_slot + (size_t)s * stride, nn * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  for (int s = 0; s < h->mb; ++s)
    for (size_t k = 0; k < nn; ++k)
      if (s >= count[k]) row[(size_t)s * nn + k] = slot[(size_t)s * nn + k] = -1;
  return KID_OK;
}
// fp64 fields the last row permutation (compaction or re-binning) moved; the others were zeros that stayed where they were.
// A hook for tests/test_rows_gpu.py, which must see the skip rule at work; exported, but not part of include/kid.h.
int kid_perm_moved_fields(kid_handle *h, int64_t *count) {
  if (!h || !count) return KID_EINVAL;
  *count = h->rplan.nmf;
  return KID_OK;
}
// Cold fields: are any deferred behind a permutation now, and how many times have they been gathered into row order so far?
// A hook for tests/test_cold_rows_gpu.py like the one above; it looks at the handle only and moves nothing.
int kid_cold_state(kid_handle *h, int32_t *deferred, int64_t *materialised_count) {
  if (!h) return KID_EINVAL;
  if (deferred) *deferred = h->cold.deferred ? 1 : 0;
  if (materialised_count) *materialised_count = h->cold.materialised;
  return KID_OK;
}

}  // extern "C"
