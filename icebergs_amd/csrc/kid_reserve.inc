// kid_reserve.inc -- growing a handle: kid_capacity, kid_reserve, kid_set_auto_reserve, and the growth the entry points that
// append rows ask for before they write (auto_reserve).  The arithmetic and the order in which blocks move are
// kid_reserve_plan.hpp; this file lists the handle's blocks (DESIGN.md section 3 has the table) and supplies the HIP side.
// Rows keep their numbers, so bond tables, resident halo rows and rows waiting to be packed all survive.  No kernel: every
// copy is a device-to-device copy of the first n rows of a block.  Textual unit of kid_hip.hip, included once.

namespace {
// the plan's allocator on the handle's two memory owners.  Fills and copies are on the handle's stream, in that order; an old
// block goes back only once the stream has drained, so no copy can still be reading it.
struct ReserveOps {
  kid_handle *h;
  HipMem &owner(int o) const { return o ? h->rp_mem : h->mem; }
  int alloc(int o, void **p, size_t bytes, int fill) const { return owner(o).alloc(p, bytes, kid::MEM_DEVICE, fill); }
  int release(int o, void **p) const {
    if (!*p) return 0;
    const int e = (int)hipStreamSynchronize(h->stream);
    const int e2 = owner(o).release(p);
    return e ? e : e2;
  }
  int copy(void *dst, const void *src, size_t bytes) const { return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->stream); }
  // the way back of a bond table after a failed allocation: ranges that overlap go through the host (never on a path that succeeds)
  int move_down(void *dst, const void *src, size_t bytes) const {
    if ((const char *)dst + bytes <= (const char *)src) return copy(dst, src, bytes);
    std::vector<char> tmp(bytes);
    int e = (int)hipStreamSynchronize(h->stream);
    if (!e) e = (int)hipMemcpy(tmp.data(), src, bytes, hipMemcpyDeviceToHost);
    if (!e) e = (int)hipMemcpy(dst, tmp.data(), bytes, hipMemcpyHostToDevice);
    return e;
  }
  int fill(void *p, int byte, size_t bytes) const { return (int)hipMemsetAsync(p, byte, bytes, h->stream); }
};

// The blocks of a handle that are sized or strided by its capacity.  The plan swaps untyped pointers: it works on copies
// (`value`) and store() puts them back into the typed members, whatever the outcome.
struct ReserveList {
  struct Back { void (*put)(void *member, void *v); void *member; };
  std::vector<kid::ReserveBlock> blocks;
  std::vector<void *> value;
  std::vector<Back> back;
  template <class T>
  void add(T *&p, int kind, int fill = kid::RESERVE_NOFILL, size_t slots = 1, int owner = 0, size_t fixed_bytes = 0, size_t *bytes = nullptr, size_t elem = sizeof(T)) {
    if (!p) return;   // a feature that was never switched on has nothing to move
    blocks.push_back(kid::ReserveBlock{nullptr, bytes, kind, owner, fill, elem, slots, fixed_bytes});
    value.push_back((void *)p);
    back.push_back(Back{[](void *member, void *v) { *static_cast<T **>(member) = static_cast<T *>(v); }, (void *)&p});
  }
  void add(Scratch &t, int kind, int owner = 0, size_t fixed_bytes = 0) {
    if (!t.p) return;
    blocks.push_back(kid::ReserveBlock{nullptr, &t.bytes, kind, owner, kid::RESERVE_NOFILL, 1, 1, fixed_bytes ? fixed_bytes : 1});
    value.push_back(t.p);
    back.push_back(Back{[](void *member, void *v) { *static_cast<void **>(member) = v; }, (void *)&t.p});
  }
  void bind() { for (size_t q = 0; q < blocks.size(); ++q) blocks[q].member = &value[q]; }
  void store() { for (size_t q = 0; q < blocks.size(); ++q) back[q].put(back[q].member, value[q]); }
};
}  // namespace

extern "C" {

static int reserve_list(kid_handle *h, int64_t new_cap, ReserveList &L) {
  using namespace kid;
  const size_t cap = (size_t)new_cap;
  // ---- state: n rows of each are copied ----
  for (auto &field : h->bp.f) L.add(field, RESERVE_STATE, 0);
  for (auto &field : h->bp.i) L.add(field, RESERVE_STATE, 0);
  L.add(h->bp.id, RESERVE_STATE, 0);
  if (h->mts_ready) {
    const size_t mbs = (size_t)(h->mb > 0 ? h->mb : 1);   // slot-major, stride = capacity: every slot's rows move to the new stride
    L.add(h->mts.bcount, RESERVE_STATE, 0);
    L.add(h->mts.bother_id, RESERVE_STATE, 0, mbs);
    L.add(h->mts.bbroken, RESERVE_STATE, 0, mbs);
    L.add(h->mts.bother_row, RESERVE_STATE, 0xff, mbs);
    L.add(h->mts.bother_slot, RESERVE_STATE, 0xff, mbs);
    for (auto &field : h->mts.bf) L.add(field, RESERVE_STATE, 0, mbs);
    // what the last sort and the last labelling left per row: kept, so that an unchanged population is still recognised as one
    for (int32_t **q : {&h->mts.rank, &h->mts.order, &h->mts.label}) L.add(*q, RESERVE_STATE);
    L.add(h->d_last_key, RESERVE_STATE);
    L.add(h->d_bond_sig, RESERVE_STATE, 0);
  }
  L.add(h->d_orient, RESERVE_STATE);
  // ---- scratch whose users expect it to exist: a new block, nothing copied ----
  L.add(h->d_lane, RESERVE_REALLOC, 0);   // the slow lane has been left: all zeros
  L.add(h->d_redo_list, RESERVE_REALLOC);
  L.add(h->d_redo_list2, RESERVE_REALLOC);
  if (h->mts_ready) {
    for (int32_t **q : {&h->mts.root_flag, &h->mts.root_scan}) L.add(*q, RESERVE_REALLOC);
    L.add(h->mts.rec, RESERVE_REALLOC, 0, 3 * 8);
    for (int q = 0; q < 2; ++q) { L.add(h->d_key64[q], RESERVE_REALLOC); L.add(h->d_rows[q], RESERVE_REALLOC); }
    size_t b1 = 0, b2 = 0;
    KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b1, h->d_key64[0], h->d_key64[1], h->d_rows[0], h->d_rows[1], cap, 0, 64, h->stream));
    KID_HIP(h, rocprim::exclusive_scan(nullptr, b2, h->mts.root_flag, h->mts.root_scan, 0, cap, rocprim::plus<int>(), h->stream));
    L.add(h->mts_tmp, RESERVE_REALLOC, 0, std::max(b1, b2));
  }
  if (h->rp.stage) {   // reproducible sums: the mode's own owner; StageTab carries the capacity as a stride, handed over at every launch
    L.add(h->rp.stage, RESERVE_REALLOC, RESERVE_NOFILL, (size_t)KID_ST_N, 1);
    L.add(h->rp.key, RESERVE_REALLOC, RESERVE_NOFILL, 1, 1);
    L.add(h->rp.mask, RESERVE_REALLOC, RESERVE_NOFILL, 1, 1);
    L.add(h->rp.srows, RESERVE_REALLOC, RESERVE_NOFILL, 1, 1);
    for (int q = 0; q < 2; ++q) {
      L.add(h->rp.k64[q], RESERVE_REALLOC, RESERVE_NOFILL, 1, 1); L.add(h->rp.rows[q], RESERVE_REALLOC, RESERVE_NOFILL, 1, 1); L.add(h->rp.k32[q], RESERVE_REALLOC, RESERVE_NOFILL, 1, 1);
    }
    size_t b64 = 0, b32 = 0;
    KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b64, h->rp.k64[0], h->rp.k64[1], h->rp.rows[0], h->rp.rows[1], cap, 0, 64, h->stream));
    KID_HIP(h, rocprim::radix_sort_pairs(nullptr, b32, h->rp.k32[0], h->rp.k32[1], h->rp.rows[0], h->rp.rows[1], cap, 0, 32, h->stream));
    L.add(h->rp.tmp, RESERVE_REALLOC, 1, std::max(b64, b32));
  }
  // ---- scratch with a lazy path: freed; whoever needs it next allocates it at the new size ----
  // everything perm_storage makes goes together (it allocates all of it when it finds d_key[0] null)
  for (auto &field : h->bp_alt.f) L.add(field, RESERVE_LAZY);
  for (auto &field : h->bp_alt.i) L.add(field, RESERVE_LAZY);
  L.add(h->bp_alt.id, RESERVE_LAZY);
  for (int32_t **q : {&h->cold.origin, &h->cold.origin_alt}) L.add(*q, RESERVE_LAZY);   // (the caller has materialised the cold fields: rows_enter)
  for (unsigned **q : {&h->d_key[0], &h->d_key[1], &h->d_idx[0], &h->d_idx[1], &h->d_cell_hist}) L.add(*q, RESERVE_LAZY);
  for (Scratch *t : {&h->sort_tmp, &h->scan_tmp, &h->cscan_tmp}) L.add(*t, RESERVE_LAZY);
  // the second set of bond tables (bonds_move, kid_rows.inc): it holds nothing between two permutations, and the next one makes it at the new stride
  L.add(h->bond_alt.bcount, RESERVE_LAZY); L.add(h->bond_alt.bother_id, RESERVE_LAZY); L.add(h->bond_alt.bbroken, RESERVE_LAZY);
  L.add(h->bond_alt.bother_row, RESERVE_LAZY); L.add(h->bond_alt.bother_slot, RESERVE_LAZY);
  for (auto &field : h->bond_alt.bf) L.add(field, RESERVE_LAZY);
  L.add(h->d_lane_alt, RESERVE_LAZY);
  L.add(h->d_keep, RESERVE_LAZY);
  L.add(h->d_static_rows, RESERVE_LAZY);   // a cached order, rebuilt from the rows (rows_orders_stale below)
  L.add(h->d_budget, RESERVE_LAZY);
  L.bind();
  return KID_OK;
}

// The capacity becomes new_cap (> h->capacity, within the limit).  The caller has entered through rows_enter(h, ROWS_CHANGE).
static int reserve_core(kid_handle *h, int64_t new_cap) {
  const int64_t old_cap = h->capacity;
  ReserveList L;
  { const int rc = reserve_list(h, new_cap, L); if (rc) return rc; }
  ReserveOps ops{h};
  const bool had_orient = h->bp.orient != nullptr;
  const kid::ReserveResult r = kid::reserve_apply(ops, L.blocks.data(), (int)L.blocks.size(), h->n, old_cap, new_cap);
  L.store();
  // whatever happened, pointers have changed: the device's tables follow, and nothing that was planned or captured with the
  // old ones is used again
  if (had_orient) h->bp.orient = h->d_orient;
  h->rplan = kid_handle::RebinPlan{};
  h->static_rows_cap = 0;
  h->bond_alt_rows = 0;
  rows_orders_stale(h);
  h->order_n = -1; h->labels_stale = true;
  if (h->sub_graph_exec) { (void)hipGraphExecDestroy(h->sub_graph_exec); h->sub_graph_exec = nullptr; h->sub_graph_n = -1; }
  h->tables_dirty = true; h->mts_dirty = true;
  if (r.grown) {
    h->capacity = new_cap;
    if (h->mts_ready) h->mts.stride = (long long)new_cap;
  }
  int rc = h->mts_ready ? mts_refresh(h) : refresh_tables(h);
  if (!rc) { const hipError_t e = hipStreamSynchronize(h->stream); if (e != hipSuccess) { h->err = std::string("kid_reserve: ") + hipGetErrorString(e); rc = KID_EHIP; } }
  if (r.error) {
    h->err = std::string("kid_reserve: ") + hipGetErrorString((hipError_t)r.error) +
             (r.grown ? " while freeing a block of the old capacity (the handle is at the new capacity)"
                      : " while growing from " + std::to_string(old_cap) + " to " + std::to_string(new_cap) + " rows (the handle keeps the old capacity)") +
             (r.restride_failed ? "; the bond tables could not be put back to the old stride and hold nothing usable: upload the bonds again" : "");
    if (r.restride_failed) h->have_bonds = false;
    return KID_EHIP;
  }
  return rc;
}

// An entry point is about to hold `need` rows.  Mode off, or room enough: nothing happens and the caller's own check reports
// as it always did.  Otherwise the growth rule; a need beyond max_capacity is KID_ECAPACITY before anything is written.
static int auto_reserve(kid_handle *h, int64_t need, const char *what) {
  if (h->auto_growth == 0. || need <= h->capacity) return KID_OK;
  int64_t next = h->capacity;
  const int rc_n = kid::reserve_next_capacity(h->capacity, need, h->auto_growth, h->auto_max_capacity, &next);
  if (rc_n == kid::RESERVE_ECAPACITY) {
    h->err = std::string(what) + ": " + std::to_string(need) + " rows are needed, more than the max_capacity of kid_set_auto_reserve, " +
             std::to_string(kid::reserve_max_capacity(h->auto_max_capacity)) + "; nothing was written";
    return KID_ECAPACITY;
  }
  if (rc_n) { h->err = std::string(what) + ": auto-reserve was given a count that is no row count"; return KID_EINVAL; }
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  return reserve_core(h, next);
}

int kid_capacity(kid_handle *h, int64_t *rows) {
  if (!h || !rows) return KID_EINVAL;
  *rows = h->capacity;
  return KID_OK;
}

int kid_reserve(kid_handle *h, int64_t rows) {
  if (!h) return KID_EINVAL;
  if (rows > kid::RESERVE_MAX_ROWS) { h->err = "kid_reserve: more than 2^29 rows (the per-berg kernel addresses a row by a 32-bit byte offset)"; return KID_EINVAL; }
  if (rows <= h->capacity) return KID_OK;   // the handle never shrinks
  { const int rc = rows_enter(h, ROWS_CHANGE); if (rc) return rc; }
  return reserve_core(h, rows);
}

int kid_set_auto_reserve(kid_handle *h, int64_t min_free, double growth, int64_t max_capacity) {
  if (!h) return KID_EINVAL;
  if (!kid::reserve_policy_valid(min_free, growth, max_capacity)) {
    h->err = "kid_set_auto_reserve: growth is 0 (off) or >= 1, min_free >= 0, max_capacity between 0 (meaning 2^29) and 2^29";
    return KID_EINVAL;
  }
  h->auto_growth = growth;
  h->auto_min_free = growth == 0. ? 0 : min_free;
  h->auto_max_capacity = growth == 0. ? 0 : max_capacity;
  return KID_OK;
}

}  // extern "C"
