// kid_reserve_plan.hpp -- growing a handle's row capacity, as plain C++17: no HIP header, no handle.  Three things are written
// down here once: the next capacity of the growth rule (kid_set_auto_reserve), what a block sized by the capacity is (its
// kind, its shape), and the order in which kid_reserve moves the blocks, against an allocator it is handed.  kid_reserve.inc
// lists the handle's blocks and supplies the HIP allocator; tests/reserve_plan_host.cpp runs the same sequence on the host
// against an allocator made of malloc that can be told to fail.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace kid {

constexpr int64_t RESERVE_MAX_ROWS = int64_t(1) << 29;   // the limit kid_create states (a row is addressed by a 32-bit byte offset)
enum { RESERVE_OK = 0, RESERVE_EINVAL = -1, RESERVE_ECAPACITY = -4 };   // the values of KID_OK, KID_EINVAL, KID_ECAPACITY
enum { RESERVE_NOFILL = -1 };                                            // MEM_NOFILL of kid_mem.hpp

// the arguments of kid_set_auto_reserve: growth = 0 switches the mode off, whatever the others are
inline bool reserve_policy_valid(int64_t min_free, double growth, int64_t max_capacity) {
  if (growth == 0.) return true;
  return growth >= 1. && std::isfinite(growth) && min_free >= 0 && max_capacity >= 0 && max_capacity <= RESERVE_MAX_ROWS;
}
inline int64_t reserve_max_capacity(int64_t max_capacity) { return max_capacity > 0 && max_capacity < RESERVE_MAX_ROWS ? max_capacity : RESERVE_MAX_ROWS; }

// next = min(max_capacity, max(need, ceil(capacity * growth))), never below the capacity.  need > max_capacity: RESERVE_ECAPACITY
// and *next is left alone.  The product is clamped as a double before it becomes an integer, so no growth factor overflows.
inline int reserve_next_capacity(int64_t capacity, int64_t need, double growth, int64_t max_capacity, int64_t *next) {
  if (capacity < 0 || need < 0 || !(growth >= 1.) || !next) return RESERVE_EINVAL;
  const int64_t top = reserve_max_capacity(max_capacity);
  if (need > top) return RESERVE_ECAPACITY;
  const double g = std::ceil((double)capacity * growth);
  const int64_t grown = g >= (double)top ? top : (int64_t)g;
  int64_t nx = need > grown ? need : grown;
  if (nx > top) nx = top;
  *next = nx > capacity ? nx : capacity;
  return RESERVE_OK;
}

// A block whose size follows the capacity.
//   STATE   : rows [0, n) of each slot are kept -- allocate new, copy, swap the member, free old
//   REALLOC : scratch whose user expects it to exist -- allocate new, swap, free old; nothing is copied
//   LAZY    : scratch whose user allocates it when it finds the pointer null -- freed, before anything is allocated
// A block is `slots` runs of `capacity` rows of `elem` bytes.  slots > 1 with STATE are the slot-major bond tables, whose
// stride IS the capacity: their rows move to the new stride.  fixed_bytes != 0: the size is not slots * capacity * elem
// (temporary storage whose size a library names); such a block is never STATE.
enum ReserveKind { RESERVE_STATE, RESERVE_REALLOC, RESERVE_LAZY };
struct ReserveBlock {
  void **member;       // the pointer the handle keeps
  size_t *bytes;       // where the handle keeps the block's size, or null
  int kind, owner;     // owner: handed through to the allocator (a handle has more than one memory owner)
  int fill;            // byte every new block is set to before the copy (rows beyond n read as in a fresh handle), or RESERVE_NOFILL
  size_t elem, slots, fixed_bytes;
};
inline size_t reserve_block_bytes(const ReserveBlock &b, int64_t capacity) { return b.fixed_bytes ? b.fixed_bytes : b.slots * (size_t)capacity * b.elem; }

struct ReserveResult {
  int error = 0;               // the allocator's code of the first failure (0: none)
  int failed_block = -1;       // the block whose allocation or copy failed
  bool grown = false;          // every block is at the new capacity (an error then comes from freeing an old block)
  bool restride_failed = false;   // ... and the way back of a bond table failed too: the tables hold nothing usable
};

// Alloc: int alloc(int owner, void **p, size_t bytes, int fill)   a new block, set to `fill` unless RESERVE_NOFILL; *p null on failure
//        int release(int owner, void **p)                         frees *p and nulls it (null: nothing to do)
//        int copy(void *dst, const void *src, size_t bytes)       ranges do not overlap
//        int move_down(void *dst, const void *src, size_t bytes)  dst < src, ranges may overlap
//        int fill(void *p, int byte, size_t bytes)
// each 0 or the allocator's error code.
//
// The sequence.  LAZY blocks go first: nothing of them is needed and the peak is lower without them.  Then the others in the
// order of the list, one at a time, so that the most held at any moment is the new total plus one old block.  A block
// that cannot be allocated or copied ends the call: the blocks before it are larger than the old capacity needs, which
// harms nobody, except that a slot-major table already stands at the new stride while the tables after it do not -- those
// are put back to the old stride inside their new blocks (slot s moves down by s * (new - old) rows, lowest slot first, and
// the rows behind n are set to the fill value again).  The caller keeps the old capacity and stride in that case.
template <class Alloc>
ReserveResult reserve_apply(Alloc &a, ReserveBlock *blocks, int nblocks, int64_t n, int64_t old_cap, int64_t new_cap) {
  ReserveResult r;
  auto note = [&r](int e) { if (e && !r.error) r.error = e; };
  for (int i = 0; i < nblocks; ++i) {
    ReserveBlock &b = blocks[i];
    if (b.kind != RESERVE_LAZY) continue;
    note(a.release(b.owner, b.member));
    if (b.bytes) *b.bytes = 0;
  }
  if (r.error) return r;   // (a block the owner does not know: nothing has been allocated yet)
  const size_t rows = (size_t)n, oc = (size_t)old_cap, nc = (size_t)new_cap;
  for (int i = 0; i < nblocks; ++i) {
    ReserveBlock &b = blocks[i];
    if (b.kind == RESERVE_LAZY) continue;
    const size_t bytes = reserve_block_bytes(b, new_cap);
    void *q = nullptr;
    int e = a.alloc(b.owner, &q, bytes, b.fill);
    if (!e && b.kind == RESERVE_STATE && *b.member && rows)
      for (size_t s = 0; s < b.slots && !e; ++s)
        e = a.copy((char *)q + s * nc * b.elem, (const char *)*b.member + s * oc * b.elem, rows * b.elem);
    if (e) {
      if (q) (void)a.release(b.owner, &q);
      r.error = e; r.failed_block = i;
      for (int j = 0; j < i; ++j) {   // the bond tables already moved: back to the old stride
        const ReserveBlock &t = blocks[j];
        if (t.kind != RESERVE_STATE || t.slots < 2 || !*t.member) continue;
        char *base = (char *)*t.member;
        int e2 = 0;
        for (size_t s = 1; s < t.slots && !e2 && rows; ++s) e2 = a.move_down(base + s * oc * t.elem, base + s * nc * t.elem, rows * t.elem);
        if (t.fill != RESERVE_NOFILL && oc > rows)
          for (size_t s = 0; s < t.slots && !e2; ++s) e2 = a.fill(base + (s * oc + rows) * t.elem, t.fill, (oc - rows) * t.elem);
        if (e2) r.restride_failed = true;
      }
      return r;
    }
    void *old = *b.member;
    *b.member = q;
    if (b.bytes) *b.bytes = bytes;
    note(a.release(b.owner, &old));
  }
  r.grown = true;
  return r;
}

}  // namespace kid
