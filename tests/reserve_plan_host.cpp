// The plan of kid_reserve (icebergs_amd/csrc/kid_reserve_plan.hpp) on the host: the next capacity of the growth rule against
// values written out by hand, and the allocate-copy-swap-free sequence against an allocator made of malloc that counts what it
// holds and can be told to fail at its k-th allocation.  Plain C++17 with its own main (tests/test_reserve_cpu.py builds it
// with the address and undefined-behaviour sanitizers, which see every read of a freed block and every write past one); no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../icebergs_amd/csrc/kid_reserve_plan.hpp"

using namespace kid;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// ---- the fake owner ----
struct FakeAlloc {
  enum { E_NOMEM = 2, E_UNKNOWN = 1 };
  std::map<void *, size_t> live[2];   // per owner
  std::set<void *> freed_once;        // every pointer ever released
  size_t in_use = 0, high_water = 0;
  int allocs = 0, fail_at = -1, double_free = 0, overlap_copies = 0;
  int alloc(int owner, void **p, size_t bytes, int fill) {
    *p = nullptr;
    if (allocs++ == fail_at) return E_NOMEM;
    void *q = std::malloc(bytes ? bytes : 1);
    std::memset(q, fill == RESERVE_NOFILL ? 0x5a : fill, bytes ? bytes : 1);   // 0x5a: what no test value looks like
    live[owner][q] = bytes;
    in_use += bytes;
    if (in_use > high_water) high_water = in_use;
    *p = q;
    return 0;
  }
  int release(int owner, void **p) {
    if (!*p) return 0;
    const auto it = live[owner].find(*p);
    if (it == live[owner].end()) { ++double_free; return E_UNKNOWN; }
    in_use -= it->second;
    live[owner].erase(it);
    freed_once.insert(*p);
    std::free(*p);
    *p = nullptr;
    return 0;
  }
  int copy(void *dst, const void *src, size_t bytes) {
    const char *d = (const char *)dst, *s = (const char *)src;
    if (d < s + bytes && s < d + bytes) ++overlap_copies;
    std::memcpy(dst, src, bytes);
    return 0;
  }
  int move_down(void *dst, const void *src, size_t bytes) { std::memmove(dst, src, bytes); return 0; }
  int fill(void *p, int byte, size_t bytes) { std::memset(p, byte, bytes); return 0; }
  size_t size_of(int owner, void *p) const { const auto it = live[owner].find(p); return it == live[owner].end() ? 0 : it->second; }
};

// ---- a handle in miniature: one of every shape the real one has ----
struct Mini {
  double *f0 = nullptr, *f1 = nullptr;       // SoA fields (state, filled 0)
  int32_t *alive = nullptr;                  // (state)
  int64_t *bond_id = nullptr;                // slot-major, 3 slots (state, filled 0)
  int32_t *bond_row = nullptr;               // slot-major, 3 slots (state, filled 0xff)
  double *orient = nullptr;                  // (state, not filled)
  int32_t *lane = nullptr;                   // realloc, filled 0
  double *stage = nullptr;                   // realloc on the second owner, 5 slots
  void *tmp = nullptr; size_t tmp_bytes = 0; // realloc, size named by a library
  double *alt = nullptr;                     // lazy
  int32_t *never = nullptr;                  // a feature that is off: stays null
  int64_t cap = 0, n = 0, stride = 0;
};
enum { SLOTS = 3 };
static double f0_of(int64_t k) { return 1000.5 + (double)k; }
static double f1_of(int64_t k) { return -7.25 * (double)k; }
static int64_t bond_of(int s, int64_t k) { return (int64_t)(s + 1) * 1000000 + k; }
static int32_t row_of(int s, int64_t k) { return (int32_t)(k * 4 + s); }

static void mini_create(FakeAlloc &a, Mini &m, int64_t cap, int64_t n) {
  const size_t c = (size_t)cap;
  m.cap = cap; m.n = n; m.stride = cap;
  a.alloc(0, (void **)&m.f0, c * 8, 0); a.alloc(0, (void **)&m.f1, c * 8, 0); a.alloc(0, (void **)&m.alive, c * 4, 0);
  a.alloc(0, (void **)&m.bond_id, SLOTS * c * 8, 0); a.alloc(0, (void **)&m.bond_row, SLOTS * c * 4, 0xff);
  a.alloc(0, (void **)&m.orient, c * 8, RESERVE_NOFILL);
  a.alloc(0, (void **)&m.lane, c * 4, 0); a.alloc(1, (void **)&m.stage, 5 * c * 8, RESERVE_NOFILL);
  m.tmp_bytes = 100 + c; a.alloc(0, &m.tmp, m.tmp_bytes, RESERVE_NOFILL);
  a.alloc(0, (void **)&m.alt, c * 8, RESERVE_NOFILL);
  for (int64_t k = 0; k < n; ++k) {
    m.f0[k] = f0_of(k); m.f1[k] = f1_of(k); m.alive[k] = 1; m.orient[k] = 0.5 * (double)k;
    for (int s = 0; s < SLOTS; ++s) { m.bond_id[s * c + k] = bond_of(s, k); m.bond_row[s * c + k] = row_of(s, k); }
  }
}
static int mini_blocks(Mini &m, int64_t new_cap, ReserveBlock *b) {
  int nb = 0;
  b[nb++] = ReserveBlock{(void **)&m.f0, nullptr, RESERVE_STATE, 0, 0, 8, 1, 0};
  b[nb++] = ReserveBlock{(void **)&m.f1, nullptr, RESERVE_STATE, 0, 0, 8, 1, 0};
  b[nb++] = ReserveBlock{(void **)&m.alive, nullptr, RESERVE_STATE, 0, 0, 4, 1, 0};
  b[nb++] = ReserveBlock{(void **)&m.bond_id, nullptr, RESERVE_STATE, 0, 0, 8, SLOTS, 0};
  b[nb++] = ReserveBlock{(void **)&m.bond_row, nullptr, RESERVE_STATE, 0, 0xff, 4, SLOTS, 0};
  b[nb++] = ReserveBlock{(void **)&m.orient, nullptr, RESERVE_STATE, 0, RESERVE_NOFILL, 8, 1, 0};
  b[nb++] = ReserveBlock{(void **)&m.lane, nullptr, RESERVE_REALLOC, 0, 0, 4, 1, 0};
  b[nb++] = ReserveBlock{(void **)&m.stage, nullptr, RESERVE_REALLOC, 1, RESERVE_NOFILL, 8, 5, 0};
  b[nb++] = ReserveBlock{&m.tmp, &m.tmp_bytes, RESERVE_REALLOC, 0, RESERVE_NOFILL, 1, 1, 100 + (size_t)new_cap};
  b[nb++] = ReserveBlock{(void **)&m.alt, nullptr, RESERVE_LAZY, 0, RESERVE_NOFILL, 8, 1, 0};
  return nb;
}
static size_t mini_total(int64_t cap, bool with_lazy) {
  const size_t c = (size_t)cap;
  return c * 8 * 2 + c * 4 + SLOTS * c * 8 + SLOTS * c * 4 + c * 8 + c * 4 + 5 * c * 8 + 100 + c + (with_lazy ? c * 8 : 0);
}
// every member is a live block large enough for `cap` rows, the rows are what was written, the bond tables stand at `stride`,
// and the rows behind n read as in a fresh handle
static void mini_check(const FakeAlloc &a, const Mini &m, int64_t cap, int64_t stride, int line) {
  const size_t c = (size_t)cap, st = (size_t)stride;
  bool ok = a.size_of(0, m.f0) >= c * 8 && a.size_of(0, m.f1) >= c * 8 && a.size_of(0, m.alive) >= c * 4 && a.size_of(0, m.orient) >= c * 8 &&
            a.size_of(0, m.bond_id) >= SLOTS * st * 8 && a.size_of(0, m.bond_row) >= SLOTS * st * 4 && st >= c &&
            a.size_of(0, m.lane) >= c * 4 && a.size_of(1, m.stage) >= 5 * c * 8 && a.size_of(0, m.tmp) == m.tmp_bytes && m.tmp_bytes >= 100 + c &&
            (m.alt == nullptr || a.size_of(0, m.alt) >= c * 8) && m.never == nullptr;
  if (!ok) { std::printf("FAILED line %d: a member does not point at a live block of capacity %lld\n", line, (long long)cap); ++failures; return; }
  for (int64_t k = 0; k < m.n && ok; ++k) {
    ok = m.f0[k] == f0_of(k) && m.f1[k] == f1_of(k) && m.alive[k] == 1 && m.orient[k] == 0.5 * (double)k;
    for (int s = 0; s < SLOTS && ok; ++s) ok = m.bond_id[s * st + k] == bond_of(s, k) && m.bond_row[s * st + k] == row_of(s, k);
  }
  for (int64_t k = m.n; k < cap && ok; ++k) {
    ok = m.f0[k] == 0. && m.f1[k] == 0. && m.alive[k] == 0;
    for (int s = 0; s < SLOTS && ok; ++s) ok = m.bond_id[s * st + k] == 0 && m.bond_row[s * st + k] == -1;
  }
  if (!ok) { std::printf("FAILED line %d: rows are not what they were (capacity %lld, stride %lld)\n", line, (long long)cap, (long long)stride); ++failures; }
}
static void mini_destroy(FakeAlloc &a, Mini &m) {
  a.release(0, (void **)&m.f0); a.release(0, (void **)&m.f1); a.release(0, (void **)&m.alive); a.release(0, (void **)&m.bond_id);
  a.release(0, (void **)&m.bond_row); a.release(0, (void **)&m.orient); a.release(0, (void **)&m.lane); a.release(1, (void **)&m.stage);
  a.release(0, &m.tmp); a.release(0, (void **)&m.alt);
}

static void run_case(int64_t old_cap, int64_t n, int64_t new_cap) {
  // how many allocations a run that succeeds makes, and what it must look like
  int nallocs = 0;
  {
    FakeAlloc a; Mini m;
    mini_create(a, m, old_cap, n);
    const std::set<void *> before = {m.f0, m.f1, m.alive, m.bond_id, m.bond_row, m.orient, m.lane, m.stage, m.tmp, m.alt};
    size_t largest_old = 0;
    for (void *p : before) largest_old = std::max(largest_old, std::max(a.size_of(0, p), a.size_of(1, p)));
    CHECK(a.in_use == mini_total(old_cap, true));
    ReserveBlock b[16];
    const int nb = mini_blocks(m, new_cap, b), a0 = a.allocs;
    a.high_water = a.in_use;
    const ReserveResult r = reserve_apply(a, b, nb, n, old_cap, new_cap);
    nallocs = a.allocs - a0;
    CHECK(r.error == 0 && r.grown && r.failed_block == -1 && !r.restride_failed);
    CHECK(nallocs == nb - 1);   // every block but the lazy one
    CHECK(m.alt == nullptr);
    CHECK(a.in_use == mini_total(new_cap, false));
    CHECK(a.high_water <= mini_total(new_cap, false) + largest_old);   // the new total plus one old block, not twice the state
    CHECK(a.double_free == 0 && a.overlap_copies == 0);
    // every block held before was freed exactly once (swapped: its member now points elsewhere), and none of them is live
    for (void *p : before) CHECK(a.freed_once.count(p) == 1 && a.size_of(0, p) == 0 && a.size_of(1, p) == 0);
    CHECK(a.live[0].size() + a.live[1].size() == (size_t)nb - 1);
    mini_check(a, m, new_cap, new_cap, __LINE__);
    for (int64_t k = 0; k < new_cap; ++k) CHECK(m.lane[k] == 0);
    mini_destroy(a, m);
    CHECK(a.in_use == 0 && a.live[0].empty() && a.live[1].empty() && a.double_free == 0);
  }
  // a failure at each allocation in turn
  for (int k = 0; k < nallocs; ++k) {
    FakeAlloc a; Mini m;
    mini_create(a, m, old_cap, n);
    ReserveBlock b[16];
    const int nb = mini_blocks(m, new_cap, b);
    a.fail_at = a.allocs + k;
    const ReserveResult r = reserve_apply(a, b, nb, n, old_cap, new_cap);
    CHECK(r.error == FakeAlloc::E_NOMEM && !r.grown && r.failed_block == k && !r.restride_failed);
    CHECK(m.alt == nullptr);   // (the lazy block went first; its user allocates it again)
    // a valid handle at the OLD capacity: every member live and at least that large, the bond tables all at the old stride
    mini_check(a, m, old_cap, old_cap, __LINE__);
    CHECK(a.double_free == 0);
    // nothing leaked: what is live is exactly what the members point at
    CHECK(a.live[0].size() + a.live[1].size() == (size_t)nb - 1);
    // ... and the handle can still grow once memory is back
    a.fail_at = -1;
    const int nb2 = mini_blocks(m, new_cap, b);
    const ReserveResult r2 = reserve_apply(a, b, nb2, n, old_cap, new_cap);
    CHECK(r2.error == 0 && r2.grown);
    mini_check(a, m, new_cap, new_cap, __LINE__);
    CHECK(a.in_use == mini_total(new_cap, false));
    mini_destroy(a, m);
    CHECK(a.in_use == 0 && a.live[0].empty() && a.live[1].empty() && a.double_free == 0);
  }
}

int main() {
  // ---- next capacity ----
  int64_t nx = -1;
  CHECK(reserve_next_capacity(1000, 1001, 1.5, 0, &nx) == RESERVE_OK && nx == 1500);         // need below capacity * growth
  CHECK(reserve_next_capacity(1000, 1800, 1.5, 0, &nx) == RESERVE_OK && nx == 1800);         // need above it
  CHECK(reserve_next_capacity(1001, 1002, 1.5, 0, &nx) == RESERVE_OK && nx == 1502);         // ceil(1501.5)
  CHECK(reserve_next_capacity(1000, 1001, 1.0, 0, &nx) == RESERVE_OK && nx == 1001);         // growth = 1: exactly what is needed
  CHECK(reserve_next_capacity(1000, 1200, 2.0, 1500, &nx) == RESERVE_OK && nx == 1500);      // the clamp at max_capacity
  CHECK(reserve_next_capacity(1000, 1500, 2.0, 1500, &nx) == RESERVE_OK && nx == 1500);      // need == max_capacity still fits
  nx = -1;
  CHECK(reserve_next_capacity(1000, 1501, 2.0, 1500, &nx) == RESERVE_ECAPACITY && nx == -1); // need above it: nothing is named
  CHECK(reserve_next_capacity(0, 1, 1.5, 0, &nx) == RESERVE_OK && nx == 1);                  // an empty handle
  CHECK(reserve_next_capacity(400000000, 400000001, 1.5, 0, &nx) == RESERVE_OK && nx == RESERVE_MAX_ROWS);   // max_capacity = 0 means 2^29
  CHECK(reserve_next_capacity(RESERVE_MAX_ROWS - 1, RESERVE_MAX_ROWS, 1.0, 0, &nx) == RESERVE_OK && nx == RESERVE_MAX_ROWS);
  CHECK(reserve_next_capacity(RESERVE_MAX_ROWS, RESERVE_MAX_ROWS + 1, 1.5, 0, &nx) == RESERVE_ECAPACITY);
  CHECK(reserve_next_capacity(1000, 2000, 1e300, 0, &nx) == RESERVE_OK && nx == RESERVE_MAX_ROWS);           // no factor overflows
  CHECK(reserve_next_capacity(1000, 1001, 1.5, int64_t(1) << 40, &nx) == RESERVE_OK && nx == 1500);          // a max beyond the limit is the limit
  CHECK(reserve_next_capacity(2000, 1500, 1.5, 1600, &nx) == RESERVE_OK && nx == 2000);      // never below the capacity
  CHECK(reserve_next_capacity(1000, 1001, 0.5, 0, &nx) == RESERVE_EINVAL);
  CHECK(reserve_next_capacity(1000, -1, 1.5, 0, &nx) == RESERVE_EINVAL);
  CHECK(reserve_max_capacity(0) == RESERVE_MAX_ROWS && reserve_max_capacity(77) == 77);
  // ---- the arguments of kid_set_auto_reserve ----
  CHECK(reserve_policy_valid(0, 0., 0) && reserve_policy_valid(-5, 0., -5));   // off: the others are not looked at
  CHECK(reserve_policy_valid(0, 1., 0) && reserve_policy_valid(64, 1.5, 1 << 20) && reserve_policy_valid(0, 2., RESERVE_MAX_ROWS));
  CHECK(!reserve_policy_valid(0, 0.5, 0) && !reserve_policy_valid(0, 0.999, 0) && !reserve_policy_valid(0, -1., 0));
  CHECK(!reserve_policy_valid(-1, 1.5, 0) && !reserve_policy_valid(0, 1.5, -1) && !reserve_policy_valid(0, 1.5, RESERVE_MAX_ROWS + 1));
  CHECK(!reserve_policy_valid(0, std::nan(""), 0) && !reserve_policy_valid(0, HUGE_VAL, 0));

  // ---- the sequence ----
  run_case(10, 10, 25);    // a full handle, more than doubled: no slot of a bond table overlaps its old place
  run_case(10, 7, 11);     // one row more: on the way back every slot overlaps itself
  run_case(64, 0, 100);    // an empty handle: nothing to copy
  run_case(9, 9, 13);      // odd sizes
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("reserve plan: all checks passed\n");
  return 0;
}
