// The bookkeeping of icebergs_amd/csrc/kid_mem.hpp alone, driven with malloc / free: built with -fsanitize=address,undefined and
// run by tests/test_mem_owner_cpu.py.  A leak, a double free or a free of a foreign pointer ends the run through the sanitizer;
// everything else is checked here.  Prints "ok" and returns 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include "../icebergs_amd/csrc/kid_mem.hpp"

using namespace kid;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Counters { std::set<void *> live; int allocs = 0, frees = 0, fail_alloc_at = -1, fail_copy = 0, fail_free = 0; };
struct HostAllocator {
  static constexpr int unknown_error = 77;
  Counters *c;
  int alloc(void **p, size_t bytes, MemKind) const {
    if (c->allocs == c->fail_alloc_at) { ++c->allocs; return 2; }
    ++c->allocs; *p = std::malloc(bytes); c->live.insert(*p); return 0;
  }
  int release(void *p, MemKind) const {
    if (!c->live.erase(p)) return 99;   // not live: a double free, or a pointer that is not ours (never reached if the owner is right)
    std::free(p); ++c->frees;
    return c->fail_free ? 5 : 0;        // (the block is gone either way: only the report is exercised)
  }
  int fill(void *p, int byte, size_t bytes) const { std::memset(p, byte, bytes); return 0; }
  int copy(void *dst, const void *src, size_t bytes) const { if (c->fail_copy) return 3; std::memcpy(dst, src, bytes); return 0; }
};
using Owner = MemOwner<HostAllocator>;

int main() {
  const int64_t dev0 = mem_in_use(MEM_DEVICE).load(), pin0 = mem_in_use(MEM_PINNED).load();
  Counters c;
  {
    Owner m(HostAllocator{&c});
    // record and forget, byte counts per kind and process-wide
    void *a = nullptr, *b = nullptr, *p = nullptr;
    CHECK(m.alloc(&a, 100, MEM_DEVICE, 0) == 0 && a);
    CHECK(m.alloc(&b, 40, MEM_DEVICE, 0xff) == 0 && b);
    CHECK(m.alloc(&p, 8, MEM_PINNED) == 0 && p);
    CHECK(((unsigned char *)a)[99] == 0 && ((unsigned char *)b)[0] == 0xff && ((unsigned char *)b)[39] == 0xff);
    CHECK(m.blocks() == 3 && m.bytes(MEM_DEVICE) == 140 && m.bytes(MEM_PINNED) == 8);
    CHECK(mem_in_use(MEM_DEVICE).load() == dev0 + 140 && mem_in_use(MEM_PINNED).load() == pin0 + 8);
    CHECK(m.owns(a) && m.owns(p));
    CHECK(m.release(&p) == 0 && p == nullptr && m.bytes(MEM_PINNED) == 0 && c.frees == 1);
    CHECK(m.release(&p) == 0 && c.frees == 1);   // a null pointer: nothing to do
    // a failed allocation records nothing and leaves the pointer null
    void *f = (void *)&c;
    c.fail_alloc_at = c.allocs;
    CHECK(m.alloc(&f, 16, MEM_DEVICE) == 2 && f == nullptr && m.blocks() == 2 && m.bytes(MEM_DEVICE) == 140);
    // forgetting an unknown pointer is an error and frees nothing
    int on_stack = 0; void *u = &on_stack;
    CHECK(m.release(&u) == HostAllocator::unknown_error && u == &on_stack && c.frees == 1 && m.blocks() == 2);
    CHECK(!m.forget(&on_stack) && m.bytes(MEM_DEVICE) == 140);
    CHECK(m.grow(&u, 0, 8) == HostAllocator::unknown_error && u == &on_stack && m.blocks() == 2);
    // grow keeps the prefix
    void *g = nullptr;
    CHECK(m.grow(&g, 0, 4) == 0 && g && m.bytes(MEM_DEVICE) == 144);   // from nothing: an allocation
    std::memcpy(g, "abcd", 4);
    void *g_old = g;
    CHECK(m.grow(&g, 4, 64) == 0 && g != nullptr && !m.owns(g_old) && m.owns(g));
    CHECK(std::memcmp(g, "abcd", 4) == 0 && m.bytes(MEM_DEVICE) == 204 && m.blocks() == 3);
    // ... and loses nothing when a step fails: the old block stays, the new one goes back
    const int frees_before = c.frees; const size_t live_before = c.live.size();
    g_old = g; c.fail_copy = 1;
    CHECK(m.grow(&g, 4, 128) == 3 && g == g_old && m.owns(g) && m.bytes(MEM_DEVICE) == 204 && c.frees == frees_before + 1 && c.live.size() == live_before);
    c.fail_copy = 0; c.fail_alloc_at = c.allocs;
    CHECK(m.grow(&g, 4, 128) == 2 && g == g_old && m.owns(g) && m.bytes(MEM_DEVICE) == 204 && c.live.size() == live_before);
    CHECK(std::memcmp(g, "abcd", 4) == 0);
    // two recorded pointers swapped between their holders are each freed once by the drain
    std::swap(a, b);
    std::swap(a, g);
    const int before = c.frees;
    CHECK(m.free_all() == 0 && c.frees == before + 3 && c.live.empty());
    // byte counts return to zero; a second drain is a no-op
    CHECK(m.blocks() == 0 && m.bytes(MEM_DEVICE) == 0 && m.bytes(MEM_PINNED) == 0);
    CHECK(mem_in_use(MEM_DEVICE).load() == dev0 && mem_in_use(MEM_PINNED).load() == pin0);
    CHECK(m.free_all() == 0 && c.frees == before + 3);
    // the first failed free is reported; the rest is freed all the same
    void *x = nullptr, *y = nullptr;
    CHECK(m.alloc(&x, 8, MEM_DEVICE) == 0 && m.alloc(&y, 8, MEM_DEVICE) == 0);
    c.fail_free = 1;
    CHECK(m.free_all() == 5 && c.live.empty() && m.blocks() == 0);
    CHECK(mem_in_use(MEM_DEVICE).load() == dev0);
    c.fail_free = 0;
  }
  // two owners at once share the process-wide totals and nothing else
  {
    Owner m1(HostAllocator{&c}), m2(HostAllocator{&c});
    void *p1 = nullptr, *p2 = nullptr;
    CHECK(m1.alloc(&p1, 10, MEM_DEVICE) == 0 && m2.alloc(&p2, 20, MEM_DEVICE) == 0);
    CHECK(mem_in_use(MEM_DEVICE).load() == dev0 + 30 && !m1.owns(p2) && !m2.owns(p1));
    CHECK(m1.release(&p2) == HostAllocator::unknown_error && p2 != nullptr);
    CHECK(m1.free_all() == 0 && mem_in_use(MEM_DEVICE).load() == dev0 + 20 && m2.owns(p2));
    CHECK(m2.free_all() == 0 && mem_in_use(MEM_DEVICE).load() == dev0 && c.live.empty());
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
