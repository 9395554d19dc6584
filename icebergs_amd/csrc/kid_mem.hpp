// kid_mem.hpp -- who owns a handle's device and pinned memory.  No HIP in this file: the allocator is a template
// parameter (kid_handle.hpp supplies the HIP one, tests/mem_owner_host.cpp one made of malloc / free).
//
// A MemOwner records every block it hands out under the pointer's VALUE.  Which member of the handle holds a pointer on a given day
// is of no interest to it: members may swap their buffers freely (compaction, re-binning, the lane arrays) and free_all() still frees
// each block exactly once.  Memory the caller bound (kid_bind_*) never passes through alloc() and is therefore never freed here.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <unordered_map>

namespace kid {
enum MemKind { MEM_DEVICE = 0, MEM_PINNED = 1 };
enum { MEM_NOFILL = -1 };   // `fill` arguments: this, or the value every byte of a new block is set to (0, 0xff)

// bytes handed out and not yet returned, over every owner of the process (kid_memory_in_use)
inline std::atomic<int64_t> &mem_in_use(MemKind k) { static std::atomic<int64_t> total[2]; return total[k]; }

// Backend: int alloc(void **, size_t, MemKind), int release(void *, MemKind), int fill(void *, int byte, size_t),
// int copy(void *dst, const void *src, size_t), each 0 or the backend's error code, which is passed on; unknown_error is
// what release() and grow() answer for a pointer this owner never handed out.
template <class Backend>
class MemOwner {
 public:
  explicit MemOwner(Backend b = Backend()) : backend_(b) {}
  MemOwner(const MemOwner &) = delete;
  MemOwner &operator=(const MemOwner &) = delete;
  // a new block of `bytes` in *pp; on failure nothing is recorded and *pp is null
  int alloc(void **pp, size_t bytes, MemKind kind, int fill = MEM_NOFILL) {
    void *q = *pp = nullptr;
    int e = backend_.alloc(&q, bytes ? bytes : 1, kind);
    if (!e && fill != MEM_NOFILL && bytes && (e = backend_.fill(q, fill, bytes)) != 0) (void)backend_.release(q, kind);
    if (!e) { record(q, bytes, kind); *pp = q; }
    return e;
  }
  // free *pp, forget it and null it (a null *pp: nothing to do); an unknown pointer is neither freed nor nulled
  int release(void **pp) {
    MemKind kind;
    if (!*pp) return 0;
    if (!forget(*pp, &kind)) return Backend::unknown_error;
    const int e = backend_.release(*pp, kind);
    *pp = nullptr;
    return e;
  }
  // *pp becomes a device block of `bytes` whose first `keep` bytes are those of the old one.  If the allocation or the
  // copy fails, *pp and the old block stay as they were and the new block goes back to the backend.
  int grow(void **pp, size_t keep, size_t bytes) {
    if (*pp && !owns(*pp)) return Backend::unknown_error;
    void *q = nullptr;
    int e = backend_.alloc(&q, bytes ? bytes : 1, MEM_DEVICE);
    if (e) return e;
    if (*pp && keep && (e = backend_.copy(q, *pp, keep)) != 0) { (void)backend_.release(q, MEM_DEVICE); return e; }
    record(q, bytes, MEM_DEVICE);
    e = release(pp);
    *pp = q;
    return e;
  }
  // free whatever is still recorded, each block once, whatever fails; returns the first failure (0: none)
  int free_all() {
    int first = 0;
    for (const auto &b : blocks_) {
      const int e = backend_.release(b.first, b.second.kind);
      if (!first) first = e;
      mem_in_use(b.second.kind) -= (int64_t)b.second.bytes;
    }
    blocks_.clear();
    bytes_[0] = bytes_[1] = 0;
    return first;
  }
  // the bookkeeping alone
  void record(void *p, size_t bytes, MemKind kind) { blocks_[p] = Block{bytes, kind}; count(kind, (int64_t)bytes); }
  bool forget(void *p, MemKind *kind = nullptr) {
    const auto it = blocks_.find(p);
    if (it == blocks_.end()) return false;
    const Block b = it->second;
    if (kind) *kind = b.kind;
    count(b.kind, -(int64_t)b.bytes);
    blocks_.erase(it);
    return true;
  }
  bool owns(const void *p) const { return blocks_.count(const_cast<void *>(p)) != 0; }
  size_t blocks() const { return blocks_.size(); }
  int64_t bytes(MemKind kind) const { return bytes_[kind]; }

 private:
  struct Block { size_t bytes; MemKind kind; };
  void count(MemKind k, int64_t d) { bytes_[k] += d; mem_in_use(k) += d; }
  Backend backend_;
  std::unordered_map<void *, Block> blocks_;
  int64_t bytes_[2] = {0, 0};
};

}  // namespace kid
