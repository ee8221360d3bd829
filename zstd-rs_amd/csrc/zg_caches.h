// zg_caches.h — the two process-wide caches behind the streaming decoders (zg_stream.cpp): pinned host blocks and idle engines. Both are
// reached from every thread that owns a stream, so both are templates over what they allocate: the product instantiates them with
// hipHostMalloc / hipHostFree and Engine, tests/emu/zg_emu_caches.cpp with a counting allocator under ThreadSanitizer.
#pragma once
#include <stddef.h>
#include <mutex>
#include <vector>

namespace zg {

// Pinned host memory is expensive to get (the pages are faulted in and locked: ~0.1 s per few hundred MiB) and a stream needs a ring and
// staging buffers of that size: blocks are kept for the next stream of the process (bounded), not returned to the runtime.
// Mem: void* alloc(size_t n) (null when there is none), void free(void* p); both are called outside the cache's lock except in trim().
template <class Mem>
struct PinnedCache {
  struct Blk { void* p; size_t n; };
  Mem mem;
  std::mutex mu;
  std::vector<Blk> free_;
  size_t held = 0;
  static constexpr size_t kMaxHeld = 3ull << 30;
  void* get(size_t n) {
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t best = free_.size();
      for (size_t i = 0; i < free_.size(); i++)
        if (free_[i].n >= n && free_[i].n <= n + n / 4 + (1u << 20) && (best == free_.size() || free_[i].n < free_[best].n)) best = i;
      if (best != free_.size()) {
        void* p = free_[best].p;
        held -= free_[best].n;
        sizes_.push_back(Blk{p, free_[best].n});
        free_.erase(free_.begin() + best);
        return p;
      }
    }
    void* p = mem.alloc(n);
    if (!p) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    sizes_.push_back(Blk{p, n});
    return p;
  }
  void put(void* p) {
    size_t n = 0;
    {
      std::lock_guard<std::mutex> lk(mu);
      for (size_t i = 0; i < sizes_.size(); i++)
        if (sizes_[i].p == p) { n = sizes_[i].n; sizes_.erase(sizes_.begin() + i); break; }
      if (n && held + n <= kMaxHeld) { free_.push_back(Blk{p, n}); held += n; return; }
    }
    mem.free(p);
  }
  void trim() {
    std::lock_guard<std::mutex> lk(mu);
    for (const Blk& b : free_) mem.free(b.p);
    free_.clear(); held = 0;
  }
  std::vector<Blk> sizes_;   // blocks handed out (their real sizes)
};

// Engines of streaming decoders that are not in use. A stream whose worker thread decodes ahead has an engine of its own (streams, scratch
// buffers sized to its runs); the next stream on the same device takes it over instead of allocating all of that again. Process-wide (a
// stream may outlive the context it was made from), at most two per device.
// E: int device() const, deletable.
template <class E>
struct IdleEngines {
  std::mutex mu;
  std::vector<E*> v;
  E* take(int device) {
    std::lock_guard<std::mutex> lk(mu);
    for (size_t i = 0; i < v.size(); i++) if (v[i]->device() == device) { E* e = v[i]; v.erase(v.begin() + i); return e; }
    return nullptr;
  }
  void give(E* e) {
    {
      std::lock_guard<std::mutex> lk(mu);
      size_t same = 0;
      for (E* x : v) same += x->device() == e->device();
      if (same < 2) { v.push_back(e); return; }
    }
    delete e;
  }
  void trim() {
    std::vector<E*> all;
    { std::lock_guard<std::mutex> lk(mu); all.swap(v); }
    for (E* e : all) delete e;
  }
};

}  // namespace zg
