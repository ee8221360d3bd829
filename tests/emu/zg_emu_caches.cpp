// TEST-ONLY: the two process-wide caches of the streaming decoders (zstd-rs_amd/csrc/zg_caches.h) under eight holder threads and a ninth
// that trims, as a stand-alone program for ThreadSanitizer (tests/emu/Makefile: caches_tsan; tests/test_caches_cpu.py). The product
// instantiates the same templates with hipHostMalloc / hipHostFree and Engine; here the memory is malloc's behind a counting allocator and
// the engine is a counter. A block of n bytes is backed by min(n, kBacked) real bytes, so that sizes up to 1 GiB reach the kMaxHeld bound
// without that much memory; the holder's pattern covers the backed bytes.
//
// Held throughout: no block and no engine has two holders; a block's pattern is intact when its holder verifies it; a block handed out for n
// bytes has between n and n + n/4 + 1 MiB; `held` is the sum of free_ and never exceeds kMaxHeld; at most two idle engines per device;
// nothing that a holder holds is ever freed (trim frees what is in free_ only); after the last put / give and a trim nothing is alive.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_caches.h"

#define CHECK(c, ...) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); _exit(1); } } while (0)

namespace {
constexpr size_t kBacked = 32u << 10;
constexpr int kHolders = 8, kRounds = 1500, kDevices = 2;

// every block that exists: its size as the cache asked for it and its holder (0: none — it lies in free_, or is on its way in or out)
std::mutex g_reg_mu;
struct Rec { size_t n; int holder; };
std::map<void*, Rec> g_blocks;
std::atomic<long> g_live{0}, g_allocs{0}, g_frees{0};
thread_local bool t_allocated = false;   // the calling thread's last get() went to the allocator

struct CountingMem {
  void* alloc(size_t n) {
    void* p = malloc(n < kBacked ? (n ? n : 1) : kBacked);
    if (!p) return nullptr;
    t_allocated = true;
    std::lock_guard<std::mutex> lk(g_reg_mu);
    CHECK(g_blocks.find(p) == g_blocks.end(), "a block is allocated twice");
    g_blocks[p] = Rec{n, 0};
    g_live++; g_allocs++;
    return p;
  }
  void free(void* p) {
    {
      std::lock_guard<std::mutex> lk(g_reg_mu);
      auto it = g_blocks.find(p);
      CHECK(it != g_blocks.end(), "a block that does not exist is freed");
      CHECK(it->second.holder == 0, "a block is freed while holder %d has it", it->second.holder);
      g_blocks.erase(it);
      g_live--; g_frees++;
    }
    ::free(p);
  }
};

struct FakeEngine {
  static std::atomic<long> live, made;
  int dev;
  std::atomic<int> holder{0};
  uint64_t scratch = 0;   // (what a holder writes: a second holder is a data race here as well)
  explicit FakeEngine(int d) : dev(d) { live++; made++; }
  ~FakeEngine() { CHECK(holder.load() == 0, "an engine is deleted while holder %d has it", holder.load()); live--; }
  int device() const { return dev; }
};
std::atomic<long> FakeEngine::live{0}, FakeEngine::made{0};

zg::PinnedCache<CountingMem> g_pinned;
zg::IdleEngines<FakeEngine> g_engines;
std::atomic<bool> g_stop{false};
std::atomic<long> g_reused{0}, g_trims{0};

uint64_t next(uint64_t& s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return s >> 17; }
size_t backed(size_t n) { return n < kBacked ? n : kBacked; }
void fill(uint8_t* p, size_t n, uint64_t seed) { for (size_t i = 0; i < backed(n); i++) p[i] = (uint8_t)(next(seed) >> 3); }
bool intact(const uint8_t* p, size_t n, uint64_t seed) { for (size_t i = 0; i < backed(n); i++) if (p[i] != (uint8_t)(next(seed) >> 3)) return false; return true; }

void check_cache_state() {
  {
    std::lock_guard<std::mutex> lk(g_pinned.mu);
    size_t sum = 0;
    for (const auto& b : g_pinned.free_) sum += b.n;
    CHECK(sum == g_pinned.held, "held %zu, free_ holds %zu", g_pinned.held, sum);
    CHECK(g_pinned.held <= g_pinned.kMaxHeld, "held %zu", g_pinned.held);
  }
  std::lock_guard<std::mutex> lk(g_engines.mu);
  int per[kDevices] = {0};
  for (FakeEngine* e : g_engines.v) { CHECK(e->holder.load() == 0, "an idle engine has a holder"); per[e->dev]++; }
  for (int d = 0; d < kDevices; d++) CHECK(per[d] <= 2, "%d idle engines on device %d", per[d], d);
}

struct Mine { uint8_t* p; size_t n; uint64_t seed; };

void holder(int id) {
  uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)id;
  std::vector<Mine> mine;
  // a stream's sizes: small staging buffers, rings of some MiB in a few classes (so that blocks fit the next taker), a few huge ones (the bound)
  static const size_t classes[] = {1, 4096, 1u << 20, (1u << 20) + 4096, 4u << 20, 5u << 20, 64u << 20, 700u << 20, 1u << 30};
  for (int r = 0; r < kRounds; r++) {
    const uint64_t what = next(s) % 8;
    if (what < 3 && mine.size() < 4) {
      size_t n = classes[next(s) % (sizeof(classes) / sizeof(classes[0]))];
      if (next(s) & 1) n += next(s) % 1000;
      t_allocated = false;
      uint8_t* p = (uint8_t*)g_pinned.get(n);
      CHECK(p, "malloc failed");
      size_t real;
      {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        auto it = g_blocks.find(p);
        CHECK(it != g_blocks.end(), "get returned a block that does not exist");
        CHECK(it->second.holder == 0, "holders %d and %d have one block", it->second.holder, id);
        it->second.holder = id;
        real = it->second.n;
      }
      CHECK(real >= n && real <= n + n / 4 + (1u << 20), "asked for %zu, got a block of %zu", n, real);
      if (!t_allocated) g_reused++;
      const uint64_t seed = next(s);
      fill(p, n, seed);
      mine.push_back(Mine{p, n, seed});
    } else if (what < 6 && !mine.empty()) {
      const size_t k = next(s) % mine.size();
      const Mine m = mine[k];
      mine.erase(mine.begin() + k);
      CHECK(intact(m.p, m.n, m.seed), "holder %d: the pattern of a block of %zu bytes changed", id, m.n);
      {
        std::lock_guard<std::mutex> lk(g_reg_mu);
        auto it = g_blocks.find(m.p);
        CHECK(it != g_blocks.end() && it->second.holder == id, "holder %d lost its block", id);
        it->second.holder = 0;
      }
      g_pinned.put(m.p);
      check_cache_state();
    } else if (what == 6) {
      for (const Mine& m : mine) CHECK(intact(m.p, m.n, m.seed), "holder %d: the pattern of a block of %zu bytes changed", id, m.n);
    } else {
      const int dev = (int)(next(s) % kDevices);
      FakeEngine* e = g_engines.take(dev);
      if (!e) e = new FakeEngine(dev);
      CHECK(e->device() == dev, "take(%d) gave an engine of device %d", dev, e->device());
      const int was = e->holder.exchange(id);
      CHECK(was == 0, "holders %d and %d have one engine", was, id);
      e->scratch = next(s);
      const uint64_t mark = e->scratch;
      if (next(s) & 1) std::this_thread::yield();
      CHECK(e->scratch == mark, "an engine's scratch changed under its holder");
      e->holder.store(0);
      g_engines.give(e);
      check_cache_state();
    }
  }
  for (const Mine& m : mine) {
    CHECK(intact(m.p, m.n, m.seed), "holder %d: the pattern of a block of %zu bytes changed", id, m.n);
    { std::lock_guard<std::mutex> lk(g_reg_mu); g_blocks[m.p].holder = 0; }
    g_pinned.put(m.p);
  }
}

void trimmer() {
  uint64_t s = 77;
  while (!g_stop.load()) {
    if (next(s) & 1) g_pinned.trim(); else g_engines.trim();   // (CountingMem::free refuses a block that has a holder)
    g_trims++;
    check_cache_state();
    usleep(200 + next(s) % 800);
  }
}
}  // namespace

int main() {
  // the bound alone, on one thread: blocks of 1 GiB until put() no longer keeps them
  {
    std::vector<void*> ps;
    for (int i = 0; i < 5; i++) ps.push_back(g_pinned.get(1u << 30));
    for (void* p : ps) { g_pinned.put(p); check_cache_state(); }
    CHECK(g_pinned.held == 3ull << 30 && g_live.load() == 3, "held %zu, alive %ld", g_pinned.held, g_live.load());
    void* p = g_pinned.get((1u << 30) - (200u << 20));          // within n + n/4 + 1 MiB of a block of 1 GiB: taken from free_
    CHECK(g_allocs.load() == 5 && g_pinned.held == 2ull << 30, "a block that fits was not reused");
    void* q = g_pinned.get(512u << 20);                         // a block of 1 GiB is too large for it: a new one
    CHECK(g_allocs.load() == 6, "a block of twice the size was handed out");
    g_pinned.put(p); g_pinned.put(q);
    g_pinned.trim();
    CHECK(g_live.load() == 0 && g_pinned.held == 0 && g_pinned.sizes_.empty(), "alive after trim: %ld", g_live.load());
  }
  std::thread t9(trimmer);
  std::vector<std::thread> ts;
  for (int i = 1; i <= kHolders; i++) ts.emplace_back(holder, i);
  for (auto& t : ts) t.join();
  g_stop.store(true);
  t9.join();
  check_cache_state();
  g_pinned.trim();
  g_engines.trim();
  CHECK(g_live.load() == 0 && g_blocks.empty(), "%ld blocks alive after the last put and a trim", g_live.load());
  CHECK(g_pinned.sizes_.empty() && g_pinned.free_.empty() && g_pinned.held == 0, "the cache still lists blocks");
  CHECK(FakeEngine::live.load() == 0, "%ld engines alive after the last give and a trim", FakeEngine::live.load());
  CHECK(g_reused.load() > 0 && g_trims.load() > 0, "no block was reused or nothing was trimmed: the run tested nothing");
  printf("caches ok: %ld blocks allocated, %ld freed, %ld gets served from the cache, %ld engines made, %ld trims\n", g_allocs.load(), g_frees.load(),
         g_reused.load(), FakeEngine::made.load(), g_trims.load());
  return 0;
}
