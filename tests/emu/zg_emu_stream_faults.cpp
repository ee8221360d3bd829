// TEST-ONLY: the worker-thread fault cases of tests/test_stream_faults_cpu.py as a program of its own, so that they run under
// ThreadSanitizer and AddressSanitizer without an interpreter around them (Makefile: stream_faults_tsan, stream_faults_asan). It links
// zg_emu_stream.cpp and drives it through the same C entry points as the Python tests: a fixed list of configurations in PIPE mode, each
// once clean (calls per kind), then with the nth call of each kind failing, and the rule of include/zgpu.h (zgpu_streaming_read) checked
// after every read. Exit status 0 and "stream faults ok" when nothing was violated.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <set>
#include <string>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_xxh64.h"

extern "C" {
void* zgemu_stream_new(const uint8_t* src, size_t src_len, const uint8_t* plain, size_t plain_len, const uint32_t* out, const uint32_t* status,
                       const uint8_t* far, uint32_t nblocks, uint64_t window, int has_checksum, uint32_t checksum, uint64_t content_size,
                       uint64_t read_ahead, uint64_t pipe_after, uint32_t first_run_blocks, uint32_t copy_threads, int hash, uint64_t max_run_src,
                       int callback, size_t chunk);
void zgemu_stream_free(void* h);
int zgemu_stream_read(void* h, uint8_t* dst, size_t cap, size_t* n);
uint32_t zgemu_stream_checksum(void* h);
void zgemu_stream_stats(void* h, uint64_t* out);
void zgemu_stream_fail(void* h, int kind, uint64_t nth, int code);
void zgemu_stream_stats2(void* h, uint64_t* out);
int64_t zgemu_stream_live_allocs(void);
}

namespace {

const char* const kKinds[10] = {"prepare", "launch", "wait", "run", "commit", "fetch", "fetch_wait", "rebase", "pipe_begin", "host_alloc"};
constexpr uint32_t K = 128u << 10;

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  uint32_t below(uint32_t n) { return n ? next() % n : 0; }
};

struct Frame {
  std::vector<uint8_t> src, plain, far;
  std::vector<uint32_t> out, status;
  uint64_t window = 0;
  bool has_checksum = false;
  uint32_t checksum = 0;
};

// raw and RLE blocks (the stand-in does not decode: sizes are all that matter)
Frame make_frame(uint64_t seed, uint32_t nblocks, uint64_t window, bool has_checksum, bool small) {
  Frame f;
  Rng r{seed};
  f.window = window; f.has_checksum = has_checksum;
  for (uint32_t i = 0; i < nblocks; i++) {
    const bool last = i == nblocks - 1;
    uint32_t n;
    if (small) n = r.below(2000);
    else { const uint32_t c = r.below(4); n = c < 2 ? K : c == 2 ? 1 + r.below(K) : r.below(300); }
    if (r.below(3) == 0) {
      const uint8_t b = (uint8_t)r.next();
      const uint32_t h = (n << 3) | (1u << 1) | (last ? 1u : 0u);
      f.src.push_back((uint8_t)h); f.src.push_back((uint8_t)(h >> 8)); f.src.push_back((uint8_t)(h >> 16)); f.src.push_back(b);
      f.plain.insert(f.plain.end(), n, b);
    } else {
      const uint32_t h = (n << 3) | (last ? 1u : 0u);
      f.src.push_back((uint8_t)h); f.src.push_back((uint8_t)(h >> 8)); f.src.push_back((uint8_t)(h >> 16));
      for (uint32_t k = 0; k < n; k++) { const uint8_t b = (uint8_t)(r.next() >> 7); f.src.push_back(b); f.plain.push_back(b); }
    }
    f.out.push_back(n);
  }
  f.status.assign(nblocks, 0); f.far.assign(nblocks, 0);
  f.checksum = r.next();
  if (has_checksum) for (int k = 0; k < 4; k++) f.src.push_back((uint8_t)(f.checksum >> (8 * k)));
  return f;
}

struct Config {
  const Frame* fr;
  std::vector<size_t> reads;
  uint64_t read_ahead, pipe_after, max_run_src, content_size;
  bool hash, callback;
  size_t chunk;
  const char* name;
};

struct Result {
  uint64_t calls[10] = {};
  bool fired = false, error_seen = false;
  int bad = 0;
};

int g_bad = 0;
void violation(const Config& c, int kind, uint64_t nth, const char* what) {
  fprintf(stderr, "VIOLATION %s: %s #%llu: %s\n", c.name, kind >= 0 ? kKinds[kind] : "clean", (unsigned long long)nth, what);
  g_bad++;
}

Result run_case(const Config& c, int kind, uint64_t nth, int code) {
  const Frame& f = *c.fr;
  Result res;
  void* h = zgemu_stream_new(f.src.data(), f.src.size(), f.plain.data(), f.plain.size(), f.out.data(), f.status.data(), f.far.data(), (uint32_t)f.out.size(),
                             f.window, f.has_checksum ? 1 : 0, f.checksum, c.content_size, c.read_ahead, c.pipe_after, 1, 2, c.hash ? 1 : 0, c.max_run_src,
                             c.callback ? 1 : 0, c.chunk);
  if (!h) { violation(c, kind, nth, "no stream"); return res; }
  if (kind >= 0) zgemu_stream_fail(h, kind, nth, code);
  size_t cap_max = 3u << 20;
  for (size_t r : c.reads) if (r > cap_max) cap_max = r;
  static std::vector<uint8_t> buf;                           // (one for all cases: every read is checked against the plaintext, stale bytes cannot pass)
  if (buf.size() < cap_max) buf.resize(cap_max);
  zg::Xxh64 hash;
  hash.reset(0);
  size_t pos = 0;                                            // bytes delivered
  const size_t after[8] = {8192, 1, 0, K + 1, 3u << 20, 100, 65536, 8192};
  std::vector<size_t> todo = c.reads;
  for (size_t i = 0; i < todo.size(); i++) {
    size_t n = 12345;
    const int e = zgemu_stream_read(h, buf.data(), todo[i], &n);
    if (e) {
      if (e != code || n != 0) violation(c, kind, nth, "a read returned another code than the injected one, or bytes beside it");
      if (!res.error_seen) { res.error_seen = true; todo.resize(i + 1); todo.insert(todo.end(), after, after + 8); }
      continue;
    }
    if (res.error_seen) { violation(c, kind, nth, "a read behind the error succeeded"); continue; }
    // a clean frame: every read returns what it asked for until the frame ends (the reference's read loop), and the frame's bytes there
    const size_t want = todo[i] < f.plain.size() - pos ? todo[i] : f.plain.size() - pos;
    if (n != want) violation(c, kind, nth, "a read in front of the error returned another size than the reference's");
    if (pos + n > f.plain.size() || memcmp(buf.data(), f.plain.data() + pos, n) != 0) { violation(c, kind, nth, "bytes that are not the frame's plaintext"); break; }
    hash.update(buf.data(), n);
    pos += n;
  }
  uint64_t s1[16], s2[20];
  const uint32_t cs = zgemu_stream_checksum(h);
  zgemu_stream_stats(h, s1);
  zgemu_stream_stats2(h, s2);
  for (int k = 0; k < 10; k++) res.calls[k] = s2[k];
  res.fired = s2[10] != 0;
  zg::Xxh64 none;
  none.reset(0);
  if (cs != (uint32_t)(c.hash ? hash.digest() : none.digest())) violation(c, kind, nth, "the calculated checksum is not the hash of the delivered bytes");
  if ((uint32_t)s1[8]) violation(c, kind, nth, "the stand-in objected (wrong source bytes, a run on a run, too little kept)");
  const bool silent = kind == 8 || kind == 9;
  if (res.fired && !silent) {
    if (!res.error_seen) violation(c, kind, nth, "the fault fired and no read returned it");
    if (s2[11] || s2[12]) violation(c, kind, nth, "the engine or the source was called behind the error");
    if (s1[9]) violation(c, kind, nth, "is_finished behind an engine error");
    if (s2[13] || s2[15]) violation(c, kind, nth, "the pipe was not down when the failing read returned");
    if ((int)s2[14] != code) violation(c, kind, nth, "the stored error is not the injected one");
  } else {
    if (res.error_seen || pos != f.plain.size() || !s1[9]) violation(c, kind, nth, "a stream without an engine error did not deliver the whole frame");
    if (silent && res.fired && (s1[0] == 1 || s1[14])) violation(c, kind, nth, "the worker thread was used although it could not be set up");
  }
  const auto t0 = std::chrono::steady_clock::now();
  zgemu_stream_free(h);
  if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) violation(c, kind, nth, "freeing the stream took more than 10 s");
  if (zgemu_stream_live_allocs() != 0) violation(c, kind, nth, "a host allocation was not freed");
  return res;
}

std::vector<size_t> pattern(size_t total, size_t each) {
  std::vector<size_t> r;
  for (size_t done = 0; done <= total + 3 * K; done += each) r.push_back(each);
  r.push_back(8192); r.push_back(1);
  return r;
}

}  // namespace

int main() {
  const Frame small_cs = make_frame(1, 200, 1024, true, true), small = make_frame(2, 200, 1024, false, true);
  const Frame mixed_cs = make_frame(3, 40, K, true, false);
  const uint64_t ring = (8u << 20) + (512u << 10);
  std::vector<Config> cfgs;
  auto add = [&](const char* name, const Frame* f, std::vector<size_t> reads, bool is_small, bool hash, bool callback, size_t chunk, bool at_once) {
    Config c;
    c.fr = f; c.reads = std::move(reads); c.read_ahead = (2u << 20) + f->window; c.pipe_after = is_small ? (20u << 10) : (256u << 10);
    c.max_run_src = is_small ? (24u << 10) : (1u << 20); c.content_size = at_once ? f->plain.size() : 0;
    c.hash = hash; c.callback = callback; c.chunk = chunk; c.name = name;
    cfgs.push_back(c);
  };
  add("small/cs/callback1000/8192", &small_cs, pattern(small_cs.plain.size(), 8192), true, true, true, 1000, false);
  add("small/slice/nohash/1000", &small, pattern(small.plain.size(), 1000), true, false, false, 0, false);
  add("mixed/cs/slice/32768", &mixed_cs, pattern(mixed_cs.plain.size(), 32768), false, true, false, 0, false);
  add("mixed/cs/callback1000/one-read", &mixed_cs, std::vector<size_t>{(size_t)ring + (1u << 20) + 3, 8192, 1}, false, true, true, 1000, true);
  int cases = 0, unfired = 0, turn = 0;
  for (const Config& c : cfgs) {
    const Result clean = run_case(c, -1, 0, 0);
    for (int kind = 0; kind < 10; kind++) {
      const uint64_t n = clean.calls[kind];
      std::set<uint64_t> ords;
      if (n <= 6) for (uint64_t k = 1; k <= n; k++) ords.insert(k);
      else ords = {1, 2, 3, (n + 1) / 2, n - 1, n};
      for (uint64_t nth : ords) {
        const Result r = run_case(c, kind, nth, 90 + (turn++ % 3));
        cases++;
        if (!r.fired) unfired++;
      }
    }
  }
  if (unfired * 10 > cases) { fprintf(stderr, "VIOLATION: %d of %d faults were not reached\n", unfired, cases); g_bad++; }
  if (g_bad) { fprintf(stderr, "%d violations\n", g_bad); return 1; }
  printf("stream faults ok: %d cases, %d not reached\n", cases, unfired);
  return 0;
}
