// zg_frames.cpp — zgpu_decode_frames (include/zgpu.h): n independent buffers, each what FrameDecoder::decode_all (frame_decoder.rs:541-577)
// would take, decoded in few submits, with a verdict per buffer and the content checksums of the frames it held.
//
// Every entry is walked on its own (parse_frames, decode_all's rule: the first header that cannot be read ends the walk of THAT entry) and its
// frames are appended to one submit (Engine::prepare_entries); frames decode independently on the device, so an entry's verdict is
// zgpu_decode_all's logic applied to its own frames: a device error in them, else its walk error, else TargetTooSmall, else success.
// Entries the one-submit path does not serve as zgpu_decode_all would (dictionary frames; Unsupported / Internal) are decoded again on their
// own after the submit. Submits hold at most kFramesSubmitBytes of plaintext (bounded from the block headers); an entry is never split.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <thread>
#include <utility>
#include <vector>
#include "zg_capi_int.h"
#include "zg_xxh64_dev.h"

using namespace zg;

namespace {

// plaintext per submit: bounds the device output (+ 4x its size of flatten scratch) and the pinned staging of one submit
constexpr uint64_t kFramesSubmitBytes = 512ull << 20;
// Where a submit's frames are hashed (LABNOTES.md "decode_frames", measured on MI355X): on the device one lane runs XXH64 at ~225 MB/s (a lone
// 4 MiB frame: 18.6 ms), all lanes together at ~1 TB/s (65,536 x 128 KiB: 8.6 ms); a host core at >= 10 GB/s, and the host copies every byte
// to the caller anyway, on up to kHostThreads threads. A submit's frames go to the device only when the estimate of the kernel —
// max(longest frame / lane rate, all bytes / device rate) — beats the estimate of hashing them on the host threads, and never a frame longer
// than kHashDeviceMax. Many short frames go to the device; a lone frame, or a few long ones, stay on the host.
constexpr uint64_t kHashDeviceMax = 4ull << 20;
constexpr double kLaneBytesPerUs = 225.0, kDeviceBytesPerUs = 1.0e6, kHostBytesPerUs = 1.0e4, kLaunchUs = 50.0;
constexpr unsigned kHostThreads = 16;

unsigned host_threads() {
  const unsigned t = std::thread::hardware_concurrency();
  return t == 0 ? 1u : t > kHostThreads ? kHostThreads : t;
}

// the frames of `cand` (lengths len[f]) hashed on the device: all of them, if the estimate says the kernel is faster than the host threads
bool hash_on_device(const std::vector<uint32_t>& cand, const std::vector<ZgFrameOut>& fo) {
  uint64_t longest = 0, total = 0;
  for (uint32_t f : cand) { longest = fo[f].out_size > longest ? fo[f].out_size : longest; total += fo[f].out_size; }
  if (cand.empty()) return false;
  const double dev = kLaunchUs + (longest / kLaneBytesPerUs > total / kDeviceBytesPerUs ? longest / kLaneBytesPerUs : total / kDeviceBytesPerUs);
  const double th = total / (kHostBytesPerUs * host_threads()), t1 = longest / kHostBytesPerUs;   // (a frame is hashed by one thread)
  const double host = th > t1 ? th : t1;
  return dev < host;
}

// f(i) for i in [0, n) on up to kHostThreads threads (the caller's included), about one per `grain` bytes of work
template <class F> void parallel_for(uint32_t n, uint64_t work, uint64_t grain, F f) {
  unsigned t = host_threads();
  const uint64_t want = work / grain + 1;
  if (t > want) t = (unsigned)want;
  if (t > n) t = n ? n : 1;
  std::atomic<uint32_t> next{0};
  auto body = [&]() { for (uint32_t i; (i = next.fetch_add(1)) < n;) f(i); };
  std::vector<std::thread> th;
  for (unsigned k = 1; k < t; k++) {
    try { th.emplace_back(body); } catch (...) { break; }
  }
  body();
  for (std::thread& x : th) x.join();
}

// host memory for one submit's staging: pinned from the process-wide cache when it can be had, else pageable
struct Staging {
  uint8_t* p = nullptr;
  bool pinned = false;
  int get(size_t n) {
    p = (uint8_t*)zg_pinned_get(n ? n : 1);
    pinned = p != nullptr;
    if (!p) p = (uint8_t*)malloc(n ? n : 1);
    return p ? ZGPU_OK : ZGPU_E_NOMEM;
  }
  ~Staging() { if (p) { if (pinned) zg_pinned_put(p); else free(p); } }
};

struct Call {
  zgpu_ctx* c;
  const uint8_t* const* srcs;
  const size_t* lens;
  uint8_t* const* dsts;
  const size_t* caps;
  zgpu_entry_result* res;
  bool hash_forced;                                // (development build, ZGPU_HASH_DEVICE_MAX) frames up to hash_max on the device, no estimate
  uint64_t hash_max;
  std::vector<std::pair<uint32_t, bool>> again;   // entries decoded again on their own after the submits (true: the walk met a dictionary frame)
};

// one submit: the entries idx[0 .. n)
int run_submit(Call& k, const uint32_t* idx, uint32_t n) {
  std::vector<uint64_t> off(n), len(n);
  uint64_t total_in = 0;
  for (uint32_t j = 0; j < n; j++) { off[j] = total_in; len[j] = k.lens[idx[j]]; total_in += len[j]; }
  Staging in;
  int st = in.get(total_in);
  if (st) return st;
  parallel_for(n, total_in, 8u << 20, [&](uint32_t j) { if (len[j]) memcpy(in.p + off[j], k.srcs[idx[j]], len[j]); });
  Batch* b = nullptr;
  std::vector<int> walk;
  std::vector<uint32_t> ff;
  if ((st = k.c->eng->prepare_entries(in.p, total_in, off.data(), len.data(), n, &b, &walk, &ff))) return st;
  b->drain_rule = ZG_DRAIN_DECODE_ALL;   // (as zgpu_decode_all: decode_all drains its DecodeBuffer every MiB, zg_exact.h)
  if ((st = b->run()) || (st = b->sync())) { delete b; return st; }
  const std::vector<ZgFrameOut>& fo = b->frame_out;
  if (fo.size() != b->info.size()) { delete b; return ZGPU_E_INTERNAL; }

  // verdicts (zgpu_decode_all, zg_capi.cpp, on the entry's own frames)
  std::vector<uint32_t> dev_hash;   // frames hashed on the device
  uint64_t down = 0;                // output bytes the host needs (of entries that succeed)
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t i = idx[j];
    zgpu_entry_result& r = k.res[i];
    if (walk[j] == ZGPU_E_DICT_NOT_PROVIDED && !k.c->dicts.empty()) { k.again.push_back({i, true}); continue; }   // zgpu_decode_all's frame-by-frame path
    int dev = 0;
    uint64_t bytes = 0;
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      if (!dev && fo[f].status) dev = (int)fo[f].status;
      bytes += fo[f].out_size;
    }
    if (dev == ZGPU_E_UNSUPPORTED || dev == ZGPU_E_INTERNAL) { k.again.push_back({i, false}); continue; }
    r.status = dev ? dev : walk[j] ? walk[j] : bytes > k.caps[i] ? ZGPU_E_TARGET_TOO_SMALL : ZGPU_OK;
    if (r.status) continue;
    r.written = bytes;
    r.nframes = ff[j + 1] - ff[j];
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      if (fo[f].out_size <= k.hash_max) dev_hash.push_back(f);   // (candidates)
      const uint64_t e = fo[f].out_base + fo[f].out_size;
      if (e > down) down = e;
    }
  }
  if (!k.hash_forced && !hash_on_device(dev_hash, fo)) dev_hash.clear();
  std::vector<uint8_t> on_dev(fo.size(), 0);
  for (uint32_t f : dev_hash) on_dev[f] = 1;
  // the device hashes its frames while the output comes back
  if ((st = b->hash_launch(dev_hash.data(), (uint32_t)dev_hash.size()))) { delete b; return st; }
  Staging out;
  if ((st = out.get(down)) || (st = b->read_output(0, out.p, down))) { delete b; return st; }
  std::vector<uint64_t> digest(fo.size(), 0);
  {
    std::vector<uint64_t> dh(dev_hash.size());
    if ((st = b->hash_wait(dh.data()))) { delete b; return st; }
    for (size_t q = 0; q < dev_hash.size(); q++) digest[dev_hash[q]] = dh[q];
  }
  // bytes to the callers' buffers; the long frames hashed here, from those bytes
  parallel_for(n, down, 4u << 20, [&](uint32_t j) {
    zgpu_entry_result& r = k.res[idx[j]];
    if (r.status || r.nframes == 0 || walk[j] == ZGPU_E_DICT_NOT_PROVIDED) return;
    uint8_t* d = k.dsts[idx[j]];
    uint64_t at = 0;
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      const uint8_t* s = out.p + fo[f].out_base;
      if (fo[f].out_size) memcpy(d + at, s, fo[f].out_size);
      at += fo[f].out_size;
      if (!on_dev[f]) digest[f] = zgx::xxh64(s, fo[f].out_size, 0);
    }
  });
  for (uint32_t j = 0; j < n; j++) {
    zgpu_entry_result& r = k.res[idx[j]];
    if (r.status || r.nframes == 0) continue;
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      const FrameInfo& fi = b->info[f];
      const uint32_t calc = (uint32_t)digest[f];
      if (f == ff[j]) { r.checksum_from_data = fi.has_checksum ? fi.checksum : 0u; r.calculated_checksum = calc; }
      if (fi.has_checksum) { r.checksums++; if (fi.checksum != calc) r.checksum_mismatches++; }
    }
  }
  delete b;
  return ZGPU_OK;
}

// an entry the submit did not serve: zgpu_decode_all on it alone (its dictionary frames go frame by frame through the FrameDecoder mirror,
// which also hashes what it hands out)
int decode_alone(Call& k, uint32_t i, bool dict_walk) {
  zgpu_entry_result& r = k.res[i];
  memset(&r, 0, sizeof r);
  ZgFrameSums sums;
  size_t w = 0;
  int st;
  bool sums_ok = true;
  if (dict_walk) {
    // (what zgpu_decode_all does with this entry: its walk meets a dictionary frame, and dictionaries are registered)
    st = zg_decode_all_per_frame(k.c, k.srcs[i], k.lens[i], k.dsts[i], k.caps[i], &w, &sums);
  } else {
    st = zgpu_decode_all(k.c, k.srcs[i], k.lens[i], k.dsts[i], k.caps[i], &w);
    if (!st) {
      // (Unsupported / Internal in a larger submit, but not alone — never seen; the status stays zgpu_decode_all's.) The checksums come from a
      // second, frame-by-frame pass into a buffer of its own; should that pass fail or disagree, the entry reports none rather than a wrong one.
      size_t w2 = 0;
      uint8_t* tmp = (uint8_t*)malloc(w ? w : 1);
      if (!tmp) return ZGPU_E_NOMEM;
      const int s2 = zg_decode_all_per_frame(k.c, k.srcs[i], k.lens[i], tmp, w, &w2, &sums);
      sums_ok = s2 == ZGPU_OK && w2 == w && (w == 0 || memcmp(tmp, k.dsts[i], w) == 0);
      free(tmp);
      if (s2 == ZGPU_E_NOMEM || s2 == ZGPU_E_HIP) return s2;
    }
  }
  if (st == ZGPU_E_NOMEM || st == ZGPU_E_HIP) return st;
  r.status = st;
  if (st) return ZGPU_OK;
  if (!sums_ok) {   // the frames are counted from their headers; no checksum is reported
    std::vector<FrameSpan> sp;
    (void)split_frames(k.srcs[i], k.lens[i], &sp);
    r.written = w;
    for (const FrameSpan& x : sp) r.nframes += x.skippable ? 0u : 1u;
    return ZGPU_OK;
  }
  r.written = w;
  r.nframes = sums.nframes; r.checksums = sums.checksums; r.checksum_mismatches = sums.mismatches;
  r.checksum_from_data = sums.first_data; r.calculated_checksum = sums.first_calc;
  return ZGPU_OK;
}

}  // namespace

extern "C" int zgpu_decode_frames(zgpu_ctx* c, const uint8_t* const* srcs, const size_t* lens, uint32_t n, uint8_t* const* dsts, const size_t* caps,
                                  zgpu_entry_result* results) {
  if (!c || (n && (!srcs || !lens || !dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  const Tuning& tn = c->eng->tuning();
  Call k{c, srcs, lens, dsts, caps, results, tn.hash_device_max_set, tn.hash_device_max_set ? tn.hash_device_max : kHashDeviceMax, {}};
  const uint64_t S = tn.frames_submit_bytes ? tn.frames_submit_bytes : kFramesSubmitBytes;
  c->frames_submits = 0;
  std::vector<uint32_t> group;
  uint64_t in_group = 0, in_bytes = 0;   // plaintext bound and input bytes of the submit being gathered (both bounded by S)
  int st = ZGPU_OK;
  for (uint32_t i = 0; i <= n && !st; i++) {
    uint64_t bound = 0;
    if (i < n) {
      memset(&results[i], 0, sizeof results[i]);
      if ((!srcs[i] && lens[i]) || (!dsts[i] && caps[i])) { results[i].status = ZGPU_E_BAD_ARG; continue; }   // (what zgpu_decode_all returns)
      bound = plaintext_bound(srcs[i], lens[i]);
    }
    // the submit is full (or this is the end): run it. An entry larger than S is a submit of its own. (The input is bounded too: entries that
    // yield nothing — skippable frames, garbage — still travel to the device, through the pinned staging.)
    if (!group.empty() && (i == n || in_group + bound > S || in_bytes + lens[i] > S)) {
      st = run_submit(k, group.data(), (uint32_t)group.size());
      c->frames_submits++;
      group.clear();
      in_group = 0; in_bytes = 0;
    }
    if (i < n) { group.push_back(i); in_group += bound; in_bytes += lens[i]; }
  }
  for (size_t q = 0; q < k.again.size() && !st; q++) st = decode_alone(k, k.again[q].first, k.again[q].second);
  return st;
}

extern "C" uint64_t zgpu_plaintext_bound(const uint8_t* src, size_t len) { return src || !len ? plaintext_bound(src, len) : 0; }
extern "C" uint32_t zgpu_debug_frames_submits(const zgpu_ctx* c) { return c ? c->frames_submits : 0u; }
