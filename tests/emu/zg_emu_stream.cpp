// TEST-ONLY: the host side of the streaming decoder (zstd-rs_amd/csrc/zg_stream.h: source handling, runs decoded ahead, the worker /
// hasher / copy threads, the ring, the fall back to the reference's block-by-block schedule) on the CPU, against a TABLE-DRIVEN
// stand-in for the engine. The stand-in knows the frame's plaintext and, per block, how many bytes it yields, whether it fails and
// whether it "sets an offset beyond the window" (tests choose these freely): a run reports what the engine would report for those
// blocks, and checks that the bytes it is handed ARE those blocks. Not part of the product, nothing here is a decoder.
// It can also FAIL: zgemu_stream_fail makes the nth call of one kind return an engine error without doing its work (a fetch queues no
// copy, a fetch_wait copies nothing, a host_alloc returns null), and zgemu_stream_stats2 tells what the core did about it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_stream.h"

using namespace zg;

namespace {

struct Table {
  std::vector<uint8_t> src;            // the frame behind its header: block headers + bodies (+ checksum)
  std::vector<uint8_t> plain;
  std::vector<uint32_t> out;           // bytes block i yields
  std::vector<uint32_t> status;        // != 0: block i fails with this
  std::vector<uint8_t> far;            // block i sets an offset beyond the window
  std::vector<size_t> off, end;        // block i's header .. body end in src
  std::vector<uint64_t> out_off;
  bool has_checksum = false;
  uint32_t checksum = 0;
};

enum FaultKind { F_PREPARE = 0, F_LAUNCH, F_WAIT, F_RUN, F_COMMIT, F_FETCH, F_FETCH_WAIT, F_REBASE, F_PIPE_BEGIN, F_HOST_ALLOC, F_KINDS };
std::atomic<int64_t> g_live_allocs{0};   // host_alloc without its host_free, over all streams of the process

class TableBackend : public StreamBackend {
 public:
  Table* t;
  // the one fault of this stream: the nth call (1-based) of fault_kind returns fault_code. Calls come from the reader's thread and from
  // the worker's, so everything here is atomic.
  int fault_kind = -1;
  uint64_t fault_nth = 0;
  int fault_code = 0;
  std::atomic<uint64_t> calls[F_KINDS] = {};
  std::atomic<bool> fired{false};
  std::atomic<uint64_t> calls_after{0};  // calls of the ten kinds that came after the fault had been returned
  std::atomic<int64_t> live{0};
  bool hit(int kind) {
    const uint64_t n = calls[kind].fetch_add(1, std::memory_order_relaxed) + 1;
    if (fired.load(std::memory_order_acquire)) { calls_after.fetch_add(1, std::memory_order_relaxed); return false; }
    if (kind != fault_kind || n != fault_nth) return false;
    fired.store(true, std::memory_order_release);
    return true;
  }
  uint32_t next = 0;                   // first block that is not committed yet
  uint64_t produced = 0;
  // the run in flight
  bool have_run = false;
  uint32_t run_blocks = 0, run_good = 0;
  uint64_t run_out = 0;
  uint64_t committed_off = 0;
  struct Pending { uint8_t* dst; uint64_t off, n; };
  std::vector<Pending> pend;
  // what the tests look at
  uint64_t nruns = 0, ncommits = 0, ndiscards = 0, nrebase = 0, rebase_bytes = 0, bad_src = 0, max_keep_gap = 0, pipe_begins = 0;
  uint64_t window = 0;
  bool in_pipe = false;
  uint64_t last_reason = 0;
  void obj(uint64_t why) { bad_src++; last_reason = why; }

  // prepare / launch / wait like the engine's backend: one run may be prepared while another is "on the device"
  const uint8_t* p_src = nullptr; size_t p_len = 0; uint32_t p_nblocks = 0; bool have_prep = false;
  StreamRun cur;
  bool launched = false;
  int run(const uint8_t* src, size_t len, uint32_t nblocks, uint64_t keep, StreamRun* out) override {
    if (hit(F_RUN)) return fault_code;
    return StreamBackend::run(src, len, nblocks, keep, out);
  }
  int prepare(const uint8_t* src, size_t len, uint32_t nblocks) override {
    if (hit(F_PREPARE)) return fault_code;
    if (have_prep) obj(7);
    p_src = src; p_len = len; p_nblocks = nblocks; have_prep = true;
    return ZG_OK;
  }
  void drop_prepared() override { have_prep = false; }
  int launch(uint64_t keep) override {
    if (hit(F_LAUNCH)) return fault_code;
    if (!have_prep) { obj(8); return ZG_INTERNAL; }
    have_prep = false;
    const int e = run_now(p_src, p_len, p_nblocks, keep, &cur);
    launched = e == ZG_OK;
    return e;
  }
  int wait(StreamRun* o) override {
    if (hit(F_WAIT)) return fault_code;
    if (!launched) { obj(9); return ZG_INTERNAL; }
    launched = false;
    *o = cur;
    return ZG_OK;
  }
  int run_now(const uint8_t* src, size_t len, uint32_t nblocks, uint64_t keep, StreamRun* o) {
    nruns++;
    if (have_run) obj(1);                                               // a run must be committed or dropped before the next one
    if (next + nblocks > t->out.size() || nblocks == 0) { obj(2); return ZG_INTERNAL; }
    // the bytes must be exactly those blocks (+ the checksum behind the frame's last block, if it is there)
    const size_t b0 = t->off[next], b1 = t->end[next + nblocks - 1];
    const bool is_last = (t->src[t->off[next + nblocks - 1]] & 1u) != 0;   // the Last_Block bit of the run's last block header
    const size_t want = b1 - b0;
    if (!(len == want || (is_last && t->has_checksum && len == want + 4)) || memcmp(src, t->src.data() + b0, len) != 0) obj(3);
    // what must stay in reach: at least the window (or everything there is)
    const uint64_t need = produced < window ? produced : window;
    if (keep < need) obj(4);
    o->nblocks = nblocks; o->status = 0; o->good_blocks = nblocks; o->far = false; o->out_size = 0;
    for (uint32_t i = 0; i < nblocks; i++) {
      if (t->far[next + i]) o->far = true;                              // (the engine's flag covers the whole run, also behind a failing block)
      if (!o->status && t->status[next + i]) { o->status = (int)t->status[next + i]; o->good_blocks = i; }
      if (!o->status) o->out_size += t->out[next + i];
    }
    o->saw_last = is_last && !o->status;
    o->has_checksum = o->saw_last && t->has_checksum && len == want + 4;
    o->checksum = o->has_checksum ? t->checksum : 0;
    have_run = true; run_blocks = nblocks; run_good = o->good_blocks; run_out = o->out_size;
    return ZG_OK;
  }

  int commit() override {
    if (hit(F_COMMIT)) return fault_code;
    if (!have_run) { obj(5); return ZG_INTERNAL; }
    have_run = false; ncommits++;
    committed_off = t->out_off[next];
    next += run_good; produced += run_out;
    return ZG_OK;
  }
  void discard() override { if (have_run) ndiscards++; have_run = false; }
  int fetch(uint8_t* dst, uint64_t off, uint64_t n) override {           // lands at fetch_wait, like a DMA
    if (hit(F_FETCH)) return fault_code;
    pend.push_back(Pending{dst, off, n});
    return ZG_OK;
  }
  int fetch_wait() override {
    if (hit(F_FETCH_WAIT)) return fault_code;
    for (const Pending& p : pend) memcpy(p.dst, t->plain.data() + committed_off + p.off, p.n);
    pend.clear();
    return ZG_OK;
  }
  int rebase(const uint8_t* held, uint64_t n) override {
    if (hit(F_REBASE)) return fault_code;
    nrebase++; rebase_bytes = n;
    if (n > produced || memcmp(held, t->plain.data() + produced - n, n) != 0) obj(6);
    return ZG_OK;
  }
  int pipe_begin(uint64_t) override {
    if (hit(F_PIPE_BEGIN)) return fault_code;
    pipe_begins++; in_pipe = true; pipe_ends_owed++;
    return ZG_OK;
  }
  void pipe_end() override { in_pipe = false; pipe_ends_owed = 0; }
  uint64_t pipe_ends_owed = 0;         // a pipe_begin that succeeded and has not seen its pipe_end
  void* host_alloc(size_t n) override {
    if (hit(F_HOST_ALLOC)) return nullptr;
    void* p = malloc(n);
    if (p) { live.fetch_add(1, std::memory_order_relaxed); g_live_allocs.fetch_add(1, std::memory_order_relaxed); }
    return p;
  }
  void host_free(void* p, size_t) override {
    if (p) { live.fetch_sub(1, std::memory_order_relaxed); g_live_allocs.fetch_sub(1, std::memory_order_relaxed); }
    free(p);
  }
};

struct Harness {
  Table t;
  TableBackend be;
  StreamCore* core = nullptr;
  // callback source
  size_t cb_pos = 0, cb_chunk = 0;
  uint64_t cb_calls = 0;
  bool err_returned = false;           // a read() has returned the injected code to the caller
  uint64_t cb_after = 0;               // source callbacks behind that
  uint64_t cb_after_fault = 0;         // source callbacks after the backend had returned the fault (the worker's faults race with the reader's pulls)
};

size_t cb_read(void* user, uint8_t* dst, size_t n) {
  Harness* h = (Harness*)user;
  h->cb_calls++;
  if (h->err_returned) h->cb_after++;
  if (h->be.fired.load(std::memory_order_acquire)) h->cb_after_fault++;
  size_t k = h->t.src.size() - h->cb_pos;
  if (k > n) k = n;
  if (h->cb_chunk && k > h->cb_chunk) k = h->cb_chunk;                  // a source that returns short reads
  memcpy(dst, h->t.src.data() + h->cb_pos, k);
  h->cb_pos += k;
  return k;
}

}  // namespace

extern "C" {

// src: the frame behind its header (it may be cut off, or have bytes of something else behind it: src_len says how much the SOURCE
// yields; the table describes the blocks that are whole). callback != 0: an io::Read source that returns at most chunk bytes per call.
void* zgemu_stream_new(const uint8_t* src, size_t src_len, const uint8_t* plain, size_t plain_len, const uint32_t* out, const uint32_t* status,
                       const uint8_t* far, uint32_t nblocks, uint64_t window, int has_checksum, uint32_t checksum, uint64_t content_size,
                       uint64_t read_ahead, uint64_t pipe_after, uint32_t first_run_blocks, uint32_t copy_threads, int hash, uint64_t max_run_src,
                       int callback, size_t chunk) {
  Harness* h = new Harness();
  h->t.src.assign(src, src + src_len);
  h->t.plain.assign(plain, plain + plain_len);
  h->t.out.assign(out, out + nblocks); h->t.status.assign(status, status + nblocks); h->t.far.assign(far, far + nblocks);
  h->t.has_checksum = has_checksum != 0; h->t.checksum = checksum;
  size_t p = 0;
  uint64_t oo = 0;
  for (uint32_t i = 0; i < nblocks; i++) {
    BlockHeader bh;
    if (p + 3 > src_len || read_block_header(src + p, &bh) || p + 3 + bh.content_size > src_len) { delete h; return nullptr; }
    h->t.off.push_back(p); p += 3 + bh.content_size; h->t.end.push_back(p);
    h->t.out_off.push_back(oo); oo += out[i];
  }
  h->be.t = &h->t; h->be.window = window;
  StreamOpts o;
  o.read_ahead = read_ahead; o.hash = hash != 0;
  if (pipe_after) o.pipe_after = pipe_after;
  if (first_run_blocks) o.first_run_blocks = first_run_blocks;
  o.copy_threads = copy_threads;
  if (max_run_src) o.max_run_src = max_run_src;
  if (const char* e = getenv("ZGEMU_FAIL_THREAD")) o.test_fail_thread = (uint32_t)atoi(e);
  h->core = new StreamCore(&h->be, o);
  h->core->window = window; h->core->content_size = content_size; h->core->header_bytes = 0;
  h->core->src.has_checksum = has_checksum != 0;
  if (callback) { h->core->src.read = cb_read; h->core->src.user = h; h->cb_chunk = chunk; }
  else { h->core->src.slice = h->t.src.data(); h->core->src.slice_len = h->t.src.size(); }
  return h;
}
void zgemu_stream_free(void* hp) { Harness* h = (Harness*)hp; if (!h) return; delete h->core; delete h; }
int zgemu_stream_read(void* hp, uint8_t* dst, size_t cap, size_t* n) {
  Harness* h = (Harness*)hp;
  const int e = h->core->read(dst, cap, n);
  if (e && h->be.fired.load() && e == h->be.fault_code) h->err_returned = true;
  return e;
}
// One fault per stream, set before the first read: the nth call (1-based) of `kind` — 0 prepare, 1 launch, 2 wait, 3 run (the three in one,
// as the caller's thread uses them), 4 commit, 5 fetch, 6 fetch_wait, 7 rebase, 8 pipe_begin, 9 host_alloc — returns `code` and does
// nothing (host_alloc: returns null).
void zgemu_stream_fail(void* hp, int kind, uint64_t nth, int code) {
  Harness* h = (Harness*)hp;
  h->be.fault_kind = kind; h->be.fault_nth = nth; h->be.fault_code = code;
}
// out: [0..9] calls per kind (as above) [10] the fault fired [11] calls of these kinds that the backend got after it had returned the fault
// [12] source callbacks after a read() had returned the fault's code to the caller (the worker meets a fault while the reader may be
// taking a run from the source: what counts is what happens once the caller knows) [13] host allocations of this stream still live
// [14] the engine error the core has stored [15] a pipe_begin still waits for its pipe_end [16] source callbacks after the backend had
// returned the fault (0 whenever the fault was met on the caller's thread). out holds 20 values.
void zgemu_stream_stats2(void* hp, uint64_t* out) {
  Harness* h = (Harness*)hp;
  for (int k = 0; k < F_KINDS; k++) out[k] = h->be.calls[k].load();
  out[10] = h->be.fired.load() ? 1u : 0u;
  out[11] = h->be.calls_after.load();
  out[12] = h->cb_after;
  out[13] = (uint64_t)h->be.live.load();
  out[14] = (uint64_t)h->core->error();
  out[15] = h->be.pipe_ends_owed;
  out[16] = h->cb_after_fault; out[17] = out[18] = out[19] = 0;
}
int64_t zgemu_stream_live_allocs(void) { return g_live_allocs.load(); }   // over all streams, freed ones included: 0 when every host_alloc had its host_free
uint32_t zgemu_stream_checksum(void* hp) { return ((Harness*)hp)->core->calculated_checksum(); }
// out: [0] mode [1] runs taken [2] runs dropped [3] backend runs [4] commits [5] discards [6] rebases [7] bytes the source has given
// [8] things the stand-in objected to (wrong source bytes, a run on top of a run, too little kept) [9] is_finished [10] blocks decoded
// [11] bytes_read_from_source [12] checksum from data present [13] its value [14] pipe begins [15] source callbacks
void zgemu_stream_stats(void* hp, uint64_t* out) {
  Harness* h = (Harness*)hp;
  StreamCore* c = h->core;
  uint32_t cs = 0;
  const bool hc = c->checksum_from_data(&cs);
  const uint64_t v[16] = {(uint64_t)c->mode(), c->runs(), c->dropped_runs(), h->be.nruns, h->be.ncommits, h->be.ndiscards, h->be.nrebase,
                          c->src.is_slice() ? (uint64_t)c->src.slice_pos : (uint64_t)h->cb_pos, h->be.bad_src | (h->be.last_reason << 32), c->is_finished() ? 1u : 0u,
                          c->blocks_decoded(), c->bytes_read_from_source(), hc ? 1u : 0u, cs, h->be.pipe_begins, h->cb_calls};
  memcpy(out, v, sizeof v);
}

}  // extern "C"

// StreamCopyPool on its own: every size around the share boundaries with 1..4 helpers; returns the number of sizes that copied wrong
extern "C" int zgemu_pool_selftest(uint32_t seed) {
  int bad = 0;
  std::vector<uint8_t> src(12u << 20), dst(12u << 20);
  uint32_t x = seed * 2654435761u + 1u;
  for (auto& b : src) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
  for (uint32_t nt = 1; nt <= 4; nt++) {
    StreamCopyPool pool;
    pool.start(nt);
    for (uint32_t k = 0; k < 160; k++) {
      x = x * 1664525u + 1013904223u;
      const size_t unit = (size_t)((x >> 8) % 600 + 128) * 4096;            // a page-aligned share ...
      for (int d = -2; d <= 2; d++) {                                       // ... times (nt + 1), and a few bytes around it
        const size_t n = unit * (nt + 1) + (size_t)(d + 2);
        if (n > src.size()) continue;
        memset(dst.data(), 0, n);
        pool.copy(dst.data(), src.data(), n);
        if (memcmp(dst.data(), src.data(), n) != 0) bad++;
      }
    }
    pool.stop();
  }
  return bad;
}
