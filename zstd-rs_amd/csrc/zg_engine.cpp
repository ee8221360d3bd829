// zg_engine.cpp — see zg_engine.h. Compiled by hipcc as host code.
#include "zg_engine.h"
#include <stdlib.h>
#include <algorithm>
#include <string.h>

namespace zg {

#define ZG_HIP(call)                                  \
  do {                                                \
    hipError_t e_ = (call);                           \
    if (e_ != hipSuccess) return eng->fail(e_, #call); \
  } while (0)

#ifdef ZG_DEV_SWITCHES
static int g_poison = -1;
static uint64_t g_poisoned = 0;          // (submits are prepared by one thread at a time per process in the tests that read it: a diagnostic)
uint64_t Poison::scratch_cap = 0;
int Poison::value() { return g_poison; }
void Poison::set(int v) { g_poison = v; }
void Poison::fill(void* p, size_t n, hipStream_t s) {
  if (g_poison < 0 || !p || !n) return;
  if (hipMemsetAsync(p, g_poison, n, s) == hipSuccess) g_poisoned += n;
}
void Poison::fill_now(void* p, size_t n) {
  if (g_poison < 0 || !p || !n) return;
  if (hipMemset(p, g_poison, n) == hipSuccess && hipDeviceSynchronize() == hipSuccess) g_poisoned += n;
}
void Poison::begin_submit() { g_poisoned = 0; }
uint64_t Poison::bytes() { return g_poisoned; }
#endif

int DevBuf::reserve(size_t n, bool keep, hipStream_t s) {
  if (n <= cap && p) return 0;
  size_t ncap = n < 256 ? 256 : n;
  // a buffer that grows again: amortise, but by no more than 256 MiB (the large ones are sized exactly by their callers)
  if (p) { const size_t slack = cap / 2 < (256u << 20) ? cap / 2 : (256u << 20); if (ncap < cap + slack) ncap = cap + slack; }
  if (p && !(keep && cap)) { (void)hipFree(p); p = nullptr; cap = 0; }   // nothing to keep: free first (old + new need not fit together)
  void* np = nullptr;
  if (hipMalloc(&np, ncap) != hipSuccess) { (void)hipGetLastError(); return ZG_NOMEM; }   // (the failure must not stay behind as the runtime's last error: the next launch check would report it)
  if (p) {
    if (hipMemcpyAsync(np, p, cap, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
      (void)hipFree(np);
      return ZG_HIP_ERROR;
    }
    (void)hipFree(p);
  }
  p = np;
  cap = ncap;
  return 0;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}

int SidePass::reserve(size_t bytes) {
  const int st = buf.reserve(bytes);
  if (st) return st;
  Poison::fill_now(buf.p, buf.cap);   // (every site uploads and launches behind its reserve, and has waited for the pass in front)
  for (hipEvent_t& e : ev) if (!e && hipEventCreate(&e) != hipSuccess) return ZG_HIP_ERROR;
  return 0;
}
hipError_t SidePass::upload(const void* a, size_t ab, const void* b, size_t bb, hipStream_t s) const {
  const hipError_t e = hipMemcpyAsync(buf.p, a, ab, hipMemcpyHostToDevice, s);
  return e != hipSuccess || !bb ? e : hipMemcpyAsync(at<uint8_t>(ab), b, bb, hipMemcpyHostToDevice, s);
}
hipError_t SidePass::end(hipStream_t s) const {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : hipEventRecord(ev[1], s);
}
// the time between two recorded events in microseconds, rounded; *us is left alone on an error
static hipError_t us_between(hipEvent_t a, hipEvent_t b, uint64_t* us) {
  float ms = 0;
  const hipError_t e = hipEventElapsedTime(&ms, a, b);
  if (e == hipSuccess) *us = (uint64_t)(ms * 1000.0f + 0.5f);
  return e;
}
hipError_t SidePass::elapsed_us(uint64_t* us) const { return us_between(ev[0], ev[1], us); }
void SidePass::release(int device) {
  if (buf.p && device >= 0) (void)hipSetDevice(device);
  buf.release();
  for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  n = 0;
}

int Scratch::init_events() {
  if (have_events) return 0;
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return ZG_HIP_ERROR;
  for (auto& e : ev_huf)
    if (hipEventCreate(&e) != hipSuccess) return ZG_HIP_ERROR;
  if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) return ZG_HIP_ERROR;
  if (hipEventCreateWithFlags(&ev_fork3, hipEventDisableTiming) != hipSuccess) return ZG_HIP_ERROR;
  if (hipEventCreateWithFlags(&ev_up, hipEventDisableTiming) != hipSuccess) return ZG_HIP_ERROR;
  for (auto& e : ev_sw)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ZG_HIP_ERROR;
  for (auto& e : ev_flat)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ZG_HIP_ERROR;
  have_events = true;
  return 0;
}
void Scratch::release_but_output() {
  DevBuf* all[] = {&d_src, &d_aux, &d_fparsed, &d_slot_log, &d_fse, &d_huf, &d_hufmax, &d_lit, &d_seq, &d_og, &d_raw};
  for (DevBuf* b : all) b->release();
}
template <class F> void Scratch::each_buf(F f) {
  DevBuf* all[] = {&d_src, &d_blocks, &d_frames, &d_aux, &d_fparsed, &d_slot_log, &d_fse, &d_huf, &d_hufmax, &d_status, &d_lit, &d_seq, &d_seqout, &d_pos,
                   &d_frameout, &d_dst, &d_seqblocks, &d_hufitems, &d_hufgroups, &d_totals, &d_og, &d_units, &d_unitinfo, &d_stepunits, &d_swdesc,
                   &d_dbg, &d_raw, &d_unitlist};
  for (DevBuf* b : all) f(*b);
}
void Scratch::release() {
  each_buf([](DevBuf& b) { b.release(); });
  for (auto& e : ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  for (auto& e : ev_huf)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  if (ev_fork) { (void)hipEventDestroy(ev_fork); ev_fork = nullptr; }
  if (ev_fork3) { (void)hipEventDestroy(ev_fork3); ev_fork3 = nullptr; }
  if (ev_up) { (void)hipEventDestroy(ev_up); ev_up = nullptr; }
  for (auto& e : ev_sw)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  for (auto& e : ev_flat)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  have_events = false;
}

int Engine::fail(hipError_t e, const char* what) {
  last_error = std::string(what) + ": " + hipGetErrorString(e);
  return ZG_HIP_ERROR;
}

Tuning Tuning::from_env() {
  Tuning t;
#ifdef ZG_DEV_SWITCHES   // the development build only (libzgpu_dev.so): the product library never looks at the environment
  t.dev_build = true;
  // (a negative value is ignored, not wrapped into a huge unsigned one: ADVICE r5)
  auto num = [](const char* name, uint32_t* v, bool positive) { const char* e = getenv(name); if (e && atoi(e) >= (positive ? 1 : 0)) *v = (uint32_t)atoi(e); return e != nullptr && atoi(e) >= 0; };
  auto is0 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
  num("ZGPU_UNIT_BLOCKS", &t.unit_blocks, true);
  t.direct = !is0("ZGPU_DIRECT");
  num("ZGPU_RAMP", &t.ramp_percent, false);
  t.sparse_set = num("ZGPU_SPARSE_MAX", &t.sparse_max, false);
  if (is0("ZGPU_LIT_DIRECT")) t.lit_direct = 0;
  else { const char* e = getenv("ZGPU_LIT_DIRECT"); if (e && e[0] == '1') t.lit_direct = 1; }
  { uint32_t v = 0; if (num("ZGPU_DIRECT_SHARE", &v, true) && v >= 10) t.direct_share10 = v; }
  t.debug_timers = getenv("ZGPU_DEBUG_TIMERS") != nullptr;
  { const char* e = getenv("ZGPU_FORCE_INORDER"); t.force_inorder = e && e[0] == '1'; }
  num("ZGPU_FLAT_MODE", &t.flat_mode, false);
  num("ZGPU_SWEEP_W", &t.sweep_w, true);
  t.overlap = !is0("ZGPU_OVERLAP");
  t.no_sweep = getenv("ZGPU_DEBUG_NO_SWEEP") != nullptr;
  t.sweep_split = !is0("ZGPU_SWEEP_SPLIT");
  t.no_exact = getenv("ZGPU_DEBUG_NO_EXACT") != nullptr;
  t.no_presize = is0("ZGPU_PRESIZE");
  { uint32_t v = 0; if (num("ZGPU_FLAT4", &v, false)) t.flat4 = (int)v; }
  { uint32_t v = 0; if (num("ZGPU_SEQ_PACKED", &v, false)) t.seq_packed = (int)v; }
  { const char* e = getenv("ZGPU_FLAT_T"); t.flat_shape = (e && atoi(e) == 512) ? 1 : 0; }   // "512": 512 threads x 8 KiB tiles, two workgroups per CU; else the default
  num("ZGPU_SWEEP_MODE", &t.sweep.mode, false);
  num("ZGPU_SWEEP_NB", &t.sweep.nbatch, true);
  num("ZGPU_SWEEP_GROUP", &t.sweep.group, true);
  num("ZGPU_SWEEP_HEAD_LDS", &t.sweep.head_lds, false);
  num("ZGPU_SWEEP_HEAD_NB", &t.sweep.head_nbatch, true);
  { const char* e = getenv("ZGPU_FRAMES_SUBMIT_BYTES"); if (e && atoll(e) > 0) t.frames_submit_bytes = (uint64_t)atoll(e); }
  { const char* e = getenv("ZGPU_MEASURE_SUBMIT_BYTES"); if (e && atoll(e) > 0) t.measure_submit_bytes = (uint64_t)atoll(e); }
  num("ZGPU_SCATTER_CHUNK", &t.scatter_chunk, true);
  { const char* e = getenv("ZGPU_POISON"); if (e && e[0] && atoi(e) >= 0 && atoi(e) <= 255) t.poison = atoi(e); }
  { const char* e = getenv("ZGPU_HASH_DEVICE_MAX"); if (e && atoll(e) >= 0) { t.hash_device_max_set = true; t.hash_device_max = (uint64_t)atoll(e); } }
#endif
  return t;
}

int Engine::create(int device, Engine** out) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n) return ZG_HIP_ERROR;  // no GPU: fail loudly, no CPU path
  if (hipSetDevice(device) != hipSuccess) return ZG_HIP_ERROR;
  Engine* e = new Engine();
  e->device_ = device;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->cus_ = prop.multiProcessorCount;
    e->tn_ = Tuning::from_env();                        // the only place the engine looks at the environment
    e->flat_shape_ = e->tn_.flat_shape;
    e->no_presize_ = e->tn_.no_presize;
#ifdef ZG_DEV_SWITCHES
    Poison::set(e->tn_.poison);
#endif
  }
  // two streams: the sequences chain is the critical one (its kernels last as long as one block's serial chain), so its
  // workgroups are dispatched first; the literals chain fills what is left
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (hipStreamCreateWithPriority(&e->stream_, hipStreamNonBlocking, prio_hi) != hipSuccess) { delete e; return ZG_HIP_ERROR; }
  if (hipStreamCreateWithPriority(&e->stream2_, hipStreamNonBlocking, prio_lo) != hipSuccess) { delete e; return ZG_HIP_ERROR; }
  if (hipStreamCreateWithPriority(&e->stream3_, hipStreamNonBlocking, prio_hi) != hipSuccess) { delete e; return ZG_HIP_ERROR; }
  if (hipStreamCreateWithPriority(&e->stream4_, hipStreamNonBlocking, prio_lo) != hipSuccess) { delete e; return ZG_HIP_ERROR; }
  if (hipStreamCreateWithPriority(&e->stream5_, hipStreamNonBlocking, prio_hi) != hipSuccess) { delete e; return ZG_HIP_ERROR; }
  *out = e;
  return ZG_OK;
}
Engine::~Engine() {
  (void)hipSetDevice(device_);
  for (Scratch* s : free_) { s->release(); delete s; }
  if (stream_) (void)hipStreamDestroy(stream_);
  if (stream2_) (void)hipStreamDestroy(stream2_);
  if (stream3_) (void)hipStreamDestroy(stream3_);
  if (stream4_) (void)hipStreamDestroy(stream4_);
  if (stream5_) (void)hipStreamDestroy(stream5_);
}
Scratch* Engine::acquire() {
  if (!free_.empty()) { Scratch* s = free_.back(); free_.pop_back(); return s; }
  return new Scratch();
}
void Engine::recycle(Scratch* s) {
  if (free_.size() < 2) free_.push_back(s);   // what a streaming decoder or a queue worker alternates between
  else { s->release(); delete s; }
}

Batch::~Batch() {
  // a run uses all three of the engine's streams (Huffman chain and sweep heads on the second, the ramped chain on the third) and
  // joins them by events only when it reaches its end: nothing may be in flight on any of them when the buffers go back
  if (sc && eng) {
    (void)hipSetDevice(eng->device_);
    (void)hipStreamSynchronize(eng->stream_); (void)hipStreamSynchronize(eng->stream2_); (void)hipStreamSynchronize(eng->stream3_);
    if (wait_upload) (void)hipStreamSynchronize(eng->stream4_);   // (prepared beside another submit and never run)
    (void)hipStreamSynchronize(eng->stream5_);                      // (the second half of a download)
    eng->recycle(sc);
  }
  for (SidePass& p : side_) p.release(eng ? eng->device_ : -1);   // (no engine: nothing was ever reserved)
}

void FrameState::reset() {
  base = 0; have = 0; produced = 0; counted = 0; hist[0] = 1; hist[1] = 4; hist[2] = 8;
  logs[0] = logs[1] = logs[2] = logs[3] = 0; huf_maxbits = 0; carry_mask = 0; window_size = 0;
}
void FrameState::release() { d_out.release(); d_fse.release(); d_huf.release(); d_tmp.release(); }

int FrameState::make_room(uint64_t extra, uint64_t keep, hipStream_t s) {
  if (keep > have) keep = have;
  // With a dictionary in front, the window is kept the way the reference keeps it: DecodeBuffer holds the undrained bytes and nothing older,
  // and a match that starts in front of them is served from the dictionary's tail and then from the OLDEST undrained byte
  // (repeat_from_dict, decode_buffer.rs:144-179) — bytes that have been drained are not in between. So they are not in between here either:
  // [dictionary content][undrained bytes], and every kernel's copy "offset bytes back" lands where the reference's does. (Only such a
  // non-conforming match can tell the difference; a conforming one stays inside the window, which is never drained.)
  if (base && keep < have && d_out.p) {
    uint8_t* dst = out_ptr() + base;
    const uint8_t* src = dst + (have - keep);
    hipError_t e = hipSuccess;
    if (keep && have - keep >= keep) e = hipMemcpyAsync(dst, src, keep, hipMemcpyDeviceToDevice, s);   // the ranges do not overlap
    else if (keep) {
      if (d_tmp.reserve(keep)) return ZG_NOMEM;
      Poison::fill(d_tmp.p, d_tmp.cap, s);
      e = hipMemcpyAsync(d_tmp.p, src, keep, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(dst, d_tmp.p, keep, hipMemcpyDeviceToDevice, s);
    }
    if (e != hipSuccess) return ZG_HIP_ERROR;
    have = keep;
  }
  const uint64_t need = kOutFront + base + have + extra + 64;
  if (d_out.p && need <= d_out.cap) return 0;
  // In place: the buffer is large enough for what must stay plus the new bytes once the dropped ones are gone (a streaming decoder that
  // reads ahead reserves its window once, reserve_window, and then only ever gets here: no allocation on the submit path). The kept tail
  // moves to the front — through the staging buffer when the two ranges overlap.
  if (d_out.p && !base && kOutFront + keep + extra + 64 <= d_out.cap) {
    uint8_t* dst = out_ptr();
    const uint8_t* src = dst + (have - keep);
    hipError_t e = hipSuccess;
    if (keep && have - keep >= keep) e = hipMemcpyAsync(dst, src, keep, hipMemcpyDeviceToDevice, s);
    else if (keep) {
      if (d_tmp.reserve(keep)) return ZG_NOMEM;
      Poison::fill(d_tmp.p, d_tmp.cap, s);
      e = hipMemcpyAsync(d_tmp.p, src, keep, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(dst, d_tmp.p, keep, hipMemcpyDeviceToDevice, s);
    }
    if (e != hipSuccess) return ZG_HIP_ERROR;
    have = keep;
    return 0;
  }
  // rebuild: [dictionary][the last `keep` frame bytes] move to a new buffer with room to grow; what the caller has drained
  // and no match can reach any more (decode_buffer.rs:182-219) is dropped here, so the device window stays bounded
  const uint64_t live = base + keep;
  uint64_t ncap = kOutFront + live + extra + 64;
  const uint64_t slack = live + extra > (8u << 20) ? (live + extra) / 2 : (4u << 20);
  ncap += slack;
  void* np = nullptr;
  if (hipMalloc(&np, ncap) != hipSuccess) { (void)hipGetLastError(); return ZG_NOMEM; }   // (the failure must not stay behind as the runtime's last error: the next launch check would report it)
  if (d_out.p) {
    hipError_t e = hipSuccess;
    if (base) e = hipMemcpyAsync((uint8_t*)np + kOutFront, out_ptr(), base, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && keep) e = hipMemcpyAsync((uint8_t*)np + kOutFront + base, out_ptr() + base + (have - keep), keep, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(np); return ZG_HIP_ERROR; }
    (void)hipFree(d_out.p);
  }
  d_out.p = np; d_out.cap = ncap;
  have = keep;
  return 0;
}

// Room for `payload` bytes behind the front pad ([dictionary][frame bytes]), what exists is kept: a streaming decoder that reads ahead
// reserves the window + two runs once, so that make_room never allocates while a run's plaintext is still travelling to the host.
int FrameState::reserve_window(uint64_t payload, hipStream_t s) {
  const uint64_t ncap = kOutFront + payload + 64;
  if (d_out.p && d_out.cap >= ncap) return 0;
  void* np = nullptr;
  if (hipMalloc(&np, ncap) != hipSuccess) { (void)hipGetLastError(); return ZG_NOMEM; }
  if (d_out.p) {
    hipError_t e = hipSuccess;
    if (base + have) e = hipMemcpyAsync((uint8_t*)np + kOutFront, out_ptr(), base + have, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(np); return ZG_HIP_ERROR; }
    (void)hipFree(d_out.p);
  }
  d_out.p = np; d_out.cap = ncap;
  return 0;
}

int parse_block_run(const uint8_t* src, size_t len, uint64_t window, bool has_checksum, const uint32_t hist[3], uint32_t carry_mask,
                    uint32_t max_blocks, BatchBuilder* bb, std::vector<FrameInfo>* info, size_t* consumed, bool* saw_last) {
  // the block loop of FrameDecoder::decode_blocks (frame_decoder.rs:319-375) on a run that starts at a block header.
  // Blocks in front of a truncated one stay in the run (the reference decodes them before it fails).
  FrameInfo fi;
  fi.window_size = window;
  bb->begin_frame(window, hist, carry_mask);
  size_t p = 0;
  int st = ZG_OK;
  *saw_last = false;
  for (;;) {
    if (len - p < 3) { st = ZG_FAILED_READ_BLOCK_HEADER; break; }
    BlockHeader bh;
    if ((st = read_block_header(src + p, &bh))) break;
    if (len - p - 3 < bh.content_size) { st = ZG_FAILED_READ_BLOCK_BODY; break; }
    p += 3;
    st = bb->add_block(bh, src + p, p);
    p += bh.content_size;
    fi.nblocks++;
    if (st) break;
    if (bh.last) {
      *saw_last = true;
      if (has_checksum) {
        if (len - p < 4) { st = ZG_FAILED_READ_CHECKSUM; break; }
        memcpy(&fi.checksum, src + p, 4);
        fi.has_checksum = true;
        p += 4;
      }
      break;
    }
    if (max_blocks && fi.nblocks >= max_blocks) break;
  }
  fi.src_end = p;
  fi.host_status = st;
  info->push_back(fi);
  *consumed = p;
  return st;
}

// a parsed submit whose frames all declare a Frame_Content_Size: their sum (the output can be sized before the run)
static void sum_declared(Batch* b) {
  b->all_declared = !b->info.empty();
  for (const FrameInfo& fi : b->info) {
    if (!fi.header.has_fcs()) { b->all_declared = false; break; }
    b->declared_total += fi.header.frame_content_size;
  }
  if (!b->all_declared || b->declared_total > (1ull << 40)) { b->all_declared = false; b->declared_total = 0; }
}

int Engine::prepare(const uint8_t* src, size_t len, Batch** out) {
  Batch* b = new Batch();
  b->eng = this;
  b->src_len = len;
  b->parse_status = parse_frames(src, len, max_window, &b->bb, &b->info);
  sum_declared(b);
  return upload(b, src, len, out);
}

int Engine::prepare_entries(const uint8_t* src, size_t len, const uint64_t* off, const uint64_t* elen, uint32_t n, Batch** out,
                            std::vector<int>* walk, std::vector<uint32_t>* first_frame, const DictLookup* dicts) {
  Batch* b = new Batch();
  b->eng = this;
  b->src_len = len;
  walk->assign(n, 0);
  first_frame->assign(n + 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    (*first_frame)[i] = (uint32_t)b->info.size();
    (*walk)[i] = parse_frames(src + off[i], elen[i], max_window, &b->bb, &b->info, off[i], dicts);
    if (!b->parse_status) b->parse_status = (*walk)[i];
  }
  (*first_frame)[n] = (uint32_t)b->info.size();
  sum_declared(b);
  return upload(b, src, len, out);
}

// device memory and events of the lane passes of one call
struct Engine::LaneTmp : SidePass {
  DevBuf& lanes = buf;   // (the pass's own buffer holds the lanes)
  DevBuf out, extra;
  ~LaneTmp() { release(); out.release(); extra.release(); }
};

template <class Launch>
int Engine::lane_pass(LaneTmp& t, const void* lanes, size_t lane_bytes, Down out, Down extra, uint64_t* stats, Launch launch) {
  Engine* eng = this;
  ZG_HIP(hipSetDevice(device_));
  hipStream_t s = stream_;
  int st;
  if ((st = t.reserve(lane_bytes)) || (st = t.out.reserve(out.bytes)) || (extra.host && (st = t.extra.reserve(extra.bytes)))) return st;
  Poison::fill_now(t.out.p, t.out.cap);
  if (extra.host) Poison::fill_now(t.extra.p, t.extra.cap);
  ZG_HIP(t.upload(lanes, lane_bytes, nullptr, 0, s));
  ZG_HIP(hipStreamSynchronize(s));   // (pageable)
  ZG_HIP(t.begin(s));
  launch(t, s);
  ZG_HIP(t.end(s));
  ZG_HIP(hipMemcpyAsync(out.host, t.out.p, out.bytes, hipMemcpyDeviceToHost, s));
  if (extra.bytes) ZG_HIP(hipMemcpyAsync(extra.host, t.extra.p, extra.bytes, hipMemcpyDeviceToHost, s));
  ZG_HIP(hipStreamSynchronize(s));
  uint64_t us = 0;
  ZG_HIP(t.elapsed_us(&us));
  stats[kPassLaunches] += 1; stats[kPassUs] += us; stats[kPassBytes] += out.bytes + extra.bytes;
  return ZG_OK;
}

int Engine::walk_entries(const DevEntry* e, uint32_t n, Skeleton* sk, uint64_t* stats) {
  sk->recs.clear();
  sk->first.assign((size_t)n + 1, 0);
  sk->ends.assign(n, zgw::End{0, 0, 0});
  if (!n) return ZG_OK;
  LaneTmp t;
  std::vector<zgw::Lane> lanes(n);
  for (uint32_t i = 0; i < n; i++) lanes[i] = zgw::Lane{e[i].src, e[i].len, 0, 0};
  const size_t lane_bytes = (size_t)n * sizeof(zgw::Lane), end_bytes = (size_t)n * sizeof(zgw::End);
  // count pass: how many records every entry has
  int st = lane_pass(t, lanes.data(), lane_bytes, Down{sk->ends.data(), end_bytes}, Down{}, stats, [&](LaneTmp& d, hipStream_t s) {
    zg_launch_walk(d.lanes.as<zgw::Lane>(), n, d.out.as<zgw::End>(), nullptr, s);
  });
  if (st) return st;
  for (uint32_t i = 0; i < n; i++) {
    lanes[i].first = sk->first[i];
    lanes[i].limit = sk->ends[i].nrec;
    sk->first[i + 1] = sk->first[i] + sk->ends[i].nrec;
  }
  const uint64_t total = sk->first[n];
  if (!total) return ZG_OK;
  // emit pass: every lane writes its own range of records, and no other
  sk->recs.resize(total);
  std::vector<zgw::End> again(n);
  st = lane_pass(t, lanes.data(), lane_bytes, Down{again.data(), end_bytes}, Down{sk->recs.data(), total * sizeof(zgw::Rec)}, stats,
                 [&](LaneTmp& d, hipStream_t s) { zg_launch_walk(d.lanes.as<zgw::Lane>(), n, d.out.as<zgw::End>(), d.extra.as<zgw::Rec>(), s); });
  if (st) return st;
  for (uint32_t i = 0; i < n; i++)   // (a source that changed between the passes: the caller's promise broken, nothing of the skeleton is used)
    if (again[i].nrec != sk->ends[i].nrec || again[i].stop_off != sk->ends[i].stop_off || again[i].why != sk->ends[i].why) {
      last_error = "zgpu_decode_frames_device_src: a source changed while it was walked";
      return ZG_INTERNAL;
    }
  return ZG_OK;
}

int Engine::index_pass(const DevEntry* e, uint32_t n, const uint64_t* first, const zgi::Entry* sum, zgi::Entry* out, zgi::FrameRec* recs, uint64_t* stats) {
  if (!n) return ZG_OK;
  LaneTmp t;
  std::vector<zgw::Lane> lanes(n);
  for (uint32_t i = 0; i < n; i++) lanes[i] = zgw::Lane{e[i].src, e[i].len, first ? first[i] : 0, first ? (uint64_t)sum[i].nrec : 0};
  const Down down_recs = first ? Down{recs, (size_t)first[n] * sizeof(zgi::FrameRec)} : Down{};
  return lane_pass(t, lanes.data(), (size_t)n * sizeof(zgw::Lane), Down{out, (size_t)n * sizeof(zgi::Entry)}, down_recs, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_index(d.lanes.as<zgw::Lane>(), n, d.out.as<zgi::Entry>(), d.extra.as<zgi::FrameRec>(), s); });
}

int Engine::seek_pass(const zgk::Lane* lanes, uint32_t n, zgk::Seek* out, uint64_t* stats) {
  if (!n) return ZG_OK;
  LaneTmp t;
  return lane_pass(t, lanes, (size_t)n * sizeof(zgk::Lane), Down{out, (size_t)n * sizeof(zgk::Seek)}, Down{}, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_seek(d.lanes.as<zgk::Lane>(), n, d.out.as<zgk::Seek>(), s); });
}

int Engine::seektab_pass(const zgt::Lane* lanes, uint32_t n, zgk::Seek* out, uint64_t* stats) {
  if (!n) return ZG_OK;
  LaneTmp t;
  return lane_pass(t, lanes, (size_t)n * sizeof(zgt::Lane), Down{out, (size_t)n * sizeof(zgk::Seek)}, Down{}, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_seektab(d.lanes.as<zgt::Lane>(), n, d.out.as<zgk::Seek>(), s); });
}

int Engine::seekmany_prefixes(const DevEntry* e, uint32_t ne, zgm::Loc* loc, uint64_t* pre, DevBuf* scratch, uint64_t* npairs, uint64_t* stats, ManyStats* more) {
  Engine* eng = this;
  *npairs = 0;
  // locate: what every entry's table frame is
  if (ne) {
    LaneTmp t;
    std::vector<zgm::Ent> ents(ne);
    for (uint32_t i = 0; i < ne; i++) ents[i] = zgm::Ent{e[i].src, e[i].len};
    const int st = lane_pass(t, ents.data(), (size_t)ne * sizeof(zgm::Ent), Down{loc, (size_t)ne * sizeof(zgm::Loc)}, Down{}, stats,
                             [&](LaneTmp& d, hipStream_t s) { zg_launch_seekmany_locate(d.lanes.as<zgm::Ent>(), ne, d.out.as<zgm::Loc>(), s); });
    if (st) return st;
  }
  // the scratch laid out from the located row counts: every usable entry's prefixes, then every usable entry's chunk totals
  std::vector<zgm::Work> work;
  uint64_t pairs = 0, chunks = 0;
  for (uint32_t i = 0; i < ne; i++) {
    const zgm::Loc& l = loc[i];
    pre[i] = 0;
    if (l.why) continue;
    // (what the host relies on below is checked here, not believed: the rows lie inside the entry)
    if (l.nf > zgt::kMaxFrames || (l.es != 8 && l.es != 12) || l.tab > e[i].len || (uint64_t)l.nf * l.es + zgt::kFraming != e[i].len - l.tab) {
      last_error = "zg_k_seekmany_locate: a table frame that leaves its entry";
      return ZG_INTERNAL;
    }
    pre[i] = pairs;
    pairs += (uint64_t)l.nf + 1;
    chunks += zgm::chunks_of(l.nf, zgm::kChunkRows);
  }
  if (chunks > 0xFFFFFFFFull || pairs + chunks > SIZE_MAX / sizeof(zgm::Pair)) return ZG_NOMEM;
  if (!pairs) return ZG_OK;
  LaneTmp tp;   // (lanes: the chunks of work)
  work.reserve((size_t)chunks);
  uint64_t tot = pairs;
  for (uint32_t i = 0; i < ne; i++) {
    const zgm::Loc& l = loc[i];
    if (l.why) continue;
    const uint32_t nq = zgm::chunks_of(l.nf, zgm::kChunkRows);
    for (uint32_t q = 0; q < nq; q++) work.push_back(zgm::Work{e[i].src, l.tab + 8, pre[i], tot, l.nf, l.es, q, nq});
    tot += nq;
  }
  const size_t bytes = (size_t)(pairs + chunks) * sizeof(zgm::Pair), wbytes = work.size() * sizeof(zgm::Work);
  ZG_HIP(hipSetDevice(device_));
  int st;
  // (lane_pass's steps without its download: nothing of the prefixes comes back, and nothing is added to stats[])
  if ((st = scratch->reserve(bytes)) || (st = tp.reserve(wbytes))) return st;
  Poison::fill_now(scratch->p, scratch->cap);
  ZG_HIP(tp.upload(work.data(), wbytes, nullptr, 0, stream_));
  ZG_HIP(hipStreamSynchronize(stream_));   // (pageable)
  ZG_HIP(tp.begin(stream_));
  zg_launch_seekmany_prefix(tp.lanes.as<zgm::Work>(), (uint32_t)work.size(), scratch->as<zgm::Pair>(), stream_);
  ZG_HIP(tp.end(stream_));
  ZG_HIP(hipStreamSynchronize(stream_));
  uint64_t us = 0;
  ZG_HIP(tp.elapsed_us(&us));
  more->prefix_launches += 2; more->prefix_us += us; more->scratch_bytes += (uint64_t)pairs * sizeof(zgm::Pair);
  *npairs = pairs;
  return ZG_OK;
}

int Engine::seekmany_find(const zgm::Find* lanes, uint32_t m, const zgm::Pair* pairs, zgk::Seek* out, uint64_t* stats, ManyStats* more) {
  if (!m) return ZG_OK;
  LaneTmp t;
  uint64_t pass[3] = {0, 0, 0};
  const int st = lane_pass(t, lanes, (size_t)m * sizeof(zgm::Find), Down{out, (size_t)m * sizeof(zgk::Seek)}, Down{}, pass,
                           [&](LaneTmp& d, hipStream_t s) { zg_launch_seekmany_find(d.lanes.as<zgm::Find>(), m, pairs, d.out.as<zgk::Seek>(), s); });
  if (st) return st;
  more->find_launches += pass[kPassLaunches]; more->find_us += pass[kPassUs];
  if (stats) stats[kPassBytes] += pass[kPassBytes];
  return ZG_OK;
}

int Engine::seekmany_pass(const DevEntry* e, uint32_t ne, const ManyRange* ranges, uint32_t m, zgk::Seek* out, uint64_t* stats, ManyStats* more) {
  if (!m) return ZG_OK;
  std::vector<zgm::Loc> loc(ne);
  std::vector<uint64_t> pre(ne, 0);
  DevBuf scratch;   // (lives for the call)
  uint64_t npairs = 0;
  int st = seekmany_prefixes(e, ne, loc.data(), pre.data(), &scratch, &npairs, stats, more);
  if (!st) {
    // find: one lane per range
    std::vector<zgm::Find> lanes(m);
    for (uint32_t j = 0; j < m; j++) {
      const ManyRange& r = ranges[j];
      if (!r.rlen || r.entry >= ne) { lanes[j] = zgm::Find{r.begin, 0, 0, 0, 0, 0, 0, 0}; continue; }
      const zgm::Loc& l = loc[r.entry];
      lanes[j] = zgm::Find{r.begin, r.rlen, pre[r.entry], l.tab, l.why ? 0u : l.nf, l.why, 0, 0};
    }
    st = seekmany_find(lanes.data(), m, scratch.as<zgm::Pair>(), out, stats, more);
  }
  scratch.release();
  return st;
}

int Engine::seekidx_rows_pass(const zgx::Lane* lanes, uint32_t n, zgm::Pair* pairs, zgx::Rows* out, uint64_t* stats) {
  if (!n) return ZG_OK;
  LaneTmp t;
  return lane_pass(t, lanes, (size_t)n * sizeof(zgx::Lane), Down{out, (size_t)n * sizeof(zgx::Rows)}, Down{}, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_seekidx_rows(d.lanes.as<zgx::Lane>(), n, pairs, d.out.as<zgx::Rows>(), s); });
}

int Engine::records_find(const zgr::Find* lanes, uint32_t m, const uint64_t* recs, zgr::Found* out, uint64_t* stats) {
  if (!m) return ZG_OK;
  LaneTmp t;
  return lane_pass(t, lanes, (size_t)m * sizeof(zgr::Find), Down{out, (size_t)m * sizeof(zgr::Found)}, Down{}, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_recs_find(d.lanes.as<zgr::Find>(), m, recs, d.out.as<zgr::Found>(), s); });
}

int Engine::fill_pass(const zgs::Seg* regions, uint32_t n, uint32_t byte, uint64_t* stats) {
  Engine* eng = this;
  std::vector<zgs::Chunk> ch;
  zgs::plan_chunks(regions, n, zgs::kFillChunk, &ch);
  if (ch.empty()) return ZG_OK;
  if (ch.size() > 0xFFFFFFFFull) return ZG_INTERNAL;
  uint64_t bytes = 0;
  for (const zgs::Chunk& c : ch) bytes += c.len;
  ZG_HIP(hipSetDevice(device_));
  LaneTmp t;   // (lanes: the regions, the chunk table behind them; nothing comes back)
  const size_t sb = (size_t)n * sizeof(zgs::Seg), cb = ch.size() * sizeof(zgs::Chunk);
  const int st = t.reserve(sb + cb);
  if (st) return st;
  ZG_HIP(t.upload(regions, sb, ch.data(), cb, stream_));
  ZG_HIP(hipStreamSynchronize(stream_));   // (pageable)
  ZG_HIP(t.begin(stream_));
  zg_launch_fill(t.at<zgs::Seg>(0), t.at<zgs::Chunk>(sb), (uint32_t)ch.size(), byte, stream_);
  ZG_HIP(t.end(stream_));
  ZG_HIP(hipStreamSynchronize(stream_));
  uint64_t us = 0;
  ZG_HIP(t.elapsed_us(&us));
  stats[kPassLaunches] += 1; stats[kPassUs] += us; stats[kPassBytes] += bytes;
  return ZG_OK;
}

int Engine::hash_ranges_pass(const uint8_t* base, const ZgHashRange* ranges, uint32_t n, int kernel, uint64_t* digests, uint64_t* stats) {
  if (!n) return ZG_OK;
  LaneTmp t;
  return lane_pass(t, ranges, (size_t)n * sizeof(ZgHashRange), Down{digests, (size_t)n * sizeof(uint64_t)}, Down{}, stats,
                   [&](LaneTmp& d, hipStream_t s) { zg_launch_xxh64_with(base, d.lanes.as<ZgHashRange>(), d.out.as<uint64_t>(), n, s, kernel); });
}

int Engine::prepare_entries_device(const DevEntry* e, const Skeleton& sk, const uint32_t* idx, const uint64_t* off, uint32_t n, size_t total, Batch** out,
                                   std::vector<int>* walk, std::vector<uint32_t>* first_frame, const DictLookup* dicts) {
  Batch* b = new Batch();
  b->eng = this;
  b->src_len = total;
  walk->assign(n, 0);
  first_frame->assign((size_t)n + 1, 0);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t i = idx[j];
    bool consistent = true;
    (*first_frame)[j] = (uint32_t)b->info.size();
    (*walk)[j] = parse_frames_skel(sk.recs.data() + sk.first[i], (uint32_t)(sk.first[i + 1] - sk.first[i]), e[i].len, max_window, &b->bb, &b->info, off[j],
                                   &consistent, dicts);
    if (!consistent) { delete b; last_error = "zgpu_decode_frames_device_src: skeleton records out of step with the walk"; return ZG_INTERNAL; }
    if (!b->parse_status) b->parse_status = (*walk)[j];
  }
  (*first_frame)[n] = (uint32_t)b->info.size();
  sum_declared(b);
  const GatherPlan g{e, idx, off, n};
  return upload(b, nullptr, total, out, false, &g);
}

int Engine::prepare_run(const uint8_t* src, size_t len, FrameState* fs, bool has_checksum, uint32_t max_blocks, uint64_t keep, Batch** out, size_t* consumed,
                        bool side, const uint32_t* carry_mask_now) {
  Batch* b = new Batch();
  b->eng = this;
  b->fs = fs;
  b->keep_bytes = keep;
  // (carry_mask_now: the run in front has not been folded into fs yet — its caller says which tables will exist when this one starts; the
  //  offset history is taken when the run is launched, Batch::run)
  b->carry_mask_in = carry_mask_now ? *carry_mask_now : fs->carry_mask;
  b->parse_status = parse_block_run(src, len, fs->window_size, has_checksum, fs->hist, b->carry_mask_in, max_blocks, &b->bb, &b->info, consumed,
                                    &b->saw_last_block);
  b->src_len = *consumed;
  b->bb.frames[0].fixed_base = 1;   // where its bytes go is decided in run(), when the size of the run is known
  int st;
  if ((st = fs->d_fse.reserve(ZG_FSE_SLOT_U32 * 4)) || (st = fs->d_huf.reserve(ZG_HUF_SLOT_U16 * 2))) { delete b; return st; }   // the tables it will carry on
  return upload(b, src, *consumed, out, side);
}

int Engine::prepare_blocks(const uint8_t* src, size_t len, const HostBlock* hb, size_t n, FrameState* fs, uint64_t keep, Batch** out) {
  // the block loop of FrameDecoder::decode_blocks (frame_decoder.rs:319-375) with the headers already read by the caller
  Batch* b = new Batch();
  b->eng = this;
  b->fs = fs;
  b->keep_bytes = keep;
  b->src_len = len;
  FrameInfo fi;
  fi.window_size = fs->window_size;
  b->bb.begin_frame(fs->window_size, fs->hist, fs->carry_mask);
  int st = ZG_OK;
  for (size_t i = 0; i < n && !st; i++) {
    const HostBlock& h = hb[i];
    BlockHeader bh;
    bh.last = h.last != 0; bh.type = h.type;
    if (h.type > ZG_BT_COMPRESSED) { st = ZG_RESERVED_BLOCK; b->bb.fail_frame(st); break; }                 // block_decoder.rs:226-228
    if ((h.type == ZG_BT_COMPRESSED ? h.src_len : h.raw_rle_size) > kMaxBlockSize) { st = ZG_BLOCK_SIZE_TOO_LARGE; b->bb.fail_frame(st); break; }   // :259-266
    if (h.src_off > len || h.src_len > len - h.src_off) { st = ZG_FAILED_READ_BLOCK_BODY; b->bb.fail_frame(st); break; }
    bh.decompressed_size = h.type == ZG_BT_COMPRESSED ? 0 : h.raw_rle_size;
    bh.content_size = h.type == ZG_BT_RLE ? 1 : h.src_len;
    if (h.type == ZG_BT_RAW && h.src_len != h.raw_rle_size) { st = ZG_FAILED_READ_BLOCK_BODY; b->bb.fail_frame(st); break; }
    if (h.type == ZG_BT_RLE && h.src_len < 1) { st = ZG_FAILED_READ_BLOCK_BODY; b->bb.fail_frame(st); break; }
    st = b->bb.add_block(bh, src + h.src_off, h.src_off);
    fi.nblocks++;
    if (bh.last) { b->saw_last_block = true; break; }
  }
  fi.host_status = st;
  b->info.push_back(fi);
  b->parse_status = st;
  b->bb.frames[0].fixed_base = 1;
  if ((st = fs->d_fse.reserve(ZG_FSE_SLOT_U32 * 4)) || (st = fs->d_huf.reserve(ZG_HUF_SLOT_U16 * 2))) { delete b; return st; }
  return upload(b, src, len, out);
}

int Engine::upload(Batch* b, const uint8_t* src, size_t len, Batch** out, bool side, const GatherPlan* g) {
  Engine* eng = this;
  ZG_HIP(hipSetDevice(device_));
  // side: the submit in front is still running on the main stream — everything this one brings to the device travels on the upload stream
  // beside it, and its run() waits for the event instead of the host waiting here
  hipStream_t us = side ? stream4_ : stream_;
  // a frame-layer error after some good frames: the good frames are still uploaded (callers such as the
  // FrameDecoder mirror may want them); decode_all reports parse_status.
  const Tuning& tn = tn_;                                      // (measurement / test switches, read when the engine was created)
  if (tn.unit_blocks) b->bb.unit_blocks = tn.unit_blocks;
  if (!tn.direct) b->bb.direct_units = false;
  b->bb.ramp_percent = tn.ramp_percent;                        // N > 0: one long frame in units growing by +-N %, the sweep chain beside the flatten
  if (tn.sparse_set) { b->bb.sparse_max = tn.sparse_max; b->bb.sparse_per_block = 1u << 20; }   // (tests) sequences per frame up to which zg_k_sparse replaces the sweep, whatever their density; 0: never
  b->bb.flat_slots = (uint32_t)cus_ * (flat_shape_ == 0 ? 1u : 2u);   // zg_k_flatten: workgroups the device holds at once
  b->bb.chain_slots = (uint32_t)cus_ * 32u;                            // zg_k_seq: blocks whose chains run at once
  if (tn.lit_direct == 0) b->bb.lit_direct_allowed = false;
  b->bb.lit_direct_force = tn.lit_direct == 1;
  b->bb.seq_packed_force = tn.seq_packed;
  if (tn.direct_share10) b->bb.direct_share10 = tn.direct_share10;   // (measurement) tenths
  b->bb.finish();
  BatchBuilder& bb = b->bb;
  Scratch* sc = b->sc = acquire();
  Poison::begin_submit();
  const uint32_t nb = (uint32_t)bb.blocks.size(), nf = (uint32_t)bb.frames.size();
  auto up = [&](DevBuf& d, const void* h, size_t bytes) -> int {
    int st = d.reserve(bytes ? bytes : 16);
    if (st) return st;
    Poison::fill(d.p, d.cap, us);                                  // (the whole capacity, in front of the upload)
    if (bytes && hipMemcpyAsync(d.p, h, bytes, hipMemcpyHostToDevice, us) != hipSuccess) return ZG_HIP_ERROR;
    return 0;
  };
  int st = 0;
  // compressed bytes, padded so that 8-byte bit-window loads near the end stay inside the allocation
  // ... and 64 bytes in front for the 16-byte windows of the sequence decoder
  if ((st = sc->d_src.reserve(len + 128))) { delete b; return st; }
  Poison::fill(sc->d_src.p, sc->d_src.cap, us);                    // (in front of the two zero pads and the bytes)
  (void)hipMemsetAsync(sc->d_src.p, 0, 64, us);
  if (g) {
    // the bytes are on the device already: one launch copies every entry to its place behind the front pad (zg_k_gather: the lanes read
    // [src, src + len) of an entry and nothing else, and write [d_src + 64 + off, + len), which the reserve above covers)
    const uint64_t at = (uint64_t)(uintptr_t)sc->d_src.p + 64;
    for (uint32_t j = 0; j < g->n; j++) {
      const DevEntry& en = g->e[g->idx[j]];
      if (en.len > len || g->off[j] > len - en.len) { delete b; return ZG_INTERNAL; }
      if (en.len) b->gather_segs_.push_back(zgs::Seg{en.src, at + g->off[j], en.len});
    }
    zgs::plan_chunks(b->gather_segs_.data(), (uint32_t)b->gather_segs_.size(), tn.scatter_chunk, &b->gather_chunks_);
    if (b->gather_chunks_.size() > 0xFFFFFFFFull) { delete b; return ZG_INTERNAL; }
    if (!b->gather_chunks_.empty()) {
      const size_t sb = b->gather_segs_.size() * sizeof(zgs::Seg), cb = b->gather_chunks_.size() * sizeof(zgs::Chunk);
      SidePass& p = b->side_[Batch::kSideGather];
      if ((st = p.reserve(sb + cb))) { delete b; return st; }
      // (no wait behind the upload: the tables travel from the batch's own vectors, which outlive the copies)
      bool ok = p.upload(b->gather_segs_.data(), sb, b->gather_chunks_.data(), cb, us) == hipSuccess && p.begin(us) == hipSuccess;
      if (ok) zg_launch_gather(p.at<zgs::Seg>(0), p.at<zgs::Chunk>(sb), (uint32_t)b->gather_chunks_.size(), us);
      ok = ok && p.end(us) == hipSuccess;
      if (!ok) { delete b; return ZG_HIP_ERROR; }
      b->gather_launched = true;
    }
  } else if (len && hipMemcpyAsync((uint8_t*)sc->d_src.p + 64, src, len, hipMemcpyHostToDevice, us) != hipSuccess) { delete b; return ZG_HIP_ERROR; }
  (void)hipMemsetAsync((uint8_t*)sc->d_src.p + 64 + len, 0, 64, us);
  const uint32_t nslots = bb.nslots();
  if ((st = up(sc->d_blocks, bb.blocks.data(), nb * sizeof(ZgBlock))) || (st = up(sc->d_frames, bb.frames.data(), nf * sizeof(ZgFrame))) ||
      (st = up(sc->d_seqblocks, bb.seq_blocks.data(), bb.seq_blocks.size() * 4)) ||
      (st = up(sc->d_hufitems, bb.huf_items.data(), bb.huf_items.size() * 4)) ||
      (st = up(sc->d_hufgroups, bb.huf_groups.data(), bb.huf_groups.size() * sizeof(ZgHufGroup))) ||
      (st = up(sc->d_units, bb.units.data(), bb.units.size() * sizeof(ZgUnit))) ||
      (st = up(sc->d_stepunits, bb.step_units.data(), bb.step_units.size() * 4)) ||
      (st = up(sc->d_unitlist, bb.unit_list.data(), bb.unit_list.size() * 4)) ||
      (st = sc->d_aux.reserve((size_t)nb * sizeof(ZgBlockAux) + 16)) || (st = sc->d_fparsed.reserve((size_t)nb * sizeof(ZgFtabParsed) + 16)) || (st = sc->d_slot_log.reserve((size_t)nslots * 4)) ||
      (st = sc->d_fse.reserve((size_t)nslots * ZG_FSE_SLOT_U32 * 4)) || (st = sc->d_huf.reserve((size_t)(bb.nhuf_slots + 1) * ZG_HUF_SLOT_U16 * 2)) ||
      (st = sc->d_hufmax.reserve(bb.nhuf_slots + 16)) || (st = sc->d_status.reserve(7 * ((size_t)nb * 4 + 16))) ||
      (st = sc->d_lit.reserve(bb.lit_bytes + 128)) || (st = sc->d_seq.reserve((bb.seq_count + 2) * sizeof(ZgSeq))) ||
      (st = sc->d_raw.reserve((bb.seq_count + 8) * 4)) ||
      (st = sc->d_seqout.reserve((size_t)nb * sizeof(ZgBlockSeqOut) + 16)) || (st = sc->d_pos.reserve((size_t)nb * sizeof(ZgBlockPos) + 16)) ||
      (st = sc->d_frameout.reserve((size_t)nf * sizeof(ZgFrameOut) + 16)) || (st = sc->d_totals.reserve(64)) ||
      (st = sc->d_swdesc.reserve(bb.step_units.size() * sizeof(ZgSweepDesc) + 32)) ||
      (st = sc->d_unitinfo.reserve(bb.units.size() * sizeof(ZgUnitInfo) + 16)) || (st = sc->d_dbg.reserve(8192)) || (st = sc->init_events())) {
    delete b;
    return st;
  }
  if (Poison::value() >= 0) {
    // the arenas only kernels write (run() enqueues them behind this), and what the Scratch still holds of an earlier submit's output and
    // flatten scratch; the uploaded tables were filled in front of their uploads
    DevBuf* up_bufs[] = {&sc->d_src, &sc->d_blocks, &sc->d_frames, &sc->d_seqblocks, &sc->d_hufitems, &sc->d_hufgroups, &sc->d_units, &sc->d_stepunits, &sc->d_unitlist};
    sc->each_buf([&](DevBuf& x) {
      bool uploaded = false;
      for (DevBuf* u : up_bufs) uploaded = uploaded || u == &x;
      if (!uploaded) Poison::fill(x.p, x.cap, us);
    });
#ifdef ZG_DEV_SWITCHES
    Poison::scratch_cap = 0;
    sc->each_buf([&](DevBuf& x) { Poison::scratch_cap += x.p ? x.cap : 0; });
#endif
  }
  // the output and the flatten scratch are sized in run(), when the exact output size of every frame is known
  ZgBatchDev& d = b->dev;
  d.src = sc->d_src.as<uint8_t>() + 64; d.src_len = len;
  d.blocks = sc->d_blocks.as<ZgBlock>(); d.nblocks = nb;
  d.frames = sc->d_frames.as<ZgFrame>(); d.nframes = nf;
  d.nslots = nslots; d.nhuf_slots = bb.nhuf_slots;
  d.aux = sc->d_aux.as<ZgBlockAux>(); d.ftab_parsed = sc->d_fparsed.as<ZgFtabParsed>(); d.slot_log = sc->d_slot_log.as<uint8_t>();
  d.fse_arena = sc->d_fse.as<uint32_t>(); d.huf_arena = sc->d_huf.as<uint16_t>(); d.huf_maxbits = sc->d_hufmax.as<uint8_t>();
  d.status = sc->d_status.as<uint32_t>(); d.tab_status = d.status + nb + 4; d.lit_status = d.tab_status + nb + 4;
  d.lit_counts = d.lit_status + nb + 4;     // [4 * nblocks], written by zg_k_huf (no reset needed)
  d.lit_arena = sc->d_lit.as<uint8_t>() + 64;   // (zg_k_flatten reads literal windows that start up to 7 bytes in front of a block's literals)
  d.seq_arena = sc->d_seq.as<ZgSeq>(); d.raw_arena = sc->d_raw.as<uint32_t>();
  d.seq_out = sc->d_seqout.as<ZgBlockSeqOut>(); d.pos = sc->d_pos.as<ZgBlockPos>(); d.frame_out = sc->d_frameout.as<ZgFrameOut>();
  d.dst = nullptr; d.dst_cap = 0; d.og = nullptr;
  d.dict = nullptr;
  d.seq_blocks = sc->d_seqblocks.as<uint32_t>(); d.nseq_blocks = (uint32_t)bb.seq_blocks.size();
  d.huf_items = sc->d_hufitems.as<uint32_t>(); d.huf_groups = sc->d_hufgroups.as<ZgHufGroup>(); d.nhuf_groups = (uint32_t)bb.huf_groups.size();
  d.totals = sc->d_totals.as<uint32_t>();
  d.units = sc->d_units.as<ZgUnit>(); d.nunits = (uint32_t)bb.units.size(); d.unit_info = sc->d_unitinfo.as<ZgUnitInfo>();
  d.step_units = sc->d_stepunits.as<uint32_t>();
  d.unit_list = sc->d_unitlist.as<uint32_t>(); d.ndirect = bb.n_direct;
  d.sweep_desc = sc->d_swdesc.as<ZgSweepDesc>();
  b->sweep_steps.clear();
  for (const ZgStepRange& r : bb.steps) {
    ZgSweepStep ss;
    ss.list_off = r.list_off; ss.nunits = r.nunits; ss.slices = r.max_blocks * (kMaxBlockSize / ZG_SW_BATCH); ss.pad = 0;   // zg_k_sweep: ZG_SW_BATCH bytes of output per workgroup
    b->sweep_steps.push_back(ss);
  }
  d.dbg = tn.debug_timers ? sc->d_dbg.as<unsigned long long>() : nullptr;
  d.flags = tn.force_inorder ? 1u : 0u;
  d.flags |= (uint32_t)flat_shape_ << 2;
  d.flags |= ((tn.flat_mode & 3u) << 4) | ((tn.flat_mode & 4u) << 5);   // (timing experiments) zg_k_flatten without scratch stores / gathers
  d.sweep_window = tn.sweep_w;
  if (side) {
    if (hipEventRecord(sc->ev_up, us) != hipSuccess) { delete b; return ZG_HIP_ERROR; }
    b->wait_upload = true;
  } else if (hipStreamSynchronize(stream_) != hipSuccess) { delete b; return ZG_HIP_ERROR; }
  if (b->gather_launched && !side && b->side_[Batch::kSideGather].elapsed_us(&b->gather_us) != hipSuccess) { delete b; return ZG_HIP_ERROR; }
  *out = b;
  return ZG_OK;
}

int Batch::run() {
  ZG_HIP(hipSetDevice(eng->device_));
  hipStream_t s = eng->stream_;
  ZgBatchDev& d = dev;
  if (d.nframes == 0) { ran = true; total_out = 0; return ZG_OK; }
  if (d.nblocks == 0) {
    // frames without a single block (the walk stopped at the first block header of each: parse_status / FrameInfo::host_status say why):
    // nothing to launch — a grid of zero workgroups is an error to the runtime (tools/dev/soak_batch.py) — and nothing comes out
    frame_out.assign(d.nframes, ZgFrameOut{});
    for (ZgFrameOut& fo : frame_out) fo.err_packed = 0xFFFFFFFFu;
    total_out = 0; ran = false; synced = true;
    return ZG_OK;
  }
  hipEvent_t* ev = sc->ev;
  // every frame declares its content size: output and flatten scratch are sized now, and nothing below waits for the host
  presized = false;
  d.dst_cap_pre = 0;
  // ... and the declared sizes are possible at all: a block regenerates at most 128 KiB on this path, and Frame_Content_Size is a field
  // the reference never believes (a corrupted one must not become a 600 GB allocation: the sizes are then taken from the scan)
  // (bb.out_bound: what the host already knows the blocks can produce at most — exact for raw and RLE blocks, 128 KiB per compressed block.
  //  A declared size beyond it is a lie whatever else is true — 500,000 empty raw blocks behind an FCS of 64 GiB must not become a 320 GiB
  //  allocation — and a reserve that fails all the same is no error either: the reference never looks at the field, so the
  //  submit falls back to sizes taken from the scan.)
  // (not with ramped units, a measurement switch: their sweep chain polls flags that the flatten of a no-op run never raises — ADVICE r4)
  // (not for a declared total of 0: the device's "sized in advance" marker is a capacity > 0, and a submit that declares nothing but produces
  //  one byte kept its promise by that marker while the host's capacity said 0 — zgpu_batch_read refused the byte, tools/dev/soak_batch.py)
  // (nor a shared submit with dictionary frames: the host places their contents once it knows where the scan put the frames)
  dictfill_launches = 0; dictfill_bytes = 0; dictfill_us = 0; side_[kSideFill0].n = side_[kSideFill1].n = 0;
  if (!fs && all_declared && declared_total && !eng->no_presize_ && declared_total <= bb.out_bound && !bb.ramped && frame_dicts_.empty()) {
    // (the scratch first: it is four times the output. When either reserve fails nothing of the attempt stays allocated — the sizes taken
    //  from the scan may well fit where the declared ones did not: ADVICE r5)
    if (sc->d_og.reserve(declared_total * 4 + 64) == 0 && sc->d_dst.reserve(kOutFront + declared_total + 64) == 0) {
      Poison::fill(sc->d_og.p, sc->d_og.cap, s); Poison::fill(sc->d_dst.p, sc->d_dst.cap, s);   // (a reserve may have given new memory)
      d.dst = sc->d_dst.as<uint8_t>() + kOutFront; d.dst_cap = declared_total;
      d.og = sc->d_og.as<uint32_t>(); d.og_words = og_words = declared_total;
      d.dst_cap_pre = declared_total;                        // (0 means "not sized in advance")
      presized = true;
    } else { sc->d_og.release(); sc->d_dst.release(); }
  }
  if (wait_upload) { ZG_HIP(hipStreamWaitEvent(s, sc->ev_up, 0)); wait_upload = false; }
  ZG_HIP(hipEventRecord(ev[0], s));
  if (fs) {
    // a continued frame: the offset history is the one the run in front has left (that run may have been folded into fs after this one
    // was prepared: the streaming decoder prepares run k + 1 while run k is on the GPU)
    ZgFrame& fr0 = bb.frames[0];
    fr0.hist_init[0] = fs->hist[0]; fr0.hist_init[1] = fs->hist[1]; fr0.hist_init[2] = fs->hist[2];
    ZG_HIP(hipMemcpyAsync((void*)d.frames, bb.frames.data(), sizeof(ZgFrame), hipMemcpyHostToDevice, s));
  }
  zg_launch_reset(d, s);   // status words, slot logs, totals, d.dbg: one kernel (in front of the carried tables and dictionary fills, which write into what it clears)
  if (fs && Poison::value() >= 0) {   // the carried tables that do not exist
    const uint32_t offs[3] = {ZG_FSE_LL_OFF, ZG_FSE_OF_OFF, ZG_FSE_ML_OFF}, nent[3] = {512, 256, 512};
    for (int k = 0; k < 3; k++) if (!(fs->carry_mask & (2u << k))) Poison::fill(fs->d_fse.as<uint32_t>() + offs[k], nent[k] * 4, s);
    if (!(fs->carry_mask & 1u)) Poison::fill(fs->d_huf.p, ZG_HUF_SLOT_U16 * 2, s);
  }
  if (fs && fs->carry_mask) {   // tables carried into this run: the frame's carry slots of the two arenas
    const ZgFrame& fr = bb.frames[0];
    ZG_HIP(hipMemcpyAsync(d.fse_arena + (size_t)fr.carry_slot * ZG_FSE_SLOT_U32, fs->d_fse.p, ZG_FSE_SLOT_U32 * 4, hipMemcpyDeviceToDevice, s));
    ZG_HIP(hipMemcpyAsync(d.slot_log + (size_t)fr.carry_slot * 4, fs->logs, 4, hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(d.huf_arena + (size_t)fr.carry_huf_slot * ZG_HUF_SLOT_U16, fs->d_huf.p, ZG_HUF_SLOT_U16 * 2, hipMemcpyDeviceToDevice, s));
    ZG_HIP(hipMemcpyAsync(d.huf_maxbits + fr.carry_huf_slot, &fs->huf_maxbits, 1, hipMemcpyHostToDevice, s));
  }
  if (!frame_dicts_.empty()) { const int st = dictfill_launch(0); if (st) return st; }   // (behind the resets above, in front of the first kernel that reads a carry slot)
  // ---- phase 1: entropy stages + scan. Literals (Huffman tree descriptions -> streams) and sequences (FSE descriptions ->
  // state chains -> post-pass) of a block are independent, and all of these kernels are latency-bound chains that leave most
  // of the chip idle: the two chains run side by side on two streams and meet again in zg_k_merge.
  hipStream_t s2 = eng->stream2_;
  zg_launch_tables(d, s, 1);
  ZG_HIP(hipEventRecord(ev[1], s));
  // The literals chain starts when the FSE tables are done, i.e. together with zg_k_seq: the dispatcher then places the
  // high-priority zg_k_seq workgroups first (all of them must be resident at once: the kernel lasts as long as one
  // block's chain) and the Huffman workgroups fill the LDS that is left. Started earlier, they would sit in the CUs
  // when zg_k_seq arrives and push half of its workgroups into a second round.
  ZG_HIP(hipEventRecord(sc->ev_fork, s));
  ZG_HIP(hipStreamWaitEvent(s2, sc->ev_fork, 0));
  // (literal-heavy submits, BatchBuilder::finish: only the tree descriptions here; the streams are decoded after the scan, when
  //  the blocks without sequences know their place in the output — phase 2)
  const bool lit_direct = bb.lit_direct;
  d.flags &= ~ZG_FLAG_LIT_DIRECT;
  ZG_HIP(hipEventRecord(sc->ev_huf[0], s2));
  zg_launch_tables(d, s2, 0);
  if (!lit_direct) zg_launch_huf(d, s2);
  ZG_HIP(hipEventRecord(sc->ev_huf[1], s2));
  ZG_HIP(hipEventRecord(ev[2], s));
  // (more blocks with sequences than chains the device runs at once — CUs x 32 —: the kernel is then bound by chains per unit of time, not by
  //  the length of one chain, and the packed-entry form holds half as many again per CU)
  zg_launch_seq(d, s, bb.seq_packed);   // (BatchBuilder::finish decided: more blocks with sequences than one round holds -> the packed form)
  ZG_HIP(hipEventRecord(ev[3], s));
  zg_launch_seqpost(d, s);
  ZG_HIP(hipStreamWaitEvent(s, sc->ev_huf[1], 0));
  zg_launch_merge(d, s);
  ZG_HIP(hipEventRecord(ev[4], s));
  { uint32_t mb = 0; for (const ZgFrame& fr : bb.frames) mb = fr.nblocks > mb ? fr.nblocks : mb; zg_launch_scan(d, s, mb); }
  ZG_HIP(hipEventRecord(ev[5], s));
  // ---- the output buffer and the flatten scratch are sized to the frames' exact sizes, which the scan has just computed: one host
  // round trip — unless every frame declares its content size: then both were sized before the run (above), the LZ77 stages go
  // behind the scan right away, and the device checks the promise (zg_k_scanf; a frame that produces more than it declared turns
  // them into no-ops and sync() repeats them the slow way: Frame_Content_Size is never checked by the reference, frame_decoder.rs:541-577).
  if (!presized) { const int st = size_output(); if (st) return st; }
  if (!frame_dicts_.empty()) { const int st = dictfill_launch(1); if (st) return st; }   // (in front of the first kernel that reads or writes the output)
  const int st2 = launch_phase2();
  if (st2) return st2;
  ZG_HIP(hipGetLastError());
  ran = true;
  return ZG_OK;
}

// run()'s phase 1 without the literals chain, with zg_k_seqsize where run() has zg_k_seqpost, and with nothing behind the scan: the sizes
// of the frames and the statuses the sequence stages find, in frame_out. (zg_k_merge is what folds the Huffman chain's verdicts and the
// host's sequences-header verdict into the block statuses; the former do not exist here, and the latter is FrameInfo::host_status of the
// frame, which the caller looks at anyway.) No frame is placed (zg_k_scanf): nothing is produced.
int Batch::measure(uint64_t* phase1_us) {
  ZG_HIP(hipSetDevice(eng->device_));
  hipStream_t s = eng->stream_;
  ZgBatchDev& d = dev;
  if (phase1_us) *phase1_us = 0;
  frame_out.assign(d.nframes, ZgFrameOut{});
  total_out = 0; ran = false; synced = true;
  if (wait_upload) { ZG_HIP(hipStreamWaitEvent(s, sc->ev_up, 0)); wait_upload = false; }
  if (d.nframes == 0 || d.nblocks == 0 || fs) {   // (no block: nothing to launch, as in run(); a continued frame is not measured)
    ZG_HIP(hipStreamSynchronize(s));
    return fs ? ZG_BAD_ARG : ZG_OK;
  }
  hipEvent_t* ev = sc->ev;
  d.dst_cap_pre = 0;
  d.flags &= ~ZG_FLAG_LIT_DIRECT;
  ZG_HIP(hipEventRecord(ev[0], s));
  zg_launch_reset(d, s);
  zg_launch_tables(d, s, 1);
  zg_launch_seq(d, s, bb.seq_packed);
  zg_launch_seqsize(d, s);
  { uint32_t mb = 0; for (const ZgFrame& fr : bb.frames) mb = fr.nblocks > mb ? fr.nblocks : mb; zg_launch_scan_sizes(d, s, mb); }
  ZG_HIP(hipGetLastError());
  ZG_HIP(hipEventRecord(ev[1], s));
  ZG_HIP(hipMemcpyAsync(frame_out.data(), d.frame_out, (size_t)d.nframes * sizeof(ZgFrameOut), hipMemcpyDeviceToHost, s));
  ZG_HIP(hipStreamSynchronize(s));
  if (phase1_us) (void)us_between(ev[0], ev[1], phase1_us);
  return ZG_OK;
}

int Batch::set_frame_dicts(std::vector<zgd::DictImage> images) {
  if (fs || images.size() != bb.frames.size()) return ZG_BAD_ARG;
  bool any = false;
  for (size_t f = 0; f < images.size(); f++) {
    if (images[f].content_len != bb.frames[f].dict_len) return ZG_BAD_ARG;   // (what the walk was told of the dictionary is what the image holds)
    any = any || images[f].content_len;
  }
  if (any) frame_dicts_ = std::move(images);
  else frame_dicts_.clear();
  return ZG_OK;
}

// part 0: every dictionary frame's tables into its carry slots of the two arenas; part 1: every dictionary frame's content into the gap in front of
// its plaintext (frame_out holds the scan's placement: size_output). One launch each; a segment that would leave its buffer is refused.
int Batch::dictfill_launch(int part) {
  const ZgBatchDev& d = dev;
  std::vector<zgd::Seg> segs;
  auto at = [](const void* p) { return (uint64_t)(uintptr_t)p; };
  for (uint32_t f = 0; f < d.nframes; f++) {
    const zgd::DictImage& im = frame_dicts_[f];
    if (!im.content_len) continue;
    const ZgFrame& fr = bb.frames[f];
    if (part == 0) {
      if (fr.carry_slot >= d.nslots || fr.carry_huf_slot < 0 || (uint32_t)fr.carry_huf_slot >= d.nhuf_slots) return ZG_INTERNAL;   // (never: BatchBuilder::finish)
      segs.push_back(zgd::Seg{im.fse, at(d.fse_arena + (size_t)fr.carry_slot * ZG_FSE_SLOT_U32), zgd::kFseBytes});
      segs.push_back(zgd::Seg{im.logs, at(d.slot_log + (size_t)fr.carry_slot * 4), 4});
      segs.push_back(zgd::Seg{im.huf, at(d.huf_arena + (size_t)fr.carry_huf_slot * ZG_HUF_SLOT_U16), zgd::kHufBytes});
      segs.push_back(zgd::Seg{im.maxbits, at(d.huf_maxbits + fr.carry_huf_slot), 1});
    } else {
      const ZgFrameOut& fo = frame_out[f];
      if (fo.out_base < fr.dict_len || fo.out_base > d.dst_cap || fo.out_size > d.dst_cap - fo.out_base) {   // (never: zg_k_scanf laid the gap out)
        eng->last_error = "zg_k_dictfill: a dictionary frame's gap outside the output";
        return ZG_INTERNAL;
      }
      segs.push_back(zgd::Seg{im.content, at(d.dst + (fo.out_base - fr.dict_len)), fr.dict_len});
    }
  }
  if (segs.empty() || segs.size() > 0xFFFFFFFFull) return segs.empty() ? ZG_OK : ZG_INTERNAL;
  std::vector<zgs::Chunk> ch;
  zgd::plan_fill(segs.data(), (uint32_t)segs.size(), 0, &ch);
  if (ch.empty() || ch.size() > 0xFFFFFFFFull) return ch.empty() ? ZG_OK : ZG_INTERNAL;
  const size_t sb = segs.size() * sizeof(zgd::Seg), cb = ch.size() * sizeof(zgs::Chunk);
  SidePass& t = side_[kSideFill0 + part];
  int st = t.reserve(sb + cb);
  if (st) return st;
  hipStream_t s = eng->stream_;
  ZG_HIP(t.upload(segs.data(), sb, ch.data(), cb, s));
  ZG_HIP(hipStreamSynchronize(s));   // (the tables are pageable and go out of scope; the stream is idle here: the uploads, or the scan, were waited for)
  ZG_HIP(t.begin(s));
  zg_launch_dictfill(t.at<zgd::Seg>(0), t.at<zgs::Chunk>(sb), (uint32_t)ch.size(), s);
  ZG_HIP(t.end(s));
  t.n = 1;
  dictfill_launches++;
  for (const zgd::Seg& x : segs) dictfill_bytes += x.len;
  return ZG_OK;
}

int Batch::size_output() {
  hipStream_t s = eng->stream_;
  ZgBatchDev& d = dev;
  frame_out.resize(d.nframes);
  uint32_t totals[4] = {0, 0, 0, 0};
  ZG_HIP(hipMemcpyAsync(frame_out.data(), d.frame_out, (size_t)d.nframes * sizeof(ZgFrameOut), hipMemcpyDeviceToHost, s));
  ZG_HIP(hipMemcpyAsync(totals, d.totals, 16, hipMemcpyDeviceToHost, s));
  ZG_HIP(hipStreamSynchronize(s));
  total_out = (uint64_t)totals[0] | ((uint64_t)totals[1] << 32);
  far_seen = totals[3] != 0;
  int st = 0;
  bool any_fast = false;
  for (const ZgFrameOut& fo : frame_out) any_fast |= fo.fast != 0;
  if (fs) {
    const uint64_t add = frame_out[0].out_size;
    if ((st = fs->make_room(add + kMaxBlockSize, keep_bytes, s))) return st;   // (+ a block: what a block that fails in sequence execution leaves behind the run, zg_k_partial)
    // this run continues the frame: its bytes go right behind what exists, and matches may reach back into it — as far as
    // the caller still holds bytes (DecodeBuffer semantics: repeat() sees only what has not been drained)
    ZgFrame& fr = bb.frames[0];
    fr.prior_out = fs->produced;
    fr.prior_reach = keep_bytes < fs->have ? keep_bytes : fs->have;
    fr.prior_counted = fs->counted;
    fr.dict_len = fs->base;
    fr.out_base_fixed = fs->base + fs->have;
    ZG_HIP(hipMemcpyAsync((void*)d.frames, bb.frames.data(), sizeof(ZgFrame), hipMemcpyHostToDevice, s));
    ZG_HIP(hipMemcpyAsync(&d.frame_out[0].out_base, &fr.out_base_fixed, 8, hipMemcpyHostToDevice, s));
    frame_out[0].out_base = fr.out_base_fixed;
    Poison::fill(fs->d_out.p, kOutFront, s);                                                   // the front pad, and what lies behind [dictionary][have]
    Poison::fill(fs->out_ptr() + fs->base + fs->have, fs->d_out.cap - kOutFront - fs->base - fs->have, s);
    d.dst = fs->out_ptr(); d.dst_cap = fs->base + fs->have + add;
    og_words = add;
  } else {
    if ((st = sc->d_dst.reserve(kOutFront + total_out + 64))) return st;
    Poison::fill(sc->d_dst.p, sc->d_dst.cap, s);
    d.dst = sc->d_dst.as<uint8_t>() + kOutFront; d.dst_cap = total_out;
    og_words = total_out;
  }
  if (any_fast && (st = sc->d_og.reserve(og_words * 4 + 64))) return st;
  Poison::fill(sc->d_og.p, sc->d_og.cap, s);
  d.og = sc->d_og.as<uint32_t>();
  d.og_words = og_words;
  return ZG_OK;
}

int Batch::launch_phase2() {
  hipStream_t s = eng->stream_;
  ZgBatchDev& d = dev;
  hipEvent_t* ev = sc->ev;
  // ---- phase 2: LZ77 execution (and, for literal-heavy submits, the Huffman streams in front of it)
  if (bb.lit_direct) {
    d.flags |= ZG_FLAG_LIT_DIRECT;
    ZG_HIP(hipEventRecord(sc->ev_huf[0], s));
    zg_launch_huf(d, s);
    zg_launch_litfix(d, s);
    ZG_HIP(hipEventRecord(sc->ev_huf[1], s));
  }
  zg_launch_lit(d, s);
  ZG_HIP(hipEventRecord(ev[6], s));
  sweep_mode = 0; synced = false;
  // The direct units (a frame's first unit, resolved to bytes: zg_flat4.h) have a kernel of their own, and with it their own occupancy.
  // ONE unit is flattened fastest by 1024 threads on 16 KiB tiles (the pointer-mode units' kernel, one workgroup per CU); a submit of
  // many direct units — single-block frames, BASELINE config 4b — is flattened fastest by small workgroups, eight to a CU, which overlap
  // each other's barriers (measured on 16384 single-block frames, flatten ms: one kernel 5.23; zg_k_flatten4 with 1024 / 512 / 256 threads
  // and 8 / 4 / 2 KiB tiles 4.23 / 3.84 / 3.59; on 64 x (1 direct + 1 pointer unit) the one kernel is the fastest: 15.3 against 15.7 - 16.9).
  int flat4 = eng->tn_.flat4;
  if (flat4 < 0) {
    const uint32_t cus = (uint32_t)eng->cus_, nd = d.ndirect;
    flat4 = nd >= 16u * cus ? 6 : nd >= 8u * cus ? 4 : nd >= 4u * cus ? 1 : 0;
  }
  // One long frame in ramped units (BatchBuilder::finish): the flatten goes to its own stream and the sweep chain starts at once;
  // a step waits for its unit's flag (zg_k_flatten sets it, zg_k_sweep polls it). ZGPU_OVERLAP=0: one after the other.
  const bool overlap = bb.ramped && eng->tn_.overlap && !eng->tn_.no_sweep;
  d.overlap_epoch = overlap ? ++epoch_ : 0u;
  if (overlap) {
    // the flatten stays on the main stream and is enqueued FIRST; the chain goes to the third stream. (Should the two streams
    // share a hardware queue, the chain then simply runs behind the flatten; the other way round its first step would sit in
    // front of the kernel it waits for.)
    hipStream_t s3 = eng->stream3_;
    ZG_HIP(hipMemsetAsync(d.unit_info, 0, (size_t)d.nunits * sizeof(ZgUnitInfo), s));   // the flags of earlier users of this memory
    ZG_HIP(hipEventRecord(sc->ev_fork3, s));
    zg_launch_flat(d, s, eng->stream2_, sc->ev_flat, flat4);
    ZG_HIP(hipEventRecord(ev[7], s));
    ZG_HIP(hipStreamWaitEvent(s3, sc->ev_fork3, 0));
    launch_sweep(true, s3);
    ZG_HIP(hipEventRecord(sc->ev_fork3, s3));
    ZG_HIP(hipStreamWaitEvent(s, sc->ev_fork3, 0));
  } else {
    zg_launch_flat(d, s, eng->stream2_, sc->ev_flat, flat4);
    { bool any = false; for (const ZgFrame& fr : bb.frames) any = any || fr.sparse; if (any) zg_launch_sparse(d, s); }
    ZG_HIP(hipEventRecord(ev[7], s));
    if (!eng->tn_.no_sweep) launch_sweep(true);
  }
  ZG_HIP(hipEventRecord(ev[8], s));
  zg_launch_lz(d, s);   // only frames that left the flatten path (a block regenerating > 128 KiB)
  ZG_HIP(hipEventRecord(ev[9], s));
  return ZG_OK;
}

// The sweep. split: tails on the main stream, heads beside them on the second one, which is right as long as no match
// reaches further back than its frame's window (zg_k_seqpost reports one that does: sync() then repeats the sweep the plain way).
void Batch::launch_sweep(bool split, hipStream_t main) {
  if (!main) main = eng->stream_;
  if (!eng->tn_.sweep_split) split = false;
  uint64_t wmax = 0, wmin = ~0ull;
  for (const ZgFrame& fr : bb.frames) {
    wmax = fr.window_size > wmax ? fr.window_size : wmax;
    wmin = fr.window_size < wmin ? fr.window_size : wmin;
    // an initial history other than the format's (dictionary, continued frame) may hold offsets nobody checked against the window
    if (fr.hist_init[0] != 1 || fr.hist_init[1] != 4 || fr.hist_init[2] != 8 || fr.dict_len || fr.prior_out) split = false;
  }
  if (dev.sweep_window) wmax = wmin = dev.sweep_window;
  if (wmax > 0x7FFFFFFFull) wmax = 0x7FFFFFFFull;
  if (wmin > wmax) wmin = wmax;
  split_sweep = zg_launch_sweep(dev, main, sweep_steps.data(), (uint32_t)sweep_steps.size(), eng->stream2_, sc->ev_sw, split ? 80u : 0u,
                                bb.unit_blocks_used * kMaxBlockSize, (uint32_t)wmax, (uint32_t)wmin, eng->tn_.sweep);
  sweep_mode = split_sweep ? 1u : sweep_mode;
}

void Batch::release_scratch() {
  if (!sc || !eng || !synced) return;
  (void)hipSetDevice(eng->device_);
  sc->release_but_output();
  dev.og = nullptr; dev.src = nullptr; dev.lit_arena = nullptr; dev.seq_arena = nullptr; dev.raw_arena = nullptr;
  ran = false;                     // (the submit cannot be run again; reading its output stays possible)
}

int Batch::sync() {
  ZG_HIP(hipSetDevice(eng->device_));
  ZG_HIP(hipStreamSynchronize(eng->stream_));
  if (dev.nframes == 0 || !ran) return ZG_OK;
  if (presized) {
    // what run() did not wait for: the frames' sizes, and whether they kept their promise
    uint32_t totals[4] = {0, 0, 0, 0};
    ZG_HIP(hipMemcpy(totals, dev.totals, 16, hipMemcpyDeviceToHost));
    total_out = (uint64_t)totals[0] | ((uint64_t)totals[1] << 32);
    far_seen = totals[3] != 0;
    frame_out.resize(dev.nframes);
    if (totals[2]) {
      // a frame produced more than it declared: the LZ77 stages did nothing (every kernel checks the flag). Size the buffers from
      // what the scan found and run them now, the way a submit without declared sizes goes.
      presized = false;
      dev.dst_cap_pre = 0;
      uint32_t zero = 0;
      ZG_HIP(hipMemcpy(dev.totals + 2, &zero, 4, hipMemcpyHostToDevice));
      int st = size_output();
      if (!st) st = launch_phase2();
      if (st) return st;
      ZG_HIP(hipStreamSynchronize(eng->stream_));
    }
  }
  if (split_sweep) {
    uint32_t far = 0;
    ZG_HIP(hipMemcpy(&far, dev.totals + 3, 4, hipMemcpyDeviceToHost));
    if (far) {   // a match longer than the window: the heads may have copied bytes that were not final yet
      launch_sweep(false);
      ZG_HIP(hipStreamSynchronize(eng->stream_));
      sweep_mode = 2;
    }
    split_sweep = false;
  }
  ZG_HIP(hipMemcpy(frame_out.data(), dev.frame_out, (size_t)dev.nframes * sizeof(ZgFrameOut), hipMemcpyDeviceToHost));
  {
    // The fast path treats every byte the frame has produced as reachable and approximates which of the two "offset too far"
    // errors applies; the reference's DecodeBuffer is stricter (zg_exact.h). Where that can change a verdict — an offset beyond
    // the window was seen, a frame ended with one of those errors, a dictionary is involved — the exact bookkeeping is replayed.
    bool need = far_seen;
    for (uint32_t f = 0; f < dev.nframes && !need; f++) {
      const ZgFrame& fr = bb.frames[f];
      const uint32_t st = frame_out[f].status;
      need = st == (uint32_t)ZG_EXE_OFFSET_TOO_BIG || st == (uint32_t)ZG_EXE_DICT_TOO_SMALL || fr.dict_len != 0 ||
             st == (uint32_t)ZG_EXE_NOT_ENOUGH_LITERALS || st == (uint32_t)ZG_EXE_ZERO_OFFSET ||   // (a sequence in front of the rejected one may reach too far: that comes first)
             fr.hist_init[0] > fr.window_size || fr.hist_init[1] > fr.window_size || fr.hist_init[2] > fr.window_size;
    }
    if (need && !eng->tn_.no_exact) {
      zg_launch_exact(dev, eng->stream_, drain_rule);
      ZG_HIP(hipStreamSynchronize(eng->stream_));
      ZG_HIP(hipMemcpy(frame_out.data(), dev.frame_out, (size_t)dev.nframes * sizeof(ZgFrameOut), hipMemcpyDeviceToHost));
      exact_ran = true;
    }
  }
  // a frame that failed in the execution stage (zg_k_flatten / zg_k_exact / zg_k_lz) still carries the size of all its blocks:
  // what it produced ends with its last good block, as for the entropy errors zg_k_scan trims itself
  // (host-side only: total_out and the device copy of frame_out keep the untrimmed sizes. One copy per failed frame while they are few; a
  //  submit of many corrupt frames fetches the block positions once instead of paying a round trip per frame — ADVICE r4)
  {
    uint32_t nfail = 0;
    for (uint32_t f = 0; f < dev.nframes; f++) nfail += frame_out[f].status && frame_out[f].good_blocks < bb.frames[f].nblocks;
    std::vector<ZgBlockPos> all_pos;
    if (nfail > 8) { all_pos.resize(dev.nblocks); ZG_HIP(hipMemcpy(all_pos.data(), dev.pos, (size_t)dev.nblocks * sizeof(ZgBlockPos), hipMemcpyDeviceToHost)); }
    for (uint32_t f = 0; f < dev.nframes && nfail; f++) {
      ZgFrameOut& fo = frame_out[f];
      const ZgFrame& fr = bb.frames[f];
      if (!fo.status || fo.good_blocks >= fr.nblocks) continue;
      ZgBlockPos p;
      if (!all_pos.empty()) p = all_pos[fr.first_block + fo.good_blocks];
      else ZG_HIP(hipMemcpy(&p, dev.pos + fr.first_block + fo.good_blocks, sizeof p, hipMemcpyDeviceToHost));
      if (p.out_base < fo.out_size) fo.out_size = p.out_base;
    }
  }
  // A run of ONE frame that is decoded run by run (the FrameDecoder mirror, the thin boundary, the streaming decoder: fs) and failed in
  // sequence execution: the reference's decode buffer also holds what the failing block wrote before it failed — the output of the
  // sequences in front of the one that could not be executed, and that one's literals unless it was the literals that ran out
  // (sequence_execution.rs:6-52) — and hands it out like any other byte (collect / read after the Err). zg_k_partial produces exactly
  // that behind the good blocks' bytes. (Frames of a many-frame submit end with their last good block: include/zgpu.h.)
  if (fs && dev.nframes == 1 && !frame_out.empty()) {
    ZgFrameOut& fo = frame_out[0];
    const ZgFrame& fr = bb.frames[0];
    const uint32_t st = fo.status;
    const bool exe = st == (uint32_t)ZG_EXE_NOT_ENOUGH_LITERALS || st == (uint32_t)ZG_EXE_ZERO_OFFSET || st == (uint32_t)ZG_EXE_OFFSET_TOO_BIG ||
                     st == (uint32_t)ZG_EXE_DICT_TOO_SMALL;
    if (exe && fo.good_blocks < fr.nblocks) {
      const uint32_t b = fr.first_block + fo.good_blocks;
      const ZgBlock& blk = bb.blocks[b];
      ZgBlockSeqOut so;
      memset(&so, 0, sizeof so);
      if (blk.btype == ZG_BT_COMPRESSED && blk.nseq && !blk.host_status)
        ZG_HIP(hipMemcpy(&so, dev.seq_out + b, sizeof so, hipMemcpyDeviceToHost));
      if (so.pad && so.pad <= blk.nseq) {                       // 1 + the sequence that failed (zg_k_seqpost, or zg_k_exact where it decided)
        const uint32_t j = so.pad - 1u;
        const bool lits = st != (uint32_t)ZG_EXE_NOT_ENOUGH_LITERALS;   // (:14-19 come before the push; the offset checks :28-38 behind it)
        // room behind the good blocks: the block of slack size_output reserved — and, when the scan still counted the failing block (an
        // error found while executing: the in-order path, the flatten), that block's own place
        const uint64_t used = kOutFront + fs->base + fs->have + fo.out_size;
        const uint64_t room = fs->d_out.cap > used + 64 ? fs->d_out.cap - used - 64 : 0;
        const uint32_t limit = room > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)room;
        zg_launch_partial(dev, eng->stream_, 0, b, j, lits, limit);
        ZG_HIP(hipStreamSynchronize(eng->stream_));
        uint32_t psize = 0;
        ZG_HIP(hipMemcpy(&psize, dev.totals + 5, 4, hipMemcpyDeviceToHost));
        if (psize != 0xFFFFFFFFu) {                             // (else: more than there is room for — a block beyond 128 KiB rejected by zg_k_seqpost: left out)
          fo.out_size += psize;
          dev.dst_cap += psize;
        }
      }
    }
  }
  hipEvent_t* ev = sc->ev;
  for (int i = 0; i < ZG_T_TOTAL; i++) {
    float m = 0;
    if (hipEventElapsedTime(&m, ev[i], ev[i + 1]) == hipSuccess) ms[i] = m;
  }
  float m = 0;
  dictfill_us = 0;
  for (int k = 0; k < 2; k++) {
    uint64_t us = 0;
    if (side_[kSideFill0 + k].n && side_[kSideFill0 + k].elapsed_us(&us) == hipSuccess) dictfill_us += us;
  }
  if (hipEventElapsedTime(&m, sc->ev_huf[0], sc->ev_huf[1]) == hipSuccess) ms[ZG_T_HUF] = m;   // beside seq + seqpost, not in line ...
  if (dev.flags & ZG_FLAG_LIT_DIRECT) ms[ZG_T_LIT] = ms[ZG_T_LIT] > ms[ZG_T_HUF] ? ms[ZG_T_LIT] - ms[ZG_T_HUF] : 0.f;   // ... or, after the scan, in front of zg_k_lit
  if (hipEventElapsedTime(&m, ev[0], ev[ZG_T_TOTAL]) == hipSuccess) ms[ZG_T_TOTAL] = m;
  synced = true;
  return ZG_OK;
}

// which tables exist once this run has been folded into the frame's state (what commit() will leave in FrameState::carry_mask): the
// streaming decoder prepares the NEXT run while this one is still on the GPU
uint32_t Batch::carry_mask_after() const {
  uint32_t m = carry_mask_in;
  if (bb.frames.empty()) return m;
  const Lineage fl = bb.final_lineage();
  const int32_t sl[3] = {fl.ll, fl.of, fl.ml};
  const int32_t carry = (int32_t)bb.frames[0].carry_slot;
  for (int k = 0; k < 3; k++) if (sl[k] >= 0 && sl[k] != carry) m |= 2u << k;
  if (fl.huf >= 0 && fl.huf != (int32_t)bb.frames[0].carry_huf_slot) m |= 1u;
  return m;
}

int Batch::commit(FrameState* st) {
  // fold a finished streaming run into the frame state: DecoderScratch after decode_block_content
  if (dev.nframes != 1 || frame_out.size() != 1) return ZG_BAD_ARG;
  const ZgFrameOut& fo = frame_out[0];
  st->produced += fo.out_size;
  st->have += fo.out_size;
  st->hist[0] = fo.hist_end[0]; st->hist[1] = fo.hist_end[1]; st->hist[2] = fo.hist_end[2];
  st->counted += fo.counted;
  if (fo.status) return ZG_OK;   // the frame failed: the caller reports it; tables are not needed any more
  const Lineage fl = bb.final_lineage();
  hipStream_t s = eng->stream_;
  const int32_t sl[3] = {fl.ll, fl.of, fl.ml};
  const uint32_t offs[3] = {ZG_FSE_LL_OFF, ZG_FSE_OF_OFF, ZG_FSE_ML_OFF}, nent[3] = {512, 256, 512};
  const int32_t carry = (int32_t)bb.frames[0].carry_slot;
  for (int k = 0; k < 3; k++) {
    if (sl[k] < 0 || sl[k] == carry) continue;   // never set, or still the carried table
    ZG_HIP(hipMemcpyAsync(st->d_fse.as<uint32_t>() + offs[k], dev.fse_arena + (size_t)sl[k] * ZG_FSE_SLOT_U32 + offs[k], nent[k] * 4,
                          hipMemcpyDeviceToDevice, s));
    ZG_HIP(hipMemcpyAsync(&st->logs[k], dev.slot_log + (size_t)sl[k] * 4 + k, 1, hipMemcpyDeviceToHost, s));
    st->carry_mask |= 2u << k;
  }
  if (fl.huf >= 0 && fl.huf != bb.frames[0].carry_huf_slot) {
    ZG_HIP(hipMemcpyAsync(st->d_huf.p, dev.huf_arena + (size_t)fl.huf * ZG_HUF_SLOT_U16, ZG_HUF_SLOT_U16 * 2, hipMemcpyDeviceToDevice, s));
    ZG_HIP(hipMemcpyAsync(&st->huf_maxbits, dev.huf_maxbits + fl.huf, 1, hipMemcpyDeviceToHost, s));
    st->carry_mask |= 1u;
  }
  ZG_HIP(hipStreamSynchronize(s));
  return ZG_OK;
}

int Batch::read_output(uint64_t off, uint8_t* dst, uint64_t n) {
  if (ran && !synced) { const int st = sync(); if (st) return st; }   // (sync() may still have to repeat the sweep)
  if (off + n > dev.dst_cap) return ZG_BAD_ARG;
  if (n) {   // on the engine's second stream (idle once the run is synced): several engines' downloads and uploads overlap
    // (a large download as two halves on two streams: a single copy may get one copy engine, ~28 GB/s, where two copies get one each — what a
    //  process has done on the device before decides, LABNOTES round 6)
    const uint64_t h = n >= (8u << 20) ? (n / 2 + 4095) & ~4095ull : n;
    ZG_HIP(hipMemcpyAsync(dst, dev.dst + off, h, hipMemcpyDeviceToHost, eng->stream2_));
    if (n > h) ZG_HIP(hipMemcpyAsync(dst + h, dev.dst + off + h, n - h, hipMemcpyDeviceToHost, eng->stream5_));
    ZG_HIP(hipStreamSynchronize(eng->stream2_));
    if (n > h) ZG_HIP(hipStreamSynchronize(eng->stream5_));
  }
  return ZG_OK;
}
int Batch::hash_launch(const uint32_t* frames, uint32_t n, uint32_t quad_max_ranges) {
  ZG_HIP(hipSetDevice(eng->device_));
  SidePass& p = side_[kSideHash];
  p.n = 0;
  if (!n) return ZG_OK;
  if (!synced) return ZG_BAD_ARG;
  // longest first: the 64 lanes of a wave get ranges of similar length (a wave lasts as long as its longest lane), and the longest waves start first
  std::vector<ZgHashRange> r(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t f = frames[i];
    if (f >= frame_out.size()) return ZG_BAD_ARG;
    r[i].off = frame_out[f].out_base; r[i].len = frame_out[f].out_size; r[i].slot = i; r[i].pad = 0;
    if (r[i].len && (r[i].off > dev.dst_cap || r[i].len > dev.dst_cap - r[i].off)) return ZG_INTERNAL;   // (never: sync() trims, it does not grow)
  }
  std::stable_sort(r.begin(), r.end(), [](const ZgHashRange& a, const ZgHashRange& b) { return a.len > b.len; });
  const size_t rb = (size_t)n * sizeof(ZgHashRange);
  int st = p.reserve(rb + (size_t)n * 8);
  if (st) return st;
  hipStream_t s = eng->stream_;
  ZG_HIP(p.upload(r.data(), rb, nullptr, 0, s));
  ZG_HIP(hipStreamSynchronize(s));   // (r is pageable and goes out of scope)
  ZG_HIP(p.begin(s));
  zg_launch_xxh64_with(dev.dst, p.at<ZgHashRange>(0), p.at<uint64_t>(rb), n, s, n <= quad_max_ranges ? 4 : 0);
  ZG_HIP(p.end(s));
  p.n = n;
  p.back = rb;
  return ZG_OK;
}
int Batch::hash_wait(uint64_t* out, uint64_t* kernel_us) {
  SidePass& p = side_[kSideHash];
  if (kernel_us) *kernel_us = 0;
  if (!p.n) return ZG_OK;
  ZG_HIP(hipSetDevice(eng->device_));
  ZG_HIP(hipStreamSynchronize(eng->stream_));
  if (kernel_us) ZG_HIP(p.elapsed_us(kernel_us));
  ZG_HIP(hipMemcpy(out, p.at<uint8_t>(p.back), (size_t)p.n * 8, hipMemcpyDeviceToHost));
  p.n = 0;
  return ZG_OK;
}
int Batch::scatter_launch(const zgs::Seg* segs, uint32_t n, uint32_t chunk) {
  ZG_HIP(hipSetDevice(eng->device_));
  SidePass& p = side_[kSideScatter];
  p.n = 0;
  if (!n) return ZG_OK;
  if (!synced) return ZG_BAD_ARG;
  for (uint32_t i = 0; i < n; i++)   // reads stay inside the output: the lanes read [src_off, src_off + len) and nothing else (zg_scatter.h)
    if (segs[i].len && (segs[i].src_off > dev.dst_cap || segs[i].len > dev.dst_cap - segs[i].src_off)) return ZG_INTERNAL;
  std::vector<zgs::Chunk> ch;
  zgs::plan_chunks(segs, n, chunk, &ch);
  if (ch.empty()) return ZG_OK;
  if (ch.size() > 0xFFFFFFFFull) return ZG_INTERNAL;
  const size_t sb = (size_t)n * sizeof(zgs::Seg), cb = ch.size() * sizeof(zgs::Chunk);
  int st = p.reserve(sb + cb);
  if (st) return st;
  hipStream_t s = eng->stream2_;
  ZG_HIP(p.upload(segs, sb, ch.data(), cb, s));
  ZG_HIP(hipStreamSynchronize(s));   // (the tables are pageable, and ch goes out of scope)
  ZG_HIP(p.begin(s));
  zg_launch_scatter(dev.dst, p.at<zgs::Seg>(0), p.at<zgs::Chunk>(sb), (uint32_t)ch.size(), s);
  ZG_HIP(p.end(s));
  p.n = 1;
  return ZG_OK;
}
int Batch::scatter_wait(uint64_t* kernel_us, bool* launched) {
  SidePass& p = side_[kSideScatter];
  *kernel_us = 0;
  *launched = p.n != 0;
  if (!p.n) return ZG_OK;
  ZG_HIP(hipSetDevice(eng->device_));
  p.n = 0;
  ZG_HIP(hipStreamSynchronize(eng->stream2_));
  ZG_HIP(p.elapsed_us(kernel_us));
  return ZG_OK;
}
// What the two compare launches share. L: the route's Lane (frame_lo, frame_n: its slice). p's buffer holds lanes | frames | records; the
// tables travel on the second stream (idle: the scatter waits for the verdicts) and launch(lanes, frames, digests, records, stream) goes
// behind the hash kernel on the first, which is not waited for.
template <class L, class Launch>
int Batch::compare_launch(SidePass& p, const L* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes, Launch launch) {
  ZG_HIP(hipSetDevice(eng->device_));
  p.n = 0;
  if (!n) return ZG_OK;
  if (!synced) return ZG_BAD_ARG;
  const SidePass& h = side_[kSideHash];
  for (uint32_t i = 0; i < n; i++)   // a wave reads its own slice of the list and the digests that slice names (zg_seeksums.h)
    if (lanes[i].frame_lo > nframes || lanes[i].frame_n > nframes - lanes[i].frame_lo) return ZG_INTERNAL;
  for (uint32_t q = 0; q < nframes; q++)
    if (frames[q].slot != zgv::kNotHashed && frames[q].slot >= h.n) return ZG_INTERNAL;
  const size_t lb = (size_t)n * sizeof(L), fb = (size_t)nframes * sizeof(zgv::Frame), ob = (size_t)n * sizeof(zgv::Sums);
  int st = p.reserve(lb + fb + ob);
  if (st) return st;
  hipStream_t up = eng->stream2_, s = eng->stream_;
  ZG_HIP(p.upload(lanes, lb, frames, fb, up));
  ZG_HIP(hipStreamSynchronize(up));   // (the tables are pageable)
  ZG_HIP(p.begin(s));
  launch(p.at<L>(0), p.at<zgv::Frame>(lb), h.n ? h.at<uint64_t>(h.back) : nullptr, p.at<zgv::Sums>(lb + fb), s);
  ZG_HIP(p.end(s));
  p.n = n;
  p.back = lb + fb;
  return ZG_OK;
}
int Batch::seeksums_launch(const zgv::Lane* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes) {
  return compare_launch(side_[kSideTable], lanes, n, frames, nframes, [&](const zgv::Lane* l, const zgv::Frame* f, const uint64_t* dig, zgv::Sums* out, hipStream_t s) {
    zg_launch_seeksums(l, n, f, dig, side_[kSideHash].n, out, s);
  });
}
int Batch::idxsums_launch(const zgh::Lane* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes, const void* pairs, uint64_t npairs,
                          const uint32_t* sums, uint64_t nsums) {
  side_[kSideHandle].n = 0;
  if (n && (!synced || !pairs || (!sums && nsums))) return ZG_BAD_ARG;
  for (uint32_t i = 0; i < n; i++) {   // a wave reads pairs [first, first + taken] and sums [first, first + taken) of its entry (zg_idxsums.h)
    const zgh::Lane& l = lanes[i];
    if (l.pair0 > npairs || (uint64_t)l.nrows + 1 > npairs - l.pair0 || l.sum0 > nsums || l.nrows > nsums - l.sum0) return ZG_INTERNAL;
  }
  return compare_launch(side_[kSideHandle], lanes, n, frames, nframes, [&](const zgh::Lane* l, const zgv::Frame* f, const uint64_t* dig, zgv::Sums* out, hipStream_t s) {
    zg_launch_idxsums(l, n, pairs, sums, f, dig, side_[kSideHash].n, out, s);
  });
}
int Batch::compare_wait(bool by_handle, zgv::Sums* out, uint64_t* kernel_us, uint64_t* bytes) {
  SidePass& p = side_[by_handle ? kSideHandle : kSideTable];
  *kernel_us = 0; *bytes = 0;
  if (!p.n) return ZG_OK;
  ZG_HIP(hipSetDevice(eng->device_));
  ZG_HIP(hipStreamSynchronize(eng->stream_));
  ZG_HIP(p.elapsed_us(kernel_us));
  *bytes = (uint64_t)p.n * sizeof(zgv::Sums);
  ZG_HIP(hipMemcpy(out, p.at<uint8_t>(p.back), (size_t)*bytes, hipMemcpyDeviceToHost));
  p.n = 0;
  return ZG_OK;
}
// The records pass (zg_records.h). p's buffer holds chunks | fstart | counts | prefixes | totals; everything runs on the first stream.
int Batch::records_launch(const zgr::Chunk* chunks, uint32_t nchunks, const uint32_t* fstart, uint32_t nframes, uint32_t d) {
  ZG_HIP(hipSetDevice(eng->device_));
  SidePass& p = side_[kSideRecords];
  p.n = 0;
  rec_.emitted = false;
  if (!nchunks) return ZG_OK;
  if (!synced || d > 255u) return ZG_BAD_ARG;
  if ((uintptr_t)dev.dst % 16) return ZG_INTERNAL;   // (never: the output lies kOutFront bytes into an allocation)
  for (uint32_t i = 0; i < nchunks; i++) {   // a wave reads [out_off, out_off + len) and nothing else
    const zgr::Chunk& c = chunks[i];
    if (!c.len || c.len > zgr::kChunk || c.out_off > dev.dst_cap || c.len > dev.dst_cap - c.out_off || c.frame >= nframes) return ZG_INTERNAL;
  }
  for (uint32_t f = 0; f < nframes; f++) if (fstart[f] > fstart[f + 1] || fstart[f + 1] > nchunks) return ZG_INTERNAL;
  const size_t cb = (size_t)nchunks * sizeof(zgr::Chunk), fb = ((size_t)nframes + 1) * 4;
  rec_.counts = (cb + fb + 7) & ~(size_t)7;
  rec_.prefix = (rec_.counts + (size_t)nchunks * 4 + 7) & ~(size_t)7;
  rec_.totals = rec_.prefix + (size_t)nchunks * 8;
  rec_.nframes = nframes; rec_.d = d;
  int st = p.reserve(rec_.totals + ((size_t)nframes + 1) * 8);
  if (st) return st;
  hipStream_t s = eng->stream_;
  ZG_HIP(p.upload(chunks, cb, fstart, fb, s));
  ZG_HIP(hipStreamSynchronize(s));   // (the tables are pageable)
  ZG_HIP(p.begin(s));
  zg_launch_recs_count(dev.dst, p.at<zgr::Chunk>(0), nchunks, d, p.at<uint32_t>(rec_.counts), s);
  zg_launch_recs_scan(p.at<uint32_t>(rec_.counts), nchunks, p.at<uint32_t>(cb), nframes, p.at<uint64_t>(rec_.prefix), p.at<uint64_t>(rec_.totals), s);
  ZG_HIP(p.end(s));
  p.n = nchunks;
  return ZG_OK;
}
int Batch::records_sizes(uint64_t* total, uint64_t* ftot, uint64_t* kernel_us, uint64_t* bytes) {
  SidePass& p = side_[kSideRecords];
  *total = 0; *kernel_us = 0; *bytes = 0;
  if (!p.n) return ZG_OK;
  ZG_HIP(hipSetDevice(eng->device_));
  ZG_HIP(hipStreamSynchronize(eng->stream_));
  ZG_HIP(p.elapsed_us(kernel_us));
  std::vector<uint64_t> t((size_t)rec_.nframes + 1);
  *bytes = t.size() * 8;
  ZG_HIP(hipMemcpy(t.data(), p.at<uint8_t>(rec_.totals), (size_t)*bytes, hipMemcpyDeviceToHost));
  *total = t[0];
  uint64_t sum = 0;
  for (uint32_t f = 0; f < rec_.nframes; f++) { ftot[f] = t[1 + f]; sum += t[1 + f]; }
  return sum == t[0] ? ZG_OK : ZG_INTERNAL;   // (never: the frames' chunks are all the chunks)
}
int Batch::records_emit(uint64_t* staging, uint64_t total) {
  SidePass& p = side_[kSideRecords];
  if (!p.n || !total) return ZG_OK;
  if (!staging) return ZG_BAD_ARG;
  ZG_HIP(hipSetDevice(eng->device_));
  hipStream_t s = eng->stream_;
  ZG_HIP(p.begin(s));
  zg_launch_recs_emit(dev.dst, p.at<zgr::Chunk>(0), p.n, rec_.d, p.at<uint64_t>(rec_.prefix), staging, total, s);
  ZG_HIP(p.end(s));
  rec_.emitted = true;
  return ZG_OK;
}
int Batch::records_wait(uint64_t* kernel_us) {
  SidePass& p = side_[kSideRecords];
  *kernel_us = 0;
  const bool emitted = p.n && rec_.emitted;
  p.n = 0;
  if (!emitted) return ZG_OK;
  ZG_HIP(hipSetDevice(eng->device_));
  ZG_HIP(hipStreamSynchronize(eng->stream_));
  ZG_HIP(p.elapsed_us(kernel_us));
  return ZG_OK;
}
int Batch::read_output_async(uint64_t off, uint8_t* dst, uint64_t n, hipStream_t s) {
  if (off + n > dev.dst_cap) return ZG_BAD_ARG;
  if (n) ZG_HIP(hipMemcpyAsync(dst, dev.dst + off, n, hipMemcpyDeviceToHost, s));
  return ZG_OK;
}
int Batch::read_block_status(std::vector<uint32_t>* out) {
  out->resize(dev.nblocks);
  if (dev.nblocks) ZG_HIP(hipMemcpy(out->data(), dev.status, (size_t)dev.nblocks * 4, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::read_literals(uint32_t block, std::vector<uint8_t>* out) {
  if (block >= dev.nblocks) return ZG_BAD_ARG;
  const ZgBlock& b = bb.blocks[block];
  out->clear();
  if (b.btype != ZG_BT_COMPRESSED || b.lit_type < ZG_LT_COMPRESSED) return ZG_OK;
  out->resize(b.regen_size);
  const uint8_t* at = dev.lit_arena + b.lit_base;
  if ((dev.flags & ZG_FLAG_LIT_DIRECT) && b.nseq == 0) {   // zg_k_huf wrote them straight to the block's place in the output
    ZgBlockPos p;
    ZG_HIP(hipMemcpy(&p, dev.pos + block, sizeof p, hipMemcpyDeviceToHost));
    if (b.frame >= frame_out.size() || !p.active) { out->clear(); return ZG_OK; }
    at = dev.dst + frame_out[b.frame].out_base + p.out_base;
  }
  if (b.regen_size) ZG_HIP(hipMemcpy(out->data(), at, b.regen_size, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::read_sequences(uint32_t block, std::vector<ZgSeq>* seqs, ZgBlockSeqOut* so, ZgBlockPos* pos) {
  if (block >= dev.nblocks) return ZG_BAD_ARG;
  const ZgBlock& b = bb.blocks[block];
  seqs->resize(b.btype == ZG_BT_COMPRESSED ? b.nseq : 0);
  if (!seqs->empty()) ZG_HIP(hipMemcpy(seqs->data(), dev.seq_arena + b.seq_base, seqs->size() * sizeof(ZgSeq), hipMemcpyDeviceToHost));
  if (so) ZG_HIP(hipMemcpy(so, dev.seq_out + block, sizeof *so, hipMemcpyDeviceToHost));
  if (pos) ZG_HIP(hipMemcpy(pos, dev.pos + block, sizeof *pos, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::read_fse_slot(uint32_t slot, std::vector<uint32_t>* entries, uint8_t logs[4]) {
  if (slot >= dev.nslots) return ZG_BAD_ARG;
  entries->resize(ZG_FSE_SLOT_U32);
  ZG_HIP(hipMemcpy(entries->data(), dev.fse_arena + (size_t)slot * ZG_FSE_SLOT_U32, ZG_FSE_SLOT_U32 * 4, hipMemcpyDeviceToHost));
  ZG_HIP(hipMemcpy(logs, dev.slot_log + (size_t)slot * 4, 4, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::read_scratch(int what, uint64_t off, void* dst, uint64_t n) {
  const uint8_t* base = what == 0 ? (const uint8_t*)dev.og : what == 1 ? (const uint8_t*)dev.unit_info : nullptr;
  const uint64_t cap = what == 0 ? og_words * 4 : bb.units.size() * sizeof(ZgUnitInfo);
  if (!base || off + n > cap) return ZG_BAD_ARG;
  if (n) ZG_HIP(hipMemcpy(dst, base + off, n, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::unit_scratch_base(uint32_t unit, uint64_t* base) {
  if (unit >= bb.units.size()) return ZG_BAD_ARG;
  const ZgUnit& u = bb.units[unit];
  ZgBlockPos p;
  ZG_HIP(hipMemcpy(&p, dev.pos + u.first_block, sizeof p, hipMemcpyDeviceToHost));
  if (u.frame >= frame_out.size()) return ZG_BAD_ARG;
  *base = frame_out[u.frame].og_base + p.out_base;
  return ZG_OK;
}
int Batch::read_debug(uint64_t out[1024]) {
  for (int i = 0; i < 1024; i++) out[i] = 0;
  if (dev.dbg) ZG_HIP(hipMemcpy(out, dev.dbg, 8192, hipMemcpyDeviceToHost));
  return ZG_OK;
}
int Batch::read_huf_slot(uint32_t slot, std::vector<uint16_t>* entries, int* max_bits) {
  if (slot >= dev.nhuf_slots) return ZG_BAD_ARG;
  entries->resize(ZG_HUF_SLOT_U16);
  uint8_t mb = 0;
  ZG_HIP(hipMemcpy(entries->data(), dev.huf_arena + (size_t)slot * ZG_HUF_SLOT_U16, ZG_HUF_SLOT_U16 * 2, hipMemcpyDeviceToHost));
  ZG_HIP(hipMemcpy(&mb, dev.huf_maxbits + slot, 1, hipMemcpyDeviceToHost));
  *max_bits = mb;
  return ZG_OK;
}

}  // namespace zg
