// zg_frames.cpp — zgpu_decode_frames (include/zgpu.h): n independent buffers, each what FrameDecoder::decode_all (frame_decoder.rs:541-577)
// would take, decoded in few submits, with a verdict per buffer and the content checksums of the frames it held.
//
// Every entry is walked on its own (parse_frames, decode_all's rule: the first header that cannot be read ends the walk of THAT entry) and its
// frames are appended to one submit (Engine::prepare_entries); frames decode independently on the device, so an entry's verdict is
// zgpu_decode_all's logic applied to its own frames: a device error in them, else its walk error, else TargetTooSmall, else success.
// Entries the one-submit path does not serve as zgpu_decode_all would (dictionary frames; Unsupported / Internal) are decoded again on their
// own after the submit. Submits hold at most kFramesSubmitBytes of plaintext (bounded from the block headers); an entry is never split.
//
// zgpu_decode_frames_device is the same call with destinations in device memory of the caller: the walk, the verdicts, the again-list and the
// submit cutting are shared (decode_submit, decode_entries); what differs is the sink of a submit's plaintext — the host sink downloads it and
// copies it to the callers' buffers, the device sink leaves it where it is and lets zg_k_scatter (zg_scatter.h) copy the frames of every
// successful entry to their destinations in one launch, and hashes on the device only. Every destination is checked against the HIP runtime's
// allocations before anything is launched (check_device_range): a wrong pointer becomes a status, never a GPU fault.
//
// zgpu_decode_frames_device_src is that call with the SOURCES in device memory too. The host still owns every verdict, the lineage and the
// launch plan, but it reads a skeleton instead of the bytes: zg_k_walk (zg_walk.h) follows the header chain of every entry, one lane each, in
// two launches for the whole call, and brings back a 32-byte record per frame header, block and checksum; parse_frames_skel and
// plaintext_bound_skel (zg_host_parse.cpp) are the host's one walk run over those records. A submit's entries reach the engine's source buffer
// by one zg_k_gather launch in place of the staging copy and the H2D (Engine::prepare_entries_device). Submit cutting, verdicts, the sink and
// the again-list are the code above; an entry of the again-list is downloaded (one D2H) and decoded alone from the host copy.
//
// zgpu_set_frames_shared_dicts(ctx, 1): dictionary frames whose id is registered stay in the submit. The walk is handed a lookup (shared_lookup)
// and starts such a frame from the dictionary's history and tables; its place in the batch output is [gap of the content's length][plaintext],
// zg_k_dictfill (zg_dictfill.h) replicates the dictionary's device copy into the gaps and carry slots, and zg_k_exact replays the reference's
// buffer bookkeeping for every such frame as it does for a one-frame run. The verdict of an entry that holds a dictionary frame is put together
// in zgpu_decode_all's order for such an entry — frame by frame (zg_decode_all_per_frame) — and what the submit cannot serve exactly (an
// unregistered id, Unsupported / Internal: the dictionary splice behind a drain inside decode_all, zg_exact.h) goes alone as before.
//
// How a call is put together. A Call is what every call has (context, sources, lengths, destinations, capacities, the shared-dictionary
// lookup) plus up to three parts that are built for it and hung in: DeviceSink (device_sink: the options, the one place that refuses
// ZGPU_DEVICE_NO_HASH with ZGPU_DEVICE_VERIFY), DeviceSources (check_entries + device_sources: pointer checks, zg_k_walk, bounds) and Ranges
// (decode_selections: the clips; the one place that builds a Call with all three, for the range calls of zg_ranges.cpp, which are front-ends
// of this machinery — zg_frames_int.h declares what crosses that seam). decode_submit, the sinks, decode_alone_device and
// decode_entries ask for a part by its pointer — `if (k.sink)`, `if (k.src)`, `if (k.ranges)` — never by which field happens to be set.
// Around them: reset_stats zeroes the statistics a call family owns (kOwns*), device_ptr_ok is the one question asked of a pointer and
// check_entries / check_entry_ranges the two loops that ask it in front of the engine's lane passes, drain the two-stream wait every call
// ends with, hash_launch / hash_wait the hashing both sinks start before they copy. Every statistics slot is written under its name (zg_capi_int.h,
// kPass*).
// What an entry's result is. decode_submit and decode_alone PRODUCE facts (zg_entry.h: zge::Frame, zge::Entry) — from frame_out, info and the walk,
// or from the FrameDecoder mirror's frame-by-frame pass — and everything that turns facts into a result is written once, there: the order of
// verdicts (ladder), the two checksum verdicts (verify_fails, table_fails), the frame list of the seek-table compare (compare_list), the checksum fields (fill) and the
// pieces a clip takes of the frames (clip_pieces). The sinks and decode_alone_device keep what is theirs: launches, waits, downloads, uploads.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <thread>
#include <utility>
#include <vector>
#include "zg_frames_int.h"
#include "zg_scatter.h"
#include "zg_seeksums.h"
#include "zg_idxsums.h"
#include "zg_xxh64_dev.h"

using namespace zg;
using namespace zgf;

namespace {

// (kFramesSubmitBytes, plaintext and input per submit: zg_frames_int.h)
// Where a submit's frames are hashed (LABNOTES.md "decode_frames", measured on MI355X): on the device one lane runs XXH64 at ~225 MB/s (a lone
// 4 MiB frame: 18.6 ms), all lanes together at ~1 TB/s (65,536 x 128 KiB: 8.6 ms); a host core at >= 10 GB/s, and the host copies every byte
// to the caller anyway, on up to kHostThreads threads. A submit's frames go to the device only when the estimate of the kernel —
// max(longest frame / lane rate, all bytes / device rate) — beats the estimate of hashing them on the host threads, and never a frame longer
// than kHashDeviceMax. Many short frames go to the device; a lone frame, or a few long ones, stay on the host.
constexpr uint64_t kHashDeviceMax = 4ull << 20;
constexpr double kLaneBytesPerUs = 225.0, kDeviceBytesPerUs = 1.0e6, kHostBytesPerUs = 1.0e4, kLaunchUs = 50.0;
constexpr unsigned kHostThreads = 16;
// ZGPU_DEVICE_VERIFY_SEEK_TABLE hashes the few mid-sized frames a range takes and waits for them: up to this many frames a submit of such a call
// is hashed by zg_k_xxh64q (four lanes per frame). From tools/dev/hash_ranges.py on an MI355X (LABNOTES.md "xxh64q"): the quad kernel is 5.1 x
// (8 x 128 KiB) to 10.3 x (4096 x 128 KiB) the one-lane kernel on ranges of this kind; 4096 is the largest count of mid-sized ranges measured.
// zgpu_seek_index_hash_device (DeviceSink::hash_every) hashes whole frames and waits for them in the same way and takes the same rule. No other
// call hashes differently: ZG_XXH64Q_MAX_RANGES (zg_kernels.h) stays 0.
constexpr uint32_t kTableQuadMaxRanges = 4096;

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

// the lookup of a shared submit's walks: the context's registered dictionaries. One without content is not resolved — its frames go alone, as
// with the switch off (ZgFrame::dict_len != 0 is what marks a dictionary frame for the engine).
const DictFacts* shared_find(const void* user, uint32_t id) {
  const zgpu_ctx* c = (const zgpu_ctx*)user;
  auto it = c->dict_facts.find(id);
  return it == c->dict_facts.end() || it->second.content_len == 0 ? nullptr : &it->second;
}

// The three parts only some calls have; each lives in the frame of the function that builds it, and an absent one is a null pointer in the
// Call. DeviceSink: destinations in device memory of the caller (zg_frames_int.h).
// sources in device memory (zgpu_decode_frames_device_src): Call::srcs[i] is device memory; what was found out about every entry before the
// first submit
struct DeviceSources {
  Engine::Skeleton sk;                  // the records zg_k_walk brought back
  std::vector<Engine::DevEntry> dev;    // the entries as the engine takes them (a refused entry: length 0)
  std::vector<uint8_t> refused;         // entries whose source or destination failed the pointer check (1), or the status (> 1) of an entry
                                        // that is refused for another reason (ZGPU_E_SEEK_TABLE)
  std::vector<uint64_t> bound;          // plaintext_bound of every entry, from its records
  uint64_t* stats = nullptr;            // zgpu_ctx::frames_device_src_stats (kSrcStat*)
};
// ranges (decode_selections): the entries are selections of whole entries, each with a span of clips (zg_frames_int.h: Selection, Clip)
struct Ranges {
  std::vector<Clip>& clip;
  const std::vector<uint32_t>& first;   // n + 1 slots
  std::vector<uint64_t> declared;       // per sub-entry (Selection::declared)
  bool promise;                         // declared is a seek table's promise: it always holds
  uint64_t* stats;                      // zgpu_ctx::ranges_stats (kRangeStat*)
};

struct Call {
  zgpu_ctx* c;
  const uint8_t* const* srcs;
  const size_t* lens;
  uint8_t* const* dsts;                            // host sink: host memory; device sink: device memory of the caller (checked)
  const size_t* caps;
  zgpu_entry_result* res = nullptr;                // the host sink's results (nullptr with a device sink)
  bool hash_forced = false;                        // host sink, development build (ZGPU_HASH_DEVICE_MAX): frames up to its hash_max on the device, no estimate
  uint64_t host_hash_max = kHashDeviceMax;
  DictLookup lookup;                               // shared dictionaries (zgpu_set_frames_shared_dicts): what the walks resolve ids with
  bool shared;                                     //   the switch is on and a dictionary is registered: dicts() hands the lookup out
  std::vector<std::pair<uint32_t, bool>> again;    // entries decoded again on their own after the submits (true: the walk met a dictionary frame)
  DeviceSink* sink = nullptr;
  DeviceSources* src = nullptr;
  Ranges* ranges = nullptr;

  Call(zgpu_ctx* ctx, const uint8_t* const* s, const size_t* l, uint8_t* const* d, const size_t* cp)
      : c(ctx), srcs(s), lens(l), dsts(d), caps(cp), lookup{shared_find, ctx}, shared(ctx->frames_shared_dicts && !ctx->dicts.empty()) {}
  const DictLookup* dicts() const { return shared ? &lookup : nullptr; }
  uint64_t hash_max() const { return sink ? sink->hash_max : host_hash_max; }
  // what entry i's bytes are measured against (zg_entry.h: ladder): its capacity, or — ranges — its span of clips and what its frames declare
  zge::Mode mode(uint32_t i) const {
    zge::Mode m;
    m.cap = caps[i];
    if (!ranges) return m;
    m.ranges = true; m.promise = ranges->promise; m.declared = ranges->declared[i];
    m.clip = ranges->clip.data() + ranges->first[i]; m.nclips = ranges->first[i + 1] - ranges->first[i];
    return m;
  }
  // entry i's clips — without ranges the whole entry is one (*whole: room for it, `written` what the ladder said) — and how many
  const zge::Clip* clips(uint32_t i, uint64_t written, zge::Clip* whole, uint32_t* n) const {
    *whole = zge::Clip{0, UINT64_MAX, dsts[i], caps[i], written, false};
    *n = ranges ? ranges->first[i + 1] - ranges->first[i] : 1;
    return ranges ? ranges->clip.data() + ranges->first[i] : whole;
  }
  zgpu_entry_result& result(uint32_t i) const { return sink ? sink->res[i].r : res[i]; }
};

// the device copy of a registered dictionary, uploaded at first use (zg_dictfill.h: DictImage; the formats are zg_apply_dict's)
int dict_image(zgpu_ctx* c, uint32_t id, zgd::DictImage* out) {
  auto have = c->dict_dev.find(id);
  if (have != c->dict_dev.end()) { *out = have->second.im; return ZGPU_OK; }
  auto it = c->dicts.find(id);
  if (it == c->dicts.end()) return ZGPU_E_INTERNAL;
  const ZgDict& d = it->second;
  if (d.fse.size() != ZG_FSE_SLOT_U32 || d.huf.size() != ZG_HUF_SLOT_U16) return ZGPU_E_INTERNAL;
  ZgDictDev dd;
  int st = dd.buf.reserve(zgd::image_bytes(d.content.size()));
  if (st) return st;
  dd.im = zgd::image_at((uint64_t)(uintptr_t)dd.buf.p, d.content.size());
  const uint8_t logs[16] = {d.logs[0], d.logs[1], d.logs[2], d.logs[3]}, mb[16] = {d.huf_maxbits};
  auto up = [](uint64_t at, const void* h, size_t n) { return !n || hipMemcpy((void*)(uintptr_t)at, h, n, hipMemcpyHostToDevice) == hipSuccess; };
  if (!up(dd.im.content, d.content.data(), d.content.size()) || !up(dd.im.fse, d.fse.data(), zgd::kFseBytes) || !up(dd.im.logs, logs, 16) ||
      !up(dd.im.huf, d.huf.data(), zgd::kHufBytes) || !up(dd.im.maxbits, mb, 16)) {
    (void)hipGetLastError();
    dd.buf.release();
    return ZGPU_E_HIP;
  }
  *out = dd.im;
  c->dict_dev[id] = dd;
  return ZGPU_OK;
}

// what a submit leaves behind for its sink
struct Submit {
  Staging in;
  Batch* b = nullptr;
  std::vector<int> walk;
  std::vector<uint32_t> ff;       // entry j's frames are [ff[j], ff[j + 1])
  std::vector<uint64_t> off;      // entry j lies at off[j] of the submit's input (FrameInfo::src_begin / src_end are counted from its begin)
  std::vector<zge::Frame> fr;     // the facts (zg_entry.h), flat: every frame of the submit, hashed / slot / digest filled in by hash_launch / hash_wait ...
  std::vector<zge::Entry> ent;    // ... and entry j, a view of fr[ff[j] .. ff[j + 1])
  std::vector<uint32_t> cand;     // frames of successful entries short enough to be hashed on the device
  uint64_t down = 0;              // output bytes the successful entries reach up to
  ~Submit() { delete b; }
};

// one submit, up to its verdicts: the entries idx[0 .. n) staged, walked, decoded; status / written / nframes of every entry it serves
int decode_submit(Call& k, const uint32_t* idx, uint32_t n, Submit& u) {
  std::vector<uint64_t>& off = u.off;
  std::vector<uint64_t> len(n);
  off.assign(n, 0);
  uint64_t total_in = 0;
  for (uint32_t j = 0; j < n; j++) { off[j] = total_in; len[j] = k.lens[idx[j]]; total_in += len[j]; }
  Staging& in = u.in;
  std::vector<int>& walk = u.walk;
  std::vector<uint32_t>& ff = u.ff;
  int st;
  if (k.src) {   // the bytes are on the device: no staging, no upload — the skeleton is parsed, one zg_k_gather launch moves the entries
    if ((st = k.c->eng->prepare_entries_device(k.src->dev.data(), k.src->sk, idx, off.data(), n, total_in, &u.b, &walk, &ff, k.dicts()))) return st;
    k.src->stats[kSrcStatGatherLaunches] += u.b->gather_launched ? 1u : 0u; k.src->stats[kSrcStatGatherUs] += u.b->gather_us;
  } else {
    if ((st = in.get(total_in))) return st;
    parallel_for(n, total_in, 8u << 20, [&](uint32_t j) { if (len[j]) memcpy(in.p + off[j], k.srcs[idx[j]], len[j]); });
    if ((st = k.c->eng->prepare_entries(in.p, total_in, off.data(), len.data(), n, &u.b, &walk, &ff, k.dicts()))) return st;
  }
  Batch* b = u.b;
  // the submit's dictionary frames (none unless the walks had a lookup): their dictionaries' device copies, for zg_k_dictfill
  std::vector<uint8_t> has_dict(n, 0);
  if (k.shared) {
    std::vector<zgd::DictImage> images(b->info.size(), zgd::DictImage{});
    if (b->info.size() != b->bb.frames.size()) return ZGPU_E_INTERNAL;
    for (uint32_t j = 0; j < n; j++)
      for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
        if (!b->bb.frames[f].dict_len) continue;
        if ((st = dict_image(k.c, b->info[f].header.dict_id, &images[f]))) return st;
        has_dict[j] = 1;
      }
    if ((st = b->set_frame_dicts(std::move(images)))) return st;
  }
  b->drain_rule = ZG_DRAIN_DECODE_ALL;   // (as zgpu_decode_all: decode_all drains its DecodeBuffer every MiB, zg_exact.h)
  if ((st = b->run()) || (st = b->sync())) return st;
  const std::vector<ZgFrameOut>& fo = b->frame_out;
  if (fo.size() != b->info.size()) return ZGPU_E_INTERNAL;
  uint64_t* ds = k.c->frames_dict_stats;
  ds[kDictStatFillLaunches] += b->dictfill_launches; ds[kDictStatBytesReplicated] += b->dictfill_bytes; ds[kDictStatFillUs] += b->dictfill_us;

  // the facts: every frame's from its FrameInfo and ZgFrameOut, every entry's from its walk and its frames in stream order
  u.fr.resize(fo.size());
  u.ent.assign(n, zge::Entry{});
  for (uint32_t j = 0; j < n; j++) {
    zge::Entry& e = u.ent[j];
    e.walk = walk[j]; e.dict = has_dict[j] != 0;
    e.nframes = ff[j + 1] - ff[j]; e.fr = u.fr.data() + ff[j];
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      const FrameInfo& fi = b->info[f];
      if (!e.decode && fo[f].status) e.decode = (int)fo[f].status;
      e.total += fo[f].out_size;
      if (!e.decode && !fi.host_status) e.sound = e.total;
      u.fr[f] = zge::Frame{fi.src_begin - off[j], fi.src_end - fi.src_begin, fo[f].out_size, e.total, fi.header.frame_content_size, 0, fi.checksum,
                           zgv::kNotHashed, fi.header.has_fcs(), fi.has_checksum, false};
    }
  }
  // verdicts (zgpu_decode_all, zg_capi.cpp, on the entry's own frames): zg_entry.h's ladder
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t i = idx[j];
    const zge::Entry& e = u.ent[j];
    zgpu_entry_result& r = k.result(i);
    // zgpu_decode_all's frame-by-frame path (the switch off, or an id the lookup did not resolve)
    if (walk[j] == ZGPU_E_DICT_NOT_PROVIDED && !k.c->dicts.empty()) { k.again.push_back({i, true}); ds[kDictStatEntriesAlone] += k.shared ? 1u : 0u; continue; }
    if (e.decode == ZGPU_E_UNSUPPORTED || e.decode == ZGPU_E_INTERNAL) { k.again.push_back({i, e.dict}); ds[kDictStatEntriesAlone] += e.dict; continue; }
    if (k.ranges) { k.ranges->stats[kRangeStatFramesDecoded] += e.nframes; k.ranges->stats[kRangeStatPlaintextDecoded] += e.total; }   // (work done, failed entries too; an entry that goes alone is counted there)
    const zge::Verdict v = zge::ladder(e, k.mode(i));
    r.status = v.status;
    if (r.status) continue;
    if (has_dict[j]) for (uint32_t f = ff[j]; f < ff[j + 1]; f++) ds[kDictStatFramesShared] += b->bb.frames[f].dict_len ? 1u : 0u;
    r.written = v.written;
    r.nframes = e.nframes;
    // (the seek table's checksums, a handle's sums, the hash pass: every frame, with or without a Content_Checksum)
    const bool table_all = k.sink && ((k.sink->table_all && k.sink->compared(i)) || k.sink->hash_every);
    for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
      if (fo[f].out_size <= k.hash_max() || (k.sink && k.sink->hash_all && b->info[f].has_checksum) || table_all) u.cand.push_back(f);   // (candidates)
      const uint64_t upto = fo[f].out_base + fo[f].out_size;
      if (upto > u.down) u.down = upto;
    }
  }
  return ZGPU_OK;
}

using zge::fail_entry;
const char* const kHandleChanged = "zgpu_gather_ranges_indexed_device_src: rows or digests that leave the arrays of the checksum compare";
const char* const kTableChanged = "zgpu_decode_ranges_seek_table_device_src: a seek table changed between the seek and the checksum compare";

void count_frames(DeviceSink& sink, const zge::Hashed& h) { sink.stats[kDevStatFramesHashed] += h.hashed; sink.stats[kDevStatFramesNotHashed] += h.not_hashed; }

// What both sinks do about hashing: the frames of u.cand, as the sink left that list, are hashed by the device — hash_launch enqueues the kernel
// on the first stream, and the sink does its copying beside it; hash_wait collects the digests into the facts (*kernel_us, if asked for: the
// kernel's time). A frame's slot is its place in u.cand: where its digest lies in device memory for the compare kernels.
int hash_launch(Submit& u, uint32_t quad_max_ranges = 0) {
  for (size_t q = 0; q < u.cand.size(); q++) { u.fr[u.cand[q]].hashed = true; u.fr[u.cand[q]].slot = (uint32_t)q; }
  return u.b->hash_launch(u.cand.data(), (uint32_t)u.cand.size(), quad_max_ranges);
}
int hash_wait(Submit& u, uint64_t* kernel_us = nullptr) {
  std::vector<uint64_t> dh(u.cand.size());
  const int st = u.b->hash_wait(dh.data(), kernel_us);
  for (size_t q = 0; q < u.cand.size() && !st; q++) u.fr[u.cand[q]].digest = dh[q];
  return st;
}

// the host sink: the plaintext comes back, goes to the callers' buffers on the host threads, and the frames the device did not hash are hashed there
int sink_host(Call& k, const uint32_t* idx, uint32_t n, Submit& u) {
  Batch* b = u.b;
  const std::vector<ZgFrameOut>& fo = b->frame_out;
  const std::vector<int>& walk = u.walk;
  const std::vector<uint32_t>& ff = u.ff;
  const uint64_t down = u.down;                // output bytes the host needs (of entries that succeed)
  int st;
  if (!k.hash_forced && !hash_on_device(u.cand, fo)) u.cand.clear();   // (what stays is hashed on the device)
  // the device hashes its frames while the output comes back
  if ((st = hash_launch(u))) return st;
  Staging out;
  if ((st = out.get(down)) || (st = b->read_output(0, out.p, down)) || (st = hash_wait(u))) return st;
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
      if (!u.fr[f].hashed) { u.fr[f].digest = zgx::xxh64(s, fo[f].out_size, 0); u.fr[f].hashed = true; }
    }
  });
  for (uint32_t j = 0; j < n; j++) {
    zgpu_entry_result& r = k.res[idx[j]];
    if (r.status || r.nframes == 0) continue;
    zge::fill(u.ent[j], false, &r, nullptr, nullptr);
  }
  return ZGPU_OK;
}

// DeviceSink::records: the submit's entries that stand at status 0 behind every verdict have their decoded frames cut into chunks — each
// frame's [out_base, out_base + out_size), the ranges the hash launch takes: the dictionary gap in front of a frame is in no chunk — and the
// three kernels of zg_records.h find the delimiters: count and scan, the one round trip that sizes the submit's staging, emit. What stays is
// the staging buffer and, per sub-entry, where its offsets lie in it.
int records_submit(Call& k, const uint32_t* idx, uint32_t n, Submit& u) {
  DeviceSink& sink = *k.sink;
  DeviceSink::Records& rc = *sink.records;
  Batch* b = u.b;
  const std::vector<ZgFrameOut>& fo = b->frame_out;
  std::vector<zgr::Chunk> chunks;
  std::vector<uint32_t> fstart, owner;   // per listed frame: its first chunk, the j it belongs to
  for (uint32_t j = 0; j < n; j++) {
    const zgpu_entry_result& r = sink.res[idx[j]].r;
    if (r.status || r.nframes == 0) continue;
    uint64_t at = rc.base[idx[j]];
    for (uint32_t f = u.ff[j]; f < u.ff[j + 1]; f++) {
      fstart.push_back((uint32_t)chunks.size());
      zgr::cut_chunks(fo[f].out_base, fo[f].out_size, at, (uint32_t)owner.size(), &chunks);
      owner.push_back(j);
      at += fo[f].out_size;
      if (chunks.size() > 0x7FFFFFFFull) return ZGPU_E_INTERNAL;   // (never: a submit's plaintext is bounded)
    }
  }
  fstart.push_back((uint32_t)chunks.size());
  if (chunks.empty()) return ZGPU_OK;
  const uint32_t nf = (uint32_t)owner.size();
  int st;
  if ((st = b->records_launch(chunks.data(), (uint32_t)chunks.size(), fstart.data(), nf, rc.delimiter))) return st;
  std::vector<uint64_t> ftot(nf, 0);
  uint64_t total = 0, us = 0, back = 0;
  if ((st = b->records_sizes(&total, ftot.data(), &us, &back))) return st;
  rc.us += us; rc.bytes_back += back; rc.chunks += chunks.size();
  if (total > SIZE_MAX / 8) return ZGPU_E_NOMEM;
  if (total) {
    rc.staging.push_back(zg::DevBuf());
    if ((st = rc.staging.back().reserve((size_t)total * 8))) return st;
    if ((st = b->records_emit(rc.staging.back().as<uint64_t>(), total))) return st;
  }
  uint64_t at = 0;
  for (uint32_t q = 0; q < nf; q++) {   // (a sub-entry's frames follow each other in the list, and so do their offsets in the staging)
    DeviceSink::Records::Run& run = rc.run[idx[owner[q]]];
    if (!run.n) { run.buf = total ? (int32_t)rc.staging.size() - 1 : -1; run.at = at; }
    run.n += ftot[q];
    at += ftot[q];
  }
  if ((st = b->records_wait(&us))) return st;   // (the output goes with the submit: the emit must have read it)
  rc.us += us;
  return ZGPU_OK;
}

// the device sink: the plaintext stays on the device; one zg_k_scatter launch copies the frames of every successful entry to its destination
// (an entry's frames back to back) while the hash kernel (zg_launch_xxh64) hashes the candidates beside it; frames that are not hashed are
// counted, not verified. With ZGPU_DEVICE_VERIFY the order is hash launch, hash wait, verdicts, and only then the scatter of the entries that
// passed: an entry with a hashed frame whose digest differs from its Content_Checksum fails, and nothing of it is ever in the scatter list.
// With ZGPU_DEVICE_VERIFY_SEEK_TABLE (zg_seeksums.h) the order is hash launch, seeksums launch (behind the hash kernel on its stream), the two
// waits, the verdicts of ZGPU_DEVICE_VERIFY, the table's verdicts on what still stands, then the scatter of what still stands.
int sink_device(Call& k, const uint32_t* idx, uint32_t n, Submit& u) {
  Batch* b = u.b;
  const std::vector<ZgFrameOut>& fo = b->frame_out;
  const std::vector<uint32_t>& ff = u.ff;
  DeviceSink& sink = *k.sink;
  zgpu_device_entry_result* const dres = sink.res;
  if (sink.no_hash) u.cand.clear();
  int st;
  if ((st = hash_launch(u, sink.table_flag || sink.hash_every ? kTableQuadMaxRanges : 0u))) return st;   // (the hash pass waits for whole frames as well)
  uint64_t bytes = 0;
  auto scatter = [&]() -> int {   // the frames of every entry that stands at status 0, in one launch
    std::vector<zgs::Seg> segs;
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t i = idx[j];
      const zgpu_entry_result& r = dres[i].r;
      if (r.status || r.nframes == 0) continue;   // (failed, or waiting on the again-list: nothing of it is written here)
      // (ranges: every clip of the entry's span that has room takes its own pieces to its own destination — a clipped frame is just a shorter
      // segment, and the frames are in the output once; no ranges: the whole entry is one clip)
      zge::Clip whole;
      uint32_t nclips;
      const zge::Clip* cl = k.clips(i, r.written, &whole, &nclips);
      uint64_t total = 0;
      for (uint32_t q = 0; q < nclips; q++) {
        const uint64_t dst = (uint64_t)(uintptr_t)cl[q].dst;
        const uint64_t at = zge::clip_pieces(u.ent[j].fr, u.ent[j].nframes, cl[q], [&](const zge::Piece& p) {
          segs.push_back(zgs::Seg{fo[ff[j] + p.frame].out_base + p.in_frame, dst + p.at, p.len});
        });
        if (at != cl[q].written || at > cl[q].cap) return ZGPU_E_INTERNAL;   // (never: the verdict counted the same frames)
        total += at;
      }
      if (total != r.written) return ZGPU_E_INTERNAL;   // (never)
      bytes += total;
    }
    if (segs.size() > 0xFFFFFFFFull) return ZGPU_E_INTERNAL;
    return b->scatter_launch(segs.data(), (uint32_t)segs.size(), k.c->eng->tuning().scatter_chunk);
  };
  // ZGPU_DEVICE_VERIFY_SEEK_TABLE: one zg_k_seeksums launch for the submit's entries that stand at status 0, behind the hash kernel on its stream
  // The entries whose handle holds sums go to zg_k_idxsums (zg_idxsums.h) in the same position: a submit that holds both kinds launches both
  std::vector<uint32_t> who[2];   // their j, by route: 0 by the table, 1 by the handle
  if (sink.table_flag) {
    std::vector<zgv::Lane> lanes;
    std::vector<zgh::Lane> hlanes;
    std::vector<zgv::Frame> list[2];
    for (uint32_t j = 0; j < n; j++) {
      const zgpu_entry_result& r = dres[idx[j]].r;
      if (r.status || r.nframes == 0 || !sink.compared(idx[j])) continue;
      const bool by_handle = sink.by_handle(idx[j]);
      std::vector<zgv::Frame>& to = list[by_handle];
      const uint32_t lo = (uint32_t)to.size();
      for (uint32_t f = ff[j]; f < ff[j + 1]; f++)
        if (b->info[f].src_begin < u.off[j] || b->info[f].src_end < b->info[f].src_begin) return ZGPU_E_INTERNAL;   // (never)
      zge::compare_list(u.ent[j], [](const zge::Frame&) { return true; }, &to);   // (a submit's hashed frames are its candidates: every digest may be used)
      if (by_handle) {
        const DeviceSink::HandleEntry& e = sink.handle_verify[idx[j]];
        hlanes.push_back(zgh::Lane{e.pair0, e.sum0, e.nrows, e.first, e.taken, lo, (uint32_t)to.size() - lo, {0, 0, 0}});
      } else {
        const DeviceSink::TableEntry& e = sink.table_verify[idx[j]];
        lanes.push_back(zgv::Lane{e.src, e.len, e.first, e.taken, lo, (uint32_t)to.size() - lo});
      }
      who[by_handle].push_back(j);
    }
    if (list[0].size() > 0xFFFFFFFFull || list[1].size() > 0xFFFFFFFFull) return ZGPU_E_INTERNAL;
    if ((st = b->seeksums_launch(lanes.data(), (uint32_t)lanes.size(), list[0].data(), (uint32_t)list[0].size()))) return st;
    if (!hlanes.empty() && (st = b->idxsums_launch(hlanes.data(), (uint32_t)hlanes.size(), list[1].data(), (uint32_t)list[1].size(), sink.handle->pairs,
                                                   sink.handle->npairs, sink.handle->sums, sink.handle->nsums)))
      return st;
  }
  const bool gated = sink.verify || sink.table_flag;   // the scatter waits for the verdicts
  if (!gated && (st = scatter())) return st;
  uint64_t hash_us = 0;
  if ((st = hash_wait(u, &hash_us))) return st;
  sink.stats[kDevStatHashUs] += hash_us;
  std::vector<zgv::Sums> sums(who[0].size() + who[1].size());   // the table's records, then the handle's
  for (int route = 0; route < 2; route++) {   // (the same slots count both compare kernels)
    if (who[route].empty()) continue;
    uint64_t us = 0, back = 0;
    if ((st = b->compare_wait(route != 0, sums.data() + (route ? who[0].size() : 0), &us, &back))) return st;
    uint64_t* rs = k.ranges->stats;
    rs[kRangeStatCompareLaunches]++; rs[kRangeStatCompareUs] += us; rs[kRangeStatCompareBytesDownloaded] += back;
  }
  // the verdict of verification ranks behind every other one: only entries that stand at status 0 are looked at. (An entry that fails here
  // or below counts its frames, hashed or not, at that moment: the fill at the end no longer sees it.)
  for (uint32_t j = 0; j < n && sink.verify; j++) {
    const zgpu_entry_result& r = dres[idx[j]].r;
    if (r.status || r.nframes == 0) continue;
    if (!zge::verify_fails(dres[idx[j]], u.ent[j])) continue;
    count_frames(sink, zge::hashed_frames(u.ent[j], false));
    sink.stats[kDevStatEntriesFailedVerify]++;
  }
  // the table's verdict ranks last: only what still stands is looked at
  const zgv::Sums* rec = sums.data();
  for (int route = 0; route < 2; route++)
    for (const uint32_t j : who[route]) {
      const zgv::Sums& s = *rec++;
      if (s.why) { k.c->eng->last_error = route ? kHandleChanged : kTableChanged; return ZGPU_E_INTERNAL; }
      if (dres[idx[j]].r.status) continue;
      k.ranges->stats[kRangeStatFramesCompared] += s.compared;
      if (!zge::table_fails(dres[idx[j]], s, u.ent[j].nframes)) continue;
      count_frames(sink, zge::hashed_frames(u.ent[j], false));
      k.ranges->stats[kRangeStatEntriesFailedTable]++;
    }
  if (gated && (st = scatter())) return st;
  uint64_t us = 0;
  bool launched = false;
  if ((st = b->scatter_wait(&us, &launched))) return st;
  sink.stats[kDevStatScatterLaunches] += launched ? 1u : 0u; sink.stats[kDevStatBytesScattered] += bytes; sink.stats[kDevStatScatterUs] += us;
  for (uint32_t j = 0; j < n; j++) {
    zgpu_device_entry_result& d = dres[idx[j]];
    if (d.r.status || d.r.nframes == 0) continue;
    if (sink.collect)
      for (uint32_t f = ff[j]; f < ff[j + 1]; f++) {
        if (!u.fr[f].hashed || b->info[f].src_begin < u.off[j]) return ZGPU_E_INTERNAL;   // (never: hash_every)
        (*sink.collect)[idx[j]].push_back(DeviceSink::Digest{u.fr[f].begin, u.fr[f].clen, u.fr[f].digest});
      }
    count_frames(sink, zge::fill(u.ent[j], sink.no_hash, &d.r, &d.checksums_unverified, &d.first_hashed));
  }
  return sink.records ? records_submit(k, idx, n, u) : ZGPU_OK;
}

// one submit: the entries idx[0 .. n)
int run_submit(Call& k, const uint32_t* idx, uint32_t n) {
  Submit u;
  int st = decode_submit(k, idx, n, u);
  if (st) return st;
  return k.sink ? sink_device(k, idx, n, u) : sink_host(k, idx, n, u);
}

// host memory of an entry that is decoded alone (not zeroed: it may be as large as the entry's plaintext)
using HostBuf = std::unique_ptr<uint8_t, decltype(&free)>;
inline HostBuf host_buf(size_t n) { return HostBuf((uint8_t*)malloc(n ? n : 1), &free); }

// An entry the submit did not serve: zgpu_decode_all on it alone (its dictionary frames go frame by frame through the FrameDecoder mirror,
// which also hashes what it hands out). What comes back is the facts of the entry (zg_entry.h), as a submit produces them for its entries,
// for the same ladder and the same fill — call: the status the CALL ends with (NOMEM, HIP), then nothing else means anything.
// The differences of this producer, each a property of the facts: the decoder's status is the decode verdict and carries the walk's and, without
// ranges, zgpu_decode_all's own order (dict stays false); every frame is hashed, by the host; the digests hold 32 bits.
struct Alone { int call = ZGPU_OK; zge::Entry e; std::vector<zge::Frame> fr; };
Alone decode_alone(Call& k, uint32_t i, bool dict_walk, const uint8_t* src, uint8_t* dst, size_t cap) {
  Alone a;
  size_t w = 0;
  int st;
  if (dict_walk) {
    // (what zgpu_decode_all does with this entry: its walk meets a dictionary frame, and dictionaries are registered)
    st = zg_decode_all_per_frame(k.c, src, k.lens[i], dst, cap, &w, &a.fr);
  } else {
    st = zgpu_decode_all(k.c, src, k.lens[i], dst, cap, &w);
    if (!st) {
      // (Unsupported / Internal in a larger submit, but not alone — never seen; the status stays zgpu_decode_all's.) The frames come from a
      // second, frame-by-frame pass into a buffer of its own; should that pass fail or disagree, the frames are not known: they are counted
      // from their headers and the entry reports no checksum rather than a wrong one.
      size_t w2 = 0;
      const HostBuf tmp = host_buf(w);
      if (!tmp) { a.call = ZGPU_E_NOMEM; return a; }
      const int s2 = zg_decode_all_per_frame(k.c, src, k.lens[i], tmp.get(), w, &w2, &a.fr);
      a.e.known = s2 == ZGPU_OK && w2 == w && (w == 0 || memcmp(tmp.get(), dst, w) == 0);
      if (s2 == ZGPU_E_NOMEM || s2 == ZGPU_E_HIP) { a.call = s2; return a; }
    }
  }
  if (st == ZGPU_E_NOMEM || st == ZGPU_E_HIP) { a.call = st; return a; }
  a.e.decode = st;
  if (st || !a.e.known) a.fr.clear();
  if (st) return a;
  a.e.total = w;
  a.e.nframes = (uint32_t)a.fr.size();
  if (!a.e.known) {
    std::vector<FrameSpan> sp;
    (void)split_frames(src, k.lens[i], &sp);
    for (const FrameSpan& x : sp) a.e.nframes += x.skippable ? 0u : 1u;
  }
  a.e.fr = a.fr.data();
  return a;
}

// the host sink's entry of the again-list
int decode_alone_host(Call& k, uint32_t i, bool dict_walk) {
  const Alone a = decode_alone(k, i, dict_walk, k.srcs[i], k.dsts[i], k.caps[i]);
  if (a.call) return a.call;
  zgpu_entry_result& r = k.res[i];
  memset(&r, 0, sizeof r);
  r.status = zge::ladder(a.e, k.mode(i)).status;
  if (r.status) return ZGPU_OK;
  r.written = a.e.total; r.nframes = a.e.nframes;   // (no ranges: everything that was decoded)
  zge::fill(a.e, false, &r, nullptr, nullptr);
  return ZGPU_OK;
}

// The device sink's form: into a host buffer (no larger than the entry can need), then the entry's pieces H2D to the caller's memory — the
// same ladder, verdicts and fill as a submit's entries get (zg_entry.h). What is this path's own: the D2H of a device source, the host buffer,
// the download of footer, rows, pairs and sums for the host's form of the table compare, and the uploads.
int decode_alone_device(Call& k, uint32_t i, bool dict_walk) {
  DeviceSink& sink = *k.sink;
  std::vector<uint8_t> down;   // device sources: the entry comes to the host with one D2H (rare; correct first)
  if (k.src) {
    try { down.resize(k.lens[i] ? k.lens[i] : 1); } catch (...) { return ZGPU_E_NOMEM; }
    if (k.lens[i] && hipMemcpy(down.data(), k.srcs[i], k.lens[i], hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
    k.src->stats[kSrcStatInputBytesToHost] += k.lens[i];
  }
  const uint8_t* src = k.src ? down.data() : k.srcs[i];
  const uint64_t bound = plaintext_bound(src, k.lens[i]);
  // (beyond the bound nothing can be written: TargetTooSmall is decided as with caps[i]. Ranges: the whole selection is decoded, and clipped
  // below — the buffer holds the selection's bound, every frame's declared size or what its block headers allow where that is less, so only a
  // frame that yields more than it declares can overflow it: Entry::bound_buffer)
  const size_t cap = k.ranges ? (size_t)bound : k.caps[i] < bound ? k.caps[i] : (size_t)bound;
  const HostBuf tmp = host_buf(cap);
  if (!tmp) return ZGPU_E_NOMEM;
  Alone a = decode_alone(k, i, dict_walk, src, tmp.get(), cap);
  a.e.bound_buffer = k.ranges != nullptr;
  const zge::Entry& e = a.e;
  zgpu_device_entry_result& d = sink.res[i];
  int st = a.call;
  if (!st) {
    // (work done, counted here and not in the submit. A difference between the producers that is kept as it was found: an entry whose DECODE
    // fails alone is not counted — the decoder says nothing of its frames —, one that fails to decode in a submit is. LABNOTES.md "entry facts")
    if (k.ranges && !e.decode) { k.ranges->stats[kRangeStatFramesDecoded] += e.nframes; k.ranges->stats[kRangeStatPlaintextDecoded] += e.total; }
    const zge::Verdict v = zge::ladder(e, k.mode(i));
    fail_entry(d, v.status);   // (or status 0, for now with nothing written)
    // ZGPU_DEVICE_VERIFY: the host hashed every frame of the entry as it decoded it; a mismatch fails the entry before its uploads
    if (!d.r.status && sink.verify && zge::verify_fails(d, e)) { sink.stats[kDevStatFramesHashed] += e.nframes; sink.stats[kDevStatEntriesFailedVerify]++; }
    // ZGPU_DEVICE_VERIFY_SEEK_TABLE, last: zg_seeksums.h's rule over rows the host holds — the footer and rows [first, first + taken) come down (the
    // entry crossed to the host anyway). The host hashed every frame, but a frame longer than a nonzero hash_max_bytes passes uncompared, as in
    // a submit. Should the frames not be known (never seen), the list is empty and nothing vouches for them.
    std::vector<zgv::Frame> list;   // the frame list and digests of either route, as a submit would build them
    std::vector<uint64_t> dig;
    const bool compared = !d.r.status && e.nframes && sink.compared(i);
    if (compared) {
      zge::compare_list(e, [&](const zge::Frame& f) { return sink.table_all || f.yielded <= sink.hash_max; }, &list);
      for (const zge::Frame& f : a.fr) dig.push_back(f.digest);
    }
    // what both routes end with: a why is the call's error, else the verdict (a failed entry counts its frames as hashed: the host hashed them)
    auto verdict = [&](const zgv::Sums& rec, const char* changed) -> int {
      if (rec.why) { k.c->eng->last_error = changed; return ZGPU_E_INTERNAL; }
      k.ranges->stats[kRangeStatFramesCompared] += rec.compared;
      if (zge::table_fails(d, rec, e.nframes)) { sink.stats[kDevStatFramesHashed] += e.nframes; k.ranges->stats[kRangeStatEntriesFailedTable]++; }
      return ZGPU_OK;
    };
    if (compared && sink.table(i)) {
      const DeviceSink::TableEntry& t = sink.table_verify[i];
      zgv::Sums rec{0, 0, 0, 0, zgv::kNoRow, 0, 0, 0};
      if (e.known && t.len >= zgt::kFraming) {
        uint8_t footer[9];
        uint32_t es = 8;
        uint64_t rows_off = 0;
        if (hipMemcpy(footer, (const uint8_t*)(uintptr_t)t.src + (t.len - 9), 9, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
        rec.why = zgv::locate_rows(footer, t.len, t.first, t.taken, &es, &rows_off);
        std::vector<uint8_t> rows;
        if (!rec.why) {
          try { rows.resize((size_t)t.taken * es); } catch (...) { return ZGPU_E_NOMEM; }
          if (hipMemcpy(rows.data(), (const uint8_t*)(uintptr_t)t.src + rows_off, rows.size(), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
          k.src->stats[kSrcStatInputBytesToHost] += 9 + rows.size();
          rec = zgv::sums_rows(rows.data(), es, t.first, t.taken, list.data(), (uint32_t)list.size(), dig.data(), (uint32_t)dig.size());
        }
      } else if (e.known) rec.why = zgt::kNone;
      if ((st = verdict(rec, kTableChanged))) return st;
    }
    // the same flag by the handle (zg_idxsums.h: sums_pairs): C of rows [first, first + taken] and their sums come down from the handle's arrays
    if (compared && sink.by_handle(i)) {
      const DeviceSink::HandleEntry& t = sink.handle_verify[i];
      const DeviceSink::Handle& hd = *sink.handle;
      zgv::Sums rec{0, 0, 0, 0, zgv::kNoRow, 0, 0, 0};
      if (e.known) {
        if (t.pair0 > hd.npairs || (uint64_t)t.nrows + 1 > hd.npairs - t.pair0 || t.sum0 > hd.nsums || t.nrows > hd.nsums - t.sum0 || (uint64_t)t.first + t.taken > t.nrows)
          rec.why = zgv::kRows;
        else {
          std::vector<uint64_t> pairs, cs;
          std::vector<uint32_t> rs;
          try { pairs.resize(2 * ((size_t)t.taken + 1)); cs.resize((size_t)t.taken + 1); rs.resize(t.taken); } catch (...) { return ZGPU_E_NOMEM; }
          if (hipMemcpy(pairs.data(), (const uint8_t*)hd.pairs + 16 * (t.pair0 + t.first), pairs.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(rs.data(), hd.sums + t.sum0 + t.first, rs.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
          for (size_t q = 0; q < cs.size(); q++) cs[q] = pairs[2 * q];
          rec = zgh::sums_pairs(cs.data(), rs.data(), t.nrows, t.first, t.taken, list.data(), (uint32_t)list.size(), dig.data(), (uint32_t)dig.size());
        }
      }
      if ((st = verdict(rec, kHandleChanged))) return st;
    }
    if (sink.collect && !d.r.status) {
      if (!e.known) { k.c->eng->last_error = "zgpu_seek_index_hash_device: an entry decoded alone that could not be hashed frame by frame"; return ZGPU_E_INTERNAL; }   // (never seen)
      for (const zge::Frame& f : a.fr) (*sink.collect)[i].push_back(DeviceSink::Digest{f.begin, f.clen, f.digest});
    }
    if (sink.records && !d.r.status) {   // the record offsets of an entry decoded alone: the same definition over the host buffer (zg_records.h)
      DeviceSink::Records& rc = *sink.records;
      try { zgr::records_host(tmp.get(), e.total, rc.delimiter, rc.base[i], &rc.host[i]); } catch (...) { return ZGPU_E_NOMEM; }
      rc.run[i] = DeviceSink::Records::Run{-1, 0, (uint64_t)rc.host[i].size()};
    }
    if (!d.r.status) {
      // The uploads. The host buffer holds the frames back to back: as far as the pieces go it is ONE frame of e.total bytes (which is also all
      // that is known of an entry whose frames are not), so every clip that has room is one H2D; no ranges: the whole entry is one clip.
      zge::Frame buf{};
      buf.yielded = buf.end = e.total;
      zge::Clip whole;
      uint32_t nclips;
      const zge::Clip* cl = k.clips(i, v.written, &whole, &nclips);
      for (uint32_t q = 0; q < nclips; q++)
        zge::clip_pieces(&buf, 1, cl[q], [&](const zge::Piece& p) {
          if (!st && hipMemcpy(cl[q].dst + p.at, tmp.get() + p.cat, p.len, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); st = ZGPU_E_HIP; }
        });
      d.r.written = v.written; d.r.nframes = e.nframes;
      sink.alone_written += d.r.written;
      // (hashing off: the entry reports its checksums as unverified like every other one, though the host hashed them)
      count_frames(sink, zge::fill(e, sink.no_hash, &d.r, &d.checksums_unverified, &d.first_hashed));
    }
  }
  sink.stats[kDevStatEntriesAlone]++;
  return st;
}

// The device sources of a call whose pointers are checked (src->dev, src->refused): every entry's header chain walked on the device (two
// launches for the whole call) and its bound taken from the records, before the first submit is cut.
int device_sources(const Call& k, uint32_t n, DeviceSources* src) {
  src->stats = k.c->frames_device_src_stats;
  src->bound.assign(n, 0);
  int st = k.c->eng->walk_entries(src->dev.data(), n, &src->sk, src->stats);
  for (uint32_t i = 0; i < n && !st; i++) {
    bool consistent = true;
    const Engine::Skeleton& sk = src->sk;
    src->bound[i] = plaintext_bound_skel(sk.recs.data() + sk.first[i], (uint32_t)(sk.first[i + 1] - sk.first[i]), (size_t)src->dev[i].len, &consistent, k.dicts());
    if (!consistent) { k.c->eng->last_error = "zg_k_walk: an entry's records out of step with its length"; st = ZGPU_E_INTERNAL; }   // (never)
  }
  return st;
}

// the entries cut into submits (an entry is never split), then the again-list
int decode_entries(Call& k, uint32_t n) {
  zgpu_ctx* c = k.c;
  const Tuning& tn = c->eng->tuning();
  const uint64_t S = tn.frames_submit_bytes ? tn.frames_submit_bytes : kFramesSubmitBytes;
  std::vector<DevRange> known;
  std::vector<uint32_t> group;
  uint64_t in_group = 0, in_bytes = 0;   // plaintext bound and input bytes of the submit being gathered (both bounded by S)
  int st = ZGPU_OK;
  for (uint32_t i = 0; i <= n && !st; i++) {
    uint64_t bound = 0;
    if (i < n) {
      if (k.sink) memset(&k.sink->res[i], 0, sizeof k.sink->res[i]);
      else memset(&k.res[i], 0, sizeof k.res[i]);
      bool bad = !k.srcs[i] && k.lens[i];                                  // (host sources: what zgpu_decode_all returns)
      if (k.src) bad = k.src->refused[i] != 0;                             // (device sources: checked before the walk)
      else if (!bad) bad = k.sink ? !device_ptr_ok(c->eng->device(), k.dsts[i], k.caps[i], known) : !k.dsts[i] && k.caps[i];
      if (bad) { k.result(i).status = k.src && k.src->refused[i] > 1 ? k.src->refused[i] : ZGPU_E_BAD_ARG; continue; }   // (refused[i] > 1: the status itself)
      bound = k.src ? k.src->bound[i] : plaintext_bound(k.srcs[i], k.lens[i], k.dicts());   // (with its dictionary frames' gaps)
    }
    // the submit is full (or this is the end): run it. An entry larger than S is a submit of its own. (The input is bounded too: entries that
    // yield nothing — skippable frames, garbage — still travel to the device, through the pinned staging.)
    if (!group.empty() && (i == n || in_group + bound > S || in_bytes + k.lens[i] > S)) {
      st = run_submit(k, group.data(), (uint32_t)group.size());
      c->frames_submits++;
      group.clear();
      in_group = 0; in_bytes = 0;
    }
    if (i < n) { group.push_back(i); in_group += bound; in_bytes += k.lens[i]; }
  }
  for (size_t q = 0; q < k.again.size() && !st; q++) {
    const uint32_t i = k.again[q].first;
    st = k.sink ? decode_alone_device(k, i, k.again[q].second) : decode_alone_host(k, i, k.again[q].second);
  }
  return st;
}

// a device-sink call from its first submit to its end: the streams drained, the submits counted
int finish_device_call(Call& k, uint32_t n, int st) {
  if (!st) st = decode_entries(k, n);
  st = drain(k.c, st);
  k.sink->stats[kDevStatSubmits] = k.c->frames_submits;
  return st;
}

}  // namespace

// ---- what the front-ends share with the calls below (zg_frames_int.h) -------------------------------------------------------------------------
bool zgf::check_device_range(int device, const void* p, size_t cap, std::vector<DevRange>& known) {
  if (!p) return false;
  const uintptr_t a = (uintptr_t)p;
  if (cap > UINTPTR_MAX - a) return false;
  for (const DevRange& r : known) if (a >= r.lo && a + cap <= r.hi) return true;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (an address the runtime does not know)
  if (at.type != hipMemoryTypeDevice || at.device != device) return false;                        // (host, managed, unregistered, another GPU)
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return false; }
  const uintptr_t lo = (uintptr_t)base;
  if (a < lo || size > UINTPTR_MAX - lo || a + cap > lo + size) return false;
  known.push_back(DevRange{lo, lo + size});
  return true;
}

void zgf::reset_stats(zgpu_ctx* c, unsigned owned) {
  auto zero = [](auto& a) { for (uint64_t& x : a) x = 0; };
  if (owned & kOwnsDecode) { c->frames_submits = 0; zero(c->frames_dict_stats); }
  if (owned & kOwnsDevice) zero(c->frames_device_stats);
  if (owned & kOwnsSrc) zero(c->frames_device_src_stats);
  if (owned & kOwnsIndex) zero(c->frames_index_stats);
  if (owned & kOwnsRanges) { zero(c->ranges_stats); zero(c->ranges_many_stats); zero(c->ranges_rec_stats); zero(c->ranges_batch_stats); }
}

int zgf::drain(zgpu_ctx* c, int st) {
  if (hipStreamSynchronize(c->eng->stream()) != hipSuccess || hipStreamSynchronize(c->eng->copy_stream()) != hipSuccess) { (void)hipGetLastError(); if (!st) st = ZGPU_E_HIP; }
  return st;
}

DeviceSink zgf::device_sink(zgpu_ctx* c, const zgpu_device_opts* opts, zgpu_device_entry_result* results, int* st, bool table) {
  const uint32_t flags = opts ? opts->flags : 0u;
  DeviceSink s;
  s.res = results;
  s.hash_max = opts && opts->hash_max_bytes ? opts->hash_max_bytes : kHashDeviceMax;
  s.no_hash = (flags & ZGPU_DEVICE_NO_HASH) != 0;
  s.verify = (flags & ZGPU_DEVICE_VERIFY) != 0;
  s.hash_all = s.verify && !opts->hash_max_bytes;
  s.stats = c->frames_device_stats;
  s.table_flag = (flags & ZGPU_DEVICE_VERIFY_SEEK_TABLE) != 0;
  s.table_all = s.table_flag && !opts->hash_max_bytes;
  *st = (s.no_hash && (s.verify || s.table_flag)) || (s.table_flag && !table) ? ZGPU_E_BAD_ARG : ZGPU_OK;
  return s;
}

extern "C" int zgpu_decode_frames(zgpu_ctx* c, const uint8_t* const* srcs, const size_t* lens, uint32_t n, uint8_t* const* dsts, const size_t* caps,
                                  zgpu_entry_result* results) {
  if (!c || (n && (!srcs || !lens || !dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  reset_stats(c, kOwnsDecode);
  const Tuning& tn = c->eng->tuning();
  Call k(c, srcs, lens, dsts, caps);
  k.res = results;
  k.hash_forced = tn.hash_device_max_set;
  if (tn.hash_device_max_set) k.host_hash_max = tn.hash_device_max;
  return decode_entries(k, n);
}

extern "C" int zgpu_decode_frames_device(zgpu_ctx* c, const uint8_t* const* srcs, const size_t* lens, uint32_t n, void* const* device_dsts,
                                         const size_t* caps, const zgpu_device_opts* opts, zgpu_device_entry_result* results) {
  if (!c || (n && (!srcs || !lens || !device_dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  int st;
  DeviceSink sink = device_sink(c, opts, results, &st);
  if (st) return st;
  reset_stats(c, kOwnsDecode | kOwnsDevice);
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  Call k(c, srcs, lens, (uint8_t* const*)device_dsts, caps);
  k.sink = &sink;
  return finish_device_call(k, n, ZGPU_OK);
}

// Sources in device memory: every pointer is checked, every entry's header chain walked on the device (two launches for the whole call) and
// its bound taken from the records, before the first submit is cut — then the call above, with the skeleton in place of the bytes.
extern "C" int zgpu_decode_frames_device_src(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, void* const* device_dsts,
                                             const size_t* caps, const zgpu_device_opts* opts, zgpu_device_entry_result* results) {
  if (!c || (n && (!device_srcs || !lens || !device_dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  int st;
  DeviceSink sink = device_sink(c, opts, results, &st);
  if (st) return st;
  reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc);
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  Call k(c, (const uint8_t* const*)device_srcs, lens, (uint8_t* const*)device_dsts, caps);
  k.sink = &sink;
  DeviceSources src;
  check_entries(c, device_srcs, lens, device_dsts, caps, n, check_all, &src.dev, &src.refused);
  if ((st = device_sources(k, n, &src)))   // (no submit is cut: every entry reports nothing)
    for (uint32_t i = 0; i < n; i++) memset(&results[i], 0, sizeof results[i]);
  k.src = &src;
  return finish_device_call(k, n, st);
}

// The selections become the entries of that call's machinery: (src + lo, hi - lo) is walked, cut into submits, gathered, decoded and hashed as
// any entry is, and only the verdict (the size check), the scatter list (clipped) and the entries that go alone (the selection downloaded, the
// clipped bytes uploaded) know of the clips. The machinery's own per-entry destinations are not used: every clip has its own.
int zgf::decode_selections(zgpu_ctx* c, DeviceSink& sink, const void* const* device_srcs, const size_t* lens, const std::vector<Selection>& sel,
                           std::vector<Clip>& clip, const std::vector<uint32_t>& first, bool promise, const uint64_t* want_bound,
                           zgpu_device_entry_result* dres) {
  const uint32_t n = (uint32_t)sel.size();
  std::vector<const uint8_t*> srcs(n);
  std::vector<size_t> sub(n), no_caps(n, 0);
  std::vector<uint8_t*> no_dsts(n, nullptr);
  DeviceSources src;
  src.dev.resize(n);
  src.refused.resize(n);
  Ranges rg{clip, first, std::vector<uint64_t>(n), promise, c->ranges_stats};
  sink.res = dres;
  if (sink.table_flag) sink.table_verify.resize(n);
  if (sink.table_flag && sink.handle) sink.handle_verify.assign(n, DeviceSink::HandleEntry{0, 0, 0, 0, 0});
  if (sink.collect) sink.collect->assign(n, std::vector<DeviceSink::Digest>());
  if (sink.records) {
    if (sink.records->base.size() != n) return ZGPU_E_INTERNAL;   // (never: the caller says where every selection begins)
    sink.records->run.assign(n, DeviceSink::Records::Run());
    sink.records->host.assign(n, std::vector<uint64_t>());
  }
  for (uint32_t i = 0; i < n; i++) {
    const Selection& s = sel[i];
    srcs[i] = (const uint8_t*)device_srcs[s.entry] + s.lo;
    sub[i] = (size_t)(s.hi - s.lo);
    src.dev[i] = Engine::DevEntry{(uint64_t)(uintptr_t)srcs[i], (uint64_t)sub[i]};
    src.refused[i] = s.refused;
    rg.declared[i] = s.declared;
    if (sink.table_flag) sink.table_verify[i] = DeviceSink::TableEntry{(uint64_t)(uintptr_t)device_srcs[s.entry], (uint64_t)lens[s.entry], s.first_row, s.rows};
    if (sink.table_flag && sink.handle && sink.handle->on[s.entry]) {   // the handle vouches for this entry: not its table, should it have one
      sink.handle_verify[i] = sink.handle->ent[s.entry];
      sink.handle_verify[i].first = s.first_row; sink.handle_verify[i].taken = s.rows;
      sink.table_verify[i].taken = 0;
    }
  }
  Call k(c, srcs.data(), sub.data(), no_dsts.data(), no_caps.data());
  k.sink = &sink;
  k.ranges = &rg;
  int st = device_sources(k, n, &src);
  // (the walk and the seek read the same bytes: without dictionary gaps their bounds are one number)
  for (uint32_t i = 0; i < n && !st && want_bound && !k.shared; i++)
    if (sub[i] && src.bound[i] != want_bound[i]) {
      c->eng->last_error = "zgpu_decode_ranges_device_src: a source changed between the seek and the walk";
      st = ZGPU_E_INTERNAL;
    }
  k.src = &src;
  st = finish_device_call(k, n, st);
  rg.stats[kRangeStatInputBytesToHost] = src.stats[kSrcStatInputBytesToHost];
  rg.stats[kRangeStatBytesWritten] = sink.stats[kDevStatBytesScattered] + sink.alone_written;
  return st;
}
// ---- the hash kernels on ranges of the caller's choice (measurement and tests) ---------------------------------------------------------------
// [base, base + max(off + len)) passes the check the device sources pass before anything is launched; the ranges are sorted longest first as
// Batch::hash_launch sorts a submit's frames, and digests[i] is range i's in the caller's order (the slot travels with the range).
extern "C" int zgpu_debug_hash_ranges(zgpu_ctx* c, const void* device_base, const uint64_t* offs, const uint64_t* lens, uint32_t n, int kernel,
                                      uint64_t* digests) {
  if (!c || (n && (!offs || !lens || !digests)) || (kernel != 0 && kernel != 1 && kernel != 4)) return ZGPU_E_BAD_ARG;
  c->hash_ranges_us = 0;
  if (!n) return ZGPU_OK;
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  uint64_t end = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (lens[i] > UINT64_MAX - offs[i]) return ZGPU_E_BAD_ARG;
    if (offs[i] + lens[i] > end) end = offs[i] + lens[i];
  }
  std::vector<DevRange> known;
  if (end > SIZE_MAX || !check_device_range(c->eng->device(), device_base, (size_t)end, known)) return ZGPU_E_BAD_ARG;
  std::vector<ZgHashRange> r(n);
  for (uint32_t i = 0; i < n; i++) r[i] = ZgHashRange{offs[i], lens[i], i, 0};
  std::stable_sort(r.begin(), r.end(), [](const ZgHashRange& a, const ZgHashRange& b) { return a.len > b.len; });
  uint64_t pass[3] = {0, 0, 0};   // (one engine lane pass: the ranges are its lanes, the digests its records)
  const int st = c->eng->hash_ranges_pass((const uint8_t*)device_base, r.data(), n, kernel, digests, pass);
  if (st) return st;
  c->hash_ranges_us = pass[kPassUs];
  return ZGPU_OK;
}
extern "C" uint64_t zgpu_debug_hash_ranges_us(const zgpu_ctx* c) { return c ? c->hash_ranges_us : 0; }

// ---- one zx_* primitive on one workgroup (zg_zxprobe.h; tests/test_gpu_zxprobe.py) ----------------------------------------------------------
// Everything an operand could lead outside the three allocations with is refused by zxp::args_ok before the first HIP call. Then: allocate,
// upload, ONE launch on the context's stream, synchronise, download the results and the whole arena, free.
extern "C" int zgpu_debug_zx_probe(zgpu_ctx* c, uint32_t op, uint32_t threads, uint32_t flags, uint32_t res_off, uint32_t res_bytes, const uint32_t* in,
                                   uint32_t* out, const uint8_t* arena_in, uint8_t* arena_out, uint32_t arena_bytes) {
  if (!c || !in || !out || !arena_in || !arena_out || !zxp::args_ok(op, threads, flags, res_off, res_bytes, in, arena_bytes)) return ZGPU_E_BAD_ARG;
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  const size_t in_bytes = (size_t)threads * zxp::kIn * 4, out_bytes = (size_t)threads * zxp::kOut * 4;
  void *d_in = nullptr, *d_out = nullptr, *d_arena = nullptr;
  hipStream_t s = c->eng->stream();
  bool ok = hipMalloc(&d_in, in_bytes) == hipSuccess && hipMalloc(&d_out, out_bytes) == hipSuccess && hipMalloc(&d_arena, arena_bytes) == hipSuccess;
  ok = ok && hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
       hipMemcpyAsync(d_out, out, out_bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
       hipMemcpyAsync(d_arena, arena_in, arena_bytes, hipMemcpyHostToDevice, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  if (ok) {
    zg_launch_zxprobe(op, threads, flags, (const uint32_t*)d_in, (uint32_t*)d_out, (uint8_t*)d_arena, res_off, res_bytes, s);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  ok = ok && hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(arena_out, d_arena, arena_bytes, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); c->eng->last_error = "zgpu_debug_zx_probe: a HIP call failed"; }
  (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_arena);
  return ok ? ZGPU_OK : ZGPU_E_HIP;
}

// ---- what device-resident entries hold, from their headers alone (zg_index.h) --------------------------------------------------------------
// The stop reasons of the chain are public under the values the lanes use.
static_assert(ZGPU_CHAIN_END == zgw::kEnd && ZGPU_CHAIN_SHORT_HEADER == zgw::kShortHeader && ZGPU_CHAIN_BAD_MAGIC == zgw::kBadMagic &&
              ZGPU_CHAIN_SKIP_PAST_END == zgw::kSkipPastEnd && ZGPU_CHAIN_SHORT_BLOCK_HEADER == zgw::kShortBlockHeader &&
              ZGPU_CHAIN_RESERVED_BLOCK == zgw::kReservedBlock && ZGPU_CHAIN_BLOCK_TOO_LARGE == zgw::kBlockTooLarge &&
              ZGPU_CHAIN_BODY_PAST_END == zgw::kBodyPastEnd && ZGPU_CHAIN_SHORT_CHECKSUM == zgw::kShortChecksum, "zgw:: stop reasons");
static_assert(sizeof(zgpu_entry_index) == 40 && sizeof(zgpu_frame_index) == 64, "include/zgpu.h");
namespace {
// Both calls up to the summaries: every source checked, ONE summary launch over the entries that passed, entries[] filled.
int index_summaries(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, zgpu_entry_index* entries,
                    std::vector<Engine::DevEntry>* dev, std::vector<zgi::Entry>* sum) {
  reset_stats(c, kOwnsIndex);
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  sum->assign(n, zgi::Entry{});
  std::vector<uint8_t> refused;
  check_entries(c, device_srcs, lens, nullptr, nullptr, n, check_all, dev, &refused);
  for (uint32_t i = 0; i < n; i++) {
    memset(&entries[i], 0, sizeof entries[i]);
    if (refused[i]) entries[i].status = ZGPU_E_BAD_ARG;
  }
  const int st = drain(c, c->eng->index_pass(dev->data(), n, nullptr, nullptr, sum->data(), nullptr, c->frames_index_stats));
  if (st) return st;
  for (uint32_t i = 0; i < n; i++) {
    if (entries[i].status) { (*sum)[i] = zgi::Entry{}; continue; }
    const zgi::Entry& e = (*sum)[i];
    if (e.chain_end > lens[i]) { c->eng->last_error = "zgpu_frames_index_device: a summary that leaves its entry"; return ZGPU_E_INTERNAL; }   // (never)
    entries[i].bound = e.bound; entries[i].chain_end = e.chain_end;
    entries[i].nframes = e.nframes; entries[i].nskippable = e.nskippable; entries[i].nblocks = e.nblocks;
    entries[i].why = e.why; entries[i].flags = e.flags;
  }
  return ZGPU_OK;
}
}  // namespace

extern "C" int zgpu_frames_index_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, zgpu_entry_index* entries) {
  if (!c || (n && (!device_srcs || !lens || !entries))) return ZGPU_E_BAD_ARG;
  std::vector<Engine::DevEntry> dev;
  std::vector<zgi::Entry> sum;
  return index_summaries(c, device_srcs, lens, n, entries, &dev, &sum);
}

extern "C" int zgpu_frames_table_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, zgpu_entry_index* entries,
                                        uint64_t* frame_first, zgpu_frame_index* frames, size_t frames_cap, size_t* nframes_out) {
  if (!c || !frame_first || !nframes_out || (n && (!device_srcs || !lens || !entries)) || (frames_cap && !frames)) return ZGPU_E_BAD_ARG;
  std::vector<Engine::DevEntry> dev;
  std::vector<zgi::Entry> sum;
  *nframes_out = 0;
  frame_first[0] = 0;
  int st = index_summaries(c, device_srcs, lens, n, entries, &dev, &sum);
  if (st) return st;
  const uint64_t total = zgi::frame_ranges(sum.data(), n, frame_first);
  *nframes_out = (size_t)total;
  if (total > frames_cap) return ZGPU_E_TARGET_TOO_SMALL;
  if (!total) return ZGPU_OK;
  std::vector<zgi::Entry> again(n);
  std::vector<zgi::FrameRec> recs(total);
  st = drain(c, c->eng->index_pass(dev.data(), n, frame_first, sum.data(), again.data(), recs.data(), c->frames_index_stats));
  if (st) return st;
  for (uint32_t i = 0; i < n; i++) {
    if (entries[i].status) continue;
    if (!zgi::same_entry(again[i], sum[i])) {   // (a source that changed between the passes: the caller's promise broken)
      c->eng->last_error = "zgpu_frames_table_device: a source changed while it was indexed";
      return ZGPU_E_INTERNAL;
    }
    for (uint64_t k = frame_first[i]; k < frame_first[i + 1]; k++) {
      const zgi::FrameRec& r = recs[k];
      zgpu_frame_index& f = frames[k];
      FrameFields hf;
      frame_fields(r.b, r.have, &hf);
      memset(&f, 0, sizeof f);
      f.src_begin = r.begin; f.src_end = r.end; f.bound = r.bound;
      f.frame_content_size = hf.frame_content_size; f.window_size = hf.window_size;
      f.entry = i; f.nblocks = r.nblocks;
      f.dict_id = hf.dict_id;
      f.flags = hf.flags | r.flags;
      f.header_status = hf.header_status; f.skip_magic = hf.skip_magic;
      if (r.begin > r.end || r.end > lens[i] || ((r.flags & zgi::kSkippable) != 0) != (hf.header_status == ZGPU_E_SKIP_FRAME)) {   // (never)
        c->eng->last_error = "zgpu_frames_table_device: a frame record out of step with its header";
        return ZGPU_E_INTERNAL;
      }
    }
  }
  return ZGPU_OK;
}
extern "C" int zgpu_debug_frames_index_stats(const zgpu_ctx* c, uint64_t* out, int n) { return c ? copy_stats(c->frames_index_stats, out, n) : 0; }
extern "C" int zgpu_debug_frames_device_src_stats(const zgpu_ctx* c, uint64_t* out, int n) { return c ? copy_stats(c->frames_device_src_stats, out, n) : 0; }
extern "C" void zgpu_set_frames_shared_dicts(zgpu_ctx* c, int on) { if (c) c->frames_shared_dicts = on != 0; }
extern "C" int zgpu_frames_shared_dicts(const zgpu_ctx* c) { return c && c->frames_shared_dicts ? 1 : 0; }
extern "C" int zgpu_debug_frames_dict_stats(const zgpu_ctx* c, uint64_t* out, int n) { return c ? copy_stats(c->frames_dict_stats, out, n) : 0; }
extern "C" int zgpu_debug_frames_device_stats(const zgpu_ctx* c, uint64_t* out, int n) { return c ? copy_stats(c->frames_device_stats, out, n) : 0; }

extern "C" uint64_t zgpu_plaintext_bound(const uint8_t* src, size_t len) { return src || !len ? plaintext_bound(src, len) : 0; }
extern "C" uint32_t zgpu_debug_frames_submits(const zgpu_ctx* c) { return c ? c->frames_submits : 0u; }
