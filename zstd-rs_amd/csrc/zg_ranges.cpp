// zg_ranges.cpp — the calls of include/zgpu.h that decode byte RANGES of device-resident entries: front-ends of zg_frames.cpp's machinery.
// Each of them decides which bytes of its entries become sub-entries of that machinery (zg_frames_int.h: Selection) and what of a decoded
// sub-entry goes to which destination (Clip), and hands both to decode_selections; the seek-only twin of each returns the records alone.
// The calls with one range per entry (zg_seek.h: the header chain; zg_seektab.h: the seek table) hand over spans of one clip.
//
// zgpu_gather_ranges_seek_table_device_src takes m ranges that each name one of n seekable entries (zg_seekmany.h: every table scanned once,
// every range a binary search). The ranges of one entry whose table rows overlap form a group; a group is ONE selection, decoded once, and
// every range of it is a clip of the group's span with its own destination. zgpu_gather_ranges_indexed_device_src is the same call behind
// another selection: a zgpu_seek_index keeps the prefix sums of its entries' rows in device memory — built from their seek tables, or from
// their header chains where every frame declares its size (zg_seekidx.h) —, indexed_ranges finds every range's rows in them with one launch,
// and gather_groups is shared. zgpu_seek_index_measure_device builds the same handle for entries whose frames declare nothing: measure_entries
// cuts their frame records into runs, runs them through the device-source machinery and Batch::measure (zg_seqsize.h), and the sizes that
// come back become the pairs; zgpu_seek_index_export_seek_table writes an entry's pairs out as a seek table (zg_seektab.h).
// The calls that take record NUMBERS (zg_records.h) are a lookup in front of the indexed gather; zgpu_gather_records_batch_indexed_device_src
// lays that gather's destinations out in ONE piece of device memory (plan_rows) and pads what it left unwritten (zg_scatter.h: zg_k_fill).
#include <stddef.h>
#include <algorithm>
#include <string.h>
#include <string>
#include <vector>
#include "zg_frames_int.h"
#include "zg_seeksums.h"
#include "zg_idxsums.h"
#include "zg_records.h"

using namespace zg;
using namespace zgf;

// ---- byte ranges of device-resident entries (zg_seek.h) --------------------------------------------------------------------------------------
static_assert(sizeof(zgpu_range) == 32 && sizeof(zgpu_seek) == sizeof(zgk::Seek) && sizeof(zgpu_range_result) == sizeof(zgpu_device_entry_result) + 64,
              "include/zgpu.h");
static_assert(offsetof(zgpu_seek, plain_seen) == offsetof(zgk::Seek, plain_seen) && offsetof(zgpu_seek, status) == offsetof(zgk::Seek, status) &&
              offsetof(zgpu_seek, flags) == offsetof(zgk::Seek, flags) && ZGPU_E_BAD_ARG == zgk::kBadArg, "zgk::Seek is zgpu_seek");
static_assert(ZGPU_E_SEEK_TABLE == zgt::kSeekTable && ZGPU_SEEKTAB_NONE == zgt::kNone && ZGPU_SEEKTAB_RESERVED_BITS == zgt::kReservedBits &&
              ZGPU_SEEKTAB_TOO_LARGE == zgt::kTooLarge && ZGPU_SEEKTAB_BAD_FRAME == zgt::kBadFrame && ZGPU_SEEKTAB_PAST_TABLE == zgt::kPastTable,
              "zg_seektab.h");
static_assert(ZGPU_E_SEEK_CHECKSUM_MISMATCH == zgv::kSeekChecksumMismatch, "zg_seeksums.h");
namespace {
// The records a selection brought back, accepted: a refused range gets a record of zeros with ZGPU_E_BAD_ARG; every other record is held
// against the length of its entry, len_of(j), and may carry no status but `allowed` — one that leaves its entry ends the call (never: `text`
// in last_error) —; the frames in front of the selections are counted.
template <class Len>
int accept_records(zgpu_ctx* c, std::vector<zgk::Seek>* recs, const std::vector<uint8_t>& refused, Len len_of, uint32_t allowed, const char* text) {
  for (uint32_t j = 0; j < (uint32_t)recs->size(); j++) {
    zgk::Seek& s = (*recs)[j];
    if (refused[j]) { s = zgk::Seek{}; s.status = ZGPU_E_BAD_ARG; continue; }
    if (s.src_lo > s.src_hi || s.src_hi > len_of(j) || (s.status && s.status != allowed)) {   // (never)
      c->eng->last_error = text;
      return ZGPU_E_INTERNAL;
    }
    c->ranges_stats[kRangeStatFramesSkipped] += s.frames_skipped;
  }
  return ZGPU_OK;
}
// m records to the caller, record j to at(j): zeros when the call failed
template <class At> void records_out(const std::vector<zgk::Seek>& recs, bool failed, uint32_t m, At at) {
  for (uint32_t j = 0; j < m; j++) { if (failed) memset(at(j), 0, sizeof(zgpu_seek)); else memcpy(at(j), &recs[j], sizeof(zgpu_seek)); }
}
// the seek calls: the records themselves are the answer. select(&recs, &refused): the call's selection
template <class Select> int seek_only(zgpu_ctx* c, uint32_t m, zgpu_seek* out, Select select) {
  reset_stats(c, kOwnsRanges);
  std::vector<zgk::Seek> recs;
  std::vector<uint8_t> refused;
  const int st = select(&recs, &refused);
  records_out(recs, st != 0, m, [&](uint32_t j) { return &out[j]; });
  return st;
}

// Both calls up to the records: every pointer checked, ONE zg_k_seek launch over all n lanes (a refused entry and a range of length 0 have
// length 0 for their lane: nothing of them is read). dsts / caps: nullptr for the seek call, which has no destinations. table: the selection
// comes from the seek table at the entry's end (ONE zg_k_seektab launch, a wave per entry); an anchored range is refused, the table is the index.
int seek_ranges(zgpu_ctx* c, const void* const* srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges, void* const* dsts, const size_t* caps,
                std::vector<zgk::Seek>* out, std::vector<uint8_t>* refused, bool table) {
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  std::vector<zgk::Lane> lanes(table ? 0 : n);
  std::vector<zgt::Lane> waves(table ? n : 0);
  out->assign(n, zgk::Seek{});
  std::vector<Engine::DevEntry> dev;
  // (a range of length 0 is never refused: nothing of its entry is touched; with a seek table an anchored range is refused, the table is the index)
  check_entries(c, srcs, lens, dsts, caps, n,
                [&](uint32_t i) { return !ranges[i].len ? kPass : table && (ranges[i].anchor_src || ranges[i].anchor_plain) ? kRefuse : kCheck; }, &dev, refused);
  for (uint32_t i = 0; i < n; i++) {
    const zgpu_range& g = ranges[i];
    const bool bad = (*refused)[i] != 0;
    if (table) waves[i] = zgt::Lane{dev[i].src, dev[i].len, g.begin, bad ? 0u : g.len};
    else lanes[i] = zgk::Lane{dev[i].src, dev[i].len, g.begin, bad ? 0u : g.len, bad ? 0u : g.anchor_src, bad ? 0u : g.anchor_plain};
  }
  const int st = drain(c, table ? c->eng->seektab_pass(waves.data(), n, out->data(), c->ranges_stats) : c->eng->seek_pass(lanes.data(), n, out->data(), c->ranges_stats));
  if (st) return st;
  return accept_records(c, out, *refused, [&](uint32_t i) { return (uint64_t)lens[i]; }, table ? (uint32_t)ZGPU_E_SEEK_TABLE : (uint32_t)ZGPU_E_BAD_ARG,
                        "zgpu_frames_seek_device: a record that leaves its entry");
}
}  // namespace

extern "C" int zgpu_frames_seek_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges, zgpu_seek* out) {
  if (!c || (n && (!device_srcs || !lens || !ranges || !out))) return ZGPU_E_BAD_ARG;
  return seek_only(c, n, out, [&](auto* recs, auto* refused) { return seek_ranges(c, device_srcs, lens, n, ranges, nullptr, nullptr, recs, refused, false); });
}
extern "C" int zgpu_frames_seek_table_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges,
                                             zgpu_seek* out) {
  if (!c || (n && (!device_srcs || !lens || !ranges || !out))) return ZGPU_E_BAD_ARG;
  return seek_only(c, n, out, [&](auto* recs, auto* refused) { return seek_ranges(c, device_srcs, lens, n, ranges, nullptr, nullptr, recs, refused, true); });
}

// One selection per entry — the frames zg_k_seek found to hold its range —, one clip each: spans of one.
// table (zgpu_decode_ranges_seek_table_device_src): the selections are zg_k_seektab's. Three things differ: the seek's bound is the table's
// promise and is not compared with the walk's header bound; Selection::declared is that promise, and an entry whose decoded total differs from
// it fails with ContentSizeMismatch; an entry whose table is not usable is refused with ZGPU_E_SEEK_TABLE, unread and unwritten.
namespace {
int decode_ranges(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges, void* const* device_dsts,
                  const size_t* caps, const zgpu_device_opts* opts, zgpu_range_result* results, bool table) {
  if (!c || (n && (!device_srcs || !lens || !ranges || !device_dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  int st;
  DeviceSink sink = device_sink(c, opts, nullptr, &st, table);
  if (st) return st;
  reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc | kOwnsRanges);
  for (uint32_t i = 0; i < n; i++) memset(&results[i], 0, sizeof results[i]);
  std::vector<zgk::Seek> recs;
  std::vector<uint8_t> refused;
  if ((st = seek_ranges(c, device_srcs, lens, n, ranges, device_dsts, caps, &recs, &refused, table))) return st;
  // the selections (in place of the whole entries seek_ranges checked) and what of each is wanted. An entry of which nothing is taken stays a
  // selection, an empty one: a submit that holds only such entries is still a submit
  std::vector<Selection> sel(n);
  std::vector<Clip> clip(n);
  std::vector<uint32_t> first((size_t)n + 1);
  std::vector<uint64_t> bound(n);
  for (uint32_t i = 0; i <= n; i++) first[i] = i;
  for (uint32_t i = 0; i < n; i++) {
    const zgk::Seek& s = recs[i];
    const uint8_t ref = s.status ? (uint8_t)(s.status == ZGPU_E_SEEK_TABLE ? ZGPU_E_SEEK_TABLE : 1) : refused[i];   // (a status: an anchor behind the entry or behind begin; no usable table)
    const bool none = ref || !ranges[i].len || (s.flags & zgk::kNothing);   // (nothing is read, decoded or written)
    const bool closed = !(s.flags & (zgk::kOpenEnded | zgk::kBroken));
    const uint64_t declared = none ? (table ? 0 : UINT64_MAX) : closed ? s.plain_seen - s.plain_lo : UINT64_MAX;   // (table: an entry of which nothing is taken promises nothing)
    sel[i] = Selection{i, none ? 0 : s.src_lo, none ? 0 : s.src_hi, declared, s.frames_skipped, none ? 0u : s.frames_taken, ref};
    clip[i] = Clip{none ? 0 : ranges[i].begin - s.plain_lo, ranges[i].len, (uint8_t*)device_dsts[i], caps[i], 0, false};
    bound[i] = s.bound;
  }
  std::vector<zgpu_device_entry_result> dres(n);
  st = decode_selections(c, sink, device_srcs, lens, sel, clip, first, table, table ? nullptr : bound.data(), dres.data());   // (the table's bound is its promise: not compared)
  for (uint32_t i = 0; i < n && !st; i++) results[i].d = dres[i];
  records_out(recs, false, n, [&](uint32_t i) { return &results[i].seek; });
  return st;
}
}  // namespace

extern "C" int zgpu_decode_ranges_device_src(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges,
                                             void* const* device_dsts, const size_t* caps, const zgpu_device_opts* opts, zgpu_range_result* results) {
  return decode_ranges(c, device_srcs, lens, n, ranges, device_dsts, caps, opts, results, false);
}
extern "C" int zgpu_decode_ranges_seek_table_device_src(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                        const zgpu_range* ranges, void* const* device_dsts, const size_t* caps,
                                                        const zgpu_device_opts* opts, zgpu_range_result* results) {
  return decode_ranges(c, device_srcs, lens, n, ranges, device_dsts, caps, opts, results, true);
}
// ---- many ranges over few seekable entries (zg_seekmany.h) ------------------------------------------------------------------------------------
static_assert(sizeof(zgpu_entry_range) == 24 && offsetof(zgpu_entry_range, entry) == 16, "include/zgpu.h");
namespace {
// Both calls up to the records. Every range is looked at on its own (check_entry_ranges; a refused range has ZGPU_E_BAD_ARG in its record),
// then Engine::seekmany_pass over the entries that passed: each table scanned once, every range a binary search. dsts / caps: nullptr for
// the seek call.
int seek_many(zgpu_ctx* c, const void* const* srcs, const size_t* lens, uint32_t n, const zgpu_entry_range* ranges, uint32_t m, void* const* dsts,
              const size_t* caps, std::vector<zgk::Seek>* out, std::vector<uint8_t>* refused) {
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  out->assign(m, zgk::Seek{});
  std::vector<uint8_t> is_live;
  std::vector<uint32_t> passed;
  check_entry_ranges(c, srcs, lens, n, ranges, m, dsts, caps, check_all, refused, &is_live, &passed);
  // an entry that passed is a live entry of the pass, in the order in which it passed
  std::vector<uint32_t> live_of(n, 0);
  std::vector<Engine::DevEntry> live(passed.size());
  for (uint32_t q = 0; q < (uint32_t)passed.size(); q++) {
    live_of[passed[q]] = q;
    live[q] = Engine::DevEntry{(uint64_t)(uintptr_t)srcs[passed[q]], (uint64_t)lens[passed[q]]};
  }
  std::vector<Engine::ManyRange> mr(m);
  for (uint32_t j = 0; j < m; j++)
    mr[j] = is_live[j] ? Engine::ManyRange{ranges[j].begin, ranges[j].len, live_of[ranges[j].entry]} : Engine::ManyRange{ranges[j].begin, 0, 0};
  Engine::ManyStats more;
  const int st = drain(c, c->eng->seekmany_pass(live.data(), (uint32_t)live.size(), mr.data(), m, out->data(), c->ranges_stats, &more));
  uint64_t* ms = c->ranges_many_stats;
  ms[kManyStatPrefixLaunches] = more.prefix_launches; ms[kManyStatPrefixUs] = more.prefix_us;
  ms[kManyStatFindLaunches] = more.find_launches; ms[kManyStatFindUs] = more.find_us; ms[kManyStatPrefixScratchBytes] = more.scratch_bytes;
  if (st) return st;
  return accept_records(c, out, *refused, [&](uint32_t j) { return (uint64_t)lens[ranges[j].entry]; }, (uint32_t)ZGPU_E_SEEK_TABLE,
                        "zgpu_frames_seek_table_many_device: a record that leaves its entry");
}
}  // namespace

extern "C" int zgpu_frames_seek_table_many_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                  const zgpu_entry_range* ranges, uint32_t m, zgpu_seek* out) {
  if (!c || (n && (!device_srcs || !lens)) || (m && (!ranges || !out))) return ZGPU_E_BAD_ARG;
  return seek_only(c, m, out, [&](auto* recs, auto* refused) { return seek_many(c, device_srcs, lens, n, ranges, m, nullptr, nullptr, recs, refused); });
}

// The ranges of one entry whose rows overlap form a GROUP (zg_seekmany.h: group_ranges), and a group is ONE selection — the rows
// [gfirst, glast] its ranges take together: (src + C_gfirst, C_{glast + 1} - C_gfirst) is walked, cut into submits, gathered, decoded and
// hashed once, and every range is a clip of the group's span with its own destination. What a group's frames do — a decode or walk error, a
// size that differs from the table's promise, a checksum verdict — is the verdict of every range in it; TargetTooSmall is each range's own.
// Both gather calls (the seek-table one and the indexed one) around their selection: select(sink, &recs, &refused) leaves the m records and
// refusals, whatever produced the pairs they were found in, and everything behind it is shared.
namespace {
template <class Select>
int gather_groups(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, const zgpu_entry_range* ranges, uint32_t m, void* const* device_dsts,
                  const size_t* caps, const zgpu_device_opts* opts, zgpu_range_result* results, Select select) {
  int st;
  DeviceSink sink = device_sink(c, opts, nullptr, &st, true);
  if (st) return st;
  reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc | kOwnsRanges);
  for (uint32_t j = 0; j < m; j++) memset(&results[j], 0, sizeof results[j]);
  std::vector<zgk::Seek> recs;
  std::vector<uint8_t> refused;
  if ((st = select(sink, &recs, &refused))) return st;
  const zgm::Groups gs = zgm::group_ranges(ranges, recs.data(), refused.data(), m);
  const uint32_t G = (uint32_t)gs.groups.size();
  // the groups as selections, each with the clips of its ranges
  std::vector<Selection> sel(G);
  for (uint32_t g = 0; g < G; g++) {
    const zgm::Group& gr = gs.groups[g];
    if (gr.c_lo > gr.c_hi || gr.d_lo > gr.d_hi) { c->eng->last_error = "zgpu_gather_ranges_seek_table_device_src: records of one table out of step"; return ZGPU_E_INTERNAL; }   // (never)
    sel[g] = Selection{gr.entry, gr.c_lo, gr.c_hi, gr.d_hi - gr.d_lo, gr.gfirst, gr.glast - gr.gfirst + 1, 0};
  }
  std::vector<Clip> clip(gs.order.size());
  for (size_t q = 0; q < clip.size(); q++) {
    const uint32_t j = gs.order[q];
    clip[q] = Clip{gs.skip[q], ranges[j].len, (uint8_t*)device_dsts[j], caps[j], 0, false};
  }
  std::vector<zgpu_device_entry_result> dres(G);
  st = decode_selections(c, sink, device_srcs, lens, sel, clip, gs.first, true, nullptr, dres.data());
  c->ranges_many_stats[kManyStatGroupsDecoded] = G;
  // every range's result: the group's, with the range's own count — or its own TargetTooSmall, which ranks behind the group's decode, walk
  // and size verdicts and in front of its checksum verdicts
  records_out(recs, false, m, [&](uint32_t j) { return &results[j].seek; });
  for (uint32_t j = 0; j < m && !st; j++) {
    zgpu_device_entry_result& d = results[j].d;
    if (refused[j] || recs[j].status) { d.r.status = refused[j] ? ZGPU_E_BAD_ARG : (int)recs[j].status; continue; }
    if (!ranges[j].len || !recs[j].frames_taken) continue;   // (nothing is read, decoded or written: status 0, written 0)
    const zgpu_device_entry_result& gd = dres[gs.group_of[j]];
    const Clip& cl = clip[gs.clip_of[j]];
    const bool checks = gd.r.status == ZGPU_E_CHECKSUM_MISMATCH || gd.r.status == ZGPU_E_SEEK_CHECKSUM_MISMATCH;
    if (gd.r.status == ZGPU_E_TARGET_TOO_SMALL || ((!gd.r.status || checks) && cl.small)) { d.r.status = ZGPU_E_TARGET_TOO_SMALL; continue; }
    d = gd;
    if (!gd.r.status) d.r.written = cl.written;
  }
  return st;
}
}  // namespace

extern "C" int zgpu_gather_ranges_seek_table_device_src(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                        const zgpu_entry_range* ranges, uint32_t m, void* const* device_dsts, const size_t* caps,
                                                        const zgpu_device_opts* opts, zgpu_range_result* results) {
  if (!c || (n && (!device_srcs || !lens)) || (m && (!ranges || !device_dsts || !caps || !results))) return ZGPU_E_BAD_ARG;
  return gather_groups(c, device_srcs, lens, ranges, m, device_dsts, caps, opts, results, [&](DeviceSink&, auto* recs, auto* refused) {
    return seek_many(c, device_srcs, lens, n, ranges, m, device_dsts, caps, recs, refused);
  });
}

// ---- seek index handles (include/zgpu.h: zgpu_seek_index; zg_seekidx.h) -------------------------------------------------------------------------
static_assert(sizeof(zgpu_seek_index_info) == 40 && ZGPU_INDEX_UNSIZED == zgx::kUnsized && ZGPU_E_FRAME_INDEX == 74, "include/zgpu.h");
static_assert(ZGPU_INDEX_MEASURED == 3 && ZGPU_INDEX_UNMEASURED == 33u && ZGPU_INDEX_DICT == 34u && ZGPU_MEASURE_ALL == 0 && ZGPU_MEASURE_UNSIZED == 1,
              "include/zgpu.h");
namespace {
// an entry the index refuses: nothing of it is held
void refuse_index(zgpu_seek_index::Ent& e, uint32_t status, uint32_t why, uint32_t kind) {
  e.info.status = status; e.info.why = why; e.info.kind = kind;
  e.info.nrows = 0; e.info.compressed = 0; e.info.plaintext = 0;
  e.pre = 0; e.tab = 0;
}

// ---- measuring (zgpu_seek_index_measure_device) ------------------------------------------------------------------------------------------------
// What measuring found of one entry: its nrows + 1 pairs, or the first zstd frame of it whose measuring ended in a status.
struct Measured { std::vector<zgm::Pair> pairs; uint32_t status = 0, frame = 0; };
constexpr int kNoMeasure = -1;   // build_index: zgpu_seek_index_create_device

// The entries ent[0 .. ne) — whole chains without a dictionary frame, sum[q] their summaries — measured: the frame records of the table call
// give every row's bytes (zg_k_index<true>); runs of whole frames become the entries of the device-source machinery (zg_k_walk's skeleton,
// the host's one parse, zg_k_gather), cut at frame boundaries into submits of at most S input bytes — a frame is never split, one above S
// is a submit of its own —, and each submit is measured (Batch::measure) where a decode call runs it. d_k = the frame's out_size as
// zg_k_scan left it. No byte of an entry comes back: records and skeletons do.
int measure_entries(zgpu_ctx* c, const std::vector<Engine::DevEntry>& ent, const std::vector<zgi::Entry>& sum, std::vector<Measured>* out, uint64_t* stats) {
  zg::Engine* eng = c->eng;
  const uint32_t ne = (uint32_t)ent.size();
  out->assign(ne, Measured{});
  if (!ne) return ZGPU_OK;
  const Tuning& tn = eng->tuning();
  const uint64_t S = tn.measure_submit_bytes ? tn.measure_submit_bytes : tn.frames_submit_bytes ? tn.frames_submit_bytes : kFramesSubmitBytes;
  const char* const changed = "zgpu_seek_index_measure_device: a source changed while it was measured";
  std::vector<uint64_t> first((size_t)ne + 1);
  const uint64_t total = zgi::frame_ranges(sum.data(), ne, first.data());
  std::vector<zgi::FrameRec> recs(total);
  std::vector<zgi::Entry> again(ne);
  int st;
  if (total && (st = eng->index_pass(ent.data(), ne, first.data(), sum.data(), again.data(), recs.data(), stats))) return st;
  // the runs: consecutive frame records of one entry, up to S bytes, each with a zstd frame in it
  struct Run { uint32_t q; uint64_t k0, k1; };
  std::vector<Run> runs;
  std::vector<Engine::DevEntry> rdev;
  for (uint32_t q = 0; q < ne; q++) {
    if (total && !zgi::same_entry(again[q], sum[q])) { eng->last_error = changed; return ZGPU_E_INTERNAL; }
    uint64_t at = 0, k0 = first[q];
    bool any = false;
    auto close = [&](uint64_t k1) {
      if (any) { runs.push_back(Run{q, k0, k1}); rdev.push_back(Engine::DevEntry{ent[q].src + recs[k0].begin, recs[k1 - 1].end - recs[k0].begin}); }
      k0 = k1; any = false;
    };
    for (uint64_t k = first[q]; k < first[q + 1]; k++) {
      const zgi::FrameRec& r = recs[k];
      if (r.begin != at || r.end < r.begin || r.end > ent[q].len) { eng->last_error = changed; return ZGPU_E_INTERNAL; }
      at = r.end;
      if (k > k0 && r.end - recs[k0].begin > S) close(k);
      any = any || !(r.flags & zgi::kSkippable);
    }
    close(first[q + 1]);
    if (at != ent[q].len) { eng->last_error = changed; return ZGPU_E_INTERNAL; }
  }
  // every run's skeleton: two launches for the whole call
  Engine::Skeleton sk;
  if ((st = eng->walk_entries(rdev.data(), (uint32_t)rdev.size(), &sk, stats))) return st;
  // d_k of every record (0: a skippable frame), submit by submit
  std::vector<uint64_t> dk(total, 0);
  std::vector<uint32_t> zframes(ne, 0);   // zstd frames of the entry seen so far
  for (size_t r0 = 0; r0 < runs.size();) {
    std::vector<uint32_t> idx;
    std::vector<uint64_t> off;
    uint64_t in_bytes = 0;
    size_t r1 = r0;
    for (; r1 < runs.size() && (r1 == r0 || in_bytes + rdev[r1].len <= S); r1++) { idx.push_back((uint32_t)r1); off.push_back(in_bytes); in_bytes += rdev[r1].len; }
    Batch* b = nullptr;
    std::vector<int> walk;
    std::vector<uint32_t> ff;
    if ((st = eng->prepare_entries_device(rdev.data(), sk, idx.data(), off.data(), (uint32_t)idx.size(), (size_t)in_bytes, &b, &walk, &ff, nullptr))) return st;
    struct Del { Batch* b; ~Del() { delete b; } } del{b};
    stats[kSeekIdxStatLaunches] += b->gather_launched ? 1u : 0u; stats[kSeekIdxStatKernelUs] += b->gather_us;
    uint64_t us = 0;
    if ((st = b->measure(&us))) return st;
    stats[kSeekIdxStatMeasureSubmits]++; stats[kSeekIdxStatMeasureUs] += us;
    if (b->frame_out.size() != b->info.size()) return ZGPU_E_INTERNAL;
    for (size_t j = 0; j < idx.size(); j++) {
      const Run& run = runs[idx[j]];
      Measured& m = (*out)[run.q];
      uint32_t f = ff[j];
      for (uint64_t k = run.k0; k < run.k1; k++) {
        const zgi::FrameRec& r = recs[k];
        if (r.flags & zgi::kSkippable) continue;
        const uint32_t zf = zframes[run.q]++;
        uint32_t fst;
        if (f < ff[j + 1]) {
          const FrameInfo& fi = b->info[f];
          fst = fi.host_status ? (uint32_t)fi.host_status : b->frame_out[f].status;
          if (!fi.host_status && (fi.src_begin != off[j] + (r.begin - recs[run.k0].begin) || fi.src_end - fi.src_begin != r.end - r.begin)) {
            eng->last_error = changed;
            return ZGPU_E_INTERNAL;
          }
          dk[k] = b->frame_out[f].out_size;
          f++;
        } else {   // the host's walk of the run ended in front of this frame: at its header
          if (!walk[j]) { eng->last_error = changed; return ZGPU_E_INTERNAL; }
          fst = (uint32_t)walk[j];
        }
        if (fst && !m.status) { m.status = fst; m.frame = zf; }
        if (!fst) stats[kSeekIdxStatFramesMeasured]++;
        if (fst) break;   // (what lies behind a frame the walk stopped in is not in the submit)
      }
    }
    r0 = r1;
  }
  for (uint32_t q = 0; q < ne; q++) {
    Measured& m = (*out)[q];
    if (m.status) continue;
    const uint64_t nrows = first[q + 1] - first[q];
    m.pairs.resize((size_t)nrows + 1);
    uint64_t d = 0;
    for (uint64_t k = 0; k < nrows; k++) {
      m.pairs[k] = zgm::Pair{recs[first[q] + k].begin, d};
      const uint64_t add = dk[first[q] + k];
      d = add > UINT64_MAX - d ? UINT64_MAX : d + add;
    }
    m.pairs[nrows] = zgm::Pair{ent[q].len, d};
  }
  return ZGPU_OK;
}

// The build. The table pass works in a scratch of its own (its chunk totals lie behind the prefixes); the handle's buffer is sized exactly —
// 16 * (nrows + 1) bytes per indexed entry —, gets the table entries' pairs by one device copy each, and the declared entries' pairs straight
// from zg_k_seekidx_rows. measure (zgpu_seek_index_measure_device): ZGPU_MEASURE_ALL — no table and no declared size is looked at, every entry
// is measured —, or ZGPU_MEASURE_UNSIZED with kind = ZGPU_INDEX_AUTO — an entry is measured where AUTO answers ZGPU_INDEX_UNSIZED. The
// measured entries' pairs are built on the host (measure_entries), lie behind the others' and reach the handle in one copy.
int build_index(zgpu_ctx* c, zgpu_seek_index* x, const void* const* srcs, const size_t* lens, uint32_t n, uint32_t kind, int measure) {
  const bool all = measure == (int)ZGPU_MEASURE_ALL, unsized = measure == (int)ZGPU_MEASURE_UNSIZED;
  const std::string who = measure == kNoMeasure ? "zgpu_seek_index_create_device" : "zgpu_seek_index_measure_device";   // (the call last_error names)
  zg::Engine* eng = c->eng;
  if (hipSetDevice(eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  std::vector<Engine::DevEntry> dev;
  std::vector<uint8_t> refused;
  check_entries(c, srcs, lens, nullptr, nullptr, n, check_all, &dev, &refused);
  x->ents.assign(n, zgpu_seek_index::Ent{});
  std::vector<uint8_t> by_chain(n, 0);   // entries the chain is asked about
  for (uint32_t i = 0; i < n; i++) {
    x->ents[i].info.len = lens[i];
    if (refused[i]) refuse_index(x->ents[i], ZGPU_E_BAD_ARG, 0, all ? ZGPU_INDEX_MEASURED : kind == ZGPU_INDEX_DECLARED ? ZGPU_INDEX_DECLARED : ZGPU_INDEX_SEEK_TABLE);
    else by_chain[i] = kind == ZGPU_INDEX_DECLARED || all;
  }
  uint64_t* stats = x->stats;
  // the tables
  zg::DevBuf scratch;
  std::vector<zgm::Loc> loc;
  std::vector<uint64_t> tpre;
  std::vector<uint32_t> tab_of;   // the entries the table pass was asked about
  struct Free { zg::DevBuf& b; ~Free() { b.release(); } } free_scratch{scratch};
  if (kind != ZGPU_INDEX_DECLARED && !all) {
    std::vector<Engine::DevEntry> live;
    for (uint32_t i = 0; i < n; i++) if (!refused[i]) { tab_of.push_back(i); live.push_back(dev[i]); }
    loc.resize(live.size());
    tpre.assign(live.size(), 0);
    Engine::ManyStats more;
    uint64_t npairs = 0;
    const int st = eng->seekmany_prefixes(live.data(), (uint32_t)live.size(), loc.data(), tpre.data(), &scratch, &npairs, stats, &more);
    stats[kSeekIdxStatLaunches] += more.prefix_launches; stats[kSeekIdxStatKernelUs] += more.prefix_us;
    if (st) return st;
    for (size_t q = 0; q < tab_of.size(); q++) {
      zgpu_seek_index::Ent& e = x->ents[tab_of[q]];
      if (loc[q].why == zgt::kNone && kind == ZGPU_INDEX_AUTO) by_chain[tab_of[q]] = 1;
      else if (loc[q].why) refuse_index(e, ZGPU_E_SEEK_TABLE, loc[q].why, ZGPU_INDEX_SEEK_TABLE);
      else { e.info.kind = ZGPU_INDEX_SEEK_TABLE; e.info.nrows = loc[q].nf; e.tab = loc[q].tab; }
    }
  }
  // the chains: the summary pass says which entries can be indexed and how many rows each has
  std::vector<uint32_t> ch_of;
  std::vector<Engine::DevEntry> chain;
  for (uint32_t i = 0; i < n; i++) if (by_chain[i]) { ch_of.push_back(i); chain.push_back(dev[i]); }
  std::vector<zgi::Entry> sum(chain.size());
  int st = eng->index_pass(chain.data(), (uint32_t)chain.size(), nullptr, nullptr, sum.data(), nullptr, stats);
  if (st) return st;
  std::vector<uint32_t> meas_of;   // the entries that are measured, and (chain / sum index) where their summaries lie
  std::vector<size_t> meas_q;
  for (size_t q = 0; q < ch_of.size(); q++) {
    zgpu_seek_index::Ent& e = x->ents[ch_of[q]];
    const uint32_t why = zgx::refusal(sum[q]);
    if (sum[q].chain_end > lens[ch_of[q]]) { eng->last_error = who + ": a summary that leaves its entry"; return ZGPU_E_INTERNAL; }   // (never)
    if (all || (unsized && why == zgx::kUnsized)) {   // (kUnsized: the chain itself is whole)
      const uint32_t mw = sum[q].why ? sum[q].why : sum[q].nrec > zgt::kMaxFrames ? (uint32_t)ZGPU_SEEKTAB_TOO_LARGE : (sum[q].flags & zgi::kAnyDict) ? ZGPU_INDEX_DICT : 0u;
      if (mw) refuse_index(e, ZGPU_E_FRAME_INDEX, mw, ZGPU_INDEX_MEASURED);
      else { e.info.kind = ZGPU_INDEX_MEASURED; e.info.nrows = sum[q].nrec; e.tab = lens[ch_of[q]]; meas_of.push_back(ch_of[q]); meas_q.push_back(q); }
      continue;
    }
    if (why) refuse_index(e, ZGPU_E_FRAME_INDEX, why, ZGPU_INDEX_DECLARED);
    else if (sum[q].nrec > zgt::kMaxFrames) refuse_index(e, ZGPU_E_FRAME_INDEX, ZGPU_SEEKTAB_TOO_LARGE, ZGPU_INDEX_DECLARED);
    else { e.info.kind = ZGPU_INDEX_DECLARED; e.info.nrows = sum[q].nrec; e.tab = lens[ch_of[q]]; }
  }
  // the measured entries: an entry with a frame whose measuring ended in a status is refused, and the first of them is named
  std::vector<Measured> meas;
  {
    std::vector<Engine::DevEntry> ment(meas_of.size());
    std::vector<zgi::Entry> msum(meas_of.size());
    for (size_t t = 0; t < meas_of.size(); t++) { ment[t] = chain[meas_q[t]]; msum[t] = sum[meas_q[t]]; }
    if ((st = measure_entries(c, ment, msum, &meas, stats))) return st;
    bool named = false;
    for (size_t t = 0; t < meas_of.size(); t++) {
      if (!meas[t].status) continue;
      refuse_index(x->ents[meas_of[t]], ZGPU_E_FRAME_INDEX, ZGPU_INDEX_UNMEASURED, ZGPU_INDEX_MEASURED);
      if (!named) eng->last_error = "zgpu_seek_index_measure_device: entry " + std::to_string(meas_of[t]) + ", frame " + std::to_string(meas[t].frame) + ": " + zgpu_status_name((int)meas[t].status);
      named = true;
    }
  }
  // the handle's pairs: every indexed entry's range, the measured entries' behind the others'
  uint64_t pairs = 0, meas_pre = 0;
  for (int pass = 0; pass < 2; pass++) {
    if (pass) meas_pre = pairs;
    for (uint32_t i = 0; i < n; i++) {
      zgpu_seek_index::Ent& e = x->ents[i];
      if (e.info.status || (e.info.kind == ZGPU_INDEX_MEASURED) != (pass == 1)) continue;
      e.pre = pairs;
      pairs += (uint64_t)e.info.nrows + 1;
      e.spre = x->nsums;   // (where its sums will lie, should it get any)
      x->nsums += e.info.nrows;
    }
  }
  if (pairs > SIZE_MAX / sizeof(zgm::Pair)) return ZGPU_E_NOMEM;
  if (pairs && (st = x->pairs.reserve((size_t)pairs * sizeof(zgm::Pair)))) return st;
  x->npairs = pairs;
  stats[kSeekIdxStatDeviceBytes] = pairs * sizeof(zgm::Pair);
  zgm::Pair* dp = x->pairs.as<zgm::Pair>();
  hipStream_t s = eng->stream();
  // table kind: the prefixes move over, and each entry's closing pair comes back (16 bytes: C[nrows], D[nrows])
  std::vector<zgm::Pair> closing(tab_of.size(), zgm::Pair{0, 0});
  for (size_t q = 0; q < tab_of.size(); q++) {
    const zgpu_seek_index::Ent& e = x->ents[tab_of[q]];
    if (e.info.status || e.info.kind != ZGPU_INDEX_SEEK_TABLE) continue;
    const zgm::Pair* from = scratch.as<zgm::Pair>() + tpre[q];
    if (hipMemcpyAsync(dp + e.pre, from, ((size_t)e.info.nrows + 1) * sizeof(zgm::Pair), hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(&closing[q], from + e.info.nrows, sizeof(zgm::Pair), hipMemcpyDeviceToHost, s) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
    stats[kSeekIdxStatBytesDownloaded] += sizeof(zgm::Pair);
  }
  // measured kind: the pairs the host built, in one copy
  std::vector<zgm::Pair> mpairs;
  for (size_t t = 0; t < meas_of.size(); t++) {
    zgpu_seek_index::Ent& e = x->ents[meas_of[t]];
    if (e.info.status) continue;
    if (meas[t].pairs.size() != (size_t)e.info.nrows + 1 || e.pre != meas_pre + mpairs.size()) return ZGPU_E_INTERNAL;   // (never)
    mpairs.insert(mpairs.end(), meas[t].pairs.begin(), meas[t].pairs.end());
    e.info.compressed = meas[t].pairs.back().c; e.info.plaintext = meas[t].pairs.back().d;
  }
  if (!mpairs.empty() && hipMemcpyAsync(dp + meas_pre, mpairs.data(), mpairs.size() * sizeof(zgm::Pair), hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  for (size_t q = 0; q < tab_of.size(); q++) {
    zgpu_seek_index::Ent& e = x->ents[tab_of[q]];
    if (e.info.status || e.info.kind != ZGPU_INDEX_SEEK_TABLE) continue;
    e.info.compressed = closing[q].c; e.info.plaintext = closing[q].d;
  }
  // declared kind: the rows pass over the entries the summary pass accepted
  std::vector<zgx::Lane> lanes;
  std::vector<uint32_t> lane_of;
  for (size_t q = 0; q < ch_of.size(); q++) {
    const zgpu_seek_index::Ent& e = x->ents[ch_of[q]];
    if (e.info.status || e.info.kind != ZGPU_INDEX_DECLARED) continue;
    lane_of.push_back(ch_of[q]);
    lanes.push_back(zgx::Lane{chain[q].src, chain[q].len, e.pre, e.info.nrows});
  }
  std::vector<zgx::Rows> rows(lanes.size());
  if ((st = eng->seekidx_rows_pass(lanes.data(), (uint32_t)lanes.size(), dp, rows.data(), stats))) return st;
  for (size_t q = 0; q < lane_of.size(); q++) {
    zgpu_seek_index::Ent& e = x->ents[lane_of[q]];
    // (a source that changed between the passes — the caller's promise broken —, or pairs that do not add up to the entry)
    if (rows[q].why || rows[q].nrows != e.info.nrows || rows[q].c != e.info.len) {
      eng->last_error = who + ": a source changed while it was indexed";
      return ZGPU_E_INTERNAL;
    }
    e.info.compressed = rows[q].c; e.info.plaintext = rows[q].d;
  }
  for (const zgpu_seek_index::Ent& e : x->ents) if (!e.info.status) stats[kSeekIdxStatRows] += e.info.nrows;
  return ZGPU_OK;
}

// Both indexed calls up to the records. Every range is looked at on its own, as seek_many looks at it (check_entry_ranges), with what the
// index alone knows of an entry: one it refused is not refused again — its ranges pass untouched and get its status and why —; srcs != nullptr
// (the gather call): lens[i] must be the length the entry was indexed at; table_flag: ZGPU_DEVICE_VERIFY_SEEK_TABLE refuses the ranges of
// declared- and measured-kind entries whose handle holds no sums. Then ONE find launch over the handle's pairs.
int indexed_ranges(zgpu_ctx* c, const zgpu_seek_index* x, const void* const* srcs, const size_t* lens, const zgpu_entry_range* ranges, uint32_t m,
                   void* const* dsts, const size_t* caps, bool table_flag, std::vector<zgk::Seek>* out, std::vector<uint8_t>* refused) {
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  const uint32_t n = (uint32_t)x->ents.size();
  out->assign(m, zgk::Seek{});
  std::vector<uint8_t> is_live;
  check_entry_ranges(c, srcs, lens, n, ranges, m, dsts, caps, [&](uint32_t i) {
    const zgpu_seek_index_info& info = x->ents[i].info;
    if (info.status) return kPass;   // (the record is the entry's status and why: written below, nothing of the entry is looked at)
    // (the flag: an entry whose handle holds sums is vouched for by the handle, whatever its kind; else only a table can be enforced)
    return (srcs && (uint64_t)lens[i] != info.len) || (table_flag && info.kind != ZGPU_INDEX_SEEK_TABLE && !x->ents[i].sums.state) ? kRefuse : kCheck;
  }, refused, &is_live, nullptr);
  std::vector<zgm::Find> lanes(m);
  for (uint32_t j = 0; j < m; j++) {
    const zgpu_seek_index::Ent* e = is_live[j] ? &x->ents[ranges[j].entry] : nullptr;
    lanes[j] = e ? zgm::Find{ranges[j].begin, ranges[j].len, e->pre, e->tab, e->info.nrows, 0, 0, 0} : zgm::Find{ranges[j].begin, 0, 0, 0, 0, 0, 0, 0};
  }
  Engine::ManyStats more;
  int st = drain(c, c->eng->seekmany_find(lanes.data(), m, x->pairs.as<zgm::Pair>(), out->data(), nullptr, &more));
  c->ranges_many_stats[kManyStatFindLaunches] = more.find_launches; c->ranges_many_stats[kManyStatFindUs] = more.find_us;
  if (st) return st;
  // (every record is held against the length its entry was indexed at before anything is gathered)
  if ((st = accept_records(c, out, *refused, [&](uint32_t j) { return x->ents[ranges[j].entry].info.len; }, (uint32_t)ZGPU_E_SEEK_TABLE,
                           "zgpu_frames_seek_indexed_device: a record that leaves its entry")))
    return st;
  for (uint32_t j = 0; j < m; j++) {   // the ranges of entries the index refused (their lanes had length 0: records of zeros so far)
    if ((*refused)[j] || !ranges[j].len) continue;
    const zgpu_seek_index_info& info = x->ents[ranges[j].entry].info;
    if (info.status) { zgk::Seek& s = (*out)[j]; s = zgk::Seek{}; s.status = info.status; s.why = info.why; }
  }
  return ZGPU_OK;
}
}  // namespace

extern "C" int zgpu_seek_index_create_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, uint32_t kind,
                                             zgpu_seek_index** out) {
  if (out) *out = nullptr;
  if (!c || !out || kind > ZGPU_INDEX_AUTO || (n && (!device_srcs || !lens))) return ZGPU_E_BAD_ARG;
  zgpu_seek_index* x = new zgpu_seek_index();
  x->ctx = c;
  const int st = drain(c, build_index(c, x, device_srcs, lens, n, kind, kNoMeasure));
  if (st) { zgpu_seek_index_destroy(x); return st; }   // (nothing is left behind)
  *out = x;
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_measure_device(zgpu_ctx* c, const void* const* device_srcs, const size_t* lens, uint32_t n, uint32_t mode,
                                              zgpu_seek_index** out) {
  if (out) *out = nullptr;
  if (!c || !out || mode > ZGPU_MEASURE_UNSIZED || (n && (!device_srcs || !lens))) return ZGPU_E_BAD_ARG;
  zgpu_seek_index* x = new zgpu_seek_index();
  x->ctx = c;
  const int st = drain(c, build_index(c, x, device_srcs, lens, n, ZGPU_INDEX_AUTO, (int)mode));
  if (st) { zgpu_seek_index_destroy(x); return st; }   // (nothing is left behind)
  *out = x;
  return ZGPU_OK;
}
// The entry's 16 * (nrows + 1) bytes of pairs come down, and zg_seektab.h's serialiser writes them out: one definition of the layout.
// ZGPU_EXPORT_CHECKSUMS: the entry's sums come down too (4 bytes a row) and the sibling serialiser writes rows of 12 bytes.
extern "C" int zgpu_seek_index_export_seek_table(const zgpu_seek_index* x, uint32_t entry, uint8_t* host_dst, size_t cap, size_t* written) {
  return zgpu_seek_index_export_seek_table_ex(x, entry, 0, host_dst, cap, written);
}
extern "C" int zgpu_seek_index_export_seek_table_ex(const zgpu_seek_index* x, uint32_t entry, uint32_t flags, uint8_t* host_dst, size_t cap, size_t* written) {
  if (written) *written = 0;
  if (!x || !written || entry >= x->ents.size() || x->ents[entry].info.status || (!host_dst && cap) || (flags & ~ZGPU_EXPORT_CHECKSUMS)) return ZGPU_E_BAD_ARG;
  const zgpu_seek_index::Ent& e = x->ents[entry];
  const bool with_sums = (flags & ZGPU_EXPORT_CHECKSUMS) != 0;
  if (with_sums && !e.sums.state) return ZGPU_E_BAD_ARG;
  const uint64_t need = with_sums ? zgt::seek_table_sums_bytes(e.info.nrows) : zgt::seek_table_bytes(e.info.nrows);
  if (need > cap) { *written = (size_t)need; return ZGPU_E_TARGET_TOO_SMALL; }
  if (!x->ctx || hipSetDevice(x->ctx->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  std::vector<zgm::Pair> pairs((size_t)e.info.nrows + 1);
  if (hipMemcpy(pairs.data(), x->pairs.as<zgm::Pair>() + e.pre, pairs.size() * sizeof(zgm::Pair), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  static_assert(sizeof(zgm::Pair) == 16, "pairs as words");
  std::vector<uint32_t> sums(with_sums ? e.info.nrows : 0);
  if (!sums.empty() && hipMemcpy(sums.data(), x->sums.as<uint32_t>() + e.spre, sums.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  if (with_sums ? zgt::write_seek_table_sums((const uint64_t*)pairs.data(), sums.data(), e.info.nrows, host_dst)
                : zgt::write_seek_table((const uint64_t*)pairs.data(), e.info.nrows, host_dst))
    return ZGPU_E_SEEK_TABLE;
  *written = (size_t)need;
  return ZGPU_OK;
}
// ---- sums in the handle (include/zgpu.h: seek index checksums; zg_idxsums.h) ---------------------------------------------------------------------
static_assert(sizeof(zgpu_seek_index_sums) == 32 && offsetof(zgpu_seek_index_sums, frames) == 16 && ZGPU_EXPORT_CHECKSUMS == 1u, "include/zgpu.h");
namespace {
constexpr uint64_t kHashRunBytes = 64ull << 20;   // run_bytes == 0

// the handle's array of sums, allocated (zeros: what a skippable row holds) when the first entry gets sums. The zeros go out on the stream
// that the caller writes the sums on next, so that they are in front of them by stream order (the engine's streams do not wait for the
// null stream); s == nullptr: the null stream, for a caller whose next write is a null-stream hipMemcpy.
int ensure_sums(zgpu_seek_index* x, hipStream_t s) {
  if (x->sums.p) return ZGPU_OK;
  if (x->nsums > SIZE_MAX / 4) return ZGPU_E_NOMEM;
  const size_t bytes = (size_t)(x->nsums ? x->nsums : 1) * 4;
  const int st = x->sums.reserve(bytes);
  if (st) return st;
  if ((s ? hipMemsetAsync(x->sums.p, 0, bytes, s) : hipMemset(x->sums.p, 0, bytes)) != hipSuccess) { (void)hipGetLastError(); x->sums.release(); return ZGPU_E_HIP; }
  x->sums_stats[kSumStatSumsBytes] = x->nsums * 4;
  return ZGPU_OK;
}

// What the passes over a handle's entries share (zgpu_seek_index_hash_device, zgpu_seek_index_records_device): the argument rules — which
// chooses; an entry the index refused is passed over; a chosen entry must pass the pointer check at the length it was indexed at (refused[i]) —,
// the entry's pairs brought down, and its rows cut into runs: rows [k0, k1) of entry i, one selection each with an empty span of clips,
// decoded under the promise D[k1] - D[k0]. A run closes in front of a zstd row when it already holds one and its plaintext, with that row,
// would exceed run_bytes (0: 64 MiB); skippable rows join the run in progress.
struct Run { uint32_t i, k0, k1; };
struct RunPlan {
  const uint8_t* which = nullptr;
  std::vector<uint8_t> refused;
  std::vector<Run> runs;
  std::vector<Selection> sel;
  std::vector<std::vector<zgm::Pair>> pairs;   // of the entries that have runs (empty: not chosen, refused by the index or by the check)
  bool chosen(uint32_t i) const { return !which || which[i]; }
};
int cut_runs(zgpu_ctx* c, const zgpu_seek_index* x, const void* const* srcs, const size_t* lens, uint32_t n, const uint8_t* which, uint64_t run_bytes,
             RunPlan* rp) {
  const uint64_t limit = run_bytes ? run_bytes : kHashRunBytes;
  rp->which = which;
  std::vector<Engine::DevEntry> dev;
  std::vector<uint8_t>& refused = rp->refused;
  check_entries(c, srcs, lens, nullptr, nullptr, n, [&](uint32_t i) {
    const zgpu_seek_index_info& info = x->ents[i].info;
    return !rp->chosen(i) || info.status ? kPass : (uint64_t)lens[i] != info.len ? kRefuse : kCheck;
  }, &dev, &refused);
  std::vector<Run>& runs = rp->runs;
  std::vector<Selection>& sel = rp->sel;
  rp->pairs.assign(n, std::vector<zgm::Pair>());
  for (uint32_t i = 0; i < n; i++) {
    const zgpu_seek_index::Ent& e = x->ents[i];
    if (!rp->chosen(i) || e.info.status || refused[i]) continue;
    std::vector<zgm::Pair>& p = rp->pairs[i];
    try { p.resize((size_t)e.info.nrows + 1); } catch (...) { return ZGPU_E_NOMEM; }
    if (hipMemcpy(p.data(), x->pairs.as<zgm::Pair>() + e.pre, p.size() * sizeof(zgm::Pair), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
    uint32_t k0 = 0;
    bool any = false;   // the run in progress holds a zstd row
    auto close = [&](uint32_t k1) {
      if (k1 > k0) {
        runs.push_back(Run{i, k0, k1});
        // (a handle whose pairs do not describe the entry — never: build_index accepted them — is held against the entry's length like any record)
        const bool bad = p[k0].c > p[k1].c || p[k1].c > e.info.len || p[k0].d > p[k1].d;
        sel.push_back(Selection{i, bad ? 0 : p[k0].c, bad ? 0 : p[k1].c, bad ? UINT64_MAX : p[k1].d - p[k0].d, k0, k1 - k0, (uint8_t)(bad ? 1 : 0)});
      }
      k0 = k1; any = false;
    };
    for (uint32_t k = 0; k < e.info.nrows; k++) {
      const bool zstd = p[k + 1].d > p[k].d;
      if (zstd && any && p[k + 1].d - p[k0].d > limit) close(k);
      any = any || zstd;
    }
    close(e.info.nrows);
  }
  return ZGPU_OK;
}
// the runs decoded as the gather calls decode their groups, whatever the sink does beside: dres[r] is run r's result
int decode_runs(zgpu_ctx* c, DeviceSink& sink, const void* const* srcs, const size_t* lens, const RunPlan& rp, std::vector<zgpu_device_entry_result>* dres) {
  reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc | kOwnsRanges);
  std::vector<Clip> no_clips;
  std::vector<uint32_t> first(rp.sel.size() + 1, 0);
  dres->assign(rp.sel.size(), zgpu_device_entry_result{});
  return rp.sel.empty() ? ZGPU_OK : decode_selections(c, sink, srcs, lens, rp.sel, no_clips, first, true, nullptr, dres->data());
}
// what zgpu_last_error says of the first failing run of a pass
std::string run_failure(const char* call, const Run& run, uint32_t status) {
  return std::string(call) + ": entry " + std::to_string(run.i) + ", run of rows [" + std::to_string(run.k0) + ", " + std::to_string(run.k1) + "): " +
         zgpu_status_name((int)status);
}

// The pass. Nothing of the handle changes before every run of every chosen entry has its verdict: an engine failure leaves it as it was.
int hash_entries(zgpu_ctx* c, zgpu_seek_index* x, const void* const* srcs, const size_t* lens, uint32_t n, const uint8_t* which, uint64_t run_bytes) {
  zg::Engine* eng = c->eng;
  if (hipSetDevice(eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  RunPlan rp;
  int st = cut_runs(c, x, srcs, lens, n, which, run_bytes, &rp);
  if (st) return st;
  auto chosen = [&](uint32_t i) { return rp.chosen(i); };
  const std::vector<uint8_t>& refused = rp.refused;
  const std::vector<Run>& runs = rp.runs;
  const std::vector<std::vector<zgm::Pair>>& pairs = rp.pairs;
  // decoded as the gather calls decode their groups; the sink hashes every frame and hands the digests back
  zgpu_device_opts opts{0, ZGPU_DEVICE_VERIFY, 0};
  DeviceSink sink = device_sink(c, &opts, nullptr, &st, false);
  if (st) return st;
  sink.hash_every = true;
  std::vector<std::vector<DeviceSink::Digest>> got;
  sink.collect = &got;
  std::vector<zgpu_device_entry_result> dres;
  if ((st = decode_runs(c, sink, srcs, lens, rp, &dres))) return st;
  // every run's frames to rows; the first failing run of an entry, in row order, is its verdict
  std::vector<std::vector<uint32_t>> sums(n);
  std::vector<zgpu_seek_index_sums> rec(n, zgpu_seek_index_sums{0, 0, 0, 0, 0, 0});
  for (uint32_t i = 0; i < n; i++) if (!pairs[i].empty()) sums[i].assign(x->ents[i].info.nrows, 0);
  std::string named;
  for (size_t r = 0; r < runs.size(); r++) {
    const Run& run = runs[r];
    zgpu_seek_index_sums& o = rec[run.i];
    if (o.status) continue;
    const std::vector<zgm::Pair>& p = pairs[run.i];
    uint32_t status = (uint32_t)dres[r].r.status;
    size_t q = 0;
    for (uint32_t k = run.k0; k < run.k1 && !status; k++) {
      if (q == got[r].size()) break;
      const DeviceSink::Digest& f = got[r][q];
      if (f.begin != p[k].c - p[run.k0].c || f.clen != p[k + 1].c - p[k].c) continue;   // (a skippable row: no frame coincides with it)
      sums[run.i][k] = (uint32_t)f.digest;
      q++;
    }
    if (!status && q != got[r].size()) status = ZGPU_E_CONTENT_SIZE_MISMATCH;   // (a decoded frame that coincides with no row)
    if (status) {
      o = zgpu_seek_index_sums{status, 0, run.k0, run.k1, 0, 0};
      if (named.empty()) named = run_failure("zgpu_seek_index_hash_device", run, status);
      continue;
    }
    o.frames += got[r].size(); o.bytes += p[run.k1].d - p[run.k0].d;
  }
  // the handle: one copy per stretch of chosen entries whose sums lie back to back
  hipStream_t s = eng->stream();
  if ((st = ensure_sums(x, s))) return st;
  std::vector<uint32_t> stage;
  uint64_t at = 0;      // the index of stage[0] in the handle's array
  std::vector<std::vector<uint32_t>> keep;   // (the staging of the stretches sent so far: alive until the stream is drained)
  auto flush = [&]() -> int {
    if (stage.empty()) return ZGPU_OK;
    keep.push_back(std::move(stage));
    stage.clear();
    if (hipMemcpyAsync(x->sums.as<uint32_t>() + at, keep.back().data(), keep.back().size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
    return ZGPU_OK;
  };
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < n; i++) if (!pairs[i].empty()) order.push_back(i);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return x->ents[a].spre < x->ents[b].spre; });
  for (uint32_t i : order) {
    const zgpu_seek_index::Ent& e = x->ents[i];
    if (!stage.empty() && at + stage.size() != e.spre && (st = flush())) return st;
    if (stage.empty()) at = e.spre;
    if (rec[i].status) sums[i].assign(e.info.nrows, 0);   // (dropped)
    stage.insert(stage.end(), sums[i].begin(), sums[i].end());
  }
  if ((st = flush())) return st;
  if (hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  for (uint32_t i = 0; i < n; i++) {
    zgpu_seek_index::Ent& e = x->ents[i];
    if (!chosen(i)) continue;
    if (e.info.status) { e.sums = zgpu_seek_index_sums{e.info.status, 0, 0, 0, 0, 0}; continue; }
    if (refused[i]) { e.sums.status = ZGPU_E_BAD_ARG; continue; }   // (nothing of it was looked at: what it holds stays)
    e.sums = rec[i];
    if (!rec[i].status) { e.sums.state = 1; x->sums_stats[kSumStatFramesHashed] += rec[i].frames; }
  }
  x->sums_stats[kSumStatHashSubmits] += c->frames_submits; x->sums_stats[kSumStatHashUs] += c->frames_device_stats[kDevStatHashUs];
  x->sums_stats[kSumStatHashRuns] += runs.size();
  if (!named.empty()) eng->last_error = named;
  return ZGPU_OK;
}
}  // namespace

extern "C" int zgpu_seek_index_hash_device(zgpu_ctx* c, zgpu_seek_index* x, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                           const uint8_t* which_or_null, uint64_t run_bytes) {
  if (!c || !x || x->ctx != c || n != x->ents.size() || (n && (!device_srcs || !lens))) return ZGPU_E_BAD_ARG;
  return drain(c, hash_entries(c, x, device_srcs, lens, n, which_or_null, run_bytes));
}
extern "C" int zgpu_seek_index_set_sums(zgpu_seek_index* x, uint32_t entry, const uint32_t* sums, uint32_t nrows) {
  if (!x || entry >= x->ents.size() || x->ents[entry].info.status || nrows != x->ents[entry].info.nrows || (nrows && !sums)) return ZGPU_E_BAD_ARG;
  if (!x->ctx || hipSetDevice(x->ctx->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  int st = ensure_sums(x, nullptr);
  if (st) return st;
  zgpu_seek_index::Ent& e = x->ents[entry];
  if (nrows && hipMemcpy(x->sums.as<uint32_t>() + e.spre, sums, (size_t)nrows * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  e.sums = zgpu_seek_index_sums{0, 2, 0, 0, 0, 0};
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_read_sums(const zgpu_seek_index* x, uint32_t entry, uint32_t* dst, uint32_t cap_rows, uint32_t* nrows) {
  if (nrows) *nrows = 0;
  if (!x || !nrows || entry >= x->ents.size() || x->ents[entry].info.status || !x->ents[entry].sums.state || (!dst && cap_rows)) return ZGPU_E_BAD_ARG;
  const zgpu_seek_index::Ent& e = x->ents[entry];
  *nrows = e.info.nrows;
  if (cap_rows < e.info.nrows) return ZGPU_E_TARGET_TOO_SMALL;
  if (!x->ctx || hipSetDevice(x->ctx->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  if (e.info.nrows && hipMemcpy(dst, x->sums.as<uint32_t>() + e.spre, (size_t)e.info.nrows * 4, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_sums_of(const zgpu_seek_index* x, uint32_t i, zgpu_seek_index_sums* out) {
  if (!x || !out || i >= x->ents.size()) return ZGPU_E_BAD_ARG;
  *out = x->ents[i].sums;
  return ZGPU_OK;
}
// ---- record offsets in the handle (include/zgpu.h: record index; zg_records.h) ---------------------------------------------------------------------
static_assert(sizeof(zgpu_seek_index_records) == 32 && offsetof(zgpu_seek_index_records, nrecords) == 16 && offsetof(zgpu_seek_index_records, row_lo) == 24 &&
              sizeof(zgpu_record_range) == 24 && offsetof(zgpu_record_range, entry) == 16 && ZGPU_RECORDS_STRIP == zgr::kStrip, "include/zgpu.h");
namespace {
// One stretch of an entry's offsets on its way into the handle's array: n 64-bit words at p, device or host memory.
struct Piece { const uint64_t* p; uint64_t n; bool host; };
// The handle's array laid out anew: entry i gets the pieces news[i] and the record rec[i] if fresh[i]; any other entry keeps what it holds
// (state 0: nothing). A new array is allocated, filled in entry order — device-to-device copies but for what the host holds — on the engine's
// first stream, which is drained before the old array goes; on a failure the handle is as it was. The host pieces must outlive the call.
int relay_records(zgpu_seek_index* x, const std::vector<uint8_t>& fresh, const std::vector<std::vector<Piece>>& news, const std::vector<zgpu_seek_index_records>& rec) {
  const uint32_t n = (uint32_t)x->ents.size();
  std::vector<uint64_t> rpre(n, 0);
  uint64_t slots = 0, held = 0;
  for (uint32_t i = 0; i < n; i++) {
    const zgpu_seek_index_records& r = fresh[i] ? rec[i] : x->ents[i].recs;
    if (!r.state) continue;
    rpre[i] = slots;
    slots += r.nrecords + 1;
    held += r.nrecords;
  }
  if (slots > SIZE_MAX / 8) return ZGPU_E_NOMEM;
  zg::DevBuf nb;
  int st = nb.reserve((size_t)(slots ? slots : 1) * 8);
  if (st) return st;
  hipStream_t s = x->ctx->eng->stream();
  bool ok = true;
  for (uint32_t i = 0; i < n && ok; i++) {
    uint64_t* to = nb.as<uint64_t>() + rpre[i];
    if (!fresh[i]) {
      const zgpu_seek_index::Ent& e = x->ents[i];
      if (e.recs.state) ok = hipMemcpyAsync(to, x->recs.as<uint64_t>() + e.rpre, (size_t)(e.recs.nrecords + 1) * 8, hipMemcpyDeviceToDevice, s) == hipSuccess;
      continue;
    }
    if (!rec[i].state) continue;
    uint64_t at = 0;
    for (const Piece& pc : news[i]) {
      if (!pc.n) continue;
      if (at + pc.n > rec[i].nrecords + 1) { nb.release(); return ZGPU_E_INTERNAL; }   // (never)
      ok = ok && hipMemcpyAsync(to + at, pc.p, (size_t)pc.n * 8, pc.host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s) == hipSuccess;
      at += pc.n;
    }
    if (at != rec[i].nrecords + 1) { (void)hipStreamSynchronize(s); nb.release(); return ZGPU_E_INTERNAL; }   // (never)
  }
  if (!ok || hipStreamSynchronize(s) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(s); nb.release(); return ZGPU_E_HIP; }
  x->recs.release();
  x->recs = nb;
  x->nrec_slots = slots;
  for (uint32_t i = 0; i < n; i++) x->ents[i].rpre = rpre[i];
  x->rec_stats[kRecStatRecordsHeld] = held; x->rec_stats[kRecStatOffsetBytes] = slots * 8;
  return ZGPU_OK;
}

// The pass: hash_entries' runs behind another sink. Nothing of the handle changes before every run of every chosen entry has its verdict.
int records_entries(zgpu_ctx* c, zgpu_seek_index* x, const void* const* srcs, const size_t* lens, uint32_t n, const uint8_t* which, uint32_t delimiter,
                    uint64_t run_bytes) {
  zg::Engine* eng = c->eng;
  if (hipSetDevice(eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  RunPlan rp;
  int st = cut_runs(c, x, srcs, lens, n, which, run_bytes, &rp);
  if (st) return st;
  const std::vector<Run>& runs = rp.runs;
  // decoded as the gather calls decode their groups; no frame is hashed, and the sink finds the delimiters of what stands at status 0
  zgpu_device_opts opts{0, ZGPU_DEVICE_NO_HASH, 0};
  DeviceSink sink = device_sink(c, &opts, nullptr, &st, false);
  if (st) return st;
  DeviceSink::Records rc;
  rc.delimiter = delimiter;
  for (const Run& run : runs) rc.base.push_back(rp.pairs[run.i][run.k0].d);
  sink.records = &rc;
  std::vector<zgpu_device_entry_result> dres;
  if ((st = decode_runs(c, sink, srcs, lens, rp, &dres))) return st;
  // the first failing run of an entry, in row order, is its verdict; else its runs' offsets follow each other in row order
  std::vector<zgpu_seek_index_records> rec(n, zgpu_seek_index_records{0, 0, delimiter, 0, 0, 0, 0});
  std::vector<std::vector<Piece>> news(n);
  std::vector<uint8_t> fresh(n, 0);
  std::vector<uint64_t> consts;   // O[0] and O[R] = L of every entry: host words the copies read until the stream is drained
  consts.reserve(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    if (rp.pairs[i].empty()) continue;
    fresh[i] = 1;
    consts.push_back(0);
    news[i].push_back(Piece{&consts.back(), 1, true});
  }
  std::string named;
  uint64_t back = 0;
  for (size_t r = 0; r < runs.size(); r++) {
    const Run& run = runs[r];
    zgpu_seek_index_records& o = rec[run.i];
    if (o.status) continue;
    const uint32_t status = (uint32_t)dres[r].r.status;
    if (status) {
      o = zgpu_seek_index_records{status, 0, delimiter, 0, 0, run.k0, run.k1};
      if (named.empty()) named = run_failure("zgpu_seek_index_records_device", run, status);
      continue;
    }
    const DeviceSink::Records::Run& found = rc.run[r];
    if (!found.n) continue;
    if (found.buf < 0) news[run.i].push_back(Piece{rc.host[r].data(), found.n, true});
    else news[run.i].push_back(Piece{rc.staging[(size_t)found.buf].as<uint64_t>() + found.at, found.n, false});
    o.nrecords += found.n;
  }
  for (uint32_t i = 0; i < n; i++) {
    if (!fresh[i] || rec[i].status) continue;
    zgpu_seek_index_records& o = rec[i];
    const uint64_t L = x->ents[i].info.plaintext;
    uint64_t last = 0;   // the last offset found (O[0] where there is none)
    if (o.nrecords) {
      const Piece& pc = news[i].back();
      if (pc.host) last = pc.p[pc.n - 1];
      else {
        if (hipMemcpy(&last, pc.p + (pc.n - 1), 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
        back += 8;
      }
    }
    if (last > L) { eng->last_error = "zgpu_seek_index_records_device: an offset behind the entry's plaintext"; return ZGPU_E_INTERNAL; }   // (never: the runs kept their promise)
    if (last != L) {   // the open tail: O[R] = L
      consts.push_back(L);
      news[i].push_back(Piece{&consts.back(), 1, true});
      o.nrecords++;
      o.flags = 1;
    }
    o.state = 1;
  }
  if ((st = relay_records(x, fresh, news, rec))) return st;
  for (uint32_t i = 0; i < n; i++) {
    zgpu_seek_index::Ent& e = x->ents[i];
    if (!rp.chosen(i)) continue;
    if (e.info.status) { e.recs = zgpu_seek_index_records{e.info.status, 0, delimiter, 0, 0, 0, 0}; continue; }
    if (rp.refused[i]) { e.recs.status = ZGPU_E_BAD_ARG; continue; }   // (nothing of it was looked at: what it holds stays)
    e.recs = rec[i];
    if (rec[i].status) e.recs.nrecords = 0;
  }
  x->rec_stats[kRecStatSubmits] += c->frames_submits; x->rec_stats[kRecStatUs] += rc.us; x->rec_stats[kRecStatChunks] += rc.chunks;
  x->rec_stats[kRecStatBytesDownloaded] += rc.bytes_back + back;
  if (!named.empty()) eng->last_error = named;
  return ZGPU_OK;
}

// Both record calls up to the answers: every range's status decided on the host, then ONE zg_k_recs_find launch over the handle's offsets.
int lookup_records(zgpu_ctx* c, const zgpu_seek_index* x, const zgpu_record_range* recs, uint32_t m, std::vector<zgr::Found>* out, uint64_t* stats) {
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  const uint32_t n = (uint32_t)x->ents.size();
  std::vector<zgr::Find> lanes(m);
  for (uint32_t j = 0; j < m; j++) {
    const zgpu_record_range& g = recs[j];
    zgr::Find f{g.first, g.count, 0, 0, g.flags, 0, g.entry, 0};
    if (g.entry >= n || (g.flags & ~ZGPU_RECORDS_STRIP)) f.status = ZGPU_E_BAD_ARG;
    else {
      const zgpu_seek_index::Ent& e = x->ents[g.entry];
      if (e.info.status) f.status = e.info.status;
      else if (!e.recs.state) f.status = ZGPU_E_BAD_ARG;
      else {
        if (!x->recs.p || e.rpre > x->nrec_slots || e.recs.nrecords + 1 > x->nrec_slots - e.rpre) {   // (never: relay_records laid them out)
          c->eng->last_error = "zgpu_seek_index_record_ranges_device: an entry's offsets leave the handle's array";
          return ZGPU_E_INTERNAL;
        }
        f.rpre = e.rpre; f.nrec = e.recs.nrecords;
        f.flags = (g.flags & zgr::kStrip) | ((e.recs.flags & 1u) ? zgr::kOpenTail : 0u);
      }
    }
    lanes[j] = f;
  }
  out->assign(m, zgr::Found{0, 0, 0, 0});
  uint64_t pass[3] = {0, 0, 0};
  const int st = drain(c, c->eng->records_find(lanes.data(), m, x->recs.as<uint64_t>(), out->data(), pass));
  stats[kRecFindStatLaunches] = pass[kPassLaunches]; stats[kRecFindStatUs] = pass[kPassUs]; stats[kRecFindStatBytesDownloaded] = pass[kPassBytes];
  if (st) return st;
  for (uint32_t j = 0; j < m; j++) {   // (every answer is held against its entry's plaintext before anything is gathered)
    const zgr::Found& f = (*out)[j];
    if (f.status != lanes[j].status || f.entry != lanes[j].entry ||
        (!f.status && (f.begin > x->ents[f.entry].info.plaintext || f.len > x->ents[f.entry].info.plaintext - f.begin))) {
      c->eng->last_error = "zgpu_seek_index_record_ranges_device: an answer that leaves its entry";
      return ZGPU_E_INTERNAL;
    }
  }
  return ZGPU_OK;
}
}  // namespace

extern "C" int zgpu_seek_index_records_device(zgpu_ctx* c, zgpu_seek_index* x, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                              const uint8_t* which_or_null, uint32_t delimiter, uint64_t run_bytes) {
  if (!c || !x || x->ctx != c || n != x->ents.size() || (n && (!device_srcs || !lens)) || delimiter > 255u) return ZGPU_E_BAD_ARG;
  return drain(c, records_entries(c, x, device_srcs, lens, n, which_or_null, delimiter, run_bytes));
}
extern "C" int zgpu_seek_index_records_of(const zgpu_seek_index* x, uint32_t i, zgpu_seek_index_records* out) {
  if (!x || !out || i >= x->ents.size()) return ZGPU_E_BAD_ARG;
  *out = x->ents[i].recs;
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_read_records(const zgpu_seek_index* x, uint32_t entry, uint64_t first, uint64_t* host_dst, uint64_t cap, uint64_t* n) {
  if (n) *n = 0;
  if (!x || !n || entry >= x->ents.size() || x->ents[entry].info.status || !x->ents[entry].recs.state || (!host_dst && cap)) return ZGPU_E_BAD_ARG;
  const zgpu_seek_index::Ent& e = x->ents[entry];
  const uint64_t have = e.recs.nrecords + 1;
  if (!host_dst) { *n = have; return ZGPU_OK; }
  const uint64_t take = first >= have ? 0 : cap < have - first ? cap : have - first;
  if (!x->ctx || hipSetDevice(x->ctx->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  if (take && hipMemcpy(host_dst, x->recs.as<uint64_t>() + e.rpre + first, (size_t)take * 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  *n = take;
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_set_records(zgpu_seek_index* x, uint32_t entry, const uint64_t* offsets, uint64_t nrecords, uint32_t delimiter) {
  const uint32_t d = delimiter & ~ZGPU_RECORDS_OPEN_TAIL;
  const bool open = (delimiter & ZGPU_RECORDS_OPEN_TAIL) != 0;
  if (!x || entry >= x->ents.size() || x->ents[entry].info.status || !offsets || d > 255u || nrecords == UINT64_MAX || (open && !nrecords)) return ZGPU_E_BAD_ARG;
  if (offsets[0] != 0 || offsets[nrecords] != x->ents[entry].info.plaintext) return ZGPU_E_BAD_ARG;
  for (uint64_t r = 0; r < nrecords; r++) if (offsets[r] >= offsets[r + 1]) return ZGPU_E_BAD_ARG;
  if (!x->ctx || hipSetDevice(x->ctx->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  const uint32_t n = (uint32_t)x->ents.size();
  std::vector<uint8_t> fresh(n, 0);
  std::vector<std::vector<Piece>> news(n);
  std::vector<zgpu_seek_index_records> rec(n, zgpu_seek_index_records{0, 0, 0, 0, 0, 0, 0});
  fresh[entry] = 1;
  news[entry].push_back(Piece{offsets, nrecords + 1, true});
  rec[entry] = zgpu_seek_index_records{0, 2, d, open ? 1u : 0u, nrecords, 0, 0};
  const int st = relay_records(x, fresh, news, rec);
  if (!st) x->ents[entry].recs = rec[entry];
  return st;
}
extern "C" int zgpu_seek_index_record_ranges_device(zgpu_ctx* c, const zgpu_seek_index* x, const zgpu_record_range* recs, uint32_t m,
                                                    zgpu_entry_range* out, uint32_t* status) {
  if (!c || !x || x->ctx != c || (m && (!recs || !out || !status))) return ZGPU_E_BAD_ARG;
  reset_stats(c, kOwnsRanges);
  std::vector<zgr::Found> found;
  const int st = lookup_records(c, x, recs, m, &found, c->ranges_rec_stats);
  for (uint32_t j = 0; j < m; j++) {
    const bool ok = !st && !found[j].status;
    out[j] = zgpu_entry_range{ok ? found[j].begin : 0, ok ? found[j].len : 0, recs[j].entry, 0};
    status[j] = st ? 0u : found[j].status;
  }
  return st;
}
// The lookup, then the indexed gather on the byte ranges: a range whose lookup failed travels as a range of length 0 — the gather passes it
// untouched — and gets the lookup's status afterwards.
extern "C" int zgpu_gather_records_indexed_device_src(zgpu_ctx* c, const zgpu_seek_index* x, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                      const zgpu_record_range* recs, uint32_t m, void* const* device_dsts, const size_t* caps,
                                                      const zgpu_device_opts* opts, zgpu_range_result* results) {
  if (!c || !x || x->ctx != c || n != x->ents.size() || (n && (!device_srcs || !lens)) || (m && (!recs || !device_dsts || !caps || !results)))
    return ZGPU_E_BAD_ARG;
  for (uint32_t j = 0; j < m; j++) memset(&results[j], 0, sizeof results[j]);
  std::vector<zgr::Found> found;
  uint64_t find_stats[kRecFindStatCount] = {};
  int st = lookup_records(c, x, recs, m, &found, find_stats);
  if (st) return st;
  std::vector<zgpu_entry_range> ranges(m);
  for (uint32_t j = 0; j < m; j++)
    ranges[j] = found[j].status ? zgpu_entry_range{0, 0, 0, 0} : zgpu_entry_range{found[j].begin, found[j].len, found[j].entry, 0};
  st = zgpu_gather_ranges_indexed_device_src(c, x, device_srcs, lens, n, ranges.data(), m, device_dsts, caps, opts, results);
  for (uint32_t j = 0; j < m && !st; j++)
    if (found[j].status) { memset(&results[j], 0, sizeof results[j]); results[j].d.r.status = (int)found[j].status; }
  memcpy(c->ranges_rec_stats, find_stats, sizeof find_stats);
  return st;
}
// ---- record batches (include/zgpu.h: record batches; zg_records.h: plan_rows; zg_scatter.h: zg_k_fill) ---------------------------------------------
static_assert(sizeof(zgpu_record_batch) == 64 && offsetof(zgpu_record_batch, width) == 40 && offsetof(zgpu_record_batch, layout) == 48 &&
              sizeof(zgpu_record_batch_info) == 32 && offsetof(zgpu_record_batch_info, rows_ok) == 16 && ZGPU_BATCH_PADDED == zgr::kBatchPadded &&
              ZGPU_BATCH_PACKED == zgr::kBatchPacked, "include/zgpu.h");
// The lookup, the layout (plan_rows), the indexed gather on the byte ranges with every destination a piece of the ONE batch, then the finish:
// one zg_k_fill launch over what the gather left unwritten of every row's slot, and the two arrays from what the host holds.
extern "C" int zgpu_gather_records_batch_indexed_device_src(zgpu_ctx* c, const zgpu_seek_index* x, const void* const* device_srcs, const size_t* lens,
                                                            uint32_t n, const zgpu_record_range* recs, uint32_t m, const zgpu_record_batch* batch,
                                                            const zgpu_device_opts* opts, zgpu_range_result* results, zgpu_record_batch_info* info) {
  if (!c || !x || x->ctx != c || n != x->ents.size() || (n && (!device_srcs || !lens)) || (m && !recs) || !batch || !results || !info) return ZGPU_E_BAD_ARG;
  const zgpu_record_batch& b = *batch;
  const bool padded = b.layout == ZGPU_BATCH_PADDED, truncate = (b.flags & ZGPU_BATCH_TRUNCATE) != 0;
  if (b.layout > ZGPU_BATCH_PACKED || (b.flags & ~ZGPU_BATCH_TRUNCATE) || b.reserved || b.pad_byte > 255u || (padded && !b.width) ||
      (!padded && b.width && !truncate) || ((uintptr_t)b.device_lengths & 7) || ((uintptr_t)b.device_offsets & 7))
    return ZGPU_E_BAD_ARG;
  int st;
  (void)device_sink(c, opts, nullptr, &st, true);   // (the options the gather would refuse, refused before anything is launched)
  if (st) return st;
  if (hipSetDevice(c->eng->device()) != hipSuccess) { (void)hipGetLastError(); return ZGPU_E_HIP; }
  uint8_t* const dst = (uint8_t*)b.device_dst;
  const int device = c->eng->device();
  std::vector<DevRange> known;
  if ((b.device_lengths && m && !check_device_range(device, b.device_lengths, (size_t)m * 8, known)) ||
      (b.device_offsets && !check_device_range(device, b.device_offsets, ((size_t)m + 1) * 8, known)))
    return ZGPU_E_BAD_ARG;
  // (padded: the total is known without the lookup, and a batch that is no device memory is refused before the lookup's launch; packed: behind
  // it — the lookup reads the handle's offsets and writes nothing of the caller's)
  const auto dst_ok = [&](uint64_t total) { return !total || total > b.cap || (total <= SIZE_MAX && check_device_range(device, dst, (size_t)total, known)); };
  if (padded && (m > UINT64_MAX / b.width || !dst_ok((uint64_t)m * b.width))) return ZGPU_E_BAD_ARG;
  for (uint32_t j = 0; j < m; j++) memset(&results[j], 0, sizeof results[j]);
  std::vector<zgr::Found> found;
  uint64_t find_stats[kRecFindStatCount] = {}, batch_stats[kBatchStatCount] = {};
  if ((st = lookup_records(c, x, recs, m, &found, find_stats))) return st;
  std::vector<uint64_t> len(m);
  for (uint32_t j = 0; j < m; j++) len[j] = found[j].status ? 0 : found[j].len;
  std::vector<zgr::Row> rows(m);
  uint64_t total = 0;
  uint32_t cut = 0;
  if (!zgr::plan_rows(len.data(), m, b.layout, truncate, b.width, rows.data(), &total, &cut) || !dst_ok(total)) return ZGPU_E_BAD_ARG;
  if (b.host_record_bytes) for (uint32_t j = 0; j < m; j++) b.host_record_bytes[j] = len[j];
  *info = zgpu_record_batch_info{total, 0, 0, 0, cut, 0};
  const auto own_stats = [&]() {   // (the gather zeroed the arrays of its family: this call's lookup and finish go back in)
    memcpy(c->ranges_rec_stats, find_stats, sizeof find_stats);
    memcpy(c->ranges_batch_stats, batch_stats, sizeof batch_stats);
  };
  hipStream_t s = c->eng->stream();
  std::vector<uint64_t> lengths(m, 0), offsets((size_t)m + 1, 0);   // (host words the copies read until the stream is drained)
  if (total > b.cap) {   // the batch does not fit: the need in info->total, nothing behind the lookup is launched, no device memory is written
    reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc | kOwnsRanges);
    for (uint32_t j = 0; j < m; j++) {
      results[j].d.r.status = found[j].status ? (int)found[j].status : ZGPU_E_TARGET_TOO_SMALL;
      info->rows_failed++;
    }
    own_stats();
    return ZGPU_OK;
  }
  if (m) {
    std::vector<zgpu_entry_range> ranges(m);
    std::vector<void*> dsts(m);
    std::vector<size_t> caps(m);
    for (uint32_t j = 0; j < m; j++) {
      ranges[j] = found[j].status ? zgpu_entry_range{0, 0, 0, 0} : zgpu_entry_range{found[j].begin, rows[j].want, found[j].entry, 0};
      dsts[j] = dst + rows[j].at;
      caps[j] = (size_t)rows[j].slot;
    }
    if ((st = zgpu_gather_ranges_indexed_device_src(c, x, device_srcs, lens, n, ranges.data(), m, dsts.data(), caps.data(), opts, results))) return st;
    // the finish: what of every slot the gather did not write
    std::vector<zgs::Seg> regions(m);
    for (uint32_t j = 0; j < m; j++) {
      if (found[j].status) { memset(&results[j], 0, sizeof results[j]); results[j].d.r.status = (int)found[j].status; }
      const zgpu_entry_result& r = results[j].d.r;
      const uint64_t fin = r.status ? 0 : r.written;
      // (every region is held against the batch before the launch, as the scatter's caller holds its segments against the output)
      if (fin > rows[j].slot || rows[j].at > total || rows[j].slot > total - rows[j].at) {
        c->eng->last_error = "zgpu_gather_records_batch_indexed_device_src: a row that leaves the batch";
        return ZGPU_E_INTERNAL;
      }
      regions[j] = zgs::Seg{0, (uint64_t)(uintptr_t)dst + rows[j].at + fin, rows[j].slot - fin};
      lengths[j] = fin;
      offsets[j] = rows[j].at;
      info->bytes_filled += rows[j].slot - fin;
      if (r.status) info->rows_failed++; else info->rows_ok++;
    }
    st = c->eng->fill_pass(regions.data(), m, b.pad_byte, batch_stats);
  } else {
    reset_stats(c, kOwnsDecode | kOwnsDevice | kOwnsSrc | kOwnsRanges);
  }
  offsets[m] = total;
  if (!st && b.device_lengths && m) {
    if (hipMemcpyAsync(b.device_lengths, lengths.data(), (size_t)m * 8, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); st = ZGPU_E_HIP; }
    else batch_stats[kBatchStatBytesUploaded] += (uint64_t)m * 8;
  }
  if (!st && b.device_offsets) {
    if (hipMemcpyAsync(b.device_offsets, offsets.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) { (void)hipGetLastError(); st = ZGPU_E_HIP; }
    else batch_stats[kBatchStatBytesUploaded] += ((uint64_t)m + 1) * 8;
  }
  st = drain(c, st);
  own_stats();
  return st;
}
extern "C" void zgpu_seek_index_destroy(zgpu_seek_index* x) {
  if (!x) return;
  if (x->pairs.p && x->ctx && hipSetDevice(x->ctx->eng->device()) != hipSuccess) (void)hipGetLastError();
  x->pairs.release();
  x->sums.release();
  x->recs.release();
  delete x;
}
extern "C" uint32_t zgpu_seek_index_entries(const zgpu_seek_index* x) { return x ? (uint32_t)x->ents.size() : 0; }
extern "C" int zgpu_seek_index_info_of(const zgpu_seek_index* x, uint32_t i, zgpu_seek_index_info* out) {
  if (!x || !out || i >= x->ents.size()) return ZGPU_E_BAD_ARG;
  *out = x->ents[i].info;
  return ZGPU_OK;
}
extern "C" int zgpu_seek_index_stats(const zgpu_seek_index* x, uint64_t* out, int n) {
  if (!x) return 0;
  int k = copy_stats(x->stats, out, n);   // (the slots of the sums lie behind the others, those of the records behind them)
  if (k < (int)kSeekIdxStatCount || !out) return k;
  k += copy_stats(x->sums_stats, out + k, n - k);
  return k < (int)(kSeekIdxStatCount + kSumStatCount) ? k : k + copy_stats(x->rec_stats, out + k, n - k);
}

extern "C" int zgpu_frames_seek_indexed_device(zgpu_ctx* c, const zgpu_seek_index* x, const zgpu_entry_range* ranges, uint32_t m, zgpu_seek* out) {
  if (!c || !x || x->ctx != c || (m && (!ranges || !out))) return ZGPU_E_BAD_ARG;
  return seek_only(c, m, out, [&](auto* recs, auto* refused) { return indexed_ranges(c, x, nullptr, nullptr, ranges, m, nullptr, nullptr, false, recs, refused); });
}

extern "C" int zgpu_gather_ranges_indexed_device_src(zgpu_ctx* c, const zgpu_seek_index* x, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                     const zgpu_entry_range* ranges, uint32_t m, void* const* device_dsts, const size_t* caps,
                                                     const zgpu_device_opts* opts, zgpu_range_result* results) {
  if (!c || !x || x->ctx != c || n != x->ents.size() || (n && (!device_srcs || !lens)) || (m && (!ranges || !device_dsts || !caps || !results)))
    return ZGPU_E_BAD_ARG;
  // ZGPU_DEVICE_VERIFY_SEEK_TABLE: the entries whose handle holds sums go the handle's route (zg_idxsums.h), the others their table's
  DeviceSink::Handle hs;
  return gather_groups(c, device_srcs, lens, ranges, m, device_dsts, caps, opts, results, [&](DeviceSink& sink, auto* recs, auto* refused) {
    if (sink.table_flag && x->sums.p) {
      hs.pairs = x->pairs.p; hs.npairs = x->npairs;
      hs.sums = x->sums.as<uint32_t>(); hs.nsums = x->nsums;
      hs.ent.resize(n); hs.on.assign(n, 0);
      for (uint32_t i = 0; i < n; i++) {
        const zgpu_seek_index::Ent& e = x->ents[i];
        hs.ent[i] = DeviceSink::HandleEntry{e.pre, e.spre, e.info.nrows, 0, 0};
        hs.on[i] = !e.info.status && e.sums.state != 0;
      }
      sink.handle = &hs;
    }
    return indexed_ranges(c, x, device_srcs, lens, ranges, m, device_dsts, caps, sink.table_flag, recs, refused);
  });
}

extern "C" int zgpu_debug_ranges_stats(const zgpu_ctx* c, uint64_t* out, int n) {
  if (!c) return 0;
  int k = copy_stats(c->ranges_stats, out, n);   // (the slots of the calls with many ranges per entry lie behind the others, the record lookup's behind them)
  if (k < (int)kRangeStatCount || !out) return k;
  k += copy_stats(c->ranges_many_stats, out + k, n - k);
  if (k < (int)(kRangeStatCount + kManyStatCount)) return k;
  k += copy_stats(c->ranges_rec_stats, out + k, n - k);   // (and the finish of a record batch behind the lookup)
  return k < (int)(kRangeStatCount + kManyStatCount + kRecFindStatCount) ? k : k + copy_stats(c->ranges_batch_stats, out + k, n - k);
}
