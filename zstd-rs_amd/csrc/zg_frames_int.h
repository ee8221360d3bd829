// zg_frames_int.h — the seam between the machinery of the device-resident decode calls (zg_frames.cpp) and the front-ends that choose which
// bytes of an entry it decodes (zg_ranges.cpp): the device sink and its options, a selection and its clips with the one function that runs a
// list of them, the pointer checks, and the three helpers every call starts and ends with. Call, DeviceSources, Ranges, Submit, the sinks and
// decode_entries are zg_frames.cpp's own: a front-end that needs one of them asks too little of decode_selections. Internal (not installed).
#pragma once
#include <vector>
#include "zg_capi_int.h"
#include "zg_entry.h"

namespace zgf {

// plaintext per submit of the decode calls: bounds the device output (+ 4x its size of flatten scratch) and the pinned staging of one submit;
// their input is bounded by the same number, and so is the input of a measuring submit (zg_ranges.cpp), which produces no plaintext
constexpr uint64_t kFramesSubmitBytes = 512ull << 20;

// destinations in device memory of the caller (zgpu_decode_frames_device and every call built on it)
struct DeviceSink {
  zgpu_device_entry_result* res = nullptr;
  uint64_t hash_max = 0;          // the caller's (no estimate): frames up to this length are hashed
  bool no_hash = false;           // ZGPU_DEVICE_NO_HASH: hash no frame
  bool verify = false;            // ZGPU_DEVICE_VERIFY: a mismatch fails the entry, with nothing of it written
  bool hash_all = false;          // verify with hash_max_bytes == 0: every frame that carries a Content_Checksum is hashed
  // ZGPU_DEVICE_VERIFY_SEEK_TABLE (zg_seeksums.h): the WHOLE entries — Call::srcs are the selections — and the table rows of each selection;
  // empty: the flag is not set. An entry with taken == 0 is not looked at. table_all: hash_max_bytes == 0, every frame of such an entry is hashed
  struct TableEntry { uint64_t src, len; uint32_t first, taken; };
  std::vector<TableEntry> table_verify;
  bool table_flag = false, table_all = false;
  bool table(uint32_t i) const { return !table_verify.empty() && table_verify[i].taken != 0; }
  // The same flag on an entry whose seek index handle holds sums (zg_idxsums.h): the handle vouches, not a table. handle: set by the indexed
  // gather call before decode_selections — the handle's two arrays and, per WHOLE entry, where its rows lie in them (on: the handle holds its
  // sums); handle_verify: per sub-entry, filled by decode_selections — a sub-entry goes one route or the other (handle_verify[i].taken != 0
  // leaves table_verify[i].taken == 0)
  struct HandleEntry { uint64_t pair0, sum0; uint32_t nrows, first, taken; };
  struct Handle { const void* pairs = nullptr; uint64_t npairs = 0; const uint32_t* sums = nullptr; uint64_t nsums = 0; std::vector<HandleEntry> ent; std::vector<uint8_t> on; };
  const Handle* handle = nullptr;
  std::vector<HandleEntry> handle_verify;
  bool by_handle(uint32_t i) const { return !handle_verify.empty() && handle_verify[i].taken != 0; }
  bool compared(uint32_t i) const { return table(i) || by_handle(i); }   // the flag looks at this sub-entry, by either route
  // zgpu_seek_index_hash_device: every decoded zstd frame is hashed, with or without a Content_Checksum, whatever its length; and the collector —
  // per sub-entry that stands at status 0 behind every verdict, its decoded zstd frames in source order: where the frame begins in the
  // selection, its compressed length, its digest (of an entry decoded alone the low 32 bits only: the host's hash keeps no more)
  bool hash_every = false;
  struct Digest { uint64_t begin, clen, digest; };
  std::vector<std::vector<Digest>>* collect = nullptr;
  // zgpu_seek_index_records_device (zg_records.h): behind a submit's verdicts the bytes equal to `delimiter` in the decoded frames of every
  // sub-entry that stands at status 0 are found on the device (Batch::records_launch .. records_wait), and the offsets stay in a staging
  // buffer per submit. base[i], set by the caller: the entry coordinate of sub-entry i's first plaintext byte. run[i]: where sub-entry i's
  // n offsets lie — staging[buf] from slot `at`, or, of an entry decoded alone, host[i] (buf < 0; zgr::records_host over the host buffer).
  struct Records {
    uint32_t delimiter = 0;
    std::vector<uint64_t> base;
    struct Run { int32_t buf = -1; uint64_t at = 0, n = 0; };
    std::vector<Run> run;
    std::vector<std::vector<uint64_t>> host;
    std::vector<zg::DevBuf> staging;
    uint64_t us = 0, chunks = 0, bytes_back = 0;   // count + scan + emit microseconds (HIP events), chunks scanned, bytes the side pass brought back
    ~Records() { for (zg::DevBuf& b : staging) b.release(); }
  };
  Records* records = nullptr;
  uint64_t* stats = nullptr;     // zgpu_ctx::frames_device_stats (kDevStat*)
  uint64_t alone_written = 0;     // bytes the entries decoded alone brought to their destinations
};
// The device sink of a call, from its options. ZGPU_DEVICE_NO_HASH with ZGPU_DEVICE_VERIFY (hash nothing, verify everything) is refused: *st.
// ZGPU_DEVICE_VERIFY_SEEK_TABLE is refused the same way with ZGPU_DEVICE_NO_HASH, and on every call but those that have a seek table (table).
DeviceSink device_sink(zgpu_ctx* c, const zgpu_device_opts* opts, zgpu_device_entry_result* results, int* st, bool table = false);

// Bytes [lo, hi) of whole entry `entry` as ONE sub-entry of the machinery: walked, cut into submits, gathered, decoded and hashed as any entry is.
struct Selection {
  uint32_t entry;                 // index into the call's device_srcs / lens
  uint64_t lo, hi;                // hi == lo: nothing of it is read, decoded or written
  uint64_t declared;              // what the selection's frames declare together, UINT64_MAX if one declares nothing (promise: what its table says)
  uint32_t first_row, rows;       // DeviceSink::TableEntry::first / taken (rows == 0: not looked at)
  uint8_t refused;                // 0, 1 (its source or destination failed the pointer check), or the status itself (ZGPU_E_SEEK_TABLE)
};
// Of the concatenation of a sub-entry's decoded frames only [skip, skip + len) goes to dst (zg_entry.h, with the verdicts that fill it in).
using zge::Clip;
// The selections decoded, each a sub-entry with a SPAN of clips, clip[first[i] .. first[i + 1]), and one result in dres. promise: `declared`
// is a seek table's promise, which always holds — a selection that yields another length fails with ContentSizeMismatch. want_bound, if
// given: the plaintext bound every selection of nonzero length must walk to (not compared while shared dictionaries put gaps into the walk's).
int decode_selections(zgpu_ctx* c, DeviceSink& sink, const void* const* device_srcs, const size_t* lens, const std::vector<Selection>& sel,
                      std::vector<Clip>& clip, const std::vector<uint32_t>& first, bool promise, const uint64_t* want_bound,
                      zgpu_device_entry_result* dres);

// Is [p, p + cap) device memory of one allocation on the context's device? Asked of the HIP runtime, before any launch, of every destination
// and — zgpu_decode_frames_device_src — of every source. `known` remembers the allocations already seen in this call: entries usually share a
// few (a torch tensor cut into slots).
struct DevRange { uintptr_t lo, hi; };
bool check_device_range(int device, const void* p, size_t cap, std::vector<DevRange>& known);
// what every call asks of a pointer and its length: nothing of length 0 is touched, null with a length is bad, else the check above
inline bool device_ptr_ok(int device, const void* p, size_t len, std::vector<DevRange>& known) {
  return !len || (p && check_device_range(device, p, len, known));
}

// Every pointer of a call's entries checked, and the entries as the engine takes them: a refused entry has length 0 — nothing of it is
// read — and refused[i] = 1. dsts / caps: nullptr for a call without destinations. pre(i), the call's own reasons: kCheck — the pointers
// decide; kRefuse — refused without a look at them; kPass — never refused, whatever its pointers are (nothing of it will be touched).
enum { kCheck = 0, kRefuse, kPass };
template <class Pre>
void check_entries(zgpu_ctx* c, const void* const* srcs, const size_t* lens, void* const* dsts, const size_t* caps, uint32_t n, Pre pre,
                   std::vector<zg::Engine::DevEntry>* dev, std::vector<uint8_t>* refused) {
  dev->resize(n);
  refused->assign(n, 0);
  std::vector<DevRange> known;   // (per call: what the runtime says of an allocation holds for as long as the caller keeps its promise)
  const int device = c->eng->device();
  for (uint32_t i = 0; i < n; i++) {
    const int p = pre(i);
    bool bad = p == kRefuse;
    if (p == kCheck) bad = !device_ptr_ok(device, srcs[i], lens[i], known) || (dsts && !device_ptr_ok(device, dsts[i], caps[i], known));
    (*refused)[i] = bad;
    (*dev)[i] = zg::Engine::DevEntry{(uint64_t)(uintptr_t)srcs[i], bad ? 0u : (uint64_t)lens[i]};
  }
}
inline int check_all(uint32_t) { return kCheck; }

// The same check for m ranges that each name one of n entries and have a destination of their own. Every range is looked at on its own, in
// this order: entry >= n or pad != 0 refuses it; a length of 0 passes untouched; its entry is checked — ONCE, when the first range of nonzero
// length names it — and an entry that fails refuses the ranges that name it; a destination that fails refuses its own range. pre(i) as above,
// asked once per entry: kPass — the ranges of the entry pass untouched and are not live. srcs == nullptr: no entry has a pointer to check;
// dsts == nullptr: no range has a destination. refused[j]; live[j]: the range is to be looked up; passed, if given: the entries that passed,
// in the order in which they did.
template <class Pre>
void check_entry_ranges(zgpu_ctx* c, const void* const* srcs, const size_t* lens, uint32_t n, const zgpu_entry_range* ranges, uint32_t m,
                        void* const* dsts, const size_t* caps, Pre pre, std::vector<uint8_t>* refused, std::vector<uint8_t>* live,
                        std::vector<uint32_t>* passed) {
  refused->assign(m, 0);
  live->assign(m, 0);
  std::vector<DevRange> known;
  const int device = c->eng->device();
  enum : uint8_t { kUnseen = 0, kPassed, kRefused, kUntouched };
  std::vector<uint8_t> seen(n, kUnseen);   // (kUnseen: no range of nonzero length has named it yet)
  for (uint32_t j = 0; j < m; j++) {
    const zgpu_entry_range& g = ranges[j];
    if (g.entry >= n || g.pad) { (*refused)[j] = 1; continue; }
    if (!g.len) continue;
    const uint32_t i = g.entry;
    if (seen[i] == kUnseen) {
      const int p = pre(i);
      const bool bad = p == kRefuse || (p == kCheck && srcs && !device_ptr_ok(device, srcs[i], lens[i], known));
      seen[i] = p == kPass ? kUntouched : bad ? kRefused : kPassed;
      if (seen[i] == kPassed && passed) passed->push_back(i);
    }
    if (seen[i] == kUntouched) continue;
    if (seen[i] == kRefused || (dsts && !device_ptr_ok(device, dsts[j], caps[j], known))) { (*refused)[j] = 1; continue; }
    (*live)[j] = 1;
  }
}

// The statistics a call family owns, zeroed at its start (after its arguments passed): the one place that says which arrays a call writes.
enum : unsigned { kOwnsDecode = 1 /* frames_submits, frames_dict_stats */, kOwnsDevice = 2, kOwnsSrc = 4, kOwnsIndex = 8, kOwnsRanges = 16 };
void reset_stats(zgpu_ctx* c, unsigned owned);

// The end of every call that launched something: nothing of it is in flight on the engine's two streams (the scatter ran on the second), so
// every later operation on any stream sees its bytes. The call's first status stands.
int drain(zgpu_ctx* c, int st);

// the zgpu_debug_*_stats getters: the first n slots of an array, or all it has; returns how many
template <size_t N> int copy_stats(const uint64_t (&a)[N], uint64_t* out, int n) {
  if (!out) return 0;
  int k = 0;
  for (; k < n && k < (int)N; k++) out[k] = a[k];
  return k;
}

}  // namespace zgf
