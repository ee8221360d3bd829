// zg_entry.h — what is known about a decoded entry of the decode_frames calls, as a value, and everything that turns that value into a result,
// once: the order of verdicts include/zgpu.h promises ("the order is one — decode and walk, size, TARGET_TOO_SMALL, checksum — for every entry:
// with or without dictionary frames, in a shared submit or decoded alone"), the verdicts of ZGPU_DEVICE_VERIFY and of the table's record, the frame list of
// ZGPU_DEVICE_VERIFY_SEEK_TABLE's compare, the checksum fields of a result, and the pieces of an entry's frames its clips take. A submit
// (zg_frames.cpp: decode_submit) and an entry decoded alone (decode_alone) differ in how they PRODUCE the facts and in how they move the bytes;
// what the facts mean for the caller is written here and nowhere else. Plain C++17: no HIP call, no context — tests/emu/zg_lane_entry.cpp
// runs it on the CPU against a restatement of include/zgpu.h in Python (tests/test_entry_verdict_cpu.py).
//
// Where the two producers differ, the difference is a property of the facts, not a branch in the consumer:
//   - an entry decoded alone was hashed on the host, every frame of it, whatever hash_max_bytes says: Frame::hashed is true for all its frames.
//     Only the seek-table compare asks again (compare_list's predicate: a frame longer than a nonzero hash_max_bytes passes uncompared, as in a
//     submit); its digests hold the low 32 bits only;
//   - alone, under ranges, the host buffer holds the selection's bound: Entry::bound_buffer makes the decoder's own TargetTooSmall — a frame
//     that yields more than it declares — the ContentSizeMismatch a submit reports for it;
//   - alone, the frame-by-frame pass may have failed (never seen): Entry::known is false, the frames are counted from their headers, the sizes
//     are checked by the total, no checksum is reported and nothing vouches for the frames.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/zgpu.h"
#include "zg_seeksums.h"

namespace zge {

// Of the concatenation of a sub-entry's decoded frames only [skip, skip + len) goes to dst. small / written: the clip's own verdict and count
// once the sub-entry's frames are measured (ladder); they mean something only where the sub-entry stands at status 0.
struct Clip { uint64_t skip, len; uint8_t* dst; uint64_t cap; uint64_t written; bool small; };

// one decoded zstd frame
struct Frame {
  uint64_t begin, clen;       // where the compressed frame lies in the entry (or selection)
  uint64_t yielded;           // the bytes it yielded
  uint64_t end;               // where they end in the concatenation of the entry's frames
  uint64_t declared;          // (declares) its Frame_Content_Size
  uint64_t digest;            // (hashed) XXH64 of what it yielded; alone: the low 32 bits
  uint32_t checksum;          // (has_checksum) its Content_Checksum
  uint32_t slot;              // (hashed) where its digest lies in the array the seek-table compare reads
  bool declares, has_checksum, hashed;
};

// one entry: the frames are fr[0 .. nframes) if they are known one by one, else there is no view of them
struct Entry {
  int decode = 0;             // the first failing frame's status in stream order (alone: what the decoder returned)
  int walk = 0;               // where the walk of the entry's headers ended (alone: the decoder's status carries it)
  bool dict = false;          // holds a dictionary frame that a shared submit decoded: zgpu_decode_all takes such an entry frame by frame
  bool known = true;          // the frames are known one by one (false: the fallback of decode_alone)
  bool bound_buffer = false;  // decoded into a buffer of the selection's bound, not of the caller's capacity (alone, ranges)
  uint64_t total = 0;         // bytes the frames yielded together
  uint64_t sound = 0;         // (dict) bytes up to the last frame that decoded and parsed with no decode error in front of it
  uint32_t nframes = 0;
  const Frame* fr = nullptr;
  uint32_t viewed() const { return known ? nframes : 0; }
};

// What an entry's bytes are measured against. No ranges: the caller's capacity. Ranges: the span of clips, what the selection's frames declare
// together (UINT64_MAX if one declares nothing) and whether that number is a seek table's promise, which always holds.
struct Mode {
  bool ranges = false, promise = false;
  uint64_t cap = 0, declared = UINT64_MAX;
  Clip* clip = nullptr;
  uint32_t nclips = 0;
};
struct Verdict { int status; uint64_t written; };

// THE ORDER. Ranges have one: the decode and walk verdicts, ContentSizeMismatch (per frame against what the frame declares; by the total where
// the frames are not known; a promise by the total), TargetTooSmall by the clipped count — each clip measured on its own against its own
// capacity, a clip that is too small gets nothing and does not disturb the others, the entry is too small only if every clip is, and an empty
// span wants no byte and is never too small. Without ranges sizes are not checked, and an entry with a dictionary frame is what zgpu_decode_all
// decodes frame by frame, every frame read out before the next one is looked at: a frame that does not fit ends it with TargetTooSmall BEFORE
// a later frame's error or the walk's; any other entry reports a decode error first, then the walk's, then TargetTooSmall.
// (The checksum verdicts rank behind all of these: verify_fails, then table_fails.) Sets Clip::written and Clip::small.
inline Verdict ladder(const Entry& e, const Mode& m) {
  uint64_t fits = e.total;
  bool too_small = e.total > m.cap;
  if (m.ranges) {
    bool any = false;
    fits = 0;
    for (uint32_t q = 0; q < m.nclips; q++) {
      Clip& cl = m.clip[q];
      const uint64_t rest = e.total > cl.skip ? e.total - cl.skip : 0, w = rest < cl.len ? rest : cl.len;
      cl.small = w > cl.cap;
      cl.written = cl.small ? 0 : w;
      if (!cl.small) { fits += w; any = true; }
    }
    too_small = !any && m.nclips != 0;
  }
  int st;
  if (e.dict && !m.ranges) st = e.sound > m.cap ? ZGPU_E_TARGET_TOO_SMALL : e.decode ? e.decode : e.walk;
  else {
    bool lied = m.ranges && m.promise && e.total != m.declared;
    if (m.ranges && !e.known) lied = lied || (m.declared != UINT64_MAX && e.total != m.declared);
    for (uint32_t f = 0; m.ranges && f < e.viewed(); f++) lied = lied || (e.fr[f].declares && e.fr[f].declared != e.fr[f].yielded);
    const bool overflowed = m.ranges && e.bound_buffer && e.decode == ZGPU_E_TARGET_TOO_SMALL;
    st = overflowed ? ZGPU_E_CONTENT_SIZE_MISMATCH : e.decode ? e.decode : e.walk ? e.walk : lied ? ZGPU_E_CONTENT_SIZE_MISMATCH
       : too_small ? ZGPU_E_TARGET_TOO_SMALL : ZGPU_OK;
  }
  return Verdict{st, st ? 0 : fits};
}

// A device-sink entry fails with `status`: written = nframes = 0 like any failed entry (sums / bad / unverified: the counts of the checksum
// verdicts, which say why). The arguments are taken by value: they may be d's own fields.
inline void fail_entry(zgpu_device_entry_result& d, int status, uint32_t sums = 0, uint32_t bad = 0, uint32_t unverified = 0) {
  d = zgpu_device_entry_result{};
  d.r.status = status;
  d.r.checksums = sums; d.r.checksum_mismatches = bad;
  d.checksums_unverified = unverified;
}

// ZGPU_DEVICE_VERIFY on an entry that stands at status 0, behind every verdict of the ladder: a HASHED frame whose digest differs from its
// Content_Checksum fails it (ZGPU_E_CHECKSUM_MISMATCH) — it reports the frames that carry a checksum and those that failed. Returns whether it failed.
inline bool verify_fails(zgpu_device_entry_result& d, const Entry& e) {
  uint32_t carried = 0, differing = 0;
  for (uint32_t f = 0; f < e.viewed(); f++) {
    if (!e.fr[f].has_checksum) continue;
    carried++;
    if (e.fr[f].hashed && e.fr[f].checksum != (uint32_t)e.fr[f].digest) differing++;
  }
  if (differing) fail_entry(d, ZGPU_E_CHECKSUM_MISMATCH, carried, differing);
  return differing != 0;
}
// ZGPU_DEVICE_VERIFY_SEEK_TABLE, last, on an entry of nframes decoded zstd frames that still stands at status 0, from the compare's record
// (zg_seeksums.h: vouched; a record with a `why` is the CALL's error and never comes here). A failed entry (ZGPU_E_SEEK_CHECKSUM_MISMATCH)
// reports the frames compared, those that differ and the decoded frames not compared. Returns whether it failed.
inline bool table_fails(zgpu_device_entry_result& d, const zgv::Sums& s, uint32_t nframes) {
  if (zgv::vouched(s, nframes)) return false;
  fail_entry(d, ZGPU_E_SEEK_CHECKSUM_MISMATCH, s.compared, s.differing, nframes - s.compared);
  return true;
}

// ZGPU_DEVICE_VERIFY_SEEK_TABLE: the entry's slice of the compare's frame list (zg_seeksums.h), appended to *list. A frame of 2^32 compressed
// bytes or more is left out — no row can hold its length, it coincides with none —, a frame that is not hashed, or whose digest may not be
// used (may(frame) is false), is listed with kNotHashed.
template <class May> void compare_list(const Entry& e, May may, std::vector<zgv::Frame>* list) {
  for (uint32_t f = 0; f < e.viewed(); f++) {
    const Frame& x = e.fr[f];
    if (x.clen > 0xFFFFFFFFull) continue;
    list->push_back(zgv::Frame{x.begin, (uint32_t)x.clen, x.hashed && may(x) ? x.slot : zgv::kNotHashed});
  }
}

// The frames of an entry by whether they were hashed (no_hash: none counts as hashed) — kDevStatFramesHashed / kDevStatFramesNotHashed.
struct Hashed { uint32_t hashed, not_hashed; };
inline Hashed hashed_frames(const Entry& e, bool no_hash) {
  Hashed h{0, e.known ? 0u : e.nframes};
  for (uint32_t f = 0; f < e.viewed(); f++) (e.fr[f].hashed && !no_hash ? h.hashed : h.not_hashed)++;
  return h;
}

// The checksum fields of the result of an entry that stands at status 0 behind every verdict: r->checksums counts the frames that carry a
// Content_Checksum, r->checksum_mismatches those among the hashed ones that differ, *unverified the ones that were not hashed; the first
// frame's stored checksum and — if it was hashed: *first_hashed — its digest's low 32 bits. unverified / first_hashed: nullptr for the plain
// result of the host sink, where every frame is hashed. An entry whose frames are not known reports none.
inline Hashed fill(const Entry& e, bool no_hash, zgpu_entry_result* r, uint32_t* unverified, uint32_t* first_hashed) {
  uint32_t unv = 0;
  r->checksums = r->checksum_mismatches = r->checksum_from_data = r->calculated_checksum = 0;
  for (uint32_t f = 0; f < e.viewed(); f++) {
    const Frame& x = e.fr[f];
    const bool h = x.hashed && !no_hash;
    if (f == 0) { r->checksum_from_data = x.has_checksum ? x.checksum : 0u; r->calculated_checksum = h ? (uint32_t)x.digest : 0u; }
    if (!x.has_checksum) continue;
    r->checksums++;
    if (!h) unv++;
    else if (x.checksum != (uint32_t)x.digest) r->checksum_mismatches++;
  }
  if (unverified) *unverified = unv;
  if (first_hashed) *first_hashed = e.viewed() && e.fr[0].hashed && !no_hash ? 1u : 0u;
  return hashed_frames(e, no_hash);
}

// What one clip takes of the frames fr[0 .. n): emit(Piece) for every run of bytes that lies in one frame, in order; returns the bytes the clip
// gets. A clip that is too small takes nothing. The first frame that ends behind the clip's begin is found by a search: a call with many
// clips over many frames does not walk all frames for each.
struct Piece { uint32_t frame; uint64_t in_frame, cat, at, len; };   // bytes [in_frame, + len) of `frame` = [cat, + len) of the concatenation -> [at, + len) of the clip's destination
template <class Emit> uint64_t clip_pieces(const Frame* fr, uint32_t n, const Clip& cl, Emit emit) {
  if (cl.small) return 0;
  const uint64_t lo = cl.skip, hi = cl.len < UINT64_MAX - lo ? lo + cl.len : UINT64_MAX;
  uint32_t f = (uint32_t)(std::upper_bound(fr, fr + n, lo, [](uint64_t v, const Frame& x) { return v < x.end; }) - fr);
  uint64_t at = 0;
  for (; f < n && fr[f].end - fr[f].yielded < hi; f++) {
    const uint64_t a = fr[f].end - fr[f].yielded, s = a > lo ? a : lo, t = fr[f].end < hi ? fr[f].end : hi;
    if (s >= t) continue;
    emit(Piece{f, s - a, s, at, t - s});
    at += t - s;
  }
  return at;
}

}  // namespace zge
