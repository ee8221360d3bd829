// zg_lane_index.cpp — TEST-ONLY: runs zg_k_index's lane routine (zstd-rs_amd/csrc/zg_index.h) and the host's reading of its frame records
// (zg_host_parse.cpp: frame_fields) on the CPU. tests/test_index_cpu.py builds this file (tests/lanesuite.py) as a shared library. For every
// input the lane runs twice, summary pass and emit pass, over a reader that counts every access outside [0, len) and every access to a byte of
// a block body (the bodies as zgw::walk_entry's records give them), and a writer that counts every store outside the lane's own record range,
// which lies between guard records (zg_lane_mem.h). It also counts what the inputs reached: stop reasons, entry and frame flags, headers the
// chain could not read. Not part of the product.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
#include "zg_index.h"
#include "zg_lane_mem.h"
using namespace zg;
namespace {
using Reader = lane::Reader<uint8_t>;            // the entry as a lane may see it: bytes [0, len), and none that belongs to a block body
using Writer = lane::Array<zgi::FrameRec>;       // the lane's record range [lo, hi) of recs
using NoCount = lane::Direct<uint8_t>;
using WalkWriter = lane::DirectArray<zgw::Rec>;
constexpr uint64_t kGuard = 4;
uint64_t g_why[16], g_cases, g_flagbits[4], g_recflags[5], g_unreadable;

// one input: 0 if everything agrees, else a bit per kind of disagreement
uint32_t check(const uint8_t* data, uint64_t len, uint64_t max_window) {
  uint32_t bad = 0;
  // the reference: the walk's records and where it stopped
  const NoCount nr{data};
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, len, 0, w0.nrec);
  std::vector<uint8_t> body(len + 1, 0);
  uint32_t wframes = 0, wskip = 0, wblocks = 0;
  std::vector<const zgw::Rec*> wfr;
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind == zgw::kFrame) {
      FrameFields f;
      frame_fields(x.b, x.have, &f);
      wframes += f.header_status == ZG_OK; wskip += f.header_status == ZG_SKIP_FRAME;
      wfr.push_back(&x);
    } else if (x.kind == zgw::kBlock) {
      wblocks++;
      const uint32_t type = (x.b[0] >> 1) & 3u, size = (uint32_t)(x.b[0] >> 3) | ((uint32_t)x.b[1] << 5) | ((uint32_t)x.b[2] << 13);
      if (type == 3 || size > zgw::kBlockMax) continue;
      const uint64_t n = type == 1 ? 1 : size;
      for (uint64_t q = x.off; q < x.off + n && q < len; q++) body[q] = 1;
    }
  }
  lane::Count rc, wc;
  const Reader r = Reader::over(data, 0, len, &rc, body.data());
  const Writer none{nullptr, 0, 0, &wc};
  const zgi::Entry e0 = zgi::index_entry<false>(r, none, len, 0, 0);
  if (wc.kept || wc.bad) bad |= 1u;
  lane::Guarded<zgi::FrameRec> recs(e0.nrec, kGuard);
  const Writer w{recs.at(), recs.lo(), recs.hi(), &wc};
  const zgi::Entry e1 = zgi::index_entry<true>(r, w, len, kGuard, e0.nrec);
  if (!zgi::same_entry(e0, e1)) bad |= 2u;
  if (wc.kept != e0.nrec) bad |= 4u;
  if (rc.bad) bad |= 8u;
  if (wc.bad) bad |= 16u;
  if (rc.forbidden) bad |= 32u;
  if (!recs.intact()) bad |= 16u;
  if (e0.nrec > 1) {   // a lane whose range is shorter than its records still stays inside it, and says how many it has
    lane::Count rc2, wc2;
    std::vector<zgi::FrameRec> few(e0.nrec - 1 + 2 * kGuard);
    const Writer w2{few.data(), kGuard, kGuard + e0.nrec - 1, &wc2};
    const zgi::Entry e2 = zgi::index_entry<true>(Reader::over(data, 0, len, &rc2, body.data()), w2, len, kGuard, e0.nrec - 1);
    if (wc2.bad || rc2.bad || rc2.forbidden || wc2.kept != e0.nrec - 1 || e2.nrec != e0.nrec) bad |= 16u;
  }
  if (e0.bound != plaintext_bound(data, len)) bad |= 64u;
  if (e0.chain_end != w0.stop_off || e0.why != w0.why) bad |= 128u;
  if (e0.nframes != wframes || e0.nskippable != wskip || e0.nblocks != wblocks) bad |= 256u;
  if (e0.nrec != wfr.size() || e0.pad != 0) bad |= 512u;
  // the frame records: bounds, extents, header fields
  const zgi::FrameRec* fr = recs.mid();
  uint64_t sum = 0, at = 0, blocks = 0;
  uint32_t flags = e0.nframes ? (zgi::kAllSized | zgi::kAllComplete) : 0u;
  for (uint32_t k = 0; k < e0.nrec && k < wfr.size(); k++) {
    const zgi::FrameRec& x = fr[k];
    sum += x.bound; blocks += x.nblocks;
    if (x.begin != at || x.end < x.begin || x.end > len || x.begin != wfr[k]->off) bad |= 1024u;
    at = x.end;
    FrameFields a, b;
    frame_fields(x.b, x.have, &a);
    frame_fields(wfr[k]->b, wfr[k]->have, &b);
    if (memcmp(&a, &b, sizeof a)) bad |= 2048u;
    for (uint32_t q = x.have; q < sizeof x.b; q++) if (x.b[q]) bad |= 2048u;
    if (((x.flags & zgi::kSkippable) != 0) != (a.header_status == ZG_SKIP_FRAME) || (x.flags & ~(zgi::kSkippable | zgi::kComplete))) bad |= 2048u;
    if (a.header_status == ZG_OK) {
      if (!(a.flags & 2u)) flags &= ~zgi::kAllSized;
      if (a.dict_id) flags |= zgi::kAnyDict;
      if (a.flags & 4u) flags |= zgi::kAnyChecksum;
      if (!(x.flags & zgi::kComplete)) flags &= ~zgi::kAllComplete;
      if ((a.flags & 2u) && x.bound > a.frame_content_size) bad |= 4096u;
    } else {
      if (x.bound || x.nblocks || (x.flags & zgi::kComplete)) bad |= 4096u;
      if (a.header_status != ZG_SKIP_FRAME) { g_unreadable++; if (x.begin != x.end || k + 1 != e0.nrec) bad |= 4096u; }
    }
    for (int q = 0; q < 5; q++) if ((x.flags | a.flags) & (1u << q)) g_recflags[q]++;
  }
  if (sum != e0.bound || blocks != e0.nblocks) bad |= 8192u;
  if (at != e0.chain_end) bad |= 16384u;
  if (flags != e0.flags) bad |= 32768u;
  // against the host's parse, where it accepts the whole input: one record per frame or skippable frame, fields as FrameInfo has them
  BatchBuilder bb;
  std::vector<FrameInfo> info;
  if (parse_frames(data, len, max_window, &bb, &info, 0) == ZG_OK) {
    size_t f = 0;
    if (e0.why != zgw::kEnd || !(e0.nframes == 0 || (e0.flags & zgi::kAllComplete))) bad |= 65536u;
    for (uint32_t k = 0; k < e0.nrec; k++) {
      const zgi::FrameRec& x = fr[k];
      if (x.flags & zgi::kSkippable) continue;
      FrameFields a;
      frame_fields(x.b, x.have, &a);
      if (f >= info.size()) { bad |= 65536u; break; }
      const FrameInfo& fi = info[f++];
      if (x.begin != fi.src_begin || x.end != fi.src_end || x.nblocks != fi.nblocks || a.window_size != fi.window_size ||
          a.frame_content_size != fi.header.frame_content_size || ((a.flags & 4u) != 0) != fi.has_checksum || !(x.flags & zgi::kComplete))
        bad |= 65536u;
    }
    if (f != info.size() || e0.nframes != info.size()) bad |= 65536u;
  }
  g_cases++;
  g_why[e0.why & 15]++;
  for (int q = 0; q < 4; q++) if (e0.flags & (1u << q)) g_flagbits[q]++;
  return bad;
}
}  // namespace

extern "C" uint32_t ix_check(const uint8_t* data, uint64_t len, uint64_t max_window) { return check(data, len, max_window); }
extern "C" uint32_t ix_prefixes(const uint8_t* data, uint64_t len, uint64_t upto, uint64_t max_window, uint64_t* where) {
  const uint64_t n = len < upto ? len : upto;
  for (uint64_t k = 0; k <= n; k++) { const uint32_t bad = check(data, k, max_window); if (bad) { *where = k; return bad; } }
  return 0;
}
// single-byte edits at every frame-header byte (and the three bytes behind the header) and every block-header byte, each set to 0x00, 0xFF,
// one flipped bit and one random value (fixed seed); at most `budget` positions per input, evenly spread (0: every one)
extern "C" uint32_t ix_edits(uint8_t* data, uint64_t len, uint64_t max_window, uint64_t seed, uint64_t budget, uint64_t* where, uint64_t* nedits) {
  const NoCount nr{data};
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, len, 0, w0.nrec);
  std::vector<uint64_t> pos;
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind == zgw::kFrame) for (uint64_t q = 0; q < x.have; q++) pos.push_back(x.off + q);
    else if (x.kind == zgw::kBlock) for (uint64_t q = 0; q < 3; q++) pos.push_back(x.off - 3 + q);
  }
  uint64_t x = seed * 6364136223846793005ull + 1442695040888963407ull;
  const uint64_t step = budget && pos.size() > budget ? (pos.size() + budget - 1) / budget : 1;
  *nedits = 0;
  for (uint64_t q = 0; q < pos.size(); q += step) {
    const uint64_t p = pos[q];
    if (p >= len) continue;
    const uint8_t keep = data[p];
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const uint8_t vals[4] = {0x00, 0xFF, (uint8_t)(keep ^ (1u << ((x >> 33) & 7))), (uint8_t)(x >> 41)};
    for (uint8_t v : vals) {
      if (v == keep) continue;
      data[p] = v;
      const uint32_t bad = check(data, len, max_window);
      (*nedits)++;
      if (bad) { *where = p; data[p] = keep; return bad; }
    }
    data[p] = keep;
  }
  return 0;
}
extern "C" void ix_coverage(uint64_t* why, uint64_t* flagbits, uint64_t* recflags, uint64_t* unreadable, uint64_t* cases) {
  memcpy(why, g_why, sizeof g_why); memcpy(flagbits, g_flagbits, sizeof g_flagbits); memcpy(recflags, g_recflags, sizeof g_recflags);
  *unreadable = g_unreadable; *cases = g_cases;
}
// The emit pass over `now` with the ranges the summary pass took from `then`: out[0] stores outside the range, [1] reads outside the entry,
// [2] records written, [3] the limit, [4] whether the host would accept the pass (same_entry), [5] the count the pass reports
extern "C" void ix_changed(const uint8_t* then, uint64_t then_len, const uint8_t* now, uint64_t now_len, uint64_t* out) {
  lane::Count rc, wc;
  const Writer none{nullptr, 0, 0, &wc};
  const zgi::Entry e0 = zgi::index_entry<false>(Reader::over(then, 0, then_len, &rc), none, then_len, 0, 0);
  std::vector<zgi::FrameRec> recs(e0.nrec + 2 * kGuard);
  const Writer w{recs.data(), kGuard, kGuard + e0.nrec, &wc};
  const zgi::Entry e1 = zgi::index_entry<true>(Reader::over(now, 0, now_len, &rc), w, now_len, kGuard, e0.nrec);
  out[0] = wc.bad; out[1] = rc.bad; out[2] = wc.kept; out[3] = e0.nrec; out[4] = zgi::same_entry(e0, e1); out[5] = e1.nrec;
}
// The host's prefix sum over the summaries of n entries: first[0 .. n], returns the records a table needs
extern "C" uint64_t ix_ranges(const uint8_t* const* data, const uint64_t* lens, uint32_t n, uint64_t* first) {
  lane::Count c;
  std::vector<zgi::Entry> e(n);
  for (uint32_t i = 0; i < n; i++) e[i] = zgi::index_entry<false>(Reader::over(data[i], 0, lens[i], &c), Writer{nullptr, 0, 0, &c}, lens[i], 0, 0);
  return zgi::frame_ranges(e.data(), n, first);
}
