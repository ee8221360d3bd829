// zg_lane_seek.cpp — TEST-ONLY: runs zg_k_seek's lane routine (zstd-rs_amd/csrc/zg_seek.h) on the CPU. tests/test_seek_cpu.py builds this file
// (tests/lanesuite.py), twice: as a shared library in which, for every input and every range, the routine runs over a reader that counts every
// access outside [anchor_src, len) and every access to a byte of a block body (the bodies as zgw::walk_entry's records give them) and every
// field of its record is compared with a model computed from zgi::index_entry<true>'s frame records and frame_fields — existing code, not the
// routine under test; and — with -DSEEK_MAIN — as a stand-alone AddressSanitizer program that runs the same ranges and anchors over entries
// lying in heap blocks of exactly their length. It also counts what the ranges reached (g_cov). Not part of the product.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
#include "zg_seek.h"
#include "zg_lane_mem.h"
using namespace zg;
namespace {
using Reader = lane::Reader<uint8_t>;   // the entry as a lane may see it: bytes [lo, len), and none that belongs to a block body
using NoCount = lane::Direct<uint8_t>;
using WalkWriter = lane::DirectArray<zgw::Rec>;
using RecWriter = lane::DirectArray<zgi::FrameRec>;
// [0] cases [1] open-ended [2] the chain broke in front of the range [3] it broke inside the selection [4] an empty frame at a boundary
// [5] bit 2 [6] anchored runs [7] ranges of length 0 [8] refused anchors
uint64_t g_cov[16];

bool readable(const zgi::FrameRec& x) { FrameFields f; frame_fields(x.b, x.have, &f); return f.header_status == ZG_OK; }

// The rule of zg_seek.h over the frame records of the whole entry, from record `start` (the one that begins at anchor_src) on.
zgk::Seek model(const zgi::FrameRec* fr, uint32_t nrec, uint32_t ewhy, uint64_t len, uint64_t begin, uint64_t rlen, uint32_t start,
                uint64_t anchor_src, uint64_t anchor_plain, bool* empty_at_boundary, bool* broke_in_front) {
  zgk::Seek o;
  memset(&o, 0, sizeof o);
  if (!rlen) return o;
  if (anchor_src > len || anchor_plain > begin) { o.status = 93; return o; }
  const unsigned __int128 end = (unsigned __int128)begin + rlen;
  unsigned __int128 pos = anchor_plain;
  uint64_t lo = 0, plo = 0, hi = anchor_src;
  bool taken = false, open = false;
  uint32_t why = 0;
  const uint64_t top = ~0ull;
  for (uint32_t k = start; k < nrec; k++) {
    const zgi::FrameRec& x = fr[k];
    FrameFields f;
    frame_fields(x.b, x.have, &f);
    const bool z = f.header_status == ZG_OK, sized = (f.flags & 2u) != 0;
    o.nblocks += x.nblocks;
    hi = x.end;
    if (k + 1 == nrec && ewhy) {
      why = ewhy;
      if (!taken) { taken = true; lo = x.begin; plo = (uint64_t)pos; *broke_in_front = true; }
      if (z) { o.frames_taken++; o.bound += x.bound; }
      break;
    }
    if (!z) continue;
    if (!taken && sized && pos + f.frame_content_size <= begin) {
      if (f.frame_content_size == 0 && pos == begin) *empty_at_boundary = true;
      o.frames_skipped++; pos += f.frame_content_size;
      continue;
    }
    if (!taken) { taken = true; lo = x.begin; plo = (uint64_t)pos; }
    o.frames_taken++; o.bound += x.bound;
    if (sized) { pos += f.frame_content_size; if (pos > top) pos = top; } else open = true;
    if (!open && pos >= (end > top ? (unsigned __int128)top : end)) break;
  }
  o.src_lo = taken ? lo : hi; o.src_hi = why ? len : hi;
  o.plain_lo = taken ? plo : (uint64_t)pos; o.plain_seen = (uint64_t)pos;
  o.why = why;
  o.flags = (open ? 1u : 0u) | (why ? 2u : 0u) | (taken ? 0u : 4u);
  return o;
}

struct Input {
  const uint8_t* data; uint64_t len;
  zgi::Entry e;
  std::vector<zgi::FrameRec> fr;
  std::vector<uint8_t> body;
  std::vector<uint64_t> plain_at;   // declared plaintext offset at record k's begin (unsized frames count nothing)
  std::vector<uint8_t> sized_front; // every zstd frame in front of record k declares a size
};
void prepare(Input& in, bool bodies) {
  const NoCount nr{in.data};
  in.e = zgi::index_entry<false>(nr, RecWriter{nullptr}, in.len, 0, 0);
  in.fr.resize(in.e.nrec + 1);
  (void)zgi::index_entry<true>(nr, RecWriter{in.fr.data()}, in.len, 0, in.e.nrec);
  in.fr.resize(in.e.nrec);
  in.plain_at.assign(in.e.nrec + 1, 0);
  in.sized_front.assign(in.e.nrec + 1, 1);
  for (uint32_t k = 0; k < in.e.nrec; k++) {
    FrameFields f;
    frame_fields(in.fr[k].b, in.fr[k].have, &f);
    const bool z = f.header_status == ZG_OK, sized = (f.flags & 2u) != 0;
    uint64_t next = in.plain_at[k] + (z && sized ? f.frame_content_size : 0);
    if (next < in.plain_at[k]) next = ~0ull;
    in.plain_at[k + 1] = next;
    in.sized_front[k + 1] = in.sized_front[k] && (!z || sized);
  }
  if (!bodies) return;
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, in.len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, in.len, 0, w0.nrec);
  in.body.assign(in.len + 1, 0);
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind != zgw::kBlock) continue;
    const uint32_t type = (x.b[0] >> 1) & 3u, size = (uint32_t)(x.b[0] >> 3) | ((uint32_t)x.b[1] << 5) | ((uint32_t)x.b[2] << 13);
    if (type == 3 || size > zgw::kBlockMax) continue;
    const uint64_t n = type == 1 ? 1 : size;
    for (uint64_t q = x.off; q < x.off + n && q < in.len; q++) in.body[q] = 1;
  }
}
// every (begin, len) of the input, f(begin, len)
template <class F> void ranges(const Input& in, F f) {
  std::vector<uint64_t> begins{0};
  const uint64_t total = in.plain_at[in.e.nrec];
  for (uint32_t k = 0; k <= in.e.nrec; k++) for (int d = -1; d <= 1; d++) {
    const uint64_t b = in.plain_at[k];
    if (d < 0 && !b) continue;
    begins.push_back(b + (uint64_t)d);
  }
  begins.push_back(total); begins.push_back(total + 5);
  for (uint64_t b : begins) {
    const uint64_t lens[5] = {1, 2, total > b ? total - b : 0, 1ull << 63, 0};
    for (uint64_t l : lens) f(b, l);
  }
}

// one input: 0 if everything agrees, else a bit per kind of disagreement (*where: the begin of the range that disagreed)
uint32_t check(const uint8_t* data, uint64_t len, uint64_t* where) {
  Input in{data, len};
  prepare(in, true);
  const uint32_t nrec = in.e.nrec;
  uint32_t bad = 0;
  ranges(in, [&](uint64_t begin, uint64_t rlen) {
    if (bad) return;
    lane::Count c;
    const zgk::Seek un = zgk::seek_entry(Reader::over(data, 0, len, &c, in.body.data()), len, begin, rlen, 0, 0);
    bool empty = false, front = false;
    const zgk::Seek m = model(in.fr.data(), nrec, in.e.why, len, begin, rlen, 0, 0, 0, &empty, &front);
    if (!lane::same_seek(un, m)) bad |= 1u;
    if (c.bad) bad |= 2u;
    if (c.forbidden) bad |= 4u;
    if (un.src_lo > un.src_hi || un.src_hi > len) bad |= 8u;
    else if (un.bound != plaintext_bound(data + un.src_lo, (size_t)(un.src_hi - un.src_lo))) bad |= 16u;
    g_cov[0]++;
    if (!rlen) { g_cov[7]++; zgk::Seek z; memset(&z, 0, sizeof z); if (!lane::same_seek(un, z) || c.bad || c.forbidden) bad |= 32u; if (bad) *where = begin; return; }
    bool lo_ok = un.src_lo == len && !nrec, hi_ok = (un.flags & zgk::kBroken) ? un.src_hi == len : (un.src_hi == 0 && !nrec);
    for (uint32_t k = 0; k < nrec; k++) {
      if (in.fr[k].begin == un.src_lo || in.fr[k].end == un.src_lo) lo_ok = true;
      if (in.fr[k].begin == un.src_hi || in.fr[k].end == un.src_hi) hi_ok = true;
    }
    if (!lo_ok || !hi_ok) bad |= 64u;
    if (un.flags & zgk::kOpenEnded) g_cov[1]++;
    if ((un.flags & zgk::kBroken) && front && un.frames_skipped) g_cov[2]++;
    if ((un.flags & zgk::kBroken) && !front) g_cov[3]++;
    if (empty) g_cov[4]++;
    if (un.flags & zgk::kNothing) g_cov[5]++;
    // anchored at every boundary in front of the selection
    for (uint32_t k = 1; k <= nrec && !bad; k++) {
      const uint64_t at = k < nrec ? in.fr[k].begin : in.fr[nrec - 1].end;
      if (k == nrec && (in.e.why || at != len)) continue;
      if (k < nrec && in.fr[k].begin == in.fr[k].end && k + 1 == nrec && in.fr[k - 1].end != at) continue;
      if (!in.sized_front[k] || at > un.src_lo || in.plain_at[k] > begin) continue;
      lane::Count c2;
      const zgk::Seek an = zgk::seek_entry(Reader::over(data, at, len, &c2, in.body.data()), len, begin, rlen, at, in.plain_at[k]);
      bool e2 = false, f2 = false;
      const zgk::Seek m2 = model(in.fr.data(), nrec, in.e.why, len, begin, rlen, k, at, in.plain_at[k], &e2, &f2);
      if (!lane::same_seek(an, m2)) bad |= 128u;
      if (c2.bad) bad |= 256u;
      if (c2.forbidden) bad |= 512u;
      if (an.src_lo != un.src_lo || an.src_hi != un.src_hi || an.plain_lo != un.plain_lo || an.flags != un.flags || an.nblocks > un.nblocks ||
          an.bound != un.bound || an.status)
        bad |= 1024u;
      g_cov[6]++;
    }
    // anchors the call refuses: behind the entry, behind begin
    {
      lane::Count c3;
      const zgk::Seek r1 = zgk::seek_entry(Reader::over(data, 0, len, &c3, in.body.data()), len, begin, rlen, len + 1, 0);
      zgk::Seek z; memset(&z, 0, sizeof z); z.status = 93;
      if (!lane::same_seek(r1, z) || c3.bad) bad |= 2048u;
      if (begin != ~0ull) {
        const zgk::Seek r2 = zgk::seek_entry(Reader::over(data, 0, len, &c3, in.body.data()), len, begin, rlen, 0, begin + 1);
        if (!lane::same_seek(r2, z) || c3.bad) bad |= 2048u;
      }
      g_cov[8]++;
    }
    if (bad) *where = begin;
  });
  return bad;
}
}  // namespace

extern "C" uint32_t sk_check(const uint8_t* data, uint64_t len, uint64_t* where) { return check(data, len, where); }
extern "C" void sk_coverage(uint64_t* out) { memcpy(out, g_cov, sizeof g_cov); }
extern "C" void sk_one(const uint8_t* data, uint64_t len, uint64_t begin, uint64_t rlen, uint64_t anchor_src, uint64_t anchor_plain, void* out) {
  const zgk::Seek s = zgk::seek_entry(NoCount{data}, len, begin, rlen, anchor_src, anchor_plain);
  memcpy(out, &s, sizeof s);
}

#ifdef SEEK_MAIN
// The same ranges and anchors over entries that lie in heap blocks of exactly their length, read directly: an access outside an entry is an
// AddressSanitizer report. The file holds [u64 length][bytes] per entry.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 1 ? argv[1] : nullptr, "rb");
  uint64_t n = 0, runs = 0, sum = 0;
  for (uint64_t len; f.next(&len, 8); n++) {
    uint8_t* e = f.block(len);
    Input in{e, len};
    prepare(in, false);
    ranges(in, [&](uint64_t begin, uint64_t rlen) {
      const zgk::Seek un = zgk::seek_entry(NoCount{e}, len, begin, rlen, 0, 0);
      runs++; sum += un.src_hi + un.nblocks;
      for (uint32_t k = 1; k < in.e.nrec; k++) {
        const uint64_t at = in.fr[k].begin;
        if (!in.sized_front[k] || at > un.src_lo || in.plain_at[k] > begin) continue;
        const zgk::Seek an = zgk::seek_entry(NoCount{e}, len, begin, rlen, at, in.plain_at[k]);
        runs++; sum += an.src_hi + an.nblocks;
      }
    });
    free(e);
  }
  f.close();
  printf("seek_asan ok: %llu entries, %llu runs (%llu)\n", (unsigned long long)n, (unsigned long long)runs, (unsigned long long)sum);
  return 0;
}
#endif
