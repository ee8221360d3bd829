// zg_lane_walk.cpp — TEST-ONLY: runs zg_k_walk's lane routine (zstd-rs_amd/csrc/zg_walk.h) and the host's parse of its skeleton records
// (zg_host_parse.cpp) on the CPU. tests/test_walk_cpu.py builds this file (tests/lanesuite.py) as a shared library. For every input the lane
// runs twice, count pass and emit pass, over a reader that counts every access outside [0, len) and a writer that counts every store outside
// the lane's own record range, which lies between guard records (zg_lane_mem.h); then parse_frames_skel and plaintext_bound_skel over the
// records must give exactly what parse_frames and plaintext_bound give over the bytes. It also counts what the inputs reached: walk statuses,
// stop reasons, literals and sequences header formats, checksums. Not part of the product.
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "zg_host_parse.h"
#include "zg_lane_mem.h"
using namespace zg;
namespace {
using Reader = lane::Reader<uint8_t>;           // the entry as a lane may see it: bytes [0, len), nothing else
using Writer = lane::Array<zgw::Rec>;           // the lane's record range [lo, hi) of recs
constexpr uint64_t kGuard = 4, kBase = 64;
// coverage, over every input checked so far
uint64_t g_status[256], g_why[16], g_lit[2][4], g_seq[4], g_cksum[2], g_cases;

bool same_info(const FrameInfo& a, const FrameInfo& b) {
  return a.header.descriptor == b.header.descriptor && a.header.window_descriptor == b.header.window_descriptor &&
         a.header.has_dict_id == b.header.has_dict_id && a.header.dict_id == b.header.dict_id &&
         a.header.frame_content_size == b.header.frame_content_size && a.header.header_size == b.header.header_size &&
         a.window_size == b.window_size && a.src_begin == b.src_begin && a.src_end == b.src_end && a.has_checksum == b.has_checksum &&
         a.checksum == b.checksum && a.nblocks == b.nblocks && a.host_status == b.host_status;
}

// one input: 0 if everything agrees, else a bit per kind of disagreement
uint32_t check(const uint8_t* data, uint64_t len, uint64_t max_window) {
  uint32_t bad = 0;
  lane::Count rc, wc;
  const uint8_t* own = data;
  const Reader r = Reader::over(own, 0, len, &rc);
  const Writer none{nullptr, 0, 0, &wc};
  const zgw::End e0 = zgw::walk_entry<false>(r, none, len, 0, 0);
  if (wc.kept || wc.bad) bad |= 1u;
  lane::Guarded<zgw::Rec> recs(e0.nrec, kGuard);
  const Writer w{recs.at(), recs.lo(), recs.hi(), &wc};
  const zgw::End e1 = zgw::walk_entry<true>(r, w, len, kGuard, e0.nrec);
  if (e1.nrec != e0.nrec || e1.why != e0.why || e1.stop_off != e0.stop_off) bad |= 2u;
  if (wc.kept != e0.nrec) bad |= 4u;                      // the emit pass writes exactly the count pass's number of records
  if (rc.bad) bad |= 8u;
  if (wc.bad) bad |= 16u;
  if (!recs.intact()) bad |= 16u;
  if (e0.stop_off > len || (e0.why == zgw::kEnd && e0.stop_off != len)) bad |= 32u;
  if (e0.nrec > 1) {   // a lane whose range is shorter than its records (a source that changed between the passes) still stays inside it
    lane::Count rc2, wc2;
    std::vector<zgw::Rec> few(e0.nrec - 1 + 2 * kGuard);
    const Writer w2{few.data(), kGuard, kGuard + e0.nrec - 1, &wc2};
    (void)zgw::walk_entry<true>(Reader::over(own, 0, len, &rc2), w2, len, kGuard, e0.nrec - 1);
    if (wc2.bad || rc2.bad || wc2.kept != e0.nrec - 1) bad |= 16u;
  }
  const zgw::Rec* sk = recs.mid();
  BatchBuilder a, b;
  std::vector<FrameInfo> ia, ib;
  bool ok1 = false, ok2 = false;
  const int sa = parse_frames(data, len, max_window, &a, &ia, kBase);
  const int sb = parse_frames_skel(sk, e0.nrec, len, max_window, &b, &ib, kBase, &ok1);
  if (sa != sb) bad |= 64u;
  if (!ok1) bad |= 128u;
  const uint64_t pa = plaintext_bound(data, len), pb = plaintext_bound_skel(sk, e0.nrec, len, &ok2);
  if (pa != pb) bad |= 256u;
  if (!ok2) bad |= 512u;
  if (ia.size() != ib.size()) bad |= 1024u;
  else for (size_t i = 0; i < ia.size(); i++) if (!same_info(ia[i], ib[i])) bad |= 1024u;
  a.finish(); b.finish();
  if (a.blocks.size() != b.blocks.size() || (a.blocks.size() && memcmp(a.blocks.data(), b.blocks.data(), a.blocks.size() * sizeof(ZgBlock)))) bad |= 2048u;
  if (a.frames.size() != b.frames.size() || (a.frames.size() && memcmp(a.frames.data(), b.frames.data(), a.frames.size() * sizeof(ZgFrame)))) bad |= 4096u;
  if (a.lit_bytes != b.lit_bytes || a.seq_count != b.seq_count || a.out_bound != b.out_bound || a.nhuf_slots != b.nhuf_slots) bad |= 8192u;
  // coverage
  g_cases++;
  g_status[sa & 255]++;
  g_why[e0.why & 15]++;
  if (sa == 0) {   // formats are counted in inputs the host's walk accepts from end to end
    for (uint32_t k = 0; k < e0.nrec; k++) {
      const zgw::Rec& x = sk[k];
      if (x.kind != zgw::kBlock || ((x.b[0] >> 1) & 3) != 2 || !x.have) continue;
      g_lit[(x.b[3] & 3) >= 2][(x.b[3] >> 2) & 3]++;
      if (x.have2) g_seq[x.b[8] == 0 ? 0 : x.b[8] < 128 ? 1 : x.b[8] < 255 ? 2 : 3]++;
    }
    for (const FrameInfo& f : ia) g_cksum[f.has_checksum]++;
  }
  return bad;
}
}  // namespace

extern "C" uint32_t wk_check(const uint8_t* data, uint64_t len, uint64_t max_window) { return check(data, len, max_window); }
// every prefix of the first `upto` bytes; returns the first failing length + 1 in *where
extern "C" uint32_t wk_prefixes(const uint8_t* data, uint64_t len, uint64_t upto, uint64_t max_window, uint64_t* where) {
  const uint64_t n = len < upto ? len : upto;
  for (uint64_t k = 0; k <= n; k++) { const uint32_t bad = check(data, k, max_window); if (bad) { *where = k; return bad; } }
  return 0;
}
// single-byte edits at the bytes the host reads: frame headers, block headers, the first 5 body bytes and the 4 at the sequences section
// header of every block, each set to 0x00, 0xFF, one flipped bit and one random value (fixed seed); at most `budget` positions per input,
// evenly spread
extern "C" uint32_t wk_edits(uint8_t* data, uint64_t len, uint64_t max_window, uint64_t seed, uint64_t budget, uint64_t* where, uint64_t* nedits) {
  BatchBuilder bb;
  std::vector<FrameInfo> info;
  (void)parse_frames(data, len, 1ull << 62, &bb, &info, 0);
  std::vector<uint64_t> pos;
  for (const FrameInfo& f : info) for (uint64_t k = 0; k < f.header.header_size + 3u; k++) pos.push_back(f.src_begin + k);
  for (const ZgBlock& b : bb.blocks) {
    if (b.src_off < 3) continue;
    for (uint64_t k = 0; k < 3; k++) pos.push_back(b.src_off - 3 + k);
    if (b.btype != ZG_BT_COMPRESSED) continue;
    for (uint64_t k = 0; k < 5 && k < b.src_len; k++) pos.push_back(b.src_off + k);
    uint32_t at = 0, avail = 0;
    uint8_t head[5] = {0, 0, 0, 0, 0};
    memcpy(head, data + b.src_off, b.src_len < 5 ? b.src_len : 5);
    if (zgw::seq_header_at(head, b.src_len, &at, &avail)) for (uint64_t k = 0; k < avail; k++) pos.push_back(b.src_off + at + k);
  }
  uint64_t x = seed * 6364136223846793005ull + 1442695040888963407ull;
  const uint64_t step = pos.size() > budget ? (pos.size() + budget - 1) / budget : 1;
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
extern "C" void wk_coverage(uint64_t* status, uint64_t* why, uint64_t* lit, uint64_t* seq, uint64_t* cksum, uint64_t* cases) {
  memcpy(status, g_status, sizeof g_status); memcpy(why, g_why, sizeof g_why); memcpy(lit, g_lit, sizeof g_lit);
  memcpy(seq, g_seq, sizeof g_seq); memcpy(cksum, g_cksum, sizeof g_cksum); *cases = g_cases;
}
