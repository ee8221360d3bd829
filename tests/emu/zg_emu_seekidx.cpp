// zg_emu_seekidx.cpp — TEST-ONLY: runs the SOURCE of a declared-kind seek index (zstd-rs_amd/csrc/zg_seekidx.h: the rows routine; zg_index.h:
// the summary pass; zg_seekmany.h: the find pass) on the CPU through the SIMT emulator of zg_simt.h, laid out as zgpu_seek_index_create_device
// and zgpu_frames_seek_indexed_device lay them out: one lane per entry in waves of 64, the host's decision between the passes, the pairs sized
// from the summaries, one lane per range. tests/test_seekidx_cpu.py builds this file (tests/lanesuite.py; it is not in the Makefile's library),
// twice: as a shared library whose accessors count every read outside [0, len), every read of a block body, every pair store outside the
// lane's own range [pre, pre + limit] and every pair load outside the entry's pairs, and — with -DSEEKIDX_MAIN — as a stand-alone
// AddressSanitizer program in which every entry and the pairs lie in heap blocks of exactly their size (zg_lane_mem.h). Both hand back every
// record, and zgk::seek_entry's record for the same range (anchor 0) beside it. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "../../zstd-rs_amd/csrc/zg_seekmany.h"
#include "../../zstd-rs_amd/csrc/zg_seekidx.h"
#include "zg_lane_mem.h"

namespace {
using Reader = lane::Reader<uint8_t>;   // the entry as a lane may see it: bytes [0, len), and none that belongs to a block body
using Direct = lane::Direct<uint8_t>;
// the pairs under the names the passes use. A: lane::Array<zgm::Pair> over the pairs lane i may write, [pre, pre + limit], or over the pairs
// find may read, those of the call (an access outside is counted and dropped), or lane::DirectArray<zgm::Pair>
template <class A> struct Pairs {
  A a;
  void ld(uint64_t i, uint64_t* c, uint64_t* d) const { const zgm::Pair x = a.ld(i); *c = x.c; *d = x.d; }
  uint64_t ld_d(uint64_t i) const { return a.ld(i).d; }
  void st(uint64_t i, uint64_t c, uint64_t d) const { a.st(i, zgm::Pair{c, d}); }
};
using CountedPairs = Pairs<lane::Array<zgm::Pair>>;
using DirectPairs = Pairs<lane::DirectArray<zgm::Pair>>;
struct NoRecs { void put(uint64_t, const zgi::FrameRec&) const {} };
using WalkWriter = lane::DirectArray<zgw::Rec>;

// body[off] != 0: byte off of the entry belongs to a block body (from zgw::walk_entry's records: existing code, not the routine under test)
std::vector<uint8_t> bodies(const uint8_t* data, uint64_t len) {
  const Direct nr{data};
  const zgw::End w0 = zgw::walk_entry<false>(nr, WalkWriter{nullptr}, len, 0, 0);
  std::vector<zgw::Rec> wrecs(w0.nrec + 1);
  (void)zgw::walk_entry<true>(nr, WalkWriter{wrecs.data()}, len, 0, w0.nrec);
  std::vector<uint8_t> body(len + 1, 0);
  for (uint32_t k = 0; k < w0.nrec; k++) {
    const zgw::Rec& x = wrecs[k];
    if (x.kind != zgw::kBlock) continue;
    const uint32_t type = (x.b[0] >> 1) & 3u, size = (uint32_t)(x.b[0] >> 3) | ((uint32_t)x.b[1] << 5) | ((uint32_t)x.b[2] << 13);
    if (type == 3 || size > zgw::kBlockMax) continue;
    const uint64_t n = type == 1 ? 1 : size;
    for (uint64_t q = x.off; q < x.off + n && q < len; q++) body[q] = 1;
  }
  return body;
}

// what the build leaves of one entry: refusal = the why the host refused it with after the summary pass (0: it got a lane in the rows pass);
// ok = the host accepted the rows; pre / limit = the pair range the lane was handed
struct Built { uint32_t refusal = 0, ok = 0; uint64_t pre = 0, limit = 0, len = 0; zgx::Rows rows{}; };

// One launch of n entries and m ranges (entry, begin, rlen) as the engine lays it out. cut: the entry whose row limit is one smaller than the
// chain yields (the input changed between the passes), or -1. MakeR(i): entry i's reader; MakeSt(pairs, lo, hi) / MakeLd(pairs, n): the pair
// accessors. *pairs_out: the block the rows pass wrote, *npairs its pairs (the caller frees it). out[j]: range j's record as find's lane
// stored it — zeros for a range whose entry has no accepted index. Returns false if the memory cannot be had.
template <class MakeR, class MakeSt, class MakeLd>
bool launch(const uint64_t* lens, uint32_t n, int64_t cut, const uint64_t* ranges, uint32_t m, MakeR make_r, MakeSt make_st, MakeLd make_ld,
            std::vector<Built>* built, zgm::Pair** pairs_out, uint64_t* npairs, zgk::Seek* out) {
  // summary pass: zg_k_index<false>, one lane per entry
  std::vector<zgi::Entry> sum(n);
  for (uint32_t base = 0; base < n; base += 64)
    simt::run(64, [&]() {
      const uint32_t i = base + zx_tid();
      if (i >= n) return;
      sum[i] = zgi::index_entry<false>(make_r(i), NoRecs{}, lens[i], 0, 0);
    });
  // the host between the passes
  built->assign(n, Built{});
  std::vector<uint32_t> live;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    Built& b = (*built)[i];
    b.len = lens[i];
    b.refusal = zgx::refusal(sum[i]);
    if (!b.refusal && sum[i].nrec > zgt::kMaxFrames) b.refusal = zgt::kTooLarge;
    if (b.refusal) continue;
    b.limit = sum[i].nrec - ((int64_t)i == cut && sum[i].nrec ? 1u : 0u);
    b.pre = total;
    total += b.limit + 1;
    live.push_back(i);
  }
  zgm::Pair* pairs = (zgm::Pair*)malloc(total ? (size_t)total * sizeof(zgm::Pair) : 1);   // exactly: a store behind it is an AddressSanitizer report
  if (!pairs) return false;
  memset(pairs, lane::kFill, (size_t)total * sizeof(zgm::Pair));
  *pairs_out = pairs; *npairs = total;
  // rows pass: zg_k_seekidx_rows, one lane per entry the host accepted
  const uint32_t nl = (uint32_t)live.size();
  for (uint32_t base = 0; base < nl; base += 64)
    simt::run(64, [&]() {
      const uint32_t q = base + zx_tid();
      if (q >= nl) return;
      Built& b = (*built)[live[q]];
      b.rows = zgx::seekidx_rows(make_r(live[q]), make_st(pairs, b.pre, b.pre + b.limit), b.len, b.pre, b.limit);
    });
  for (uint32_t i : live) {
    Built& b = (*built)[i];
    b.ok = !b.rows.why && b.rows.nrows == b.limit && b.rows.c == b.len;   // (the host's check: zgpu_seek_index_create_device)
  }
  // find pass: zg_k_seekmany_find, one lane per range
  std::vector<zgk::Seek> stored(m + 1);
  if ((uintptr_t)stored.data() % 16) return false;   // (the records leave as 16-byte stores; the heap aligns to 16: never)
  memset(stored.data(), 0, (m + 1) * sizeof(zgk::Seek));
  const auto s = make_ld(pairs, total);
  for (uint32_t base = 0; base < m; base += 64)
    simt::run(64, [&]() {
      const uint32_t j = base + zx_tid();
      if (j >= m) return;
      const uint64_t e = ranges[3 * j];
      if (e >= n || !(*built)[e].ok) return;
      const Built& b = (*built)[e];
      const zgm::Find f{ranges[3 * j + 1], ranges[3 * j + 2], b.pre, b.len, (uint32_t)b.limit, 0, 0, 0};
      zgt::seektab_store(&stored[j], zgm::seekmany_find(s, f));
    });
  for (uint32_t j = 0; j < m; j++) out[j] = stored[j];
  return true;
}

bool five_same(const zgk::Seek& a, const zgk::Seek& b) {
  return a.src_lo == b.src_lo && a.src_hi == b.src_hi && a.plain_lo == b.plain_lo && a.plain_seen == b.plain_seen &&
         (a.flags & zgk::kNothing) == (b.flags & zgk::kNothing);
}
}  // namespace

// entries[i] / lens[i]: n entries; cut: see launch; ranges: m x (entry, begin, rlen); out: m records; counts: reads outside [0, len), reads of
// a block body, pair stores outside the lane's range, pair loads outside the pairs, pair stores in all; meta: per entry (refusal, accepted,
// nrows the lane counted, pre, limit, C[nrows], D[nrows], the lane's why); pairs: room for cap pairs, gets the block as the rows pass left it
// (*npairs of them). Returns how many records of accepted entries differ from zgk::seek_entry's (anchor 0) in src_lo, src_hi, plain_lo,
// plain_seen and flag bit 2; UINT32_MAX: no memory.
extern "C" uint32_t zgemu_seekidx(const uint8_t* const* entries, const uint64_t* lens, uint32_t n, int64_t cut, const uint64_t* ranges, uint32_t m,
                                  void* out, uint64_t* counts, uint64_t* meta, uint64_t* pairs, uint64_t cap, uint64_t* npairs) {
  lane::Count rc, sc, lc;   // reads of the entries, pair stores of the rows pass, pair loads of the find pass
  std::vector<std::vector<uint8_t>> body(n);
  for (uint32_t i = 0; i < n; i++) body[i] = bodies(entries[i], lens[i]);
  std::vector<Built> built;
  std::vector<zgk::Seek> recs(m ? m : 1);
  zgm::Pair* block = nullptr;
  if (!launch(lens, n, cut, ranges, m, [&](uint32_t i) { return Reader::over(entries[i], 0, lens[i], &rc, body[i].data()); },
              [&](zgm::Pair* p, uint64_t lo, uint64_t hi) { return CountedPairs{{p, lo, hi + 1, &sc}}; },
              [&](zgm::Pair* p, uint64_t np) { return CountedPairs{{p, 0, np, &lc}}; }, &built, &block, npairs, recs.data()))
    return UINT32_MAX;
  uint32_t differ = 0;
  for (uint32_t j = 0; j < m; j++) {
    const uint64_t e = ranges[3 * j];
    if (e >= n || !built[e].ok) continue;
    const zgk::Seek ref = zgk::seek_entry(Direct{entries[e]}, lens[e], ranges[3 * j + 1], ranges[3 * j + 2], 0, 0);
    if (!five_same(ref, recs[j])) differ++;
  }
  memcpy(out, recs.data(), 64 * (size_t)m);
  counts[0] = rc.bad; counts[1] = rc.forbidden; counts[2] = sc.bad; counts[3] = lc.bad; counts[4] = sc.n;
  for (uint32_t i = 0; i < n; i++) {
    const Built& b = built[i];
    uint64_t* o = meta + 8 * (size_t)i;
    o[0] = b.refusal; o[1] = b.ok; o[2] = b.rows.nrows; o[3] = b.pre; o[4] = b.limit; o[5] = b.rows.c; o[6] = b.rows.d; o[7] = b.rows.why;
  }
  for (uint64_t i = 0; i < *npairs && i < cap; i++) { pairs[2 * i] = block[i].c; pairs[2 * i + 1] = block[i].d; }
  free(block);
  return differ;
}

#ifdef SEEKIDX_MAIN
// argv[1]: per launch [u64 n][u64 m][i64 cut][n x u64 length][m x (u64 entry, u64 begin, u64 rlen)][the entries' bytes]; argv[2]: per launch
// the m records, 64 bytes each, then per entry (u64 accepted, u64 nrows). Every entry lies in a heap block of exactly its length, the pairs in
// one of exactly their size, and both are accessed directly: an access outside either is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t launches = 0, runs = 0, hdr[3];
  for (; f.next(hdr, 24); launches++) {
    const uint32_t n = (uint32_t)hdr[0], m = (uint32_t)hdr[1];
    std::vector<uint64_t> lens(n + 1), rg(3 * (size_t)m + 1);
    f.read(lens.data(), 8, n);
    f.read(rg.data(), 24, m);
    std::vector<uint8_t*> e(n + 1, nullptr);
    for (uint32_t i = 0; i < n; i++) e[i] = f.block(lens[i]);
    std::vector<Built> built;
    std::vector<zgk::Seek> recs(m ? m : 1);
    zgm::Pair* block = nullptr;
    uint64_t npairs = 0;
    if (!launch(lens.data(), n, (int64_t)hdr[2], rg.data(), m, [&](uint32_t i) { return Direct{e[i]}; },
                [&](zgm::Pair* p, uint64_t, uint64_t) { return DirectPairs{{p}}; }, [&](zgm::Pair* p, uint64_t) { return DirectPairs{{p}}; }, &built,
                &block, &npairs, recs.data()))
      return lane::kExitIO;
    g.write(recs.data(), 64, m);
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t o[2] = {built[i].ok, built[i].rows.nrows};
      g.write(o, 8, 2);
    }
    runs += m;
    free(block);
    for (uint8_t* p : e) free(p);
  }
  f.close();
  g.close();
  printf("seekidx_asan ok: %llu launches, %llu ranges\n", (unsigned long long)launches, (unsigned long long)runs);
  return 0;
}
#endif
