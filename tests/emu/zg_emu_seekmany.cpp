// zg_emu_seekmany.cpp — TEST-ONLY: runs the SOURCE of the seek-many passes (zstd-rs_amd/csrc/zg_seekmany.h: locate, total, prefix, find) on
// the CPU through the SIMT emulator of zg_simt.h, laid out as Engine::seekmany_pass lays them out: one lane per entry, one wave per chunk, one
// lane per range, the scratch sized from the located row count. tests/test_seekmany_cpu.py builds this file (tests/lanesuite.py; it is not in
// the Makefile's library), twice: as a shared library whose accessors count every access and every access outside the entry's window and
// outside the scratch, and — with -DSEEKMANY_MAIN — as a stand-alone AddressSanitizer program in which every entry and the scratch lie in heap
// blocks of exactly their length (zg_lane_mem.h). Both hand back every record (and the library the prefix sums), and both can run
// zgt::seektab_entry's wave beside every range and compare the two records (the program does for entries below 8 KiB, in its first round).
// The library also exports the host-side grouping of the gather calls (zgm::group_ranges), which needs no emulator. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "../../zstd-rs_amd/csrc/zg_seekmany.h"
#include "zg_lane_mem.h"

namespace {
using Reader = lane::Reader<uint32_t>;   // the entry as the passes may see it: bytes [lo, len)
using Direct = lane::Direct<uint32_t>;
// the scratch under the names the passes use. A: lane::Array<zgm::Pair> over its n pairs (an access outside is counted and dropped), or
// lane::DirectArray<zgm::Pair>
template <class A> struct Pairs {
  A a;
  void ld(uint64_t i, uint64_t* c, uint64_t* d) const { const zgm::Pair x = a.ld(i); *c = x.c; *d = x.d; }
  uint64_t ld_d(uint64_t i) const { return a.ld(i).d; }
  void st(uint64_t i, uint64_t c, uint64_t d) const { a.st(i, zgm::Pair{c, d}); }
};
using DirectPairs = Pairs<lane::DirectArray<zgm::Pair>>;

// One entry, n ranges, the four passes as the engine runs them. MakeR(base) / MakeS(pairs, count): the accessors. out: n records as find's
// lanes stored them; *loc: what locate stored; scratch: the block the passes used (prefixes, then chunk totals). Returns the number of ranges
// whose record differs from the one zg_k_seektab's wave gives (read directly; compare: whether to look), or UINT32_MAX if the scratch cannot be had.
template <uint32_t CH, class R, class MakeS>
uint32_t passes(const R& r, const uint8_t* entry, uint64_t len, const uint64_t* ranges, uint32_t n, zgk::Seek* out, zgm::Loc* loc,
                std::vector<zgm::Pair*>* keep, MakeS make_s, uint64_t* npairs, bool compare) {
  alignas(16) static zgm::Loc stored_loc;
  memset(&stored_loc, lane::kFill, sizeof stored_loc);
  memset(loc, 0, sizeof *loc);
  *npairs = 0;
  bool live = false;
  for (uint32_t i = 0; i < n; i++) live = live || ranges[2 * i + 1] != 0;
  zgm::Pair* pairs = nullptr;
  uint64_t pre_pairs = 0, total_pairs = 0;
  if (live) {   // (an entry that no range of nonzero length names is not read)
    simt::run(1, [&]() { zgm::seekmany_store_loc(&stored_loc, zgm::seekmany_locate(r, len)); });
    *loc = stored_loc;
    if (!loc->why) {
      const uint32_t nq = zgm::chunks_of(loc->nf, CH);
      pre_pairs = (uint64_t)loc->nf + 1;
      total_pairs = pre_pairs + nq;
      pairs = (zgm::Pair*)malloc((size_t)total_pairs * sizeof(zgm::Pair));   // exactly: a store behind it is an AddressSanitizer report
      if (!pairs) return UINT32_MAX;
      memset(pairs, lane::kFill, (size_t)total_pairs * sizeof(zgm::Pair));
      keep->push_back(pairs);
      const auto s = make_s(pairs, total_pairs);
      for (int pass = 0; pass < 2; pass++)
        for (uint32_t q = 0; q < nq; q++) {
          const zgm::Work w{0, loc->tab + 8, 0, pre_pairs, loc->nf, loc->es, q, nq};
          simt::run(64, [&]() { if (pass == 0) zgm::seekmany_total<CH>(r, s, w); else zgm::seekmany_prefix<CH>(r, s, w); });
        }
    }
  }
  *npairs = pre_pairs;
  const auto s = make_s(pairs, total_pairs);
  std::vector<zgk::Seek> stored(n + 1);
  if ((uintptr_t)stored.data() % 16) return UINT32_MAX;   // (the records leave as 16-byte stores; the heap aligns to 16: never)
  for (uint32_t base = 0; base < n; base += 64) {
    const uint32_t cnt = n - base < 64 ? n - base : 64;
    simt::run(64, [&]() {
      const uint32_t j = base + zx_tid();
      if (zx_tid() >= cnt) return;
      const uint64_t rlen = ranges[2 * j + 1];
      const zgm::Find f{ranges[2 * j], rlen, 0, loc->tab, loc->why ? 0u : loc->nf, rlen ? loc->why : 0u, 0, 0};
      zgt::seektab_store(&stored[j], zgm::seekmany_find(s, f));
    });
  }
  uint32_t differ = 0;
  for (uint32_t j = 0; j < n; j++) {
    out[j] = stored[j];
    if (!compare) continue;
    zgk::Seek ref;
    simt::run(64, [&]() { const zgk::Seek o = zgt::seektab_entry(Direct{entry}, len, ranges[2 * j], ranges[2 * j + 1]); if (zx_tid() == 0) ref = o; });
    if (!lane::same_seek(ref, out[j])) differ++;
  }
  return differ;
}
}  // namespace

// ranges: n x (begin, rlen); chunk: 128 or zgm::kChunkRows; out: n records; counts: reads of the entry, those outside [lo, len), accesses of
// the scratch, those outside it; meta: why, nframes, es, pairs of prefixes; prefix: room for cap pairs, gets the prefixes C[k], D[k].
// compare != 0: returns how many records differ from zg_k_seektab's wave, else 0 (UINT32_MAX: a chunk size that is not built, or no memory).
extern "C" uint32_t zgemu_seekmany(const uint8_t* entry, uint64_t len, uint64_t lo, const uint64_t* ranges, uint32_t n, uint32_t chunk, uint32_t compare, void* out,
                                   uint64_t* counts, uint64_t* meta, uint64_t* prefix, uint64_t cap) {
  lane::Count rc, pc;
  zgm::Loc loc;
  std::vector<zgm::Pair*> keep;
  std::vector<zgk::Seek> recs(n ? n : 1);
  uint64_t npairs = 0;
  const Reader r = Reader::over(entry, lo, len, &rc);
  auto make_s = [&](zgm::Pair* p, uint64_t np) { return Pairs<lane::Array<zgm::Pair>>{{p, 0, np, &pc}}; };
  uint32_t differ;
  if (chunk == 128) differ = passes<128>(r, entry, len, ranges, n, recs.data(), &loc, &keep, make_s, &npairs, compare != 0);
  else if (chunk == zgm::kChunkRows) differ = passes<zgm::kChunkRows>(r, entry, len, ranges, n, recs.data(), &loc, &keep, make_s, &npairs, compare != 0);
  else return UINT32_MAX;
  memcpy(out, recs.data(), 64 * (size_t)n);
  counts[0] = rc.n; counts[1] = rc.bad; counts[2] = pc.n; counts[3] = pc.bad;
  meta[0] = loc.why; meta[1] = loc.nf; meta[2] = loc.es; meta[3] = npairs;
  for (uint64_t i = 0; i < npairs && i < cap && !keep.empty(); i++) { prefix[2 * i] = keep[0][i].c; prefix[2 * i + 1] = keep[0][i].d; }
  for (zgm::Pair* p : keep) free(p);
  return differ;
}
extern "C" uint32_t zgemu_seekmany_chunk_rows() { return zgm::kChunkRows; }

// The grouping of a gather call (zgm::group_ranges: host arithmetic, the header alone). in: m x (entry, begin, len, refused, status,
// frames_skipped, frames_taken, src_lo, src_hi, plain_lo, plain_seen). groups: room for m x (entry, gfirst, glast, c_lo, c_hi, d_lo, d_hi); group_of, clip_of: m slots; order, skip:
// m slots (one per clip); first: m + 1 slots. Returns the number of groups; counts[0]: the number of clips.
extern "C" uint32_t zgemu_group_ranges(const uint64_t* in, uint32_t m, uint64_t* groups, uint32_t* group_of, uint32_t* clip_of, uint32_t* order,
                                       uint32_t* first, uint64_t* skip, uint64_t* counts) {
  struct Range { uint64_t begin, len; uint32_t entry; };
  std::vector<Range> rg(m);
  std::vector<zgk::Seek> recs(m);
  std::vector<uint8_t> refused(m);
  for (uint32_t j = 0; j < m; j++) {
    const uint64_t* r = in + 11 * (size_t)j;
    rg[j] = Range{r[1], r[2], (uint32_t)r[0]};
    refused[j] = r[3] != 0;
    recs[j] = zgk::Seek{r[7], r[8], r[9], 0, r[10], (uint32_t)r[4], (uint32_t)r[5], (uint32_t)r[6], 0, 0, 0};
  }
  const zgm::Groups g = zgm::group_ranges(rg.data(), recs.data(), refused.data(), m);
  for (size_t k = 0; k < g.groups.size(); k++) {
    const zgm::Group& x = g.groups[k];
    const uint64_t row[7] = {x.entry, x.gfirst, x.glast, x.c_lo, x.c_hi, x.d_lo, x.d_hi};
    memcpy(groups + 7 * k, row, sizeof row);
  }
  for (uint32_t j = 0; j < m; j++) { group_of[j] = g.group_of[j]; clip_of[j] = g.clip_of[j]; }
  for (size_t q = 0; q < g.order.size(); q++) { order[q] = g.order[q]; skip[q] = g.skip[q]; }
  for (size_t k = 0; k < g.first.size(); k++) first[k] = g.first[k];
  counts[0] = g.order.size();
  return (uint32_t)g.groups.size();
}

#ifdef SEEKMANY_MAIN
// argv[1]: per entry [u64 length][u64 n][n x (u64 begin, u64 rlen)][bytes]; argv[2]: the records, 64 bytes each, in that order, once per chunk
// size (128, then the product's). Every entry lies in a heap block of exactly its length, the scratch in one of exactly its size, and both are
// accessed directly: an access outside either is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t entries = 0, runs = 0;
  for (int round = 0; round < 2; round++) {
    lane::CaseFile f(argv[1], "rb");
    uint64_t hdr[2];
    for (; f.next(hdr, 16); entries++) {
      std::vector<uint64_t> rg(2 * hdr[1] + 1);
      f.read(rg.data(), 16, hdr[1]);
      uint8_t* e = f.block(hdr[0]);
      std::vector<zgk::Seek> recs(hdr[1] ? hdr[1] : 1);
      std::vector<zgm::Pair*> keep;
      zgm::Loc loc;
      uint64_t npairs = 0;
      auto make_s = [&](zgm::Pair* p, uint64_t) { return DirectPairs{{p}}; };
      const uint32_t differ = round == 0 ? passes<128>(Direct{e}, e, hdr[0], rg.data(), (uint32_t)hdr[1], recs.data(), &loc, &keep, make_s, &npairs, hdr[0] < 8192)
                                         : passes<zgm::kChunkRows>(Direct{e}, e, hdr[0], rg.data(), (uint32_t)hdr[1], recs.data(), &loc, &keep, make_s, &npairs, false);
      if (differ) { fprintf(stderr, "seekmany_asan: %u records differ from zg_k_seektab's\n", differ); return lane::kExitLanes; }
      g.write(recs.data(), 64, hdr[1]);
      runs += hdr[1];
      for (zgm::Pair* p : keep) free(p);
      free(e);
    }
    f.close();
  }
  g.close();
  printf("seekmany_asan ok: %llu entries, %llu runs\n", (unsigned long long)entries, (unsigned long long)runs);
  return 0;
}
#endif
