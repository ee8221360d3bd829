// zg_emu_idxsums.cpp — TEST-ONLY: runs the SOURCE of zg_k_idxsums' wave routine (zstd-rs_amd/csrc/zg_idxsums.h: the sums a seek index handle holds
// against the hash kernel's digests, one wave per group) on the CPU through the SIMT emulator of zg_simt.h, and the host form of the same
// rule (sums_pairs) beside it. tests/test_idxsums_cpu.py builds this file (tests/lanesuite.py; it is not in the Makefile's library), twice:
// as a shared library whose readers count every access and every access outside the windows the test allows, and — with -DIDXSUMS_MAIN — as a
// stand-alone AddressSanitizer program in which the pairs and sums the wave may read, the slice of the frame list and the digest array each
// lie in a heap block of exactly their length (zg_lane_mem.h). Both hand every record back; the test compares them with its model. Not part
// of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "../../zstd-rs_amd/csrc/zg_seeksums.h"
#include "../../zstd-rs_amd/csrc/zg_idxsums.h"
#include "zg_lane_mem.h"

namespace {
struct Pair { uint64_t c, d; };
// the handle's two arrays as the wave may see them: pairs [lo, hi) and sums [lo, hi) of the WHOLE arrays; the entry's row 0 lies at pair0 / sum0
struct Rows {
  lane::Array<const Pair> pairs;
  lane::Array<const uint32_t> sums;
  uint64_t pair0, sum0;
  uint64_t c(uint64_t k) const { return pairs.ld(pair0 + k).c; }
  uint32_t sum(uint64_t k) const { return sums.ld(sum0 + k); }
};
// blocks that begin at the group's first row
struct DirectRows {
  const Pair* pairs; const uint32_t* sums; uint64_t first;
  uint64_t c(uint64_t k) const { return pairs[k - first].c; }
  uint32_t sum(uint64_t k) const { return sums[k - first]; }
};
struct List {   // the submit's whole frame list and digest array; the wave may see its own slice and the digests that slice names
  lane::Array<const zgv::Frame> fr;
  lane::Array<const uint64_t> dig;
  bool named(uint32_t slot) const { for (uint64_t i = fr.lo; i < fr.hi; i++) if (fr.p[i].slot == slot) return true; return false; }
  uint64_t begin(uint32_t i) const { return fr.ld(fr.lo + i).begin; }
  void frame(uint32_t i, uint64_t* b, uint32_t* cl, uint32_t* slot) const {
    *b = 0; *cl = 0; *slot = zgv::kNotHashed;
    if (!fr.ok(fr.lo + i)) return;
    *b = fr.p[fr.lo + i].begin; *cl = fr.p[fr.lo + i].clen; *slot = fr.p[fr.lo + i].slot;
  }
  uint32_t digest(uint32_t slot) const { if (!named(slot)) { dig.c->n++; dig.c->bad++; return 0; } return (uint32_t)dig.ld(slot); }
};
struct DirectList {
  const zgv::Frame* fr; const uint64_t* dig;
  uint64_t begin(uint32_t i) const { return fr[i].begin; }
  void frame(uint32_t i, uint64_t* b, uint32_t* cl, uint32_t* slot) const { *b = fr[i].begin; *cl = fr[i].clen; *slot = fr[i].slot; }
  uint32_t digest(uint32_t slot) const { uint32_t v; memcpy(&v, &dig[slot], 4); return v; }
};

// one wave over one group; false if the lanes' records differ. The record is lane 0's, stored as the kernel stores it.
template <class P, class F> bool wave(const P& p, const F& f, uint32_t nrows, uint32_t first, uint32_t taken, uint32_t nfr, uint32_t ndig, zgv::Sums* out) {
  return lane::wave<zgv::Sums>(64, [&]() { return zgh::idxsums_group(p, f, nrows, first, taken, nfr, ndig); }, zgv::seeksums_store,
                               [](const zgv::Sums& a, const zgv::Sums& b) { return memcmp(&a, &b, sizeof a) == 0; }, out);
}

// the host's form of the rule: rows[0 .. taken] are the pairs of rows [first, first + taken], sums[0 .. taken) their sums (neither is looked
// at where the group leaves the entry)
zgv::Sums host(const Pair* rows, const uint32_t* sums, uint32_t nrows, uint32_t first, uint32_t taken, const zgv::Frame* fr, uint32_t nfr,
               const uint64_t* dig, uint32_t ndig) {
  std::vector<uint64_t> c;
  if (taken && (uint64_t)first + taken <= nrows) for (uint32_t k = 0; k <= taken; k++) c.push_back(rows[k].c);
  return zgh::sums_pairs(c.data(), sums, nrows, first, taken, fr, nfr, dig, ndig);
}
}  // namespace

// One case. pairs / sums: the handle's whole arrays (npairs x 16 bytes, nsums x 4 bytes), the entry's row 0 at pair0 / sum0; frames: the
// submit's whole list, the group's slice is [frame_lo, frame_lo + frame_n); win: (pairs lo, hi, sums lo, hi), indices into the whole arrays.
// out: the wave's record, then the host function's (32 bytes each); counts: accesses to pairs and sums together, pair accesses outside the
// window, sum accesses outside, list accesses outside the slice, digest reads the slice does not name. Returns 1 if the lanes disagree.
extern "C" uint32_t zgemu_idxsums(const void* pairs, const uint32_t* sums, uint64_t pair0, uint64_t sum0, uint32_t nrows, uint32_t first, uint32_t taken,
                                  const void* frames, uint32_t frame_lo, uint32_t frame_n, const uint64_t* dig, uint32_t ndig, const uint64_t* win,
                                  void* out, uint64_t* counts) {
  lane::Count pc, sc, lc, dc;
  zgv::Sums s;
  const Pair* all_pairs = (const Pair*)pairs;
  const zgv::Frame* all = (const zgv::Frame*)frames;
  const List list{{all, frame_lo, (uint64_t)frame_lo + frame_n, &lc}, {dig, 0, ndig, &dc}};
  const Rows rows{{all_pairs, win[0], win[1], &pc}, {sums, win[2], win[3], &sc}, pair0, sum0};
  const bool same = wave(rows, list, nrows, first, taken, frame_n, ndig, &s);
  const zgv::Sums h = host(all_pairs + pair0 + first, sums + sum0 + first, nrows, first, taken, all + frame_lo, frame_n, dig, ndig);
  memcpy(out, &s, 32);
  memcpy((uint8_t*)out + 32, &h, 32);
  counts[0] = pc.n + sc.n; counts[1] = pc.bad; counts[2] = sc.bad; counts[3] = lc.bad; counts[4] = dc.bad;
  return same ? 0u : 1u;
}

#ifdef IDXSUMS_MAIN
// argv[1]: per case [u32 nrows][u32 first][u32 taken][u32 frame_n][u32 ndig][u32 held] [frame_n x 16 bytes][ndig x 8 bytes] and, if held,
// [(taken + 1) x 16 bytes: the pairs of rows first .. first + taken][taken x 4 bytes: their sums]; argv[2]: the records, wave then host, 64
// bytes per case. Pairs, sums, slice and digests each lie in a heap block of exactly their length and are read directly: an access outside
// one is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t cases = 0;
  uint32_t h[6];
  for (; f.next(h, sizeof h); cases++) {
    zgv::Frame* fr = f.aligned<zgv::Frame>(h[3]);   // (16-byte records)
    uint64_t* dig = (uint64_t*)f.block((uint64_t)h[4] * 8);
    Pair* rows = f.aligned<Pair>(h[5] ? (size_t)h[2] + 1 : 0);
    uint32_t* sums = (uint32_t*)f.block(h[5] ? (uint64_t)h[2] * 4 : 0);
    zgv::Sums s;
    if (!wave(DirectRows{rows, sums, h[1]}, DirectList{fr, dig}, h[0], h[1], h[2], h[3], h[4], &s)) return lane::kExitLanes;
    const zgv::Sums hs = host(rows, sums, h[0], h[1], h[2], fr, h[3], dig, h[4]);
    g.write(&s, 32, 1);
    g.write(&hs, 32, 1);
    free(sums); free(rows); free(dig); free(fr);
  }
  f.close();
  g.close();
  printf("idxsums_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
