// zg_emu_seeksums.cpp — TEST-ONLY: runs the SOURCE of zg_k_seeksums' wave routine (zstd-rs_amd/csrc/zg_seeksums.h: the seek table's Checksum
// fields against the hash kernel's digests, one wave per entry) on the CPU through the SIMT emulator of zg_simt.h, and the host form of the
// same rule (locate_rows + sums_rows) beside it. tests/test_seeksums_cpu.py builds this file (tests/lanesuite.py; it is not in the Makefile's
// library), twice: as a shared library whose readers count every access and every access outside the windows the test allows, and — with
// -DSEEKSUMS_MAIN — as a stand-alone AddressSanitizer program in which every entry, every slice of the frame list and every digest array
// lies in a heap block of exactly its length (zg_lane_mem.h). Both hand every record back; the test compares them with its model. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "../../zstd-rs_amd/csrc/zg_seeksums.h"
#include "zg_lane_mem.h"

namespace {
using Reader = lane::Reader<uint32_t>;   // the entry as the wave may see it: the bytes of up to three windows [lo, hi)
using Direct = lane::Direct<uint32_t>;
struct List {   // the submit's whole frame list and digest array; the wave may see its own slice and the digests that slice names
  lane::Array<const zgv::Frame> fr;   // the slice [lo, lo + n) of the list
  lane::Array<const uint64_t> dig;    // [0, ndig)
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

// one wave over one entry; false if the lanes' records differ. The record is lane 0's, stored as the kernel stores it.
template <class R, class F> bool wave(const R& r, const F& f, uint64_t len, uint32_t first, uint32_t taken, uint32_t nfr, uint32_t ndig, zgv::Sums* out) {
  return lane::wave<zgv::Sums>(64, [&]() { return zgv::seeksums_entry(r, f, len, first, taken, nfr, ndig); }, zgv::seeksums_store,
                               [](const zgv::Sums& a, const zgv::Sums& b) { return memcmp(&a, &b, sizeof a) == 0; }, out);
}

// the host's form of the rule on a host copy of the entry: the footer, then the rows (the table frame's header is not looked at)
zgv::Sums host(const uint8_t* e, uint64_t len, uint32_t first, uint32_t taken, const zgv::Frame* fr, uint32_t nfr, const uint64_t* dig, uint32_t ndig) {
  zgv::Sums z{0, 0, 0, 0, 0, 0, 0, 0};
  if (!taken) return z;
  if (len < zgt::kFraming) { z.why = zgt::kNone; return z; }
  uint32_t es = 8;
  uint64_t rows = 0;
  z.why = zgv::locate_rows(e + len - 9, len, first, taken, &es, &rows);
  if (z.why) return z;
  return zgv::sums_rows(e + rows, es, first, taken, fr, nfr, dig, ndig);
}
}  // namespace

// One case. frames: the submit's whole list (nall records of 16 bytes), the entry's slice is [frame_lo, frame_lo + frame_n); win: nwin x (lo, hi).
// out: the wave's record, then the host function's (32 bytes each); counts: reads of the entry, reads outside the windows, list accesses
// outside the slice, digest reads the slice does not name. Returns 1 if the lanes of the wave disagree.
extern "C" uint32_t zgemu_seeksums(const uint8_t* entry, uint64_t len, uint32_t first, uint32_t taken, const void* frames, uint32_t nall,
                                   uint32_t frame_lo, uint32_t frame_n, const uint64_t* dig, uint32_t ndig, const uint64_t* win, uint32_t nwin,
                                   void* out, uint64_t* counts) {
  (void)nall;
  lane::Count ec, lc, dc;
  zgv::Sums s;
  const zgv::Frame* all = (const zgv::Frame*)frames;
  const List list{{all, frame_lo, (uint64_t)frame_lo + frame_n, &lc}, {dig, 0, ndig, &dc}};
  const bool same = wave(Reader::windows(entry, win, nwin, &ec), list, len, first, taken, frame_n, ndig, &s);
  const zgv::Sums h = host(entry, len, first, taken, all + frame_lo, frame_n, dig, ndig);
  memcpy(out, &s, 32);
  memcpy((uint8_t*)out + 32, &h, 32);
  counts[0] = ec.n; counts[1] = ec.bad; counts[2] = lc.bad; counts[3] = dc.bad;
  return same ? 0u : 1u;
}

#ifdef SEEKSUMS_MAIN
// argv[1]: per case [u64 length][u32 first][u32 taken][u32 frame_n][u32 ndig][frame_n x 16 bytes][ndig x 8 bytes][the entry]; argv[2]: the
// records, wave then host, 64 bytes per case. Entry, slice and digests each lie in a heap block of exactly their length and are read
// directly: an access outside one is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t cases = 0, len;
  uint32_t h[4];
  for (; f.next(&len, 8); cases++) {
    f.read(h, 4, 4);
    zgv::Frame* fr = f.aligned<zgv::Frame>(h[2]);   // (16-byte records)
    uint64_t* dig = (uint64_t*)f.block((uint64_t)h[3] * 8);
    uint8_t* e = f.block(len);
    zgv::Sums s;
    if (!wave(Direct{e}, DirectList{fr, dig}, len, h[0], h[1], h[2], h[3], &s)) return lane::kExitLanes;
    const zgv::Sums hs = host(e, len, h[0], h[1], fr, h[2], dig, h[3]);
    g.write(&s, 32, 1);
    g.write(&hs, 32, 1);
    free(e); free(dig); free(fr);
  }
  f.close();
  g.close();
  printf("seeksums_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
