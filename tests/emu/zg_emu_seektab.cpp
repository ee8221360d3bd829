// zg_emu_seektab.cpp — TEST-ONLY: runs the SOURCE of zg_k_seektab's wave routine (zstd-rs_amd/csrc/zg_seektab.h: the seekable format's seek
// table, one wave per entry, prefix sums and ballots) on the CPU through the SIMT emulator of zg_simt.h. tests/test_seektab_cpu.py builds this
// file (tests/lanesuite.py; it is not in the Makefile's library), twice: as a shared library whose reader counts every access and every access
// outside the window the test allows, and — with -DSEEKTAB_MAIN — as a stand-alone AddressSanitizer program that reads entries lying in heap
// blocks of exactly their length (zg_lane_mem.h). Both hand every record back; the test compares them with its model. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "zg_lane_mem.h"

namespace {
using Reader = lane::Reader<uint32_t>;   // the entry as the wave may see it: bytes [lo, len)
using Direct = lane::Direct<uint32_t>;

// one wave over one entry and one range; false if the lanes' records differ. The record is lane 0's, stored as the kernel stores it.
template <class R> bool wave(const R& r, uint64_t len, uint64_t begin, uint64_t rlen, zgk::Seek* out) {
  return lane::wave<zgk::Seek>(64, [&]() { return zgt::seektab_entry(r, len, begin, rlen); }, zgt::seektab_store, lane::same_seek<zgk::Seek>, out);
}
}  // namespace

// ranges: n x (begin, rlen); out: n records; counts: n x (reads, reads outside [lo, len)). Returns how many cases had lanes that disagree.
extern "C" uint32_t zgemu_seektab(const uint8_t* entry, uint64_t len, uint64_t lo, const uint64_t* ranges, uint32_t n, void* out, uint64_t* counts) {
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n; i++) {
    lane::Count c;
    zgk::Seek s;
    if (!wave(Reader::over(entry, lo, len, &c), len, ranges[2 * i], ranges[2 * i + 1], &s)) bad++;
    memcpy((uint8_t*)out + 64 * (size_t)i, &s, 64);
    counts[2 * i] = c.n; counts[2 * i + 1] = c.bad;
  }
  return bad;
}

#ifdef SEEKTAB_MAIN
// argv[1]: per entry [u64 length][u64 n][n x (u64 begin, u64 rlen)][bytes]; argv[2]: the records, 64 bytes each, in that order. Every entry
// lies in a heap block of exactly its length and is read directly: an access outside it is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t entries = 0, runs = 0, hdr[2];
  for (; f.next(hdr, 16); entries++) {
    std::vector<uint64_t> rg(2 * hdr[1] + 1);
    f.read(rg.data(), 16, hdr[1]);
    uint8_t* e = f.block(hdr[0]);
    for (uint64_t i = 0; i < hdr[1]; i++, runs++) {
      zgk::Seek s;
      if (!wave(Direct{e}, hdr[0], rg[2 * i], rg[2 * i + 1], &s)) return lane::kExitLanes;
      g.write(&s, 64, 1);
    }
    free(e);
  }
  f.close();
  g.close();
  printf("seektab_asan ok: %llu entries, %llu runs\n", (unsigned long long)entries, (unsigned long long)runs);
  return 0;
}
#endif
