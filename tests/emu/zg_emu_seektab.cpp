// zg_emu_seektab.cpp — TEST-ONLY: runs the SOURCE of zg_k_seektab's wave routine (zstd-rs_amd/csrc/zg_seektab.h: the seekable format's seek
// table, one wave per entry, prefix sums and ballots) on the CPU through the SIMT emulator of zg_simt.h. tests/test_seektab_cpu.py builds this
// file itself (it is not in the Makefile's library), twice: as a shared library whose reader counts every access and every access outside the
// window the test allows, and — with -DSEEKTAB_MAIN — as a stand-alone AddressSanitizer program that reads entries lying in heap blocks of
// exactly their length. Both hand every record back; the test compares them with its model. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"

namespace {
struct Count { uint64_t reads = 0, bad = 0; };
struct Reader {   // the entry as the wave may see it: bytes [lo, len)
  const uint8_t* p; uint64_t lo, len; Count* c;
  bool ok(uint64_t off, uint64_t n) const { c->reads++; if (off < lo || off > len || n > len - off) { c->bad++; return false; } return true; }
  uint32_t ld1(uint64_t off) const { return ok(off, 1) ? p[off] : 0u; }
  uint32_t ld4(uint64_t off) const { uint32_t v = 0; if (ok(off, 4)) memcpy(&v, p + off, 4); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { *a = *b = 0; if (ok(off, 8)) { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); } }
};
struct Direct {   // no checks: what the kernel's reader does
  const uint8_t* p;
  uint32_t ld1(uint64_t off) const { return p[off]; }
  uint32_t ld4(uint64_t off) const { uint32_t v; memcpy(&v, p + off, 4); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); }
};

// one wave over one entry and one range; false if the lanes' records differ. The record is lane 0's, stored as the kernel stores it.
template <class R> bool wave(const R& r, uint64_t len, uint64_t begin, uint64_t rlen, zgk::Seek* out) {
  static zgk::Seek all[64];
  alignas(16) static zgk::Seek stored;
  memset(&stored, 0xEE, sizeof stored);
  simt::run(64, [&]() {
    const zgk::Seek o = zgt::seektab_entry(r, len, begin, rlen);
    memcpy(&all[zx_tid()], &o, sizeof o);
    if (zx_tid() == 0) zgt::seektab_store(&stored, o);
  });
  bool same = true;
  for (int l = 0; l < 64; l++) {
    const zgk::Seek& a = all[l], & b = all[0];
    same = same && a.src_lo == b.src_lo && a.src_hi == b.src_hi && a.plain_lo == b.plain_lo && a.bound == b.bound && a.plain_seen == b.plain_seen &&
           a.status == b.status && a.frames_skipped == b.frames_skipped && a.frames_taken == b.frames_taken && a.nblocks == b.nblocks &&
           a.why == b.why && a.flags == b.flags;
  }
  memcpy(out, &stored, sizeof stored);
  return same;
}
}  // namespace

// ranges: n x (begin, rlen); out: n records; counts: n x (reads, reads outside [lo, len)). Returns how many cases had lanes that disagree.
extern "C" uint32_t zgemu_seektab(const uint8_t* entry, uint64_t len, uint64_t lo, const uint64_t* ranges, uint32_t n, void* out, uint64_t* counts) {
  uint32_t bad = 0;
  for (uint32_t i = 0; i < n; i++) {
    Count c;
    zgk::Seek s;
    if (!wave(Reader{entry, lo, len, &c}, len, ranges[2 * i], ranges[2 * i + 1], &s)) bad++;
    memcpy((uint8_t*)out + 64 * (size_t)i, &s, 64);
    counts[2 * i] = c.reads; counts[2 * i + 1] = c.bad;
  }
  return bad;
}

#ifdef SEEKTAB_MAIN
// argv[1]: per entry [u64 length][u64 n][n x (u64 begin, u64 rlen)][bytes]; argv[2]: the records, 64 bytes each, in that order. Every entry
// lies in a heap block of exactly its length and is read directly: an access outside it is an AddressSanitizer report.
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 2;
  uint64_t entries = 0, runs = 0, hdr[2];
  for (; fread(hdr, 8, 2, f) == 2; entries++) {
    std::vector<uint64_t> rg(2 * hdr[1] + 1);
    if (hdr[1] && fread(rg.data(), 16, hdr[1], f) != hdr[1]) return 2;
    uint8_t* e = (uint8_t*)malloc(hdr[0]);
    if (hdr[0] && (!e || fread(e, 1, hdr[0], f) != hdr[0])) return 2;
    for (uint64_t i = 0; i < hdr[1]; i++, runs++) {
      zgk::Seek s;
      if (!wave(Direct{e}, hdr[0], rg[2 * i], rg[2 * i + 1], &s)) return 3;
      if (fwrite(&s, 64, 1, g) != 1) return 2;
    }
    free(e);
  }
  fclose(f);
  if (fclose(g)) return 2;
  printf("seektab_asan ok: %llu entries, %llu runs\n", (unsigned long long)entries, (unsigned long long)runs);
  return 0;
}
#endif
