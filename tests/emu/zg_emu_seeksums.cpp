// zg_emu_seeksums.cpp — TEST-ONLY: runs the SOURCE of zg_k_seeksums' wave routine (zstd-rs_amd/csrc/zg_seeksums.h: the seek table's Checksum
// fields against the hash kernel's digests, one wave per entry) on the CPU through the SIMT emulator of zg_simt.h, and the host form of the
// same rule (locate_rows + sums_rows) beside it. tests/test_seeksums_cpu.py builds this file itself (it is not in the Makefile's library),
// twice: as a shared library whose readers count every access and every access outside the windows the test allows, and — with
// -DSEEKSUMS_MAIN — as a stand-alone AddressSanitizer program in which every entry, every slice of the frame list and every digest array
// lies in a heap block of exactly its length. Both hand every record back; the test compares them with its model. Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_seektab.h"
#include "../../zstd-rs_amd/csrc/zg_seeksums.h"

namespace {
struct Count { uint64_t reads = 0, bad_entry = 0, bad_list = 0, bad_digest = 0; };
struct Reader {   // the entry as the wave may see it: the bytes of up to three windows [lo, hi)
  const uint8_t* p; const uint64_t* win; uint32_t nwin; Count* c;
  bool ok(uint64_t off, uint64_t n) const {
    c->reads++;
    for (uint32_t w = 0; w < nwin; w++) if (off >= win[2 * w] && off <= win[2 * w + 1] && n <= win[2 * w + 1] - off) return true;
    c->bad_entry++;
    return false;
  }
  uint32_t ld1(uint64_t off) const { return ok(off, 1) ? p[off] : 0u; }
  uint32_t ld4(uint64_t off) const { uint32_t v = 0; if (ok(off, 4)) memcpy(&v, p + off, 4); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { *a = *b = 0; if (ok(off, 8)) { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); } }
  void ld12(uint64_t off, uint32_t* a, uint32_t* b, uint32_t* s) const {
    *a = *b = *s = 0;
    if (ok(off, 12)) { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); memcpy(s, p + off + 8, 4); }
  }
};
struct List {   // the submit's whole frame list and digest array; the wave may see its own slice and the digests that slice names
  const zgv::Frame* all; uint32_t lo, n; const uint64_t* dig; uint32_t ndig; Count* c;
  bool named(uint32_t slot) const { for (uint32_t i = 0; i < n; i++) if (all[lo + i].slot == slot) return true; return false; }
  uint64_t begin(uint32_t i) const { if (i >= n) { c->bad_list++; return 0; } return all[lo + i].begin; }
  void frame(uint32_t i, uint64_t* b, uint32_t* cl, uint32_t* slot) const {
    *b = 0; *cl = 0; *slot = zgv::kNotHashed;
    if (i >= n) { c->bad_list++; return; }
    *b = all[lo + i].begin; *cl = all[lo + i].clen; *slot = all[lo + i].slot;
  }
  uint32_t digest(uint32_t slot) const { if (slot >= ndig || !named(slot)) { c->bad_digest++; return 0; } return (uint32_t)dig[slot]; }
};
struct Direct {   // no checks: what the kernel's readers do
  const uint8_t* p;
  uint32_t ld1(uint64_t off) const { return p[off]; }
  uint32_t ld4(uint64_t off) const { uint32_t v; memcpy(&v, p + off, 4); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); }
  void ld12(uint64_t off, uint32_t* a, uint32_t* b, uint32_t* s) const { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); memcpy(s, p + off + 8, 4); }
};
struct DirectList {
  const zgv::Frame* fr; const uint64_t* dig;
  uint64_t begin(uint32_t i) const { return fr[i].begin; }
  void frame(uint32_t i, uint64_t* b, uint32_t* cl, uint32_t* slot) const { *b = fr[i].begin; *cl = fr[i].clen; *slot = fr[i].slot; }
  uint32_t digest(uint32_t slot) const { uint32_t v; memcpy(&v, &dig[slot], 4); return v; }
};

// one wave over one entry; false if the lanes' records differ. The record is lane 0's, stored as the kernel stores it.
template <class R, class F> bool wave(const R& r, const F& f, uint64_t len, uint32_t first, uint32_t taken, uint32_t nfr, uint32_t ndig, zgv::Sums* out) {
  static zgv::Sums all[64];
  alignas(16) static zgv::Sums stored;
  memset(&stored, 0xEE, sizeof stored);
  simt::run(64, [&]() {
    const zgv::Sums o = zgv::seeksums_entry(r, f, len, first, taken, nfr, ndig);
    memcpy(&all[zx_tid()], &o, sizeof o);
    if (zx_tid() == 0) zgv::seeksums_store(&stored, o);
  });
  bool same = true;
  for (int l = 1; l < 64; l++) same = same && memcmp(&all[l], &all[0], sizeof all[0]) == 0;
  memcpy(out, &stored, sizeof stored);
  return same;
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
  Count c;
  zgv::Sums s;
  const zgv::Frame* all = (const zgv::Frame*)frames;
  const bool same = wave(Reader{entry, win, nwin, &c}, List{all, frame_lo, frame_n, dig, ndig, &c}, len, first, taken, frame_n, ndig, &s);
  const zgv::Sums h = host(entry, len, first, taken, all + frame_lo, frame_n, dig, ndig);
  memcpy(out, &s, 32);
  memcpy((uint8_t*)out + 32, &h, 32);
  counts[0] = c.reads; counts[1] = c.bad_entry; counts[2] = c.bad_list; counts[3] = c.bad_digest;
  return same ? 0u : 1u;
}

#ifdef SEEKSUMS_MAIN
// argv[1]: per case [u64 length][u32 first][u32 taken][u32 frame_n][u32 ndig][frame_n x 16 bytes][ndig x 8 bytes][the entry]; argv[2]: the
// records, wave then host, 64 bytes per case. Entry, slice and digests each lie in a heap block of exactly their length and are read
// directly: an access outside one is an AddressSanitizer report.
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 2;
  uint64_t cases = 0, len;
  uint32_t h[4];
  for (; fread(&len, 8, 1, f) == 1; cases++) {
    if (fread(h, 4, 4, f) != 4) return 2;
    zgv::Frame* fr = (zgv::Frame*)aligned_alloc(16, h[2] ? (size_t)h[2] * 16 : 16);   // (16-byte records)
    uint64_t* dig = (uint64_t*)malloc((size_t)h[3] * 8);
    uint8_t* e = (uint8_t*)malloc(len);
    if (h[2] && fread(fr, 16, h[2], f) != h[2]) return 2;
    if (h[3] && fread(dig, 8, h[3], f) != h[3]) return 2;
    if (len && (!e || fread(e, 1, len, f) != len)) return 2;
    zgv::Sums s;
    if (!wave(Direct{e}, DirectList{fr, dig}, len, h[0], h[1], h[2], h[3], &s)) return 3;
    const zgv::Sums hs = host(e, len, h[0], h[1], fr, h[2], dig, h[3]);
    if (fwrite(&s, 32, 1, g) != 1 || fwrite(&hs, 32, 1, g) != 1) return 2;
    free(e); free(dig); free(fr);
  }
  fclose(f);
  if (fclose(g)) return 2;
  printf("seeksums_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
