// zg_lane_fill.cpp — TEST-ONLY: runs zg_k_fill's chunk plan and lane routine (zstd-rs_amd/csrc/zg_scatter.h: plan_chunks with kFillChunk,
// fill_chunk) on the CPU, one emulated lane after the other, and hands out the layout function of a record batch (zg_records.h: plan_rows).
// tests/test_fill_cpu.py and tests/test_recbatch_cpu.py build this file (tests/lanesuite.py) as a shared library — it counts every store
// outside the chunk's own range, every 16-byte store at an address that is no multiple of 16 and every chunk whose lanes did not write
// exactly its length (zg_lane_mem.h) — and, with -DFILL_MAIN, as a stand-alone AddressSanitizer program in which every region ends with its
// heap block. Not part of the product.
#include "zg_scatter.h"
#include "zg_records.h"
#include "zg_lane_mem.h"
namespace {
// the chunk: the len bytes at address d (the routine names addresses); 16-byte stores at multiples of 16 only
struct Writer {
  lane::Array<uint8_t> a; uint64_t d;
  void st1(uint64_t at, uint8_t v) const { a.st(at - d, v); }
  void st16(uint64_t at, const zgs::V16& v) const { a.st_n(at - d, 16, &v, 16); }
};
// no checks: what the kernel's writer does
struct Direct {
  void st1(uint64_t at, uint8_t v) const { *(uint8_t*)(uintptr_t)at = v; }
  void st16(uint64_t at, const zgs::V16& v) const { memcpy((void*)(uintptr_t)at, &v, 16); }
};
}
extern "C" uint32_t fl_chunk() { return zgs::chunk_bytes(zgs::kFillChunk); }
extern "C" uint32_t fl_threads() { return zgs::kFillThreads; }
extern "C" uint32_t fl_max_groups() { return zgs::kFillMaxGroups; }
extern "C" uint64_t fl_plan(const zgs::Seg* segs, uint32_t n, zgs::Chunk* out, uint64_t cap) {
  std::vector<zgs::Chunk> v;
  zgs::plan_chunks(segs, n, zgs::kFillChunk, &v);
  for (uint64_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
  return v.size();
}
// what the kernel does with a chunk table, one emulated lane after the other; counts[0..2] = stores outside the chunk's own range, unaligned
// 16-byte stores, chunks whose lanes did not write exactly len bytes
extern "C" void fl_run(const zgs::Seg* segs, const zgs::Chunk* chunks, uint64_t nchunks, uint32_t byte, uint32_t T, uint64_t* counts) {
  lane::Count wc;
  uint64_t wrong_total = 0;
  for (uint64_t i = 0; i < nchunks; i++) {
    const zgs::Chunk ch = chunks[i];
    const uint64_t d = segs[ch.seg].dst + ch.at;
    const Writer w{{(uint8_t*)d, 0, ch.len, &wc}, d};
    const uint64_t before = wc.kept;
    for (uint32_t t = 0; t < T; t++) zgs::fill_chunk(w, d, ch.len, (uint8_t)byte, t, T);
    if (wc.kept - before != ch.len) wrong_total++;
  }
  counts[0] = wc.bad; counts[1] = wc.unaligned; counts[2] = wrong_total;
}
// the layout: rows as m triples (at, slot, want); 1, or 0 where the layout does not fit in 64 bits
extern "C" int fl_plan_rows(const uint64_t* len, uint32_t m, uint32_t layout, int truncate, uint64_t width, uint64_t* rows, uint64_t* total,
                            uint32_t* truncated) {
  std::vector<zgr::Row> r(m);
  const bool ok = zgr::plan_rows(len, m, layout, truncate != 0, width, r.data(), total, truncated);
  for (uint32_t j = 0; j < m && ok; j++) { rows[3 * j] = r[j].at; rows[3 * j + 1] = r[j].slot; rows[3 * j + 2] = r[j].want; }
  return ok ? 1 : 0;
}

#ifdef FILL_MAIN
// argv[1]: cases of three u32 — the region's alignment mod 16, its length, the byte. Each region lies in a heap block of 16 bytes' alignment
// and exactly align + len bytes: it ENDS with its block (a store behind it is AddressSanitizer's report), and the align bytes in front of it
// hold kFill and are looked at afterwards, as is every byte of the region.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 1 ? argv[1] : nullptr, "rb");
  uint64_t cases = 0, wrong = 0;
  uint32_t h[3];
  for (; f.next(h, sizeof h); cases++) {
    const uint32_t align = h[0] & 15u, len = h[1];
    const size_t size = (size_t)align + len;
    uint8_t* exact = (uint8_t*)malloc(size);   // malloc's 16-byte alignment, exactly size bytes
    if (size && !exact) return lane::kExitIO;
    if (size && ((uintptr_t)exact & 15)) return lane::kExitIO;
    memset(exact, lane::kFill, size);
    const zgs::Seg seg{0, (uint64_t)(uintptr_t)exact + align, len};
    std::vector<zgs::Chunk> ch;
    zgs::plan_chunks(&seg, 1, zgs::kFillChunk, &ch);
    const Direct w{};
    for (const zgs::Chunk& c : ch)
      for (uint32_t t = 0; t < zgs::kFillThreads; t++) zgs::fill_chunk(w, seg.dst + c.at, c.len, (uint8_t)h[2], t, zgs::kFillThreads);
    for (uint32_t k = 0; k < align; k++) wrong += exact[k] != lane::kFill;
    for (uint32_t k = 0; k < len; k++) wrong += exact[align + k] != (uint8_t)h[2];
    free(exact);
  }
  f.close();
  if (wrong) return lane::kExitLanes;
  printf("fill_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
