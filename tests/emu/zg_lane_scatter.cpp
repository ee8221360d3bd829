// zg_lane_scatter.cpp — TEST-ONLY: runs zg_k_scatter's chunk plan and lane routine (zstd-rs_amd/csrc/zg_scatter.h) on the CPU, one emulated
// lane after the other. tests/test_scatter_cpu.py builds this file (tests/lanesuite.py) as a shared library. It counts every read outside the
// chunk's own source range, every store outside its own destination range, every 16-byte store at an address that is no multiple of 16, and
// every chunk whose lanes did not write exactly its length (zg_lane_mem.h). Not part of the product.
#include "zg_scatter.h"
#include "zg_lane_mem.h"
namespace {
// the source as the lanes may see it: bytes [lo, hi) of base, nothing else
struct Reader {
  lane::Array<const uint8_t> a;
  uint8_t ld1(uint64_t off) const { return a.ld(off); }
  zgs::V16 ld16(uint64_t off) const { zgs::V16 v; a.ld_n(off, 16, &v); return v; }
};
// the destination: the len bytes at address d (the routine names addresses); 16-byte stores at multiples of 16 only
struct Writer {
  lane::Array<uint8_t> a; uint64_t d;
  void st1(uint64_t at, uint8_t v) const { a.st(at - d, v); }
  void st16(uint64_t at, const zgs::V16& v) const { a.st_n(at - d, 16, &v, 16); }
};
}
extern "C" uint32_t sc_chunk_bytes(uint32_t want) { return zgs::chunk_bytes(want); }
extern "C" uint32_t sc_default_chunk() { return zgs::kChunkDefault; }
extern "C" uint32_t sc_threads() { return zgs::kThreads; }
extern "C" uint64_t sc_plan(const zgs::Seg* segs, uint32_t n, uint32_t chunk, zgs::Chunk* out, uint64_t cap) {
  std::vector<zgs::Chunk> v;
  zgs::plan_chunks(segs, n, chunk, &v);
  for (uint64_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
  return v.size();
}
// what the kernel does with a chunk table, one emulated lane after the other; counts[0..3] = reads outside the chunk's source range, writes
// outside its destination range, unaligned 16-byte stores, chunks whose lanes did not write exactly len bytes
extern "C" void sc_run(const uint8_t* src, const zgs::Seg* segs, const zgs::Chunk* chunks, uint64_t nchunks, uint32_t T, uint64_t* counts) {
  lane::Count rc, wc;
  uint64_t wrong_total = 0;
  for (uint64_t i = 0; i < nchunks; i++) {
    const zgs::Chunk ch = chunks[i];
    const zgs::Seg sg = segs[ch.seg];
    const uint64_t s = sg.src_off + ch.at, d = sg.dst + ch.at;
    const Reader r{{src, s, s + ch.len, &rc}};
    const Writer w{{(uint8_t*)d, 0, ch.len, &wc}, d};
    const uint64_t before = wc.kept;
    for (uint32_t t = 0; t < T; t++) zgs::copy_chunk(r, w, s, d, ch.len, t, T);
    if (wc.kept - before != ch.len) wrong_total++;
  }
  counts[0] = rc.bad; counts[1] = wc.bad; counts[2] = wc.unaligned; counts[3] = wrong_total;
}
