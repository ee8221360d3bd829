// zg_lane_dictfill.cpp — TEST-ONLY: runs zg_k_dictfill's plan and lane routine (zstd-rs_amd/csrc/zg_dictfill.h) and the host walk with a
// dictionary lookup (zg_host_parse.cpp) on the CPU. tests/test_dictfill_cpu.py builds this file (tests/lanesuite.py) as a shared library. It
// counts every read outside the chunk's own source range, every store outside its own destination range, every 16-byte store at an address
// that is no multiple of 16, and every chunk whose lanes did not write exactly its length (zg_lane_mem.h). Not part of the product.
#include "zg_dictfill.h"
#include "zg_host_parse.h"
#include "zg_lane_mem.h"
namespace {
struct Reader {   // the source as the lanes may see it: the len bytes at address s (the routine names addresses)
  lane::Array<const uint8_t> a; uint64_t s;
  uint8_t ld1(uint64_t at) const { return a.ld(at - s); }
  zgs::V16 ld16(uint64_t at) const { zgs::V16 v; a.ld_n(at - s, 16, &v); return v; }
};
struct Writer {   // the destination: the len bytes at address d; 16-byte stores at multiples of 16 only
  lane::Array<uint8_t> a; uint64_t d;
  void st1(uint64_t at, uint8_t v) const { a.st(at - d, v); }
  void st16(uint64_t at, const zgs::V16& v) const { a.st_n(at - d, 16, &v, 16); }
};
struct Dicts { uint32_t id; zg::DictFacts f; };
const zg::DictFacts* find(const void* user, uint32_t id) { const Dicts* d = (const Dicts*)user; return d->id == id ? &d->f : nullptr; }
}
extern "C" uint64_t df_plan(const zgd::Seg* segs, uint32_t n, uint32_t chunk, zgs::Chunk* out, uint64_t cap) {
  std::vector<zgs::Chunk> v;
  zgd::plan_fill(segs, n, chunk, &v);
  for (uint64_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
  return v.size();
}
extern "C" void df_run(const zgd::Seg* segs, const zgs::Chunk* chunks, uint64_t nchunks, uint32_t T, uint64_t* counts) {
  lane::Count rc, wc;
  uint64_t wrong_total = 0;
  for (uint64_t i = 0; i < nchunks; i++) {
    const zgs::Chunk ch = chunks[i];
    const zgd::Seg sg = segs[ch.seg];
    const uint64_t s = sg.src + ch.at, d = sg.dst + ch.at;
    const Reader r{{(const uint8_t*)s, 0, ch.len, &rc}, s};
    const Writer w{{(uint8_t*)d, 0, ch.len, &wc}, d};
    const uint64_t before = wc.kept;
    for (uint32_t t = 0; t < T; t++) zgd::fill_chunk(r, w, segs, ch, t, T);
    if (wc.kept - before != ch.len) wrong_total++;
  }
  counts[0] = rc.bad; counts[1] = wc.bad; counts[2] = wc.unaligned; counts[3] = wrong_total;
}
extern "C" void df_image(uint64_t base, uint64_t len, uint64_t* out) {
  const zgd::DictImage m = zgd::image_at(base, len);
  out[0] = m.content; out[1] = m.fse; out[2] = m.logs; out[3] = m.huf; out[4] = m.maxbits; out[5] = zgd::image_bytes(len);
}
// the walk of src with (id != 0) or without a lookup that knows dictionary `id`. out: [0] walk status, [1] frames, then per frame (up to 8)
// dict_len, hist[0..2], whether every table of its first block that can be carried is (mask as begin_frame took it: read back from the
// lineage of a Treeless / Repeat block is not possible here, so the mask is reported as "first block's slots are the frame's carry slots"),
// the first unit's noseq flags, nunits
extern "C" void df_walk(const uint8_t* src, uint64_t len, uint32_t id, uint64_t content_len, const uint32_t* hist, uint64_t* out) {
  zg::BatchBuilder bb;
  bb.sparse_max = 0;   // (no frame is handed to zg_k_sparse: a first unit with sequences is a direct unit wherever the builder allows one)
  std::vector<zg::FrameInfo> info;
  Dicts d{id, zg::DictFacts{content_len, {hist[0], hist[1], hist[2]}}};
  const zg::DictLookup lk{find, &d};
  out[0] = (uint64_t)zg::parse_frames(src, len, 1ull << 27, &bb, &info, 0, id ? &lk : nullptr);
  bb.finish();
  out[1] = bb.frames.size();
  out[2] = zg::plaintext_bound(src, len, id ? &lk : nullptr);
  for (size_t f = 0; f < bb.frames.size() && f < 8; f++) {
    const ZgFrame& fr = bb.frames[f];
    uint64_t* o = out + 3 + 8 * f;
    o[0] = fr.dict_len; o[1] = fr.hist_init[0]; o[2] = fr.hist_init[1]; o[3] = fr.hist_init[2];
    uint64_t carried = 0;   // bit 0 Huffman, 1 LL, 2 OF, 3 ML: a block of the frame decodes with the frame's carry slot
    for (uint32_t i = 0; i < fr.nblocks; i++) {
      const ZgBlock& b = bb.blocks[fr.first_block + i];
      if (b.btype != ZG_BT_COMPRESSED || b.host_status) continue;
      if (b.huf_slot == fr.carry_huf_slot) carried |= 1;
      if (b.nseq && b.ll_slot == (int32_t)fr.carry_slot) carried |= 2;
      if (b.nseq && b.of_slot == (int32_t)fr.carry_slot) carried |= 4;
      if (b.nseq && b.ml_slot == (int32_t)fr.carry_slot) carried |= 8;
    }
    o[4] = carried;
    o[5] = fr.nunits ? bb.units[fr.first_unit].noseq : 99;
    o[6] = fr.nunits;
    o[7] = info[f].header.has_dict_id ? info[f].header.dict_id : 0;
  }
}
