// zg_dictfill.h — zg_k_dictfill: what a registered dictionary hands to every frame of a submit that names it (zgpu_set_frames_shared_dicts),
// replicated on the device: its content into the gap in front of the frame's plaintext in the batch output, and its tables — one FSE arena
// slot with its four log bytes, one Huffman slot with its max_bits byte — into the frame's carry slots. The source is the context's one
// device copy of the dictionary (DictImage below), the destinations are the engine's own buffers.
//
// The kernel is zg_k_scatter's (zg_scatter.h): segments (src, dst, len) cut into chunks of at most 64 KiB whose inner boundaries are
// 16-byte boundaries of the DESTINATION, one 256-thread workgroup per chunk, grid-stride; zgs::copy_chunk is the lane routine — head bytes
// singly, 16-byte loads at the source's alignment and aligned 16-byte stores with four passes in flight, tail bytes singly; lanes write
// [dst, dst + len) and read [src, src + len), nothing else. What is new here is the ORDER of the chunk table. The kernel is a replicate:
// thousands of segments read the same ~100 KB, and a launch holds 2048 workgroups at a time. In segment order those 2048 workgroups would
// read 2048 different places of a dictionary at once (the whole of it, again and again: it stays in L2 all the same when it is that small,
// but a dictionary of a few MiB would not). In the order of plan_fill — by source, then by the 64 KiB window of it a chunk copies, then by
// segment — the workgroups in flight read one window of one dictionary: 64 KiB that the first wave of workgroups brings into the 4 MiB L2
// of its XCD (and into MALL) and every later one finds there, whatever the dictionary's size. The writes stream out once either way.
// Plain C++ behind the accessors of zg_scatter.h, so that g++ compiles it too (tests/test_dictfill_cpu.py).
#pragma once
#include <stddef.h>
#include <algorithm>
#include "zg_scatter.h"

namespace zgd {

struct Seg { uint64_t src, dst, len; };   // both addresses in device memory

// the context's device copy of one dictionary: [content, padded to 16][FSE slot][4 log bytes, padded to 16][Huffman slot][max_bits]
struct DictImage {
  uint64_t content, content_len;   // device addresses; the tables in the engine's packed formats (what zg_apply_dict uploads)
  uint64_t fse, logs, huf, maxbits;
};
constexpr uint64_t kFseBytes = 1280 * 4, kHufBytes = 2048 * 2;   // ZG_FSE_SLOT_U32 words, ZG_HUF_SLOT_U16 entries (zg_types.h)
static inline uint64_t image_bytes(uint64_t content_len) { return ((content_len + 15) & ~15ull) + kFseBytes + 16 + kHufBytes + 16; }
static inline DictImage image_at(uint64_t base, uint64_t content_len) {
  DictImage m;
  m.content = base; m.content_len = content_len;
  m.fse = base + ((content_len + 15) & ~15ull);
  m.logs = m.fse + kFseBytes;
  m.huf = m.logs + 16;
  m.maxbits = m.huf + kHufBytes;
  return m;
}

// The chunks of segs[0 .. n): zgs::plan_chunks' cut (every byte of every segment in exactly one chunk, none longer than chunk_bytes(chunk),
// dst + at of every chunk but a segment's first a multiple of 16), ordered by source and by the window of the source the chunk copies.
static inline void plan_fill(const Seg* segs, uint32_t n, uint32_t chunk, std::vector<zgs::Chunk>* out) {
  std::vector<zgs::Seg> s(n);
  for (uint32_t i = 0; i < n; i++) s[i] = zgs::Seg{segs[i].src, segs[i].dst, segs[i].len};
  const size_t first = out->size();
  zgs::plan_chunks(s.data(), n, chunk, out);
  const uint64_t C = zgs::chunk_bytes(chunk);
  // (a segment's k-th chunk starts at most 16 k bytes in front of k x C — the cut moves an inner boundary down to the destination's alignment —
  //  so rounding to the nearest multiple of C names k for every segment shorter than 2048 chunks; beyond that the order is merely less good)
  auto key = [&](const zgs::Chunk& c) { return (c.at + C / 2) / C; };
  std::stable_sort(out->begin() + (std::ptrdiff_t)first, out->end(), [&](const zgs::Chunk& a, const zgs::Chunk& b) {
    return segs[a.seg].src != segs[b.seg].src ? segs[a.seg].src < segs[b.seg].src : key(a) < key(b);
  });
}

// what lane t of T does for chunk c of the table
template <class R, class W> ZG_SC_FN void fill_chunk(const R& r, const W& w, const Seg* segs, const zgs::Chunk& ch, uint32_t t, uint32_t T) {
  const Seg sg = segs[ch.seg];
  zgs::copy_chunk(r, w, sg.src + ch.at, sg.dst + ch.at, ch.len, t, T);
}

}  // namespace zgd
