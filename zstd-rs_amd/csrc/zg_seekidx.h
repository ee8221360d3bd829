// zg_seekidx.h — zg_k_seekidx_rows: the rows of a seek index from an entry's HEADER CHAIN (zgpu_seek_index_create_device, kinds DECLARED and
// AUTO), for entries in DEVICE memory that carry no seek table but whose frames declare their Frame_Content_Size. zg_seekmany.h turns a seek
// table into 64-bit exclusive prefix sums C[k], D[k] and answers ranges from them; this header produces the same pairs from the chain, so
// that zg_k_seekmany_find, the grouping and the clipped scatter serve such entries unchanged. One lane per entry, like zg_k_index. The lane
// routine is plain C++ behind a reader and a pair-store accessor, like zg_index.h's, so that g++ compiles the same source
// (tests/test_seekidx_cpu.py runs it with a reader that counts every access outside [0, len) and every access to a block body, and a pair
// store that counts every store outside the lane's own range).
//
// The rows. Row k is the k-th frame record of the chain — a zstd frame or a skippable frame, what zgi::index_entry counts in nrec — with
//   c_k = end - begin of the frame;  d_k = its declared Frame_Content_Size (the 2-byte form's + 256 included), 0 for a skippable frame.
// The lane is serial anyway, so the sums are running sums: it stores pair k = { C[k], D[k] } when it has read frame k to its end, and pair
// nrows = { C[nrows], D[nrows] } behind the last row. D saturates at 2^64 - 1, as zgk::seek_entry's pos does, so it never decreases. No total
// pass, no prefix pass. C[k] is where frame k begins, and C[nrows] is where the chain ended: the entry's length, if the chain is whole.
//
// Two passes, like the table call: zg_k_index<false> gives nrec, why and flags per entry; the host indexes the entries whose chain reached
// their end (why == 0) with every zstd frame sized (kAllSized, or no zstd frame at all), lays out the pairs and hands lane i the range
// [pre, pre + limit], limit = nrec. The lane checks the limit before EVERY store: row k is stored only if k < limit, the closing pair only if
// nrows <= limit. An input that changed between the passes ends in a record the host refuses (another nrows, a why, C[nrows] != len:
// ZGPU_E_INTERNAL), not in a store outside the range. A frame that declares no size counts as a row of d_k = 0 and sets kUnsized in why; a
// frame in which the chain breaks is no row, and its stop reason is why.
//
// The chain is zgw::walk_entry's by the same stop rules (zgw::frame_stop / skip_stop / header_stop / block_stop / checksum_bytes), the header
// fields are zgi::frame_head's and the block loop is zgi::frame_blocks': one definition each, as in zg_seek.h. The lane reads no byte outside
// [src, src + len) and no byte of a block body — per block the three header bytes —, and writes only pairs [pre, pre + limit] and its own
// 32-byte Rows record. Every store is a vector store of 16 bytes at a 16-byte aligned address (global_store_dwordx4).
//
// gfx950 ISA of zg_k_seekidx_rows (hipcc -O3 --save-temps), wave64: 47 VGPRs, 41 SGPRs (.vgpr_count / .sgpr_count of the code object's
// metadata; .private_segment_fixed_size and .group_segment_fixed_size are 0: no scratch memory, no LDS, no spills) — below the 64 VGPRs up to
// which a wave64 kernel keeps full occupancy. Loads: 2 global_load_dwordx4 of the lane's 32-byte Lane and the 20 global_load_ubyte of
// zg_k_seek's chain (magic, descriptor, content size, a skippable frame's length, a block header), each group issued together in front of
// its waits. Stores: 4 global_store_dwordx4 — a row's pair, the closing pair, the two halves of the Rows record.
#pragma once
#include <stdint.h>
#include "zg_index.h"

namespace zgx {

constexpr uint32_t kThreads = 64;    // lanes of a workgroup of zg_k_seekidx_rows: one wave
constexpr uint32_t kUnsized = 32;    // Rows::why (and zgpu_seek_index_info::why, ZGPU_INDEX_UNSIZED): a zstd frame declares no Frame_Content_Size

// src: the entry's address, len its bytes; pre: the index (in pairs) of the entry's pair 0; limit: the rows the host expects
struct alignas(16) Lane { uint64_t src, len, pre, limit; };
// what the lane found: c = C[nrows] (where the chain ended), d = D[nrows], the rows it counted (stored or not) and why it stopped
struct alignas(16) Rows { uint64_t c, d; uint32_t nrows, why; uint64_t pad; };
static_assert(sizeof(Lane) == 32 && sizeof(Rows) == 32, "seek index lanes");

// What the lane of one entry does. R reads the entry (ld1(off), off counted from the entry's first byte); S stores pairs (st(index, c, d)).
template <class R, class S> ZG_WK_FN Rows seekidx_rows(const R& r, const S& s, uint64_t len, uint64_t pre, uint64_t limit) {
  uint64_t p = 0, d = 0;
  uint32_t k = 0, why = zgw::kEnd, unsized = 0;
  while (p < len) {
    const uint64_t begin = p, left = len - p;
    const uint32_t have = left < zgw::kFrameBytes ? (uint32_t)left : zgw::kFrameBytes;
    uint32_t magic = 0;
    if (have >= 4) magic = (uint32_t)r.ld1(p) | ((uint32_t)r.ld1(p + 1) << 8) | ((uint32_t)r.ld1(p + 2) << 16) | ((uint32_t)r.ld1(p + 3) << 24);
    bool skip;
    uint64_t fcs = 0;
    why = zgw::frame_stop(have, magic, &skip);
    if (!why && skip) {
      const uint64_t sl = (uint32_t)r.ld1(p + 4) | ((uint32_t)r.ld1(p + 5) << 8) | ((uint32_t)r.ld1(p + 6) << 16) | ((uint32_t)r.ld1(p + 7) << 24);
      why = zgw::skip_stop(sl, len, &p);
    } else if (!why) {
      const uint8_t desc = r.ld1(p + 4);
      uint32_t hs;
      why = zgw::header_stop(have, desc, &hs);
      if (!why) {
        const zgi::FrameHead h = zgi::frame_head(r, p, desc, hs);
        if (!h.fl) unsized = kUnsized;
        fcs = h.fcs;
        p += hs;
        uint64_t fb = 0;
        uint32_t nbl = 0;
        bool done;
        why = zgi::frame_blocks(r, len, h.has_ck, &p, &fb, &nbl, &done);
      }
    }
    if (why) break;   // (the frame in which the chain breaks is no row)
    if (k < limit) s.st(pre + k, begin, d);
    k++;
    d = fcs > UINT64_MAX - d ? UINT64_MAX : d + fcs;
  }
  if (k <= limit) s.st(pre + k, p, d);
  Rows o;
  o.c = p; o.d = d; o.nrows = k; o.why = why ? why : unsized; o.pad = 0;
  return o;
}

// Can the host index an entry by its chain, from the summary pass? 0, or the why of the refusal (the chain's stop reason, kUnsized).
static inline uint32_t refusal(const zgi::Entry& e) {
  if (e.why) return e.why;
  return e.nframes && !(e.flags & zgi::kAllSized) ? kUnsized : 0u;
}

}  // namespace zgx
