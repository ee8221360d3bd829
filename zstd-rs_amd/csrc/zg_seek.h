// zg_seek.h — zg_k_seek: which whole frames of an entry in DEVICE memory hold plaintext bytes [begin, begin + len) of it
// (zgpu_frames_seek_device, zgpu_decode_ranges_device_src), answered from frame and block headers alone, one lane per entry. The lane routine
// is plain C++ behind a reader accessor, like zg_index.h's, so that g++ compiles the same source (tests/test_seek_cpu.py runs it with a reader
// that counts every access outside [anchor_src, len) and every access to a block body, and compares every field with a model computed from
// zgi::index_entry's frame records). The chain, its stop rules, the header fields and the block loop are zg_walk.h's and zg_index.h's
// (zgw::frame_stop / skip_stop / header_stop, zgi::frame_head, zgi::frame_blocks -> zgw::block_stop / checksum_bytes): one definition each.
//
// The selection rule. p = anchor_src, pos = anchor_plain, end = begin + len (saturating). At every frame of the chain:
//   - a skippable frame is passed over: in front of the selection while nothing is taken, inside it once a frame has been;
//   - a zstd frame that declares Frame_Content_Size fcs, with nothing taken yet and pos + fcs <= begin, is SKIPPED: its block headers are
//     followed (three bytes per block, never a body), pos += fcs;
//   - any other zstd frame is TAKEN: the first one sets src_lo and plain_lo = pos; its block headers are followed the same way; a sized frame
//     adds fcs to pos (saturating), an unsized one makes the selection open-ended. Behind a taken frame the lane stops with src_hi = p as
//     soon as the selection is not open-ended and pos >= end — nothing behind is read. An open-ended selection runs to the end of the chain;
//   - where the chain breaks (why != 0: a header that cannot be read, a skippable frame or a block that leaves the entry, ...), in whatever
//     frame: bit 1, src_hi = len, and src_lo = the broken frame's begin if nothing was taken before it. A frame whose header was read and
//     whose blocks break counts as taken and adds its share to the bound; it moves pos no further and does not make the selection open-ended.
//   - the end of the entry with nothing taken: bit 2, src_lo = src_hi = where the chain ended.
// bound is plaintext_bound (zg_host_parse.cpp) of [src_lo, src_hi), always: per taken frame the minimum of its blocks' sum and a declared
// size, as zgi::index_entry counts it. frames_skipped / frames_taken count zstd frames, not skippable ones.
// A range of length 0 reads nothing and answers a record of zeros; anchor_src > len or anchor_plain > begin answers status 93 (ZGPU_E_BAD_ARG)
// and zeros. The lane reads no byte in front of anchor_src, none at or behind len, and none of a block body.
//
// gfx950 ISA of zg_k_seek (hipcc -O3 --save-temps): 57 VGPRs (below the 64 up to which a wave64 kernel keeps full occupancy), no scratch, no
// LDS. Loads: 3 global_load_dwordx4 of the lane's 48-byte Lane, and 20 global_load_ubyte — zg_k_index<false>'s chain without the dictionary id,
// which the rule does not need —, each group issued together in front of its waits: 4 of the magic, the descriptor, 8 of the content size, 4 of
// a skippable frame's length, the 3 of a block header; the block loop is those three loads, one wait chain and integer work. The Seek record
// leaves as 4 global_store_dwordx4 (the kernel stores it through a volatile 16-byte vector type: left alone, the compiler cuts the last 32
// bytes into 8 + 12 + 12). Vector stores all of them.
#pragma once
#include <stdint.h>
#include "zg_index.h"

namespace zgk {

constexpr uint32_t kThreads = 64;   // lanes of a workgroup of zg_k_seek: one wave
// Seek::flags (and zgpu_seek::flags)
constexpr uint32_t kOpenEnded = 1u, kBroken = 2u, kNothing = 4u;
constexpr uint32_t kBadArg = 93;    // ZGPU_E_BAD_ARG

struct alignas(16) Lane { uint64_t src, len, begin, rlen, anchor_src, anchor_plain; };   // src: the entry's address, len its bytes
static_assert(sizeof(Lane) == 48, "seek lane");
struct alignas(16) Seek {           // zgpu_seek (include/zgpu.h), field for field
  uint64_t src_lo, src_hi, plain_lo, bound, plain_seen;
  uint32_t status, frames_skipped, frames_taken, nblocks, why, flags;
};
static_assert(sizeof(Seek) == 64, "seek record");

// What the lane of one entry does. R reads the entry (ld1(off), off counted from the entry's first byte).
template <class R> ZG_WK_FN Seek seek_entry(const R& r, uint64_t len, uint64_t begin, uint64_t rlen, uint64_t anchor_src, uint64_t anchor_plain) {
  // (one way out: the record is put together once, at the end, and leaves in four 16-byte stores)
  const bool bad = rlen != 0 && (anchor_src > len || anchor_plain > begin), walk = rlen != 0 && !bad;
  const uint64_t end = rlen > UINT64_MAX - begin ? UINT64_MAX : begin + rlen;
  uint64_t p = anchor_src, pos = anchor_plain, lo = 0, plo = 0, bound = 0;
  uint32_t nsk = 0, ntk = 0, nbl = 0, why = zgw::kEnd;
  bool taken = false, open = false;
  if (!walk) len = 0;
  while (p < len) {
    const uint64_t fbegin = p, left = len - p;
    const uint32_t have = left < zgw::kFrameBytes ? (uint32_t)left : zgw::kFrameBytes;
    uint32_t magic = 0;
    if (have >= 4) magic = (uint32_t)r.ld1(p) | ((uint32_t)r.ld1(p + 1) << 8) | ((uint32_t)r.ld1(p + 2) << 16) | ((uint32_t)r.ld1(p + 3) << 24);
    bool skip, zframe = false;
    zgi::FrameHead h{0, 0, 0, false};
    uint64_t fb = 0;
    why = zgw::frame_stop(have, magic, &skip);
    if (!why && skip) {
      const uint64_t sl = (uint32_t)r.ld1(p + 4) | ((uint32_t)r.ld1(p + 5) << 8) | ((uint32_t)r.ld1(p + 6) << 16) | ((uint32_t)r.ld1(p + 7) << 24);
      why = zgw::skip_stop(sl, len, &p);
    } else if (!why) {
      const uint8_t d = r.ld1(p + 4);
      uint32_t hs;
      why = zgw::header_stop(have, d, &hs);
      if (!why) {
        zframe = true;
        h = zgi::frame_head(r, p, d, hs);
        p += hs;
        bool done;
        why = zgi::frame_blocks(r, len, h.has_ck, &p, &fb, &nbl, &done);
      }
    }
    const uint64_t share = h.fl && h.fcs < fb ? h.fcs : fb;
    if (why) {   // the chain broke in this frame: it and everything behind it belong to the selection
      if (!taken) { taken = true; lo = fbegin; plo = pos; }
      if (zframe) { ntk++; bound += share; }
      break;
    }
    if (!zframe) continue;
    if (!taken && h.fl && h.fcs <= begin - pos) { nsk++; pos += h.fcs; continue; }   // (pos <= begin while nothing is taken)
    if (!taken) { taken = true; lo = fbegin; plo = pos; }
    ntk++;
    bound += share;
    if (h.fl) pos = h.fcs > UINT64_MAX - pos ? UINT64_MAX : pos + h.fcs; else open = true;
    if (!open && pos >= end) break;
  }
  Seek o;
  o.src_lo = !walk ? 0 : taken ? lo : p; o.src_hi = !walk ? 0 : why ? len : p;
  o.plain_lo = !walk ? 0 : taken ? plo : pos; o.bound = bound; o.plain_seen = walk ? pos : 0;
  o.status = bad ? kBadArg : 0u; o.frames_skipped = nsk; o.frames_taken = ntk; o.nblocks = nbl; o.why = why;
  o.flags = !walk ? 0u : (open ? kOpenEnded : 0u) | (why ? kBroken : 0u) | (taken ? 0u : kNothing);
  return o;
}

}  // namespace zgk
