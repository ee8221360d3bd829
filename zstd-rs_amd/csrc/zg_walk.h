// zg_walk.h — zg_k_walk: the header chain of an entry whose compressed bytes lie in DEVICE memory (zgpu_decode_frames_device_src), followed
// by one lane per entry, and the few dozen bytes per block the host's parse reads brought back as fixed-size skeleton records. The host keeps
// every verdict, the table lineage and the launch plan: it runs its one parse (zg_host_parse.cpp: parse_frames / plaintext_bound, add_block)
// over these records instead of over the bytes. The lane routine is plain C++ behind a reader and a writer accessor, so that g++ compiles the
// same source (tests/test_walk_cpu.py runs it with a reader that counts every access outside [0, len) and a writer that counts every store
// outside the lane's own record range, and compares the parse of the records with the parse of the bytes).
//
// The chain is the only serial thing in an entry: frame header -> block header -> next block header ... (skippable frame: magic, length,
// next frame). The lane follows it as far as plaintext_bound does — further than parse_frames, whose verdicts (window, dictionary id, section
// headers, lineage) it does not know — and emits, in the order the host's walk asks for them:
//   kFrame  off = where a frame (or skippable frame) starts; b[0 .. 18) = the bytes there, `have` of them real (clipped to the entry)
//   kBlock  off = where the block's body starts (3 behind its header); b[0 .. 3) = the header; for a compressed block whose body lies
//           inside the entry b[3 .. 8) = the first `have` (<= 5) body bytes and b[8 .. 12) = the `have2` (<= 4) bytes at the position of the
//           sequences section header, which the lane computes from the literals section header with the host's own routine (lit_header)
//   kCksum  off = where a frame's Content_Checksum starts; b[0 .. 4) = its bytes, `have` of them real
// Bytes that are not there are zero. The lane decides no verdict: where it cannot continue (End::why) it stops and says where (End::stop_off).
// Every step of the chain advances by at least 3 bytes, so the walk ends on any input. Every read is clipped to [0, len) of the entry.
//
// The number of records is not known before the walk: the kernel is launched twice with the same routine — a count pass (no writer) whose
// End::nrec the host turns into record ranges (prefix sum), then an emit pass in which a lane writes records first .. first + limit and
// never another one (an input that changed between the passes ends in a count the host refuses, not in a store outside the range).
// gfx950 ISA of zg_k_walk (hipcc -O3 --save-temps): byte loads (global_load_ubyte) with their indices known at compile time — a record is
// built in registers and leaves in pieces of its fields (global_store_dwordx4 / x3 / x2 / short, vector stores all of them) —; the count
// pass keeps only the 11 byte loads the chain depends on. Count pass 28 VGPRs, emit pass 46 VGPRs, no scratch, no LDS. zg_k_gather (the
// entries of a submit copied back to back behind the engine's front pad: zgs::copy_chunk with absolute source addresses, inner chunk
// boundaries on 16 bytes of the DESTINATION, unaligned 16-byte loads that stay inside the entry): its body loop is zg_k_scatter's,
// 4 global_load_dwordx4 + 4 global_store_dwordx4 per iteration, the remainder loop one of each, head and tail global_load_ubyte /
// global_store_byte; 36 VGPRs, no scratch, no LDS.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define ZG_WK_FN __host__ __device__ __forceinline__
#define ZG_WK_UNROLL _Pragma("unroll")
#else
#define ZG_WK_FN static inline
#define ZG_WK_UNROLL
#endif

namespace zgw {

constexpr uint32_t kFrame = 1, kBlock = 2, kCksum = 3;
// why a lane stopped (no verdict: the host's parse of the records decides what the entry's status is)
enum : uint32_t {
  kEnd = 0,          // the chain reached the end of the entry
  kShortHeader,      // a frame header that is not all there
  kBadMagic,
  kSkipPastEnd,      // a skippable frame's length leads past the entry
  kShortBlockHeader, // fewer than 3 bytes left where a block header is due
  kReservedBlock,
  kBlockTooLarge,    // Block_Size above the limit
  kBodyPastEnd,
  kShortChecksum
};
constexpr uint32_t kMagicFrame = 0xFD2FB528u, kMagicSkipLo = 0x184D2A50u, kMagicSkipHi = 0x184D2A5Fu;
constexpr uint32_t kBlockMax = 128u * 1024u;
constexpr uint32_t kFrameBytes = 18;   // the longest frame header: magic, descriptor, window, 4 of dictionary id, 8 of content size
constexpr uint32_t kThreads = 64;      // lanes of a workgroup of zg_k_walk: one wave

struct alignas(16) Rec { uint64_t off; uint8_t kind, have, have2, pad; uint8_t b[20]; };
static_assert(sizeof(Rec) == 32, "skeleton record");
struct Lane { uint64_t src, len, first, limit; };   // src: the entry's address; records first .. first + limit are the lane's (count pass: limit 0)
struct End { uint64_t stop_off; uint32_t nrec, why; };

// Literals_Section_Header (literals_section.rs:117-223) from the first bytes of a block body: h = its first min(n, 5) bytes, n = Block_Size.
// Returns false when the header is not all there (then type is still set if n > 0). upper: the bytes the literals section takes behind its
// header (block_decoder.rs:120-127), so the sequences section header lies at need + upper.
struct LitHdr { uint32_t type = 0, sf = 0, need = 0, regen = 0, comp = 0, nstreams = 0, upper = 0; };
ZG_WK_FN bool lit_header(const uint8_t* h, uint32_t n, LitHdr* o) {
  if (n == 0) return false;                                     // literals_section.rs:119 (no bits to read)
  o->type = h[0] & 3u;
  const uint32_t sf = o->sf = (h[0] >> 2) & 3u;
  const bool plain = o->type <= 1;                               // Raw / RLE
  o->need = plain ? ((sf == 0 || sf == 2) ? 1u : (sf == 1 ? 2u : 3u)) : (sf <= 1 ? 3u : (sf == 2 ? 4u : 5u));
  if (n < o->need) return false;                                 // NotEnoughBytes :124-129
  if (plain) {                                                   // :132-159
    if (sf == 0 || sf == 2) o->regen = h[0] >> 3;
    else if (sf == 1) o->regen = (h[0] >> 4) + ((uint32_t)h[1] << 4);
    else o->regen = (h[0] >> 4) + ((uint32_t)h[1] << 4) + ((uint32_t)h[2] << 12);
    o->upper = o->type == 1 ? 1u : o->regen;                     // block_decoder.rs:120-127
  } else {                                                       // :161-221
    o->nstreams = sf == 0 ? 1u : 4u;
    if (sf <= 1) {
      o->regen = (h[0] >> 4) + (((uint32_t)h[1] & 0x3f) << 4);
      o->comp = (h[1] >> 6) + ((uint32_t)h[2] << 2);
    } else if (sf == 2) {
      o->regen = (h[0] >> 4) + ((uint32_t)h[1] << 4) + (((uint32_t)h[2] & 0x3) << 12);
      o->comp = (h[2] >> 2) + ((uint32_t)h[3] << 6);
    } else {
      o->regen = (h[0] >> 4) + ((uint32_t)h[1] << 4) + (((uint32_t)h[2] & 0x3F) << 12);
      o->comp = (h[2] >> 6) + ((uint32_t)h[3] << 2) + ((uint32_t)h[4] << 10);
    }
    o->upper = o->comp;
  }
  return true;
}
// Where the sequences section header of a compressed block lies and how many of its (at most 4) bytes exist: false when the literals section
// header is short or the literals leave the block (block_decoder.rs:129-134) — nothing is read there then.
ZG_WK_FN bool seq_header_at(const uint8_t* h, uint32_t n, uint32_t* pos, uint32_t* avail) {
  LitHdr lh;
  if (!lit_header(h, n, &lh)) return false;
  if (n - lh.need < lh.upper) return false;
  *pos = lh.need + lh.upper;
  const uint32_t rem = n - *pos;
  *avail = rem < 4 ? rem : 4u;
  return true;
}
// bytes of a frame header whose descriptor is d, the magic included (frame.rs:6-85, :212-239)
ZG_WK_FN uint32_t frame_header_bytes(uint8_t d) {
  const uint32_t single = (d >> 5) & 1u, did = d & 3u, fcs = d >> 6;
  return 5u + (single ? 0u : 1u) + (did == 3 ? 4u : did) + (fcs == 0 ? single : (fcs == 1 ? 2u : (fcs == 2 ? 4u : 8u)));
}

// The stop rules of the chain: ONE definition, which walk_entry below and zgi::index_entry (zg_index.h) both follow.
// Where a frame is due: `have` = the bytes left in the entry, clipped to kFrameBytes; magic = the first four of them (anything if have < 4).
// kEnd: a skippable frame (*skip = true, its length field is all there) or the magic and the descriptor of a zstd frame are there.
ZG_WK_FN uint32_t frame_stop(uint32_t have, uint32_t magic, bool* skip) {
  *skip = false;
  if (have < 4) return kShortHeader;
  if (magic >= kMagicSkipLo && magic <= kMagicSkipHi) {
    if (have < 8) return kShortHeader;
    *skip = true;
    return kEnd;
  }
  if (magic != kMagicFrame) return kBadMagic;
  return have < 5 ? kShortHeader : kEnd;
}
// a skippable frame at *p whose length field says sl: *p moves behind its 8 header bytes and, if the entry holds them, behind its sl bytes
ZG_WK_FN uint32_t skip_stop(uint64_t sl, uint64_t len, uint64_t* p) {
  *p += 8;
  if (sl > len - *p) return kSkipPastEnd;
  *p += sl;
  return kEnd;
}
// a zstd frame whose descriptor is d: *hs = the bytes of its header, all of which must be among the `have`
ZG_WK_FN uint32_t header_stop(uint32_t have, uint8_t d, uint32_t* hs) {
  *hs = frame_header_bytes(d);
  return have < *hs ? kShortHeader : kEnd;
}
// a block header (3 bytes, the caller has checked that they are there) with `left` bytes of the entry behind it
struct BlockHdr { uint32_t type, size, content; bool last; };   // content: the bytes of the body (an RLE block: 1)
ZG_WK_FN uint32_t block_stop(uint8_t b0, uint8_t b1, uint8_t b2, uint64_t left, BlockHdr* h) {
  h->last = b0 & 1;
  h->type = (b0 >> 1) & 3u;
  h->size = (uint32_t)(b0 >> 3) | ((uint32_t)b1 << 5) | ((uint32_t)b2 << 13);
  h->content = h->type == 1 ? 1u : h->size;
  if (h->type == 3) return kReservedBlock;
  if (h->size > kBlockMax) return kBlockTooLarge;
  if (left < h->content) return kBodyPastEnd;
  return kEnd;
}
// the Content_Checksum behind a last block at p: how many of its 4 bytes the entry holds (fewer than 4: kShortChecksum, after p has moved over them)
ZG_WK_FN uint32_t checksum_bytes(uint64_t len, uint64_t p) { const uint64_t cl = len - p; return cl < 4 ? (uint32_t)cl : 4u; }

// What the lane of one entry does. R reads the entry (ld1(off), off counted from the entry's first byte; the routine asks for no off >= len);
// W writes records (put(index, rec)); EMIT = false is the count pass, which writes nothing.
template <bool EMIT, class R, class W> ZG_WK_FN End walk_entry(const R& r, const W& w, uint64_t len, uint64_t first, uint64_t limit) {
  uint64_t p = 0;
  uint32_t n = 0, why = kEnd;
  auto emit = [&](const Rec& x) {
    if (EMIT && n < limit) w.put(first + n, x);
    n++;
  };
  while (p < len) {
    Rec fr;
    memset(&fr, 0, sizeof fr);
    fr.off = p; fr.kind = (uint8_t)kFrame;
    const uint64_t left = len - p;
    const uint32_t have = left < kFrameBytes ? (uint32_t)left : kFrameBytes;
    fr.have = (uint8_t)have;
ZG_WK_UNROLL
    for (uint32_t i = 0; i < kFrameBytes; i++) fr.b[i] = i < have ? r.ld1(p + i) : (uint8_t)0;
    emit(fr);
    const uint32_t magic = (uint32_t)fr.b[0] | ((uint32_t)fr.b[1] << 8) | ((uint32_t)fr.b[2] << 16) | ((uint32_t)fr.b[3] << 24);
    bool skip;
    if ((why = frame_stop(have, magic, &skip))) break;
    if (skip) {
      const uint64_t sl = (uint32_t)fr.b[4] | ((uint32_t)fr.b[5] << 8) | ((uint32_t)fr.b[6] << 16) | ((uint32_t)fr.b[7] << 24);
      if ((why = skip_stop(sl, len, &p))) break;
      continue;
    }
    uint32_t hs;
    if ((why = header_stop(have, fr.b[4], &hs))) break;
    const bool has_cksum = (fr.b[4] >> 2) & 1;
    p += hs;
    for (;;) {
      if (len - p < 3) { why = kShortBlockHeader; break; }
      Rec br;
      memset(&br, 0, sizeof br);
      br.kind = (uint8_t)kBlock;
      br.b[0] = r.ld1(p); br.b[1] = r.ld1(p + 1); br.b[2] = r.ld1(p + 2);
      const uint64_t body = p + 3;
      br.off = body;
      BlockHdr bh;
      why = block_stop(br.b[0], br.b[1], br.b[2], len - body, &bh);
      const uint32_t type = bh.type, content = bh.content;
      if (!why && type == 2) {
        const uint32_t nh = content < 5 ? content : 5u;
        br.have = (uint8_t)nh;
ZG_WK_UNROLL
        for (uint32_t i = 0; i < 5; i++) br.b[3 + i] = i < nh ? r.ld1(body + i) : (uint8_t)0;
        uint32_t pos = 0, ns = 0;
        if (seq_header_at(br.b + 3, content, &pos, &ns)) {
          br.have2 = (uint8_t)ns;
ZG_WK_UNROLL
          for (uint32_t i = 0; i < 4; i++) br.b[8 + i] = i < ns ? r.ld1(body + pos + i) : (uint8_t)0;
        }
      }
      emit(br);
      if (why) break;
      p = body + content;
      if (bh.last) {   // Last_Block
        if (has_cksum) {
          Rec cr;
          memset(&cr, 0, sizeof cr);
          cr.off = p; cr.kind = (uint8_t)kCksum;
          const uint32_t nc = checksum_bytes(len, p);
          cr.have = (uint8_t)nc;
ZG_WK_UNROLL
          for (uint32_t i = 0; i < 4; i++) cr.b[i] = i < nc ? r.ld1(p + i) : (uint8_t)0;
          emit(cr);
          p += nc;
          if (nc < 4) why = kShortChecksum;
        }
        break;
      }
    }
    if (why) break;
  }
  return End{p, n, why};
}

}  // namespace zgw
