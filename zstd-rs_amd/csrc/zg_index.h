// zg_index.h — zg_k_index: what entries whose compressed bytes lie in DEVICE memory hold (zgpu_frames_index_device, zgpu_frames_table_device),
// answered from frame and block headers alone, one lane per entry: the bound of the plaintext (zgpu_plaintext_bound of a host copy, always),
// how many frames, skippable frames and blocks the header chain read, where and why it ended — and, for the table call, one record per frame.
// No byte of the input comes back. The lane routine is plain C++ behind a reader and a writer accessor, like zg_walk.h's, so that g++
// compiles the same source (tests/test_index_cpu.py runs it with a reader that counts every access outside [0, len) and every access to a
// block body, and a writer that counts every store outside the lane's own record range).
//
// The chain is zgw::walk_entry's, by the same stop rules (zgw::frame_stop / skip_stop / header_stop / block_stop / checksum_bytes: one
// definition), but the lane never touches a block body: per block it reads the three header bytes and nothing else — one dependent load per
// block where the walk has three (header, literals section header, sequences section header). The running bound is plaintext_bound_on's
// (zg_host_parse.cpp): 128 KiB per compressed block, Block_Size per raw or RLE block — counted as soon as the header is read and valid, so a
// block whose body runs past the entry still counts —, per frame the minimum of that sum and a declared Frame_Content_Size, and the frame in
// which the chain breaks keeps the blocks it has. Of the frame header the lane decodes what the chain and the bound need — magic, descriptor,
// dictionary id (is one named?), Frame_Content_Size with the 2-byte form's + 256 —; every other field the host reads from the 18 raw bytes
// of a frame record with read_frame_header, so window, dictionary id and verdicts keep their one definition.
//
// Summary pass (EMIT = false): one 48-byte Entry per lane. Emit pass (EMIT = true, the table call only, after the host's prefix sum over
// Entry::nrec): lane i writes frame records first .. first + limit and checks the limit before every store; an input that changed between the
// passes ends in a count the host refuses (ZGPU_E_INTERNAL), not in a store outside the range.
// gfx950 ISA of zg_k_index (hipcc -O3 --save-temps): zg_k_index<false> 47 VGPRs (zg_k_walk<false>: 28; both below the 64 up to which a wave64
// kernel keeps full occupancy), no scratch, no LDS. The loads that remain are one global_load_dwordx4 of the lane's src and len and the 24
// global_load_ubyte of the chain, each group issued together in front of its waits: 4 of the magic, the descriptor, 4 of a dictionary id and
// 8 of the content size (a shorter field reads its last byte again), 4 of a skippable frame's length, and the 3 of a block header — the
// block loop is those three loads, one wait chain, and integer work. The Entry leaves as 3 global_store_dwordx4. zg_k_index<true> 68 VGPRs,
// no scratch, no LDS: 42 global_load_ubyte (the 18 header bytes besides, at indices known at compile time) and 2 global_load_dwordx4 of
// its Lane; a FrameRec is built in registers and leaves in pieces of its fields (global_store_dwordx4 / x3 / dword / short). Vector stores
// all of them.
#pragma once
#include <stdint.h>
#include <string.h>
#include "zg_walk.h"

namespace zgi {

constexpr uint32_t kThreads = 64;   // lanes of a workgroup of zg_k_index: one wave

// Entry::flags (and zgpu_entry_index::flags)
constexpr uint32_t kAllSized = 1u, kAnyDict = 2u, kAnyChecksum = 4u, kAllComplete = 8u;
// FrameRec::flags: the bits of zgpu_frame_index::flags the lane decides (the host adds the others from the header bytes)
constexpr uint32_t kSkippable = 1u, kComplete = 8u;

struct alignas(16) Entry {
  uint64_t bound, chain_end;
  uint32_t nframes, nskippable, nblocks, why;
  uint32_t flags, nrec;   // nrec: the frame records of the entry — its frames, its skippable frames, and the header the chain could not read, if it ended at one
  uint64_t pad;
};
static_assert(sizeof(Entry) == 48, "entry summary");
struct alignas(16) FrameRec {
  uint64_t begin, end;    // the frame's bytes in its entry; end = where the chain left it
  uint64_t bound;         // the frame's share of the entry's bound
  uint32_t nblocks;
  uint8_t have, flags, pad[2];
  uint8_t b[20];          // b[0 .. 18): the header's bytes at begin, `have` of them real — a header the chain read: exactly its own bytes (8 of a
                          // skippable frame); one it could not read: what the entry has left there, up to 18 — the others zero
  uint8_t pad2[12];
};
static_assert(sizeof(FrameRec) == 64, "frame record");

// The fields of a zstd frame's header that the chain and the bound need, at p (descriptor d, header of hs bytes: zgw::header_stop has said they
// are all there). ONE definition: index_entry below and zgk::seek_entry (zg_seek.h) both read a header with it.
struct FrameHead { uint64_t fcs; uint32_t id, fl; bool has_ck; };   // fl: bytes of the Frame_Content_Size field (0: the frame declares none)
template <class R> ZG_WK_FN FrameHead frame_head(const R& r, uint64_t p, uint8_t d, uint32_t hs) {
  // frame.rs:212-239: the sizes of the dictionary id and content size fields; the content size is the header's last field
  const uint32_t single = (d >> 5) & 1u, did = d & 3u, fc = d >> 6;
  const uint32_t dl = did == 3 ? 4u : did, fl = fc == 0 ? single : (fc == 1 ? 2u : (fc == 2 ? 4u : 8u));
  uint32_t id = 0;
  uint64_t fcs = 0;
  // (a field's loads are issued together: byte i of a shorter field is its last byte again, and is masked out)
  if (dl) {
ZG_WK_UNROLL
    for (uint32_t i = 0; i < 4; i++) { const uint32_t v = r.ld1(p + hs - fl - dl + (i < dl ? i : dl - 1)); id |= i < dl ? v << (8 * i) : 0u; }
  }
  if (fl) {
    uint32_t lo = 0, hi = 0;
ZG_WK_UNROLL
    for (uint32_t i = 0; i < 8; i++) {
      const uint32_t v = r.ld1(p + hs - fl + (i < fl ? i : fl - 1)), x = i < fl ? v << (8 * (i & 3)) : 0u;
      if (i < 4) lo |= x; else hi |= x;
    }
    fcs = lo | ((uint64_t)hi << 32);
  }
  if (fl == 2) fcs += 256;   // frame.rs:78-80
  return FrameHead{fcs, id, fl, (bool)((d >> 2) & 1u)};
}
// The blocks of a zstd frame from *p (behind its header) on: three header bytes per block, never a body. *p ends behind the frame (its
// Content_Checksum included) or where the chain broke; *fb += what the blocks count towards the bound, *nblocks += the headers read; *done:
// the last block was seen and the checksum is all there. Returns why the chain broke, kEnd if it did not.
template <class R> ZG_WK_FN uint32_t frame_blocks(const R& r, uint64_t len, bool has_ck, uint64_t* p, uint64_t* fb, uint32_t* nblocks, bool* done) {
  uint32_t why;
  *done = false;
  for (;;) {
    if (len - *p < 3) { why = zgw::kShortBlockHeader; break; }
    const uint8_t b0 = r.ld1(*p), b1 = r.ld1(*p + 1), b2 = r.ld1(*p + 2);
    (*nblocks)++;
    zgw::BlockHdr bh;
    why = zgw::block_stop(b0, b1, b2, len - (*p + 3), &bh);
    if (why == zgw::kReservedBlock || why == zgw::kBlockTooLarge) break;   // (read_block_header fails: the block counts nothing)
    *fb += bh.type == 2 ? (uint64_t)zgw::kBlockMax : (uint64_t)bh.size;
    if (why) break;                                                        // (the body runs past the entry: the block has counted)
    *p += 3 + (uint64_t)bh.content;
    if (bh.last) {
      *done = true;
      if (has_ck) {
        const uint32_t nc = zgw::checksum_bytes(len, *p);
        *p += nc;
        if (nc < 4) { why = zgw::kShortChecksum; *done = false; }
      }
      break;
    }
  }
  return why;
}

// What the lane of one entry does. R reads the entry (ld1(off), off counted from the entry's first byte; the routine asks for no off >= len
// and for no byte of a block body); W writes frame records (put(index, rec)); EMIT = false is the summary pass, which writes no record.
template <bool EMIT, class R, class W> ZG_WK_FN Entry index_entry(const R& r, const W& w, uint64_t len, uint64_t first, uint64_t limit) {
  uint64_t p = 0, total = 0;
  uint32_t nfr = 0, nsk = 0, nbl = 0, nrec = 0, why = zgw::kEnd;
  bool all_sized = true, any_dict = false, any_ck = false, all_done = true;
  while (p < len) {
    const uint64_t begin = p, left = len - p;
    const uint32_t have = left < zgw::kFrameBytes ? (uint32_t)left : zgw::kFrameBytes;
    uint64_t fb = 0, share = 0;
    uint32_t fblocks = 0, fflags = 0, magic = 0;
    uint32_t nb = have;   // the header's bytes: all that is left where it cannot be read, else exactly its own (what follows may be a block body)
    if (have >= 4) magic = (uint32_t)r.ld1(p) | ((uint32_t)r.ld1(p + 1) << 8) | ((uint32_t)r.ld1(p + 2) << 16) | ((uint32_t)r.ld1(p + 3) << 24);
    bool skip;
    why = zgw::frame_stop(have, magic, &skip);
    if (!why && skip) {
      const uint64_t sl = (uint32_t)r.ld1(p + 4) | ((uint32_t)r.ld1(p + 5) << 8) | ((uint32_t)r.ld1(p + 6) << 16) | ((uint32_t)r.ld1(p + 7) << 24);
      nsk++;
      fflags = kSkippable;
      nb = 8;
      why = zgw::skip_stop(sl, len, &p);
    } else if (!why) {
      const uint8_t d = r.ld1(p + 4);
      uint32_t hs;
      why = zgw::header_stop(have, d, &hs);
      if (!why) {
        nfr++;
        nb = hs;
        const FrameHead h = frame_head(r, p, d, hs);
        if (h.id) any_dict = true;   // (a dictionary id of 0 names none, frame.rs:60-62)
        if (h.has_ck) any_ck = true;
        if (!h.fl) all_sized = false;
        p += hs;
        bool done;
        why = frame_blocks(r, len, h.has_ck, &p, &fb, &fblocks, &done);
        nbl += fblocks;
        share = h.fl && h.fcs < fb ? h.fcs : fb;
        if (done) fflags = kComplete; else all_done = false;
      }
    }
    if (EMIT) {
      FrameRec fr;
      memset(&fr, 0, sizeof fr);
      fr.have = (uint8_t)nb;
ZG_WK_UNROLL
      for (uint32_t i = 0; i < zgw::kFrameBytes; i++) fr.b[i] = i < nb ? r.ld1(begin + i) : (uint8_t)0;
      fr.begin = begin; fr.end = p; fr.bound = share; fr.nblocks = fblocks; fr.flags = (uint8_t)fflags;
      if (nrec < limit) w.put(first + nrec, fr);
    }
    nrec++;
    total += share;
    if (why) break;
  }
  Entry e;
  e.bound = total; e.chain_end = p;
  e.nframes = nfr; e.nskippable = nsk; e.nblocks = nbl; e.why = why;
  e.flags = nfr ? (all_sized ? kAllSized : 0u) | (any_dict ? kAnyDict : 0u) | (any_ck ? kAnyChecksum : 0u) | (all_done ? kAllComplete : 0u) : 0u;
  e.nrec = nrec;
  e.pad = 0;
  return e;
}

// The host's prefix sum between the passes: first[i] .. first[i + 1] are entry i's frame records (first has n + 1 slots). Returns their number.
static inline uint64_t frame_ranges(const Entry* e, uint32_t n, uint64_t* first) {
  first[0] = 0;
  for (uint32_t i = 0; i < n; i++) first[i + 1] = first[i] + e[i].nrec;
  return first[n];
}
// Is what the emit pass says about an entry what the summary pass said? (No, if the source changed between them.)
static inline bool same_entry(const Entry& a, const Entry& b) {
  return a.bound == b.bound && a.chain_end == b.chain_end && a.nframes == b.nframes && a.nskippable == b.nskippable && a.nblocks == b.nblocks &&
         a.why == b.why && a.flags == b.flags && a.nrec == b.nrec;
}

}  // namespace zgi
