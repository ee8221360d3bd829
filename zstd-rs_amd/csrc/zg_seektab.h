// zg_seektab.h — zg_k_seektab: which whole frames of an entry in DEVICE memory hold plaintext bytes [begin, begin + len) of it, answered from
// the seek table of zstd's seekable format (zgpu_frames_seek_table_device, zgpu_decode_ranges_seek_table_device_src). One WAVE per entry, not
// one lane: the table is an array, so its entries come in coalesced loads and the offsets in wave-wide prefix sums — no dependent chain through
// the input, no frame or block header touched. Written against the zx_* primitives (zg_kernels.hip maps them onto gfx950 builtins,
// tests/emu/zg_simt.h onto the CPU emulator) behind a reader accessor like zg_seek.h's: tests/test_seektab_cpu.py runs this source with a
// reader that counts every access outside the table frame and compares every field with a model in Python.
//
// The format (all fields little-endian). A seekable entry is a run of frames and, behind them, ONE skippable frame:
//   Skippable_Magic 0x184D2A5E | Frame_Size = nframes * es + 9 | nframes x { Compressed_Size u32, Decompressed_Size u32 [, Checksum u32] } |
//   Number_Of_Frames u32 | Seek_Table_Descriptor u8 (bit 7 Checksum_Flag, bits 6..2 reserved and 0, bits 1..0 ignored) | 0x8F92EAB1
// es is 8, or 12 with checksums; Number_Of_Frames <= 0x8000000. Entry k describes the k-th frame of the entry (a skippable frame is entered
// with decompressed size 0): it lies at source offset C_k = the compressed sizes in front of it and yields plaintext [D_k, D_k + d_k), D_k =
// the decompressed sizes in front of it. zg_k_seektab does not read the Checksum fields; zg_k_seeksums (zg_seeksums.h) compares them with the
// digests of the decoded frames where ZGPU_DEVICE_VERIFY_SEEK_TABLE asks for it.
//
// Locating the table, wave-uniform, in this order (the first that fails is `why`):
//   1. len < 17 or the last four bytes are not the seekable magic                              kNone
//   2. descriptor & 0x7C                                                                        kReservedBits
//   3. nframes > 0x8000000 or nframes * es + 17 > len                                           kTooLarge
//   4. tab = len - (nframes * es + 17): no skippable magic at tab, or a Frame_Size other than nframes * es + 9   kBadFrame
// The scan, 64 entries a step: lane l loads entry base + l (the next step's loads are issued in front of this step's scan: they depend on
// nothing but the step number), two 64-bit inclusive prefix sums over the wave — compressed and decompressed sizes — on wave-uniform running
// carries. With end = begin + rlen (saturating):
//   first = the smallest k with D_k + d_k > begin;  last = the smallest k >= first with D_k + d_k >= end, else nframes - 1
// both by a ballot and a find-first-set (the sums do not decrease, so the lanes that satisfy either are a suffix of the step); the scan stops at
// the step that holds `last`. The record: src_lo = C_first, src_hi = C_last + c_last, plain_lo = D_first, plain_seen = D_last + d_last, bound =
// plain_seen - plain_lo (what the TABLE promises, no header bound), frames_skipped = first, frames_taken = last - first + 1 (table entries,
// zero-size ones included), nblocks = 0. No first (the range lies behind the plaintext, or the table is empty): flags bit 2, src_lo = src_hi =
// C_n, plain_lo = plain_seen = D_n, frames_skipped = nframes, frames_taken = 0. src_hi > tab: kPastTable — the table leads into itself or
// outside. Any why != 0: status = kSeekTable (ZGPU_E_SEEK_TABLE), why, and every other field 0. rlen == 0: a record of zeros, no byte read.
// The sums cannot overflow: at most 2^27 entries of less than 2^32 each.
//
// What the wave reads: 9 bytes of the footer, 8 of the frame header, the first 8 bytes of table entries — all inside [tab, len), nothing in
// front of the table frame, nothing at or behind len. The table starts wherever the frames in front of it end, so every load is a dword or
// dwordx2 load at a byte address (gfx950 runs in unaligned access mode); nothing is rounded down to an aligned address, which would touch
// bytes in front of the table.
//
// gfx950 ISA of zg_k_seektab (hipcc -O3 --save-temps): 43 VGPRs (below the 64 up to which a wave64 kernel keeps full occupancy), 36 SGPRs, no
// scratch, no LDS. Loads: 1 s_load_dwordx8 of the entry's 32-byte Lane; of the footer 2 global_load_dword (magic, Number_Of_Frames) and 1
// global_load_sbyte (descriptor), issued together; 1 global_load_dwordx2 of the frame's magic and Frame_Size; 2 global_load_dwordx2 of table
// entries — the first step's in front of the loop, and in the loop the next step's, issued in front of the scan and waited for at the top of
// the next step. The compiler proves the footer and header wave-uniform (v_readfirstlane): the loop and the checks branch on SGPRs. The scan
// primitive is __shfl_up, and the ISA shows ds_bpermute_b32, no DPP row shifts: 34 in all — 22 for the two 64-bit sums of a step (the high halves of the
// first stage are known zero and cost nothing) and 12 for the broadcasts of first / last / the carries. The record leaves lane 0 as 4
// global_store_dwordx4. Vector stores all of them.
//
// Included twice by zg_kernels.hip: through zg_kernels.h for the types, and behind the zx_* primitives for the wave routine.
#ifndef ZG_SEEKTAB_TYPES
#define ZG_SEEKTAB_TYPES
#include <stdint.h>
#include "zg_types.h"
#include "zg_seek.h"

namespace zgt {

constexpr uint32_t kThreads = 64;   // lanes of a workgroup of zg_k_seektab: one wave, one entry
// Seek::why of a table that is not usable (ZGPU_SEEKTAB_*), and the status that goes with it (ZGPU_E_SEEK_TABLE)
constexpr uint32_t kNone = 16, kReservedBits = 17, kTooLarge = 18, kBadFrame = 19, kPastTable = 20;
constexpr uint32_t kSeekTable = 72;
constexpr uint32_t kSkipMagic = 0x184D2A5Eu, kSeekMagic = 0x8F92EAB1u, kMaxFrames = 0x8000000u, kFraming = 17;

struct alignas(16) Lane { uint64_t src, len, begin, rlen; };   // src: the entry's address, len its bytes
static_assert(sizeof(Lane) == 32, "seek table lane");

// The other direction (zgpu_seek_index_export_seek_table): nrows rows WRITTEN as one seek table frame without checksums, from their
// exclusive prefix sums cd[2 * k] = C[k], cd[2 * k + 1] = D[k], k = 0 .. nrows (a zgm::Pair array seen as words) —
//   kSkipMagic | Frame_Size = 8 * nrows + 9 | nrows x { c_k u32, d_k u32 } | Number_Of_Frames | descriptor 0 | kSeekMagic
// seek_table_bytes(nrows) = 17 + 8 * nrows bytes, all little-endian, byte by byte: dst may have any alignment. A row the format cannot say
// (c_k or d_k above 0xFFFFFFFF; sums that decrease) is kSeekTable, and then NOTHING is written: the rows are looked at before the first
// store. Plain C++: g++ compiles it for tests/test_seektab_write_cpu.py.
static inline uint64_t seek_table_bytes(uint64_t nrows) { return kFraming + 8u * nrows; }
static inline uint32_t write_seek_table(const uint64_t* cd, uint32_t nrows, uint8_t* dst) {
  if (nrows > kMaxFrames) return kSeekTable;
  for (uint32_t k = 0; k < nrows; k++) {
    if (cd[2 * k + 2] < cd[2 * k] || cd[2 * k + 3] < cd[2 * k + 1]) return kSeekTable;
    if (cd[2 * k + 2] - cd[2 * k] > 0xFFFFFFFFull || cd[2 * k + 3] - cd[2 * k + 1] > 0xFFFFFFFFull) return kSeekTable;
  }
  auto le32 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); };
  le32(dst, kSkipMagic);
  le32(dst + 4, 8u * nrows + 9u);
  uint8_t* p = dst + 8;
  for (uint32_t k = 0; k < nrows; k++, p += 8) { le32(p, (uint32_t)(cd[2 * k + 2] - cd[2 * k])); le32(p + 4, (uint32_t)(cd[2 * k + 3] - cd[2 * k + 1])); }
  le32(p, nrows);
  p[4] = 0;
  le32(p + 5, kSeekMagic);
  return 0;
}
// The same frame with the Checksum fields (zgpu_seek_index_export_seek_table_ex, ZGPU_EXPORT_CHECKSUMS): rows of 12 bytes — c_k, d_k, sums[k] —,
// Frame_Size = 12 * nrows + 9, descriptor 0x80; seek_table_sums_bytes(nrows) = 17 + 12 * nrows bytes. The same refusals, nothing written.
static inline uint64_t seek_table_sums_bytes(uint64_t nrows) { return kFraming + 12u * nrows; }
static inline uint32_t write_seek_table_sums(const uint64_t* cd, const uint32_t* sums, uint32_t nrows, uint8_t* dst) {
  if (nrows > kMaxFrames) return kSeekTable;
  for (uint32_t k = 0; k < nrows; k++) {
    if (cd[2 * k + 2] < cd[2 * k] || cd[2 * k + 3] < cd[2 * k + 1]) return kSeekTable;
    if (cd[2 * k + 2] - cd[2 * k] > 0xFFFFFFFFull || cd[2 * k + 3] - cd[2 * k + 1] > 0xFFFFFFFFull) return kSeekTable;
  }
  auto le32 = [](uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); };
  le32(dst, kSkipMagic);
  le32(dst + 4, 12u * nrows + 9u);
  uint8_t* p = dst + 8;
  for (uint32_t k = 0; k < nrows; k++, p += 12) {
    le32(p, (uint32_t)(cd[2 * k + 2] - cd[2 * k])); le32(p + 4, (uint32_t)(cd[2 * k + 3] - cd[2 * k + 1])); le32(p + 8, sums[k]);
  }
  le32(p, nrows);
  p[4] = 0x80;
  le32(p + 5, kSeekMagic);
  return 0;
}

}  // namespace zgt
#endif  // ZG_SEEKTAB_TYPES

#if defined(ZX_DEV) && !defined(ZG_SEEKTAB_WAVE)
#define ZG_SEEKTAB_WAVE
namespace zgt {

// inclusive prefix sum over the wave
ZX_DEV uint64_t scan64(uint64_t v, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t lo = zx_shfl_up((uint32_t)v, o), hi = zx_shfl_up((uint32_t)(v >> 32), o);
    if (lane >= (uint32_t)o) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
ZX_DEV uint64_t lane64(uint64_t v, uint32_t l) {
  const uint32_t lo = zx_shfl((uint32_t)v, (int)l), hi = zx_shfl((uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// Checks 1 to 4 above, in that order, on the footer and the table frame's header: the `why` of a table that is not usable, else 0 and the
// number of rows, their size and where the table frame begins. No wave primitive: a wave calls it with every lane (the loads are wave-uniform),
// zg_seekmany.h's locate pass with one lane per entry. The rule's one definition.
template <class R> ZX_DEV uint32_t seektab_locate(const R& r, uint64_t len, uint32_t* nframes, uint32_t* entry_size, uint64_t* table) {
  uint32_t why = 0, nf = 0, es = 8;
  uint64_t tab = 0;
  if (len < kFraming) why = kNone;
  else {
    const uint32_t magic = r.ld4(len - 4), desc = r.ld1(len - 5);
    nf = r.ld4(len - 9);
    es = (desc & 0x80u) ? 12u : 8u;
    const uint64_t size = (uint64_t)nf * es + kFraming;
    if (magic != kSeekMagic) why = kNone;
    else if (desc & 0x7Cu) why = kReservedBits;
    else if (nf > kMaxFrames || size > len) why = kTooLarge;
    else {
      tab = len - size;
      const uint32_t m = r.ld4(tab), fs = r.ld4(tab + 4);
      if (m != kSkipMagic || fs != (uint32_t)(size - 8)) why = kBadFrame;
    }
  }
  *nframes = nf; *entry_size = es; *table = tab;
  return why;
}

// The record of a range of nonzero length from what the search found (the rules above: no first, src_hi > tab, a why). c_lo / d_lo: C_first,
// D_first; c_hi / d_hi: C_last + c_last, D_last + d_last; without a first all four are C_n, D_n. The record's one definition.
ZX_DEV zgk::Seek seektab_record(uint32_t why, uint64_t tab, uint32_t nf, bool have_first, uint32_t first, uint32_t last, uint64_t c_lo,
                                uint64_t d_lo, uint64_t c_hi, uint64_t d_hi) {
  zgk::Seek o;
  o.src_lo = o.src_hi = o.plain_lo = o.bound = o.plain_seen = 0;
  o.status = o.frames_skipped = o.frames_taken = o.nblocks = o.why = o.flags = 0;
  if (!why) {
    if (c_hi > tab) why = kPastTable;
    else {
      o.src_lo = c_lo; o.src_hi = c_hi; o.plain_lo = d_lo; o.plain_seen = d_hi; o.bound = d_hi - d_lo;
      o.frames_skipped = have_first ? first : nf; o.frames_taken = have_first ? last - first + 1 : 0u;
      o.flags = have_first ? 0u : zgk::kNothing;
    }
  }
  if (why) { o.status = kSeekTable; o.why = why; }
  return o;
}

// What the wave of one entry does; every lane calls it and every lane gets the record. R reads the entry (ld1 / ld4 / ld8 at an offset counted
// from the entry's first byte, any alignment; ld8 gives the two dwords of a table entry).
template <class R> ZX_DEV zgk::Seek seektab_entry(const R& r, uint64_t len, uint64_t begin, uint64_t rlen) {
  const uint32_t lane = zx_tid() & 63u;
  if (!rlen) {
    zgk::Seek o;
    o.src_lo = o.src_hi = o.plain_lo = o.bound = o.plain_seen = 0;
    o.status = o.frames_skipped = o.frames_taken = o.nblocks = o.why = o.flags = 0;
    return o;
  }
  uint32_t nf = 0, es = 8;
  uint64_t tab = 0;
  const uint32_t why = seektab_locate(r, len, &nf, &es, &tab);
  uint64_t cc = 0, cd = 0;                   // the sizes in front of this step
  uint64_t c_lo = 0, d_lo = 0, c_hi = 0, d_hi = 0;
  uint32_t first = 0, last = 0;
  bool have_first = false, have_last = false;
  if (!why) {
    const uint64_t end = rlen > UINT64_MAX - begin ? UINT64_MAX : begin + rlen, ent = tab + 8;
    uint32_t c = 0, d = 0;
    if (lane < nf) r.ld8(ent + (uint64_t)lane * es, &c, &d);
    for (uint32_t base = 0; base < nf; base += 64) {
      uint32_t nc = 0, nd = 0;
      if (base + 64 + lane < nf) r.ld8(ent + (uint64_t)(base + 64 + lane) * es, &nc, &nd);
      // (a lane behind the table holds 0, 0: lane 63 always holds the sums up to the end of the step)
      const uint64_t ce = cc + scan64(c, lane), de = cd + scan64(d, lane);
      const bool valid = base + lane < nf;
      if (!have_first) {
        const unsigned long long m = zx_ballot(valid && de > begin);
        if (m) {
          const uint32_t l = (uint32_t)__builtin_ctzll(m);
          have_first = true; first = base + l;
          c_lo = lane64(ce - c, l); d_lo = lane64(de - d, l);
        }
      }
      if (have_first) {
        const unsigned long long m = zx_ballot(valid && de >= end);
        if (m) {
          const uint32_t l = (uint32_t)__builtin_ctzll(m);
          have_last = true; last = base + l;
          c_hi = lane64(ce, l); d_hi = lane64(de, l);
          break;
        }
      }
      cc = lane64(ce, 63); cd = lane64(de, 63);
      c = nc; d = nd;
    }
    if (!have_first) { c_lo = cc; d_lo = cd; }
    if (!have_last) { c_hi = cc; d_hi = cd; last = nf - 1; }
  }
  return seektab_record(why, tab, nf, have_first, first, last, c_lo, d_lo, c_hi, d_hi);
}

// the record leaves as four 16-byte stores (out: 16-byte aligned)
ZX_DEV void seektab_store(zgk::Seek* out, const zgk::Seek& o) {
  uint8_t* p = (uint8_t*)out;
  ZxU4 v;
  v.x = (uint32_t)o.src_lo; v.y = (uint32_t)(o.src_lo >> 32); v.z = (uint32_t)o.src_hi; v.w = (uint32_t)(o.src_hi >> 32); zx_gst128(p, v);
  v.x = (uint32_t)o.plain_lo; v.y = (uint32_t)(o.plain_lo >> 32); v.z = (uint32_t)o.bound; v.w = (uint32_t)(o.bound >> 32); zx_gst128(p + 16, v);
  v.x = (uint32_t)o.plain_seen; v.y = (uint32_t)(o.plain_seen >> 32); v.z = o.status; v.w = o.frames_skipped; zx_gst128(p + 32, v);
  v.x = o.frames_taken; v.y = o.nblocks; v.z = o.why; v.w = o.flags; zx_gst128(p + 48, v);
}

}  // namespace zgt
#endif  // ZX_DEV
