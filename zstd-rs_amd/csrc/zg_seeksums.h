// zg_seeksums.h — zg_k_seeksums: does the seek table of an entry in DEVICE memory vouch for the frames that were decoded of it
// (ZGPU_DEVICE_VERIFY_SEEK_TABLE of zgpu_decode_ranges_seek_table_device_src)? The Checksum fields of the seekable format's table — the low 32
// bits of XXH64 (seed 0) of each frame's plaintext — are compared on the device with the digests the hash kernel left there: no byte of the
// table crosses to the host, 32 bytes per entry come back. One WAVE per entry, one launch per submit, on the engine's first stream behind the
// hash kernel. Written against the zx_* primitives like zg_seektab.h (whose format description, scan64 and lane64 it uses) behind two reader
// accessors: tests/test_seeksums_cpu.py runs this source with readers that count every access outside the windows below and compares every
// field with a model in Python (tests/seeksums.py). sums_rows / locate_rows are the same rule in plain C++ over rows the host holds: the
// entries that are decoded alone (decode_alone_device) cross to the host anyway. The rule itself is written twice, once for the wave
// (sums_step, Tally) and once for the host (sums_host): this routine and zg_idxsums.h's differ in where a row's R_k, c_k and sum come from.
//
// THE RULE (quoted in include/zgpu.h and DESIGN.md 4.7c). An entry whose selection is table rows [first, first + taken), R_k = C_k - C_first:
//   - a decoded zstd frame COINCIDES with row k if it begins at selection offset R_k and is c_k bytes long;
//   - a frame that coincides with a row and was hashed is COMPARED: the low 32 bits of its digest against the row's Checksum;
//   - rows that no decoded zstd frame coincides with are not looked at (skippable frames entered with size 0, rows outside the selection);
//   - the entry fails (ZGPU_E_SEEK_CHECKSUM_MISMATCH) if a compared frame differs, if a decoded zstd frame coincides with no row — nothing
//     vouches for it —, or if the table carries no checksums (Checksum_Flag clear);
//   - an entry of which no zstd frame is decoded (a range of length 0, nothing selected, skippable frames only) is not looked at at all.
// vouched() is that verdict from the record; the host applies it behind every other verdict of the entry.
//
// Inputs. Per entry a Lane: the WHOLE entry's address and length (not the selection's), first, taken, and [frame_lo, frame_lo + frame_n) —
// its slice of the submit's frame list. A Frame, one per decoded zstd frame in source order: begin (selection-relative, strictly increasing
// inside a slice), clen (compressed bytes; a frame of 2^32 bytes or more is left out of the list: no row can hold its length, and the host counts
// it as coinciding with none), slot (its digest's index in the hash kernel's output, kNotHashed: not hashed). The digests: Batch::hash_launch's
// output, 8 bytes per slot, still in device memory.
//
// The wave locates the table again from the footer and redoes zg_seektab.h's checks in its order (kNone, kReservedBits, kTooLarge, kBadFrame),
// then first + taken > Number_Of_Frames: kRows, and a slot at or behind the digest count: kList. A source that changed since the seek becomes
// a `why` — the host makes it ZGPU_E_INTERNAL with a last_error —, never a stray access. Any why: every other field of the record is 0.
// The scan, 64 rows a step from `first`: lane l loads row first + base + l — three dwords (c, d, Checksum) at a byte address, two where the table
// has no checksums — with the next step's loads issued in front of this step's scan; ONE 64-bit inclusive prefix sum of c on a wave-uniform
// carry gives R_k = sum - c_k; sums_step (the row's search and compare) and Tally (the wave's counts) below say the rest: coinciding,
// compared and differing frames (coinciding - compared: the unhashed ones) and first_bad, the first table row that differs (kNoRow: none).
// Two rows never coincide with one frame: rows that share an R_k all have c = 0 but the last.
// The record, 32 bytes, leaves lane 0 as two 16-byte stores: rows (= taken), coinciding, compared, differing, first_bad, why, flags
// (kNoChecksums), 0.
//
// What the wave reads: the 9 footer bytes; the 8 bytes of the table frame's header; rows [first, first + taken) — at most the 12 (or 8) bytes of
// each, nothing of the rows in front or behind; its own slice of the frame list; the low dwords of the digests that slice names. Nothing in
// front of the table frame, nothing at or behind len: an entry may end flush with its allocation. The table sits at any alignment, so a row
// is loaded dword by dword at a byte address (gfx950 runs in unaligned access mode); nothing is rounded down to an aligned address.
//
// gfx950 ISA of zg_k_seeksums (hipcc -O3 --save-temps): 23 VGPRs, 64 SGPRs, no scratch, no LDS, occupancy 8 waves per SIMD. Loads: 2 s_load_dwordx4
// of the entry's 32-byte Lane; of the footer 2 global_load_dword (magic, Number_Of_Frames) and 1 global_load_sbyte (descriptor); 1
// global_load_dwordx2 of the frame's magic and Frame_Size; of a row 2 global_load_dword, c at offset 0 and the Checksum at offset 8 — the
// source asks for the row's three dwords, the compiler drops the Decompressed_Size nothing uses (1 global_load_dword where the table has no
// checksums) —, the first step's in front of the loop and in the loop the next step's, issued in front of the scan; per probe of the binary
// search 1 global_load_dwordx2 (a frame's begin), at the hit 1 global_load_dwordx4 (the Frame) and 1 global_load_dword (the digest's low
// half). The footer and header are wave-uniform (v_readfirstlane): the loop and the checks branch on SGPRs; only the search and the compare
// diverge. 13 ds_bpermute_b32: 11 for the one 64-bit prefix sum (the first stage's high halves are known zero) and 2 for the carry's broadcast;
// 3 s_bcnt1_i32_b64 and 1 s_ff1_i32_b64 for the counts and first_bad. The record leaves lane 0 as 2 global_store_dwordx4. Vector stores both.
//
// Included twice by zg_kernels.hip: through zg_kernels.h for the types, and behind the zx_* primitives (and zg_seektab.h's wave part) for the
// wave routine.
#ifndef ZG_SEEKSUMS_TYPES
#define ZG_SEEKSUMS_TYPES
#include <stdint.h>
#include <string.h>
#include "zg_types.h"
#include "zg_seektab.h"

namespace zgv {

constexpr uint32_t kThreads = 64;                     // lanes of a workgroup of zg_k_seeksums: one wave, one entry
constexpr uint32_t kSeekChecksumMismatch = 73;        // ZGPU_E_SEEK_CHECKSUM_MISMATCH
constexpr uint32_t kNotHashed = 0xFFFFFFFFu;          // Frame::slot of a frame that was not hashed
constexpr uint32_t kNoRow = 0xFFFFFFFFu;              // Sums::first_bad: no compared frame differs
constexpr uint32_t kRows = 21, kList = 22;            // Sums::why, besides zgt::kNone .. zgt::kBadFrame
constexpr uint32_t kNoChecksums = 1;                  // Sums::flags: the table's Checksum_Flag is clear

struct alignas(16) Lane { uint64_t src, len; uint32_t first, taken, frame_lo, frame_n; };
struct alignas(16) Frame { uint64_t begin; uint32_t clen, slot; };
struct alignas(16) Sums { uint32_t rows, coinciding, compared, differing, first_bad, why, flags, pad; };
static_assert(sizeof(Lane) == 32 && sizeof(Frame) == 16 && sizeof(Sums) == 32, "seek table checksum records");

// the verdict: the table vouches for all nframes decoded zstd frames of the entry (why != 0 is the host's ZGPU_E_INTERNAL, not a verdict)
inline bool vouched(const Sums& s, uint32_t nframes) { return !s.why && !(s.flags & kNoChecksums) && !s.differing && s.coinciding == nframes; }

// ---- the same rule over rows the HOST holds (entries decoded alone) ------------------------------------------------------------------------
// Where rows [first, first + taken) of an entry of len bytes lie, from the 9 bytes of its footer: *es = bytes per row, *rows_off = the first
// row's offset. The wave's checks in the wave's order, without the one of the table frame's header (kBadFrame): the seek checked it, the host
// path does not fetch it again, and every offset handed out lies inside [0, len) whatever the header holds. Returns the `why`, 0 if the
// rows can be read.
inline uint32_t locate_rows(const uint8_t footer[9], uint64_t len, uint32_t first, uint32_t taken, uint32_t* es, uint64_t* rows_off) {
  if (len < zgt::kFraming) return zgt::kNone;
  uint32_t nf, magic;
  memcpy(&nf, footer, 4); memcpy(&magic, footer + 5, 4);
  const uint32_t desc = footer[4];
  *es = (desc & 0x80u) ? 12u : 8u;
  const uint64_t size = (uint64_t)nf * *es + zgt::kFraming;
  if (magic != zgt::kSeekMagic) return zgt::kNone;
  if (desc & 0x7Cu) return zgt::kReservedBits;
  if (nf > zgt::kMaxFrames || size > len) return zgt::kTooLarge;
  if ((uint64_t)first + taken > nf) return kRows;
  *rows_off = len - size + 8 + (uint64_t)first * *es;
  return 0;
}
// THE RULE over rows the host holds, once (sums_rows below and zg_idxsums.h's sums_pairs hand it their rows): row(k, &at, &len, &sum) gives
// R_k, c_k and the Checksum of row k, asked for k = 0 .. taken - 1 in that order; sums: the rows carry checksums; fr[0 .. nfr): the entry's
// frames; dig[0 .. ndig): their digests by slot. Every row searches on its own, as the wave's lanes do: the pairs of a stale handle need not
// increase. (Over a table's rows a merge would find the same frame: begin is strictly increasing inside a slice.)
template <class Row> Sums sums_host(Row row, bool sums, uint32_t first, uint32_t taken, const Frame* fr, uint32_t nfr, const uint64_t* dig, uint32_t ndig) {
  Sums o{taken, 0, 0, 0, kNoRow, 0, sums ? 0u : kNoChecksums, 0};
  for (uint32_t k = 0; k < taken; k++) {
    uint64_t at, len;
    uint32_t sum;
    row(k, &at, &len, &sum);
    uint32_t lo = 0, hi = nfr;   // the first frame that begins at or behind R_k
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (fr[mid].begin < at) lo = mid + 1; else hi = mid;
    }
    if (lo == nfr || fr[lo].begin != at || fr[lo].clen != len) continue;
    o.coinciding++;
    if (!sums || fr[lo].slot == kNotHashed) continue;
    if (fr[lo].slot >= ndig) return Sums{0, 0, 0, 0, 0, kList, 0, 0};
    o.compared++;
    if ((uint32_t)dig[fr[lo].slot] != sum) { o.differing++; if (o.first_bad == kNoRow) o.first_bad = first + k; }
  }
  return o;
}
// rows: taken rows of es bytes
inline Sums sums_rows(const uint8_t* rows, uint32_t es, uint32_t first, uint32_t taken, const Frame* fr, uint32_t nfr, const uint64_t* dig, uint32_t ndig) {
  uint64_t r = 0;   // R_k: the compressed sizes in front of row k
  return sums_host([&](uint32_t k, uint64_t* at, uint64_t* len, uint32_t* sum) {
    uint32_t c;
    memcpy(&c, rows + (size_t)k * es, 4);
    *sum = 0;
    if (es == 12) memcpy(sum, rows + (size_t)k * es + 8, 4);
    *at = r; *len = c;
    r += c;
  }, es == 12, first, taken, fr, nfr, dig, ndig);
}

}  // namespace zgv
#endif  // ZG_SEEKSUMS_TYPES

#if defined(ZX_DEV) && !defined(ZG_SEEKSUMS_WAVE)
#define ZG_SEEKSUMS_WAVE
namespace zgv {

// ---- what does not depend on where the rows come from (zg_idxsums.h's wave uses the same two) ------------------------------------------------
// The step of one row: this lane holds row k = (R_k, c_k, sum_k) — in: it lies inside the selection; sums: the rows carry checksums. The lane
// binary-searches its slice for the first frame that begins at or behind R_k, and at a hit loads the frame, checks the length (a c_k above
// 0xFFFFFFFF matches no frame), loads the digest's low dword and compares. F: begin(i), frame(i, &begin, &clen, &slot) for i < nfr,
// digest(slot) = the low 32 bits, for slot < ndig.
// What comes out, four predicates (separate bools: a struct of them is packed into one VGPR, the bools stay lane masks in SGPRs): hit — a
// frame coincides with the row; cmp — it was hashed and is compared; diff — it differs; oob — its slot lies at or behind the digest count.
template <class F> ZX_DEV void sums_step(const F& f, uint64_t rk, uint64_t c, uint32_t s, bool in, bool sums, uint32_t nfr, uint32_t ndig,
                                         bool& hit, bool& cmp, bool& diff, bool& oob) {
  hit = cmp = diff = oob = false;
  if (in && nfr) {
    uint32_t lo = 0, hi = nfr;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (f.begin(mid) < rk) lo = mid + 1; else hi = mid;
    }
    if (lo < nfr) {
      uint64_t fb;
      uint32_t fc, slot;
      f.frame(lo, &fb, &fc, &slot);
      hit = fb == rk && (uint64_t)fc == c;
      if (hit && sums && slot != kNotHashed) {
        oob = slot >= ndig;
        cmp = !oob;
        if (cmp) diff = f.digest(slot) != s;
      }
    }
  }
}
// The tally of a wave: tally_add takes every lane's four predicates of the 64 rows from row0 (= first + base) — three ballots and population counts, a
// find-first-set of the first step that differs —, tally_record writes them into an all-zero record: kList alone if a slot left the digests.
struct Tally { uint32_t coinciding = 0, compared = 0, differing = 0, first_bad = kNoRow; bool bad_list = false; };
ZX_DEV void tally_add(Tally& a, bool hit, bool cmp, bool diff, bool oob, uint32_t row0) {
  const unsigned long long mh = zx_ballot(hit), mc = zx_ballot(cmp), md = zx_ballot(diff);
  a.coinciding += (uint32_t)__builtin_popcountll(mh); a.compared += (uint32_t)__builtin_popcountll(mc); a.differing += (uint32_t)__builtin_popcountll(md);
  if (md && a.first_bad == kNoRow) a.first_bad = row0 + (uint32_t)__builtin_ctzll(md);
  if (zx_ballot(oob)) a.bad_list = true;
}
ZX_DEV Sums sums_zero() {
  Sums o;
  o.rows = o.coinciding = o.compared = o.differing = o.first_bad = o.why = o.flags = o.pad = 0;
  return o;
}
ZX_DEV void tally_record(const Tally& a, uint32_t taken, uint32_t flags, Sums& o) {
  if (a.bad_list) o.why = kList;
  else { o.rows = taken; o.coinciding = a.coinciding; o.compared = a.compared; o.differing = a.differing; o.first_bad = a.first_bad; o.flags = flags; }
}

// What the wave of one entry does; every lane calls it and every lane gets the record. R reads the entry (ld1 / ld4 / ld8 / ld12 at an offset
// counted from the entry's first byte, any alignment; ld8 and ld12 give c, d (and the Checksum) of a row). F reads the entry's slice of the
// frame list and the digests (sums_step).
template <class R, class F> ZX_DEV Sums seeksums_entry(const R& r, const F& f, uint64_t len, uint32_t first, uint32_t taken, uint32_t nfr, uint32_t ndig) {
  const uint32_t lane = zx_tid() & 63u;
  Sums o = sums_zero();
  if (!taken) return o;
  uint32_t why = 0, nf = 0, es = 8;
  uint64_t tab = 0;
  if (len < zgt::kFraming) why = zgt::kNone;
  else {
    const uint32_t magic = r.ld4(len - 4), desc = r.ld1(len - 5);
    nf = r.ld4(len - 9);
    es = (desc & 0x80u) ? 12u : 8u;
    const uint64_t size = (uint64_t)nf * es + zgt::kFraming;
    if (magic != zgt::kSeekMagic) why = zgt::kNone;
    else if (desc & 0x7Cu) why = zgt::kReservedBits;
    else if (nf > zgt::kMaxFrames || size > len) why = zgt::kTooLarge;
    else {
      tab = len - size;
      const uint32_t m = r.ld4(tab), fs = r.ld4(tab + 4);
      if (m != zgt::kSkipMagic || fs != (uint32_t)(size - 8)) why = zgt::kBadFrame;
      else if ((uint64_t)first + taken > nf) why = kRows;
    }
  }
  o.why = why;
  if (!why) {
    const bool sums = es == 12;
    const uint64_t ent = tab + 8 + (uint64_t)first * es;
    uint64_t carry = 0;                        // the compressed sizes in front of this step
    uint32_t c = 0, d = 0, s = 0;
    Tally t;
    if (lane < taken) { if (sums) r.ld12(ent + (uint64_t)lane * es, &c, &d, &s); else r.ld8(ent + (uint64_t)lane * es, &c, &d); }
    for (uint32_t base = 0; base < taken; base += 64) {
      uint32_t nc = 0, nd = 0, ns = 0;
      if (base + 64 + lane < taken) {
        const uint64_t at = ent + (uint64_t)(base + 64 + lane) * es;
        if (sums) r.ld12(at, &nc, &nd, &ns); else r.ld8(at, &nc, &nd);
      }
      // (a lane behind the selection holds c = 0: lane 63 always holds the sum up to the end of the step)
      const uint64_t ce = carry + zgt::scan64(c, lane);
      bool hit, cmp, diff, oob;
      sums_step(f, ce - c, c, s, base + lane < taken, sums, nfr, ndig, hit, cmp, diff, oob);
      tally_add(t, hit, cmp, diff, oob, first + base);
      carry = zgt::lane64(ce, 63);
      c = nc; d = nd; s = ns;
    }
    (void)d;
    tally_record(t, taken, sums ? 0u : kNoChecksums, o);
  }
  return o;
}

// the record leaves as two 16-byte stores (out: 16-byte aligned)
ZX_DEV void seeksums_store(Sums* out, const Sums& o) {
  uint8_t* p = (uint8_t*)out;
  ZxU4 v;
  v.x = o.rows; v.y = o.coinciding; v.z = o.compared; v.w = o.differing; zx_gst128(p, v);
  v.x = o.first_bad; v.y = o.why; v.z = o.flags; v.w = 0; zx_gst128(p + 16, v);
}

}  // namespace zgv
#endif  // ZX_DEV
