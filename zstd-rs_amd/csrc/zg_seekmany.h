// zg_seekmany.h — many ranges over few seekable entries in DEVICE memory (zgpu_frames_seek_table_many_device,
// zgpu_gather_ranges_seek_table_device_src): every entry's seek table is scanned ONCE into prefix sums, and every range finds its rows in them by
// binary search. zg_seektab.h has the format, the rule and the record; this header answers the same question for m ranges in four launches,
// whatever m is, where zg_k_seektab scans the table once per range. Written against the zx_* primitives behind two accessors — a reader of the
// entry like zg_seektab.h's, and the prefix scratch — so that tests/test_seekmany_cpu.py runs this source on the CPU (tests/emu/zg_simt.h),
// counts every access outside [tab, len) and outside the scratch, and compares every record with zgt::seektab_entry's and with a Python model.
//
// The passes. A launch boundary orders them: no kernel waits for another workgroup, no flag is polled, nothing is looked back at.
//   1. locate    one LANE per entry: zgt::seektab_locate, the checks 1 to 4 of zg_seektab.h in their order (the routine zg_k_seektab runs; the
//                rule is defined once). 32 bytes per entry come back to the host — why, nframes, es, tab — because the host sizes the scratch
//                and the grids from nframes. No byte of a table comes back.
//   2. total     one WAVE per (entry, chunk). A chunk is CH rows, a template parameter: the product uses kChunkRows, the emulator tests also
//                128. The wave sums the chunk's compressed and decompressed sizes, 64 rows a step, with zg_k_seektab's step — lane l loads row
//                base + l (ld8), the next step's loads are issued in front of this step's two scan64 — and lane 0 stores the two totals.
//   3. prefix    one WAVE per (entry, chunk). The lanes stride over the totals of the chunks in front, a wave reduction (shfl_xor) adds them
//                up, and the wave scans its chunk again on those carries and stores the EXCLUSIVE prefixes C[k], D[k] of its rows; the last
//                chunk also stores C[nf], D[nf]. An entry without rows has one chunk without rows, which stores C[0] = D[0] = 0.
//   4. find      one LANE per range. With end = begin + rlen (saturating), on the entry's D:
//                  first = the smallest k with D[k + 1] > begin;  last = the smallest k >= first with D[k + 1] >= end, else nf - 1
//                both by binary search that keeps the SMALLEST such k (zero-size rows make D non-strict). The record is zgt::seektab_record's —
//                no first, C[last + 1] > tab (kPastTable, decided per range as zg_k_seektab decides it), a why with zeros — and leaves through
//                zgt::seektab_store's four 16-byte stores. rlen == 0: a record of zeros, nothing read.
//
// The scratch is an array of pairs { C, D } of 64-bit sums, 16 bytes each, 16-byte aligned: entry e's prefixes are pairs [pre, pre + nf + 1),
// its chunk totals pairs [tot, tot + nq) (nq = chunks_of(nf)). 16 * (nf + 1) bytes of prefixes per live entry. The host lays it out from the
// located nframes and hands every wave and lane its indices; nothing on the device computes where it may write.
//
// What is read of an entry: the footer and the table frame's header by locate, the first 8 bytes of rows by total and prefix — all inside
// [tab, len), dword or dwordx2 loads at byte addresses (gfx950 runs in unaligned access mode), never rounded down to an aligned address. find
// reads the scratch only. Every store is a vector store: global_store_dwordx4 of a pair or of a quarter of a record.
//
// gfx950 ISA (hipcc -O3 --save-temps), wave64, none uses scratch memory or LDS:
//   zg_k_seekmany_locate          14 VGPRs, 18 SGPRs
//   zg_k_seekmany_total<2048>     27 VGPRs, 30 SGPRs
//   zg_k_seekmany_prefix<2048>    29 VGPRs, 32 SGPRs
//   zg_k_seekmany_find            40 VGPRs, 22 SGPRs
// (.vgpr_count / .sgpr_count of the code object's metadata; .private_segment_fixed_size and .group_segment_fixed_size are 0, no spills.)
// All below the 64 VGPRs up to which a wave64 kernel keeps full occupancy. The scan primitive is zg_seektab.h's scan64 (__shfl_up:
// ds_bpermute_b32); the two probes of a binary-search step are one global_load_dwordx2 each, and the record's sums two global_load_dwordx4.
//
// Included twice by zg_kernels.hip: through zg_kernels.h for the types, and behind the zx_* primitives (and zg_seektab.h's wave part) for the
// routines.
#ifndef ZG_SEEKMANY_TYPES
#define ZG_SEEKMANY_TYPES
#include <stdint.h>
#include "zg_seektab.h"

namespace zgm {

constexpr uint32_t kThreads = 64;       // lanes of a workgroup of every kernel here: one wave
constexpr uint32_t kChunkRows = 2048;   // rows of a chunk in the product: 32 steps of a wave, 512 waves for a table of 2^20 rows

struct alignas(16) Ent { uint64_t src, len; };                                   // locate: the entry's address and bytes
struct alignas(16) Loc { uint64_t tab; uint32_t nf, es, why, pad0; uint64_t pad1; };   // what locate found (why != 0: nf = es = tab as far as known)
// a chunk of an entry for total and prefix: ent = the offset of row 0 from src; pre / tot = the scratch indices (in pairs) of the entry's
// prefixes and chunk totals; q of nq = which chunk
struct alignas(16) Work { uint64_t src, ent, pre, tot; uint32_t nf, es, q, nq; };
// a range for find: pre = the scratch index of its entry's prefixes; tab, nf, why = what locate found of that entry
struct alignas(16) Find { uint64_t begin, rlen, pre, tab; uint32_t nf, why, pad0, pad1; };
struct alignas(16) Pair { uint64_t c, d; };
static_assert(sizeof(Ent) == 16 && sizeof(Loc) == 32 && sizeof(Work) == 48 && sizeof(Find) == 48 && sizeof(Pair) == 16, "seek-many lanes");

// chunks of a table of nf rows: at least one, so that an empty table still gets its C[0], D[0]
inline uint32_t chunks_of(uint32_t nf, uint32_t ch) { return nf ? (nf + ch - 1) / ch : 1u; }

}  // namespace zgm
#endif  // ZG_SEEKMANY_TYPES

// ---- the groups of a gather call (host only; zg_ranges.cpp: gather_groups, tests/test_seekmany_cpu.py) ------------------------------------------
// The ranges of one entry whose rows overlap form a GROUP — the rows [gfirst, glast] its ranges take together, decoded once — and every range
// of it is a clip of the group's plaintext. The ranges that take rows are sorted by (entry, first row, last row, index); one that begins at or
// in front of the last row of the group in front of it joins that group. Plain host arithmetic on the records: no HIP call.
#ifndef ZG_SEEKMANY_GROUPS
#define ZG_SEEKMANY_GROUPS
#include <algorithm>
#include <vector>
namespace zgm {

struct Group { uint32_t entry, gfirst, glast; uint64_t c_lo, c_hi, d_lo, d_hi; };
struct Groups {
  std::vector<Group> groups;
  std::vector<uint32_t> group_of, clip_of;   // per range (0 where it takes no rows)
  std::vector<uint32_t> order;               // clip q is range order[q]; group g's clips are [first[g], first[g + 1])
  std::vector<uint32_t> first;               // groups + 1 slots
  std::vector<uint64_t> skip;                // per clip: where it begins in its group's plaintext (begin - d_lo)
};
// ranges[j] (anything with .entry, .begin, .len) has the record recs[j]: rows [frames_skipped, frames_skipped + frames_taken), bytes
// [src_lo, src_hi) and plaintext [plain_lo, plain_seen) of its entry. Only a range that takes rows is in a group: one that is not refused,
// has a length, and whose record has a status of 0 and frames_taken > 0.
template <class R> Groups group_ranges(const R* ranges, const zgk::Seek* recs, const uint8_t* refused, uint32_t m) {
  Groups o;
  for (uint32_t j = 0; j < m; j++)
    if (!refused[j] && ranges[j].len && !recs[j].status && recs[j].frames_taken) o.order.push_back(j);
  std::sort(o.order.begin(), o.order.end(), [&](uint32_t a, uint32_t b) {
    const zgk::Seek& x = recs[a], & y = recs[b];
    if (ranges[a].entry != ranges[b].entry) return ranges[a].entry < ranges[b].entry;
    if (x.frames_skipped != y.frames_skipped) return x.frames_skipped < y.frames_skipped;
    if (x.frames_taken != y.frames_taken) return x.frames_taken < y.frames_taken;
    return a < b;
  });
  o.group_of.assign(m, 0);
  o.clip_of.assign(m, 0);
  o.skip.reserve(o.order.size());
  for (uint32_t q = 0; q < (uint32_t)o.order.size(); q++) {
    const uint32_t j = o.order[q];
    const zgk::Seek& s = recs[j];
    const uint32_t first = s.frames_skipped, last = s.frames_skipped + s.frames_taken - 1;
    if (o.groups.empty() || o.groups.back().entry != ranges[j].entry || first > o.groups.back().glast) {
      o.groups.push_back(Group{ranges[j].entry, first, last, s.src_lo, s.src_hi, s.plain_lo, s.plain_seen});
      o.first.push_back(q);
    } else if (last > o.groups.back().glast) {
      Group& g = o.groups.back();
      g.glast = last; g.c_hi = s.src_hi; g.d_hi = s.plain_seen;
    }
    o.group_of[j] = (uint32_t)o.groups.size() - 1;
    o.clip_of[j] = q;
    o.skip.push_back(ranges[j].begin - o.groups.back().d_lo);
  }
  o.first.push_back((uint32_t)o.order.size());
  return o;
}

}  // namespace zgm
#endif  // ZG_SEEKMANY_GROUPS

#if defined(ZX_DEV) && !defined(ZG_SEEKMANY_WAVE)
#define ZG_SEEKMANY_WAVE
namespace zgm {

// locate: one lane, one entry
template <class R> ZX_DEV Loc seekmany_locate(const R& r, uint64_t len) {
  Loc o;
  o.pad0 = 0; o.pad1 = 0;
  o.why = zgt::seektab_locate(r, len, &o.nf, &o.es, &o.tab);
  return o;
}
ZX_DEV void seekmany_store_loc(Loc* out, const Loc& o) {
  uint8_t* p = (uint8_t*)out;
  ZxU4 v;
  v.x = (uint32_t)o.tab; v.y = (uint32_t)(o.tab >> 32); v.z = o.nf; v.w = o.es; zx_gst128(p, v);
  v.x = o.why; v.y = 0; v.z = 0; v.w = 0; zx_gst128(p + 16, v);
}

// The rows of chunk w.q, 64 a step, on the carries c0 / d0: the sums at the chunk's end; STORE: every row's exclusive prefixes go to the
// scratch. Every lane of the wave calls it and every lane gets the sums. S: the scratch (ld / ld_d / st of pair i).
template <uint32_t CH, bool STORE, class R, class S>
ZX_DEV void seekmany_chunk(const R& r, const S& s, const Work& w, uint64_t c0, uint64_t d0, uint64_t* ct, uint64_t* dt) {
  const uint32_t lane = zx_tid() & 63u;
  const uint32_t lo = w.q * CH, hi = w.nf - lo < CH ? w.nf : lo + CH;
  uint64_t cc = c0, cd = d0;
  uint32_t c = 0, d = 0;
  if (lo + lane < hi) r.ld8(w.ent + (uint64_t)(lo + lane) * w.es, &c, &d);
  for (uint32_t base = lo; base < hi; base += 64) {
    uint32_t nc = 0, nd = 0;
    if (base + 64 + lane < hi) r.ld8(w.ent + (uint64_t)(base + 64 + lane) * w.es, &nc, &nd);
    // (a lane behind the chunk holds 0, 0: lane 63 always holds the sums up to the end of the step)
    const uint64_t ce = cc + zgt::scan64(c, lane), de = cd + zgt::scan64(d, lane);
    if (STORE && base + lane < hi) s.st(w.pre + base + lane, ce - c, de - d);
    cc = zgt::lane64(ce, 63); cd = zgt::lane64(de, 63);
    c = nc; d = nd;
  }
  *ct = cc; *dt = cd;
}

// total: the wave of one chunk stores the chunk's two sums
template <uint32_t CH, class R, class S> ZX_DEV void seekmany_total(const R& r, const S& s, const Work& w) {
  uint64_t ct, dt;
  seekmany_chunk<CH, false>(r, s, w, 0, 0, &ct, &dt);
  if ((zx_tid() & 63u) == 0) s.st(w.tot + w.q, ct, dt);
}

// prefix: the totals in front of the chunk added up, the chunk scanned on them, its rows' exclusive prefixes stored
template <uint32_t CH, class R, class S> ZX_DEV void seekmany_prefix(const R& r, const S& s, const Work& w) {
  const uint32_t lane = zx_tid() & 63u;
  uint64_t c0 = 0, d0 = 0;
  for (uint32_t i = lane; i < w.q; i += 64) {
    uint64_t a, b;
    s.ld(w.tot + i, &a, &b);
    c0 += a; d0 += b;
  }
  for (int sh = 32; sh >= 1; sh >>= 1) {
    c0 += ((uint64_t)zx_shfl_xor((uint32_t)(c0 >> 32), sh) << 32) | zx_shfl_xor((uint32_t)c0, sh);
    d0 += ((uint64_t)zx_shfl_xor((uint32_t)(d0 >> 32), sh) << 32) | zx_shfl_xor((uint32_t)d0, sh);
  }
  uint64_t ct, dt;
  seekmany_chunk<CH, true>(r, s, w, c0, d0, &ct, &dt);
  if (lane == 0 && w.q + 1 == w.nq) s.st(w.pre + w.nf, ct, dt);
}

// find: one lane, one range
template <class S> ZX_DEV zgk::Seek seekmany_find(const S& s, const Find& f) {
  if (!f.rlen) {
    zgk::Seek o;
    o.src_lo = o.src_hi = o.plain_lo = o.bound = o.plain_seen = 0;
    o.status = o.frames_skipped = o.frames_taken = o.nblocks = o.why = o.flags = 0;
    return o;
  }
  if (f.why) return zgt::seektab_record(f.why, 0, 0, false, 0, 0, 0, 0, 0, 0);
  const uint64_t end = f.rlen > UINT64_MAX - f.begin ? UINT64_MAX : f.begin + f.rlen;
  const uint32_t nf = f.nf;
  uint32_t lo = 0, hi = nf;
  while (lo < hi) {   // the smallest k with D[k + 1] > begin
    const uint32_t mid = lo + (hi - lo) / 2;
    if (s.ld_d(f.pre + mid + 1) > f.begin) hi = mid; else lo = mid + 1;
  }
  const uint32_t first = lo;
  const bool have_first = first < nf;
  uint32_t last = nf - 1;
  uint64_t c_lo, d_lo, c_hi, d_hi;
  if (have_first) {
    hi = nf;
    while (lo < hi) {   // the smallest k >= first with D[k + 1] >= end
      const uint32_t mid = lo + (hi - lo) / 2;
      if (s.ld_d(f.pre + mid + 1) >= end) hi = mid; else lo = mid + 1;
    }
    if (lo < nf) last = lo;
    s.ld(f.pre + first, &c_lo, &d_lo);
    s.ld(f.pre + last + 1, &c_hi, &d_hi);
  } else {
    s.ld(f.pre + nf, &c_lo, &d_lo);
    c_hi = c_lo; d_hi = d_lo;
  }
  return zgt::seektab_record(0, f.tab, nf, have_first, first, last, c_lo, d_lo, c_hi, d_hi);
}

}  // namespace zgm
#endif  // ZX_DEV
