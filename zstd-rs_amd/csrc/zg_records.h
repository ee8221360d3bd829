// zg_records.h — the record index of a seek index handle (include/zgpu.h: "record index"): where every delimited record of an indexed entry's
// plaintext begins. zgpu_seek_index_records_device decodes every frame of an entry once, in runs, as the hash pass does, and where that pass
// reduces a frame to a digest this one finds every byte equal to the delimiter d: a side pass of three kernels over the submit's output, after
// sync() — zg_k_recs_count, zg_k_recs_scan, zg_k_recs_emit —, and zg_k_recs_find, the lookup that turns record numbers into byte ranges in
// front of the indexed gather. Written against the zx_* primitives behind reader and writer accessors: tests/test_records_cpu.py runs this
// source on the CPU (tests/emu/zg_emu_records.cpp) over accessors that count every access outside the windows below and compares every
// value with a model in Python (tests/records.py). records_host is the same definition with memchr over plaintext the host holds: the
// entries that are decoded alone (decode_alone_device).
//
// DEFINITIONS (include/zgpu.h has them for the caller). P: the entry's plaintext, L bytes. A record is a maximal run of bytes that ends in d,
// which belongs to it; if L > 0 and P[L - 1] != d the bytes behind the last delimiter are one more record, the open tail. R records have
// R + 1 offsets O[0] = 0 < O[1] < ... < O[R] = L; O[r], 0 < r < R (and r == R without an open tail), lies just behind the r-th delimiter.
// Record r is P[O[r], O[r + 1]). What the kernels find is the positions behind delimiters — already in the ENTRY's coordinates —; the host
// puts O[0] in front and, for an open tail, O[R] = L behind them.
//
// THE CHUNK TABLE (host-built, Batch::records_launch). Every decoded zstd frame of a sub-entry that stands at status 0 is cut into chunks of
// kChunk bytes of its [out_base, out_base + out_size) — the ranges the hash launch uses: a dictionary gap in front of a frame is in no chunk
// —; Chunk { out_off: where the chunk begins in the submit's output; base: the ENTRY coordinate of its first byte (the run's D[k0] + the
// frames of the run in front + the chunk's place in its frame); len <= kChunk; frame: the frame's index in the submit's frame-start table }.
// Chunks lie in the order of the plaintext, so chunk order is offset order. The host checks every chunk against the output's capacity and
// that the output begins at a multiple of 16 before anything is launched.
//
// One WAVE per chunk, count and emit alike (kThreads = 64, one workgroup = one wave). A chunk is kChunk = 4096 bytes: four steps of 64 lanes
// x 16 bytes. A wave, not a larger workgroup, because the emit kernel needs the exclusive prefix of the lanes' counts in position order: inside
// one wave that is six shuffles and no LDS, no barrier; a 64 KiB frame is 16 chunks, so a submit of a few MiB already fills the 256 CUs with
// waves, and a workgroup of several waves would buy nothing but a second scan level. out_off has every alignment 0 .. 15 (frames follow each
// other byte-tight), so a chunk is three parts:
//   head      the bytes in front of the first 16-byte boundary (at most 15, fewer if the chunk ends first): lane l < head loads ONE byte,
//             the ballot of the matches is the mask in position order;
//   interior  whole 16-byte groups: lane l of step s loads group 64 * s + l with ONE 16-byte load; per dword the bytes equal to d are found
//             with x = w ^ (d * 0x01010101), t = ~(((x & 0x7F7F7F7F) + 0x7F7F7F7F) | x | 0x7F7F7F7F): bit 7 of every byte of t that is zero in
//             x. The addition never carries out of a byte (0x7F + 0x7F < 0x100), so no byte's verdict depends on its neighbour: right for
//             d = 0x00 and d = 0xFF. (The shorter (x - 0x01010101) & ~x & 0x80808080 borrows across bytes and is NOT used.)
//   tail      what is left behind the last whole group (at most 15 bytes): one byte per lane and a ballot, like the head.
//
// zg_k_recs_count: the wave's matches, counted (population counts of the masks, summed over the wave by five xor-shuffles); lane 0 stores ONE
//   uint32_t, counts[chunk]. Reads: the chunk's bytes, each exactly once, nothing in front of out_off, nothing at or behind out_off + len.
// zg_k_recs_scan: ONE workgroup of kScanThreads = 256. Thread t sums counts[t * per .. (t + 1) * per), per = ceil(nchunks / 256); the 256 sums
//   are scanned (a wave scan of 64-bit values by shuffles, the four wave totals through 4 x 8 bytes of LDS); the thread walks its stretch
//   again and stores prefix[i], 64 bits: the exclusive prefix of the counts. Thread 0 stores the total; behind a barrier thread t stores
//   ftot[f] = P(fstart[f + 1]) - P(fstart[f]) for f = t, t + 256, ..., P(i) = prefix[i], P(nchunks) = the total. 8 bytes of total and 8 per
//   frame come back to the host, which sizes the submit's staging from them: the one round trip of the pass. A submit has at most
//   512 MiB / kChunk + one chunk per frame: one workgroup is enough.
// zg_k_recs_emit: the same waves over the same chunks recompute the masks. A lane of the interior may hold up to 16 delimiters, so a ballot
//   rank is not enough: the lanes' counts get an inclusive prefix by six shfl_up steps, and lane l's j-th delimiter at byte p of the chunk is
//   stored as the 64-bit value base + p + 1 at staging[prefix[chunk] + (matches of the parts and steps in front) + (lane prefix) + j]. Every
//   slot has exactly one writer: plain 8-byte vector stores, no atomics. A slot at or behind `total` is not stored (a submit's output does not
//   change between count and emit; the guard costs one compare).
// zg_k_recs_find: one LANE per record range, one launch whatever m is. Find { first, count, rpre (where the entry's O[0] lies in the handle's
//   array), nrec (R), flags (kStrip, kOpenTail), status, entry }. A lane whose status the host set stores { 0, 0, entry, status } and reads
//   nothing. Else [first, first + count) is clipped to [0, R) (the sum saturates): a = min(first, R), b = min(first + count, R); a >= b:
//   { O[a], 0 }; else begin = O[a], len = O[b] - O[a], and with kStrip len -= 1 unless b == R and the entry has an open tail (the last record
//   taken ends in no delimiter). Reads: O[a], and O[b] where a < b — two 8-byte loads of the handle's array, nothing of any entry. The
//   24-byte answer { begin, len, entry, status } leaves as three 8-byte vector stores.
//
// Device memory. The handle's array holds 8 bytes per offset, R + 1 per entry that has records. A pass keeps every run's staging (8 bytes per
// delimiter) until every run of every chosen entry has its verdict, then allocates the new array and fills it by device-to-device copies in
// row order: PEAK EXTRA DEVICE MEMORY IS TWICE THE FINAL ARRAY (stagings + the new array), beside the array a repeated pass replaces.
//
// gfx950 ISA (hipcc -O3 --save-temps, the code objects' metadata and the .s):
//   zg_k_recs_count  14 VGPRs, 21 SGPRs, no scratch (private segment 0), no LDS. The 24-byte Chunk comes in through scalar loads. 2
//                    global_load_ubyte (head, tail), in the loop 1 global_load_dwordx4 and 4 v_bcnt_u32_b32; 6 ds_bpermute_b32 for the wave
//                    sum; the count leaves lane 0 as 1 global_store_dword.
//   zg_k_recs_scan   22 VGPRs, 12 SGPRs, no scratch, 32 bytes of LDS (the four wave totals: 1 ds_write_b64, 2 ds_read_b128), 2 s_barrier. 4
//                    global_load_dword (a count in each of the two walks, fstart[f] and fstart[f + 1]), 12 ds_bpermute_b32 (the 64-bit wave
//                    scan: two per step), 2 global_load_dwordx2 (the prefixes at a frame's ends), 3 global_store_dwordx2 (a prefix, the total,
//                    a frame's total).
//   zg_k_recs_emit   31 VGPRs, 42 SGPRs, no scratch, no LDS. 2 global_load_ubyte, in the loop 1 global_load_dwordx4, 4 v_bcnt_u32_b32 and 7
//                    ds_bpermute_b32 (six steps of the prefix, the broadcast of lane 63); 1 s_bcnt1_i32_b64 per ballot; the offsets leave as
//                    global_store_dwordx2 (6 store sites: head, tail, one per dword of a group). prefix[chunk] is a scalar load.
//   zg_k_recs_find   20 VGPRs, 12 SGPRs, no scratch, no LDS. The 48-byte Find through 2 global_load_dwordx4 and 1 global_load_dwordx3, O[a]
//                    and O[b] through 2 global_load_dwordx2; the 24-byte answer leaves as 1 global_store_dwordx4 and 1 global_store_dwordx2.
//   No kernel has a spill or an atomic: every store above is a vector store.
//
// Included twice by zg_kernels.hip: through zg_kernels.h for the types, and behind the zx_* primitives for the wave routines.
#ifndef ZG_RECORDS_TYPES
#define ZG_RECORDS_TYPES
#include <stdint.h>
#include <string.h>
#include <vector>

namespace zgr {

constexpr uint32_t kChunk = 4096;        // plaintext bytes per chunk: one wave, four steps of 64 x 16 bytes
constexpr uint32_t kThreads = 64;        // zg_k_recs_count / _emit: one wave per chunk; zg_k_recs_find: lanes per workgroup
constexpr uint32_t kScanThreads = 256;   // zg_k_recs_scan: one workgroup
constexpr uint32_t kStrip = 1u, kOpenTail = 2u;   // Find::flags (kStrip is ZGPU_RECORDS_STRIP)

struct Chunk { uint64_t out_off, base; uint32_t len, frame; };
static_assert(sizeof(Chunk) == 24, "chunk table");
struct alignas(16) Find { uint64_t first, count, rpre, nrec; uint32_t flags, status, entry, pad; };
static_assert(sizeof(Find) == 48, "record find lanes");
struct Found { uint64_t begin, len; uint32_t entry, status; };
static_assert(sizeof(Found) == 24, "record find answers");

// the chunks of one frame: [out_off, out_off + size) of the output, whose first byte is byte `base` of its entry
inline void cut_chunks(uint64_t out_off, uint64_t size, uint64_t base, uint32_t frame, std::vector<Chunk>* to) {
  for (uint64_t at = 0; at < size; at += kChunk) to->push_back(Chunk{out_off + at, base + at, (uint32_t)(size - at < kChunk ? size - at : kChunk), frame});
}

// The same definition over plaintext the HOST holds (an entry decoded alone): the positions just behind every byte equal to d, in the
// entry's coordinates (the buffer's first byte is byte `base` of the entry), appended to *to.
inline void records_host(const uint8_t* p, uint64_t n, uint32_t d, uint64_t base, std::vector<uint64_t>* to) {
  for (uint64_t at = 0; at < n;) {
    const uint8_t* q = (const uint8_t*)memchr(p + at, (int)d, (size_t)(n - at));
    if (!q) break;
    at = (uint64_t)(q - p) + 1;
    to->push_back(base + at);
  }
}

// what zg_k_recs_find answers, for the host (tests and the harness compare the lanes with it)
inline Found find_host(const uint64_t* o, const Find& f) {
  if (f.status) return Found{0, 0, f.entry, f.status};
  const uint64_t a = f.first < f.nrec ? f.first : f.nrec;
  const uint64_t e = f.count > UINT64_MAX - f.first ? UINT64_MAX : f.first + f.count;
  const uint64_t b = e < f.nrec ? e : f.nrec;
  const uint64_t begin = o[f.rpre + a];
  if (a >= b) return Found{begin, 0, f.entry, 0};
  uint64_t len = o[f.rpre + b] - begin;
  if ((f.flags & kStrip) && !(b == f.nrec && (f.flags & kOpenTail))) len -= 1;
  return Found{begin, len, f.entry, 0};
}

// The layout of a record batch (include/zgpu.h: "record batches"), decided on the host from the lookup's lengths alone, before anything is
// decoded. len[j]: range j's byte length (0 where the lookup gave a status). want = len, or min(len, width) under truncate with width > 0.
// Padded: at = j * width, slot = width, total = m * width. Packed: at = the sum of the wants in front, slot = want, total = the sum of all.
// False — and nothing of *rows is to be used — if a product or a sum does not fit in 64 bits.
constexpr uint32_t kBatchPadded = 0, kBatchPacked = 1;
struct Row { uint64_t at, slot, want; };
inline bool plan_rows(const uint64_t* len, uint32_t m, uint32_t layout, bool truncate, uint64_t width, Row* rows, uint64_t* total, uint32_t* truncated) {
  *total = 0; *truncated = 0;
  const bool cut = truncate && width > 0;
  if (layout == kBatchPadded && width && m > UINT64_MAX / width) return false;
  uint64_t at = 0;
  for (uint32_t j = 0; j < m; j++) {
    const uint64_t want = cut && len[j] > width ? width : len[j];
    if (want != len[j]) (*truncated)++;
    const uint64_t slot = layout == kBatchPadded ? width : want;
    if (slot > UINT64_MAX - at) return false;
    rows[j] = Row{at, slot, want};
    at += slot;
  }
  *total = at;
  return true;
}

}  // namespace zgr
#endif  // ZG_RECORDS_TYPES

#if defined(ZX_DEV) && !defined(ZG_RECORDS_WAVE)
#define ZG_RECORDS_WAVE
namespace zgr {

// bit 7 of every byte of the result: that byte of w equals the byte replicated in d4. No carry leaves a byte.
ZX_DEV uint32_t eq_mask(uint32_t w, uint32_t d4) {
  const uint32_t x = w ^ d4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
ZX_DEV uint32_t popc32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
ZX_DEV uint32_t popc64(unsigned long long v) { return (uint32_t)__builtin_popcountll(v); }

// the three parts of a chunk that begins at out_off: head bytes, whole groups, tail bytes
struct Parts { uint32_t head, groups, tail; };
ZX_DEV Parts parts_of(uint64_t out_off, uint32_t len) {
  Parts p;
  const uint32_t to_boundary = (uint32_t)((16u - (uint32_t)(out_off & 15u)) & 15u);
  p.head = to_boundary < len ? to_boundary : len;
  p.groups = (len - p.head) >> 4;
  p.tail = (len - p.head) & 15u;
  return p;
}

// the sum of v over the wave, in every lane
ZX_DEV uint32_t wave_sum(uint32_t v) {
  for (int m = 1; m < 64; m <<= 1) v += zx_shfl_xor(v, m);
  return v;
}
// the inclusive prefix of v over the lanes
ZX_DEV uint32_t wave_incl(uint32_t v, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = zx_shfl_up(v, o);
    if ((int)lane >= o) v += t;
  }
  return v;
}

// zg_k_recs_count's wave: every lane calls it, every lane gets the chunk's count. R: ld1(off) one byte, ld16(off) 16 bytes at a multiple of 16
// — offsets into the submit's output.
template <class R> ZX_DEV uint32_t recs_count_chunk(const R& r, uint64_t out_off, uint32_t len, uint32_t d) {
  const uint32_t lane = zx_tid() & 63u;
  const uint32_t d4 = (d & 0xFFu) * 0x01010101u;
  const Parts p = parts_of(out_off, len);
  uint32_t n = 0;
  if (lane < p.head && r.ld1(out_off + lane) == (d & 0xFFu)) n++;
  const uint64_t in0 = out_off + p.head;
  for (uint32_t g = lane; g < p.groups; g += 64) {
    const ZxU4 v = r.ld16(in0 + 16ull * g);
    n += popc32(eq_mask(v.x, d4)) + popc32(eq_mask(v.y, d4)) + popc32(eq_mask(v.z, d4)) + popc32(eq_mask(v.w, d4));
  }
  if (lane < p.tail && r.ld1(in0 + 16ull * p.groups + lane) == (d & 0xFFu)) n++;
  return wave_sum(n);
}

// zg_k_recs_emit's wave. W: st(slot, value), one 64-bit store; slots at or behind `total` are dropped. slot0: prefix[chunk].
template <class R, class W> ZX_DEV void recs_emit_chunk(const R& r, const W& w, uint64_t out_off, uint32_t len, uint64_t base, uint32_t d, uint64_t slot0,
                                                        uint64_t total) {
  const uint32_t lane = zx_tid() & 63u;
  const uint32_t d4 = (d & 0xFFu) * 0x01010101u;
  const Parts p = parts_of(out_off, len);
  uint64_t slot = slot0;
  const unsigned long long below = (1ull << lane) - 1ull;
  {   // head: one byte per lane, the ballot is the mask in position order
    const bool hit = lane < p.head && r.ld1(out_off + lane) == (d & 0xFFu);
    const unsigned long long m = zx_ballot(hit);
    const uint64_t at = slot + popc64(m & below);
    if (hit && at < total) w.st(at, base + lane + 1);
    slot += popc64(m);
  }
  const uint64_t in0 = out_off + p.head;
  for (uint32_t g0 = 0; g0 < p.groups; g0 += 64) {   // (uniform: every lane takes every step)
    const uint32_t g = g0 + lane;
    uint32_t t[4] = {0, 0, 0, 0};
    if (g < p.groups) {
      const ZxU4 v = r.ld16(in0 + 16ull * g);
      t[0] = eq_mask(v.x, d4); t[1] = eq_mask(v.y, d4); t[2] = eq_mask(v.z, d4); t[3] = eq_mask(v.w, d4);
    }
    const uint32_t n = popc32(t[0]) + popc32(t[1]) + popc32(t[2]) + popc32(t[3]);
    const uint32_t incl = wave_incl(n, lane);
    uint64_t at = slot + (incl - n);
    const uint64_t pos0 = base + p.head + 16ull * g + 1;   // (the value of a delimiter at byte 0 of the group)
    for (uint32_t q = 0; q < 4; q++)
      for (uint32_t m = t[q]; m; m &= m - 1) {
        const uint32_t byte = 4 * q + ((uint32_t)__builtin_ctz(m) >> 3);
        if (at < total) w.st(at, pos0 + byte);
        at++;
      }
    slot += zx_shfl(incl, 63);
  }
  {   // tail
    const uint64_t t0 = in0 + 16ull * p.groups;
    const bool hit = lane < p.tail && r.ld1(t0 + lane) == (d & 0xFFu);
    const unsigned long long m = zx_ballot(hit);
    const uint64_t at = slot + popc64(m & below);
    if (hit && at < total) w.st(at, base + (t0 - out_off) + lane + 1);
  }
}

// the inclusive prefix of a 64-bit value over the lanes of a wave
ZX_DEV uint64_t wave_incl64(uint64_t v, uint32_t lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = ((uint64_t)zx_shfl_up((uint32_t)(v >> 32), o) << 32) | zx_shfl_up((uint32_t)v, o);
    if ((int)lane >= o) v += t;
  }
  return v;
}

// zg_k_recs_scan's workgroup of kScanThreads. C: ld(i) = counts[i], i < nchunks; F: ld(f) = fstart[f], f <= nframes; P: the prefixes —
// st(i, v) and ld(i), i < nchunks —; T: total(v), ftot(f, v). lds: kScanThreads / 64 words of 64 bits.
template <class C, class F, class P, class T>
ZX_DEV void recs_scan(const C& c, const F& fs, const P& pre, const T& out, uint32_t nchunks, uint32_t nframes, uint64_t* lds) {
  const uint32_t t = zx_tid(), lane = t & 63u, wave = t >> 6;
  const uint32_t per = (nchunks + kScanThreads - 1) / kScanThreads;
  const uint64_t lo = (uint64_t)t * per < nchunks ? (uint64_t)t * per : nchunks;
  const uint64_t hi = lo + per < nchunks ? lo + per : nchunks;
  uint64_t s = 0;
  for (uint64_t i = lo; i < hi; i++) s += c.ld(i);
  const uint64_t incl = wave_incl64(s, lane);
  if (lane == 63) lds[wave] = incl;
  zx_syncthreads();
  uint64_t at = incl - s, total = 0;
  for (uint32_t k = 0; k < kScanThreads / 64; k++) { if (k < wave) at += lds[k]; total += lds[k]; }
  for (uint64_t i = lo; i < hi; i++) { pre.st(i, at); at += c.ld(i); }
  if (t == 0) out.total(total);
  zx_syncthreads();
  for (uint32_t f = t; f < nframes; f += kScanThreads) {
    const uint32_t a = fs.ld(f), b = fs.ld(f + 1);
    const uint64_t pa = a < nchunks ? pre.ld(a) : total, pb = b < nchunks ? pre.ld(b) : total;
    out.ftot(f, pb - pa);
  }
}

// zg_k_recs_find's lane. O: ld(i), one 64-bit load of the handle's array.
template <class O> ZX_DEV Found recs_find(const O& o, const Find& f) {
  Found r;
  r.begin = 0; r.len = 0; r.entry = f.entry; r.status = f.status;
  if (f.status) return r;
  const uint64_t a = f.first < f.nrec ? f.first : f.nrec;
  const uint64_t e = f.count > UINT64_MAX - f.first ? UINT64_MAX : f.first + f.count;
  const uint64_t b = e < f.nrec ? e : f.nrec;
  r.begin = o.ld(f.rpre + a);
  if (a >= b) return r;
  r.len = o.ld(f.rpre + b) - r.begin;
  if ((f.flags & kStrip) && !(b == f.nrec && (f.flags & kOpenTail))) r.len -= 1;
  return r;
}

}  // namespace zgr
#endif  // ZX_DEV
