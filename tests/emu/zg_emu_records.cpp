// zg_emu_records.cpp — TEST-ONLY: runs the SOURCE of the record index's kernels (zstd-rs_amd/csrc/zg_records.h: zg_k_recs_count, zg_k_recs_scan,
// zg_k_recs_emit, zg_k_recs_find) on the CPU through the SIMT emulator of zg_simt.h, and the host forms (zgr::records_host, zgr::cut_chunks,
// zgr::find_host) beside them. tests/test_records_cpu.py and tests/test_recshapes_cpu.py build this file (tests/lanesuite.py; it is not in the Makefile's library), twice: as
// a shared library whose accessors count every access outside what a wave may touch — a count or emit wave its own chunk's bytes and, the
// emit wave, its own chunk's slots of the staging; the scan workgroup the counts, the frame starts, the prefixes and the totals; a find lane
// its own entry's offsets —, and — with -DRECORDS_MAIN — as a stand-alone AddressSanitizer program in which every chunk's bytes end at the
// end of a heap block and the counts, prefixes, totals, staging and offsets each lie in a heap block of exactly their length
// (zg_lane_mem.h). Both hand everything back; the test compares it with its model (tests/records.py). Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_records.h"
#include "zg_lane_mem.h"

namespace {
// the submit's output as a wave may see it: the bytes of its own chunk; a 16-byte load at an address that is no multiple of 16 is counted
struct Bytes {
  lane::Reader<uint32_t> r; uint64_t* misaligned;
  uint32_t ld1(uint64_t off) const { return r.ld1(off); }
  ZxU4 ld16(uint64_t off) const {
    ZxU4 v;
    if (((uintptr_t)r.p + off) % 16) (*misaligned)++;
    r.get(off, &v.x, 4);
    return v;
  }
};
struct DirectBytes {
  const uint8_t* p;   // where byte 0 of the output would lie
  uint32_t ld1(uint64_t off) const { return p[off]; }
  ZxU4 ld16(uint64_t off) const {
    if (((uintptr_t)p + off) % 16) { fprintf(stderr, "misaligned 16-byte load\n"); abort(); }
    ZxU4 v; memcpy(&v, p + off, 16); return v;
  }
};
template <class A> struct Words {   // A: lane::Array<uint64_t> or lane::DirectArray<uint64_t>
  A a;
  uint64_t ld(uint64_t i) const { return a.ld(i); }
  void st(uint64_t i, uint64_t v) const { a.st(i, v); }
};
template <class A> struct Counts { A a; uint32_t ld(uint64_t i) const { return a.ld(i); } };
template <class A> struct Totals {   // [0]: the total; [1 + f]: frame f's
  A a;
  void total(uint64_t v) const { a.st(0, v); }
  void ftot(uint32_t f, uint64_t v) const { a.st(1ull + f, v); }
};

// one wave over one chunk; false if the lanes' counts differ
template <class R> bool count_wave(const R& r, const zgr::Chunk& c, uint32_t d, uint32_t* out) {
  static uint32_t all[64];
  simt::run(64, [&]() { all[zx_tid()] = zgr::recs_count_chunk(r, c.out_off, c.len, d); });
  for (int l = 1; l < 64; l++) if (all[l] != all[0]) return false;
  *out = all[0];
  return true;
}
template <class R, class W> void emit_wave(const R& r, const W& w, const zgr::Chunk& c, uint32_t d, uint64_t slot0, uint64_t total) {
  simt::run(64, [&]() { zgr::recs_emit_chunk(r, w, c.out_off, c.len, c.base, d, slot0, total); });
}
template <class C, class F, class P, class T> void scan_group(const C& c, const F& f, const P& p, const T& t, uint32_t nchunks, uint32_t nframes) {
  static uint64_t lds[zgr::kScanThreads / 64];
  simt::run(zgr::kScanThreads, [&]() { zgr::recs_scan(c, f, p, t, nchunks, nframes, lds); });
}
}  // namespace

// The three kernels over one chunk table. buf: the output (at a multiple of 16); chunks / fstart: the table, nframes + 1 frame starts;
// counts (nchunks), prefix (nchunks), totals (1 + nframes), staging (cap slots): what the kernels leave — the test sizes the staging from
// its model, the emit is told the scan's total —; counters: [0] byte reads outside the wave's chunk, [1] misaligned 16-byte loads, [2] scan
// accesses outside its arrays, [3] staging stores outside the chunk's own slots, [4] staging stores kept, [5] guard bands damaged. Returns
// 1 if the lanes of a count wave disagree.
extern "C" uint32_t zgemu_records(const uint8_t* buf, const void* chunks_, uint32_t nchunks, const uint32_t* fstart, uint32_t nframes, uint32_t d,
                                  uint32_t* counts, uint64_t* prefix, uint64_t* totals, uint64_t* staging, uint64_t cap, uint64_t* counters) {
  const zgr::Chunk* chunks = (const zgr::Chunk*)chunks_;
  lane::Count rc, sc, wc;
  uint64_t misaligned = 0;
  bool agree = true;
  lane::Guarded<uint32_t> gcounts(nchunks);
  lane::Guarded<uint64_t> gprefix(nchunks), gtotals(1ull + nframes), gstage(cap);
  for (uint32_t i = 0; i < nchunks; i++) {
    const Bytes r{lane::Reader<uint32_t>::over(buf, chunks[i].out_off, chunks[i].out_off + chunks[i].len, &rc), &misaligned};
    uint32_t v = 0;
    agree = count_wave(r, chunks[i], d, &v) && agree;
    gcounts.mid()[i] = v;
  }
  {
    // (the accessors index from the array's first element: the guarded blocks are handed over from their middles)
    const Counts<lane::Array<const uint32_t>> c{{gcounts.mid(), 0, nchunks, &sc}};
    const Counts<lane::Array<const uint32_t>> f{{fstart, 0, (uint64_t)nframes + 1, &sc}};
    const Words<lane::Array<uint64_t>> p{{gprefix.mid(), 0, nchunks, &sc}};
    const Totals<lane::Array<uint64_t>> t{{gtotals.mid(), 0, 1ull + nframes, &sc}};
    scan_group(c, f, p, t, nchunks, nframes);
  }
  const uint64_t total = gtotals.mid()[0];
  for (uint32_t i = 0; i < nchunks; i++) {
    const Bytes r{lane::Reader<uint32_t>::over(buf, chunks[i].out_off, chunks[i].out_off + chunks[i].len, &rc), &misaligned};
    const uint64_t lo = gprefix.mid()[i], hi = lo + gcounts.mid()[i];
    const Words<lane::Array<uint64_t>> w{{gstage.mid(), lo < cap ? lo : cap, hi < cap ? hi : cap, &wc}};
    emit_wave(r, w, chunks[i], d, lo, total);
  }
  memcpy(counts, gcounts.mid(), (size_t)nchunks * 4);
  memcpy(prefix, gprefix.mid(), (size_t)nchunks * 8);
  memcpy(totals, gtotals.mid(), (size_t)(1 + nframes) * 8);
  memcpy(staging, gstage.mid(), (size_t)cap * 8);
  counters[0] = rc.bad; counters[1] = misaligned; counters[2] = sc.bad; counters[3] = wc.bad; counters[4] = wc.kept;
  counters[5] = (gcounts.intact() && gprefix.intact() && gtotals.intact() && gstage.intact()) ? 0 : 1;
  return agree ? 0u : 1u;
}

// m find lanes over the handle's offsets o, in the workgroups zg_launch_recs_find launches: ceil(m / kThreads) of kThreads, lane j = workgroup *
// kThreads + thread, a thread with j >= m does nothing. A lane may read [win[2j], win[2j + 1]) of the offsets. out: the lanes' answers (every
// byte kFill where no lane stored), host: zgr::find_host's (24 bytes each); counters: [0] reads, [1] reads outside the lane's window.
extern "C" void zgemu_records_find(const uint64_t* o, const void* lanes_, uint32_t m, const uint64_t* win, void* out, void* host, uint64_t* counters) {
  const zgr::Find* lanes = (const zgr::Find*)lanes_;
  lane::Count c;
  std::vector<zgr::Found> got(m);
  memset((void*)got.data(), lane::kFill, (size_t)m * sizeof(zgr::Found));
  for (uint32_t g = 0; g < (m + zgr::kThreads - 1) / zgr::kThreads; g++)
    simt::run(zgr::kThreads, [&]() {
      const uint32_t j = g * zgr::kThreads + zx_tid();
      if (j >= m) return;
      const Words<lane::Array<const uint64_t>> w{{o, win[2 * j], win[2 * j + 1], &c}};
      got[j] = zgr::recs_find(w, lanes[j]);
    });
  memcpy(out, got.data(), (size_t)m * sizeof(zgr::Found));
  for (uint32_t j = 0; j < m; j++) { const zgr::Found h = zgr::find_host(o, lanes[j]); memcpy((uint8_t*)host + 24 * j, &h, 24); }
  counters[0] = c.n; counters[1] = c.bad;
}

// zg_k_recs_scan alone: counts (nchunks) and fstart (nframes + 1) in, prefix (nchunks) and totals (1 + nframes) out — no plaintext, so a large
// nchunks costs nothing. Every array lies between guard bands and is seen through a counted accessor of its own; counters: [0] accesses outside
// an array, [1] prefix stores kept, [2] stores of the total, [3] stores of a frame's total, [4] guard bands damaged.
namespace {
template <class A> struct SplitTotals {   // the total and the frames' totals counted apart: [0] and [1 + f] of one array
  A tot, fr;
  void total(uint64_t v) const { tot.st(0, v); }
  void ftot(uint32_t f, uint64_t v) const { fr.st(1ull + f, v); }
};
}  // namespace
extern "C" void zgemu_records_scan(const uint32_t* counts, uint32_t nchunks, const uint32_t* fstart, uint32_t nframes, uint64_t* prefix, uint64_t* totals,
                                   uint64_t* counters) {
  lane::Count cc, cf, cp, ct, cq;
  lane::Guarded<uint32_t> gcounts(nchunks), gfstart((uint64_t)nframes + 1);
  lane::Guarded<uint64_t> gprefix(nchunks), gtotals(1ull + nframes);
  memcpy(gcounts.mid(), counts, (size_t)nchunks * 4);
  memcpy(gfstart.mid(), fstart, ((size_t)nframes + 1) * 4);
  {
    const Counts<lane::Array<const uint32_t>> c{{gcounts.mid(), 0, nchunks, &cc}};
    const Counts<lane::Array<const uint32_t>> f{{gfstart.mid(), 0, (uint64_t)nframes + 1, &cf}};
    const Words<lane::Array<uint64_t>> p{{gprefix.mid(), 0, nchunks, &cp}};
    const SplitTotals<lane::Array<uint64_t>> t{{gtotals.mid(), 0, 1, &ct}, {gtotals.mid(), 1, 1ull + nframes, &cq}};
    scan_group(c, f, p, t, nchunks, nframes);
  }
  memcpy(prefix, gprefix.mid(), (size_t)nchunks * 8);
  memcpy(totals, gtotals.mid(), (size_t)(1 + nframes) * 8);
  counters[0] = cc.bad + cf.bad + cp.bad + ct.bad + cq.bad; counters[1] = cp.kept; counters[2] = ct.kept; counters[3] = cq.kept;
  counters[4] = (gcounts.intact() && gfstart.intact() && gprefix.intact() && gtotals.intact()) ? 0 : 1;
}

// zgr::records_host over p[0 .. n): the offsets to out (cap slots); returns how many there are
extern "C" uint64_t zgemu_records_host(const uint8_t* p, uint64_t n, uint32_t d, uint64_t base, uint64_t* out, uint64_t cap) {
  std::vector<uint64_t> v;
  zgr::records_host(p, n, d, base, &v);
  for (uint64_t i = 0; i < v.size() && i < cap; i++) out[i] = v[i];
  return v.size();
}

// zgr::cut_chunks of one frame: the chunks to out (cap records of 24 bytes); returns how many there are
extern "C" uint64_t zgemu_records_cut(uint64_t out_off, uint64_t size, uint64_t base, uint32_t frame, void* out, uint64_t cap) {
  std::vector<zgr::Chunk> v;
  zgr::cut_chunks(out_off, size, base, frame, &v);
  for (uint64_t i = 0; i < v.size() && i < cap; i++) memcpy((uint8_t*)out + 24 * i, &v[i], 24);
  return v.size();
}

#ifdef RECORDS_MAIN
// argv[1]: per case [u32 kind] and
//   kind 0 (the three kernels): [u32 nchunks][u32 nframes][u32 d][u64 cap] [nchunks x 24 bytes][(nframes + 1) x u32] and per chunk its len bytes;
//   kind 1 (find): [u32 m][u32 pad][u32 pad][u64 nwords] [m x 48 bytes][nwords x u64];
//   kind 2 (the scan alone): [u32 nchunks][u32 nframes][u32 pad][u64 pad] [nchunks x u32 counts][(nframes + 1) x u32].
// argv[2]: kind 0 — counts, prefixes, totals, staging as they were left; kind 1 — m answers of 24 bytes; kind 2 — prefixes, totals. A chunk's bytes end at the end of a
// heap block that begins at a multiple of 16 out_off % 16 bytes in front of them; every other array lies in a block of exactly its length and
// is accessed directly: an access outside one is an AddressSanitizer report.
int main(int argc, char** argv) {
  lane::CaseFile f(argc > 2 ? argv[1] : nullptr, "rb"), g(argc > 2 ? argv[2] : nullptr, "wb");
  uint64_t cases = 0;
  uint32_t kind;
  for (; f.next(&kind, 4); cases++) {
    uint32_t h[3];
    uint64_t big;
    f.read(h, 4, 3);
    f.read(&big, 8, 1);
    if (kind == 1) {
      zgr::Find* lanes = f.aligned<zgr::Find>(h[0]);
      uint64_t* o = (uint64_t*)f.block(big * 8);
      for (uint32_t j = 0; j < h[0]; j++) {
        zgr::Found r;
        simt::run(1, [&]() { r = zgr::recs_find(Words<lane::DirectArray<const uint64_t>>{{o}}, lanes[j]); });
        g.write(&r, 24, 1);
      }
      free(o); free(lanes);
      continue;
    }
    if (kind == 2) {
      const uint32_t nchunks = h[0], nframes = h[1];
      uint32_t* counts = (uint32_t*)f.block((uint64_t)nchunks * 4);
      uint32_t* fstart = (uint32_t*)f.block(((uint64_t)nframes + 1) * 4);
      uint64_t* prefix = (uint64_t*)malloc((size_t)nchunks * 8);
      uint64_t* totals = (uint64_t*)malloc((size_t)(1 + nframes) * 8);
      scan_group(Counts<lane::DirectArray<const uint32_t>>{{counts}}, Counts<lane::DirectArray<const uint32_t>>{{fstart}},
                 Words<lane::DirectArray<uint64_t>>{{prefix}}, Totals<lane::DirectArray<uint64_t>>{{totals}}, nchunks, nframes);
      g.write(prefix, 8, nchunks); g.write(totals, 8, 1 + (size_t)nframes);
      free(totals); free(prefix); free(fstart); free(counts);
      continue;
    }
    const uint32_t nchunks = h[0], nframes = h[1], d = h[2];
    zgr::Chunk* chunks = (zgr::Chunk*)f.block((uint64_t)nchunks * 24);
    uint32_t* fstart = (uint32_t*)f.block(((uint64_t)nframes + 1) * 4);
    uint32_t* counts = (uint32_t*)malloc((size_t)nchunks * 4);
    uint64_t* prefix = (uint64_t*)malloc((size_t)nchunks * 8);
    uint64_t* totals = (uint64_t*)malloc((size_t)(1 + nframes) * 8);
    uint64_t* staging = (uint64_t*)malloc((size_t)big * 8);
    std::vector<uint8_t*> blocks(nchunks);
    for (uint32_t i = 0; i < nchunks; i++) {
      const size_t pad = (size_t)(chunks[i].out_off % 16);
      void* blk = nullptr;   // (posix_memalign: a block of any length at a multiple of 16)
      if (posix_memalign(&blk, 16, pad + chunks[i].len)) return lane::kExitIO;
      blocks[i] = (uint8_t*)blk;
      memset(blocks[i], d, pad);   // (what lies in front of the chunk is full of delimiters)
      f.read(blocks[i] + pad, 1, chunks[i].len);
      if (!count_wave(DirectBytes{blocks[i] + pad - chunks[i].out_off}, chunks[i], d, &counts[i])) return lane::kExitLanes;
    }
    scan_group(Counts<lane::DirectArray<const uint32_t>>{{counts}}, Counts<lane::DirectArray<const uint32_t>>{{fstart}},
               Words<lane::DirectArray<uint64_t>>{{prefix}}, Totals<lane::DirectArray<uint64_t>>{{totals}}, nchunks, nframes);
    if (totals[0] != big) return lane::kExitLanes;   // (the test sized the staging from its model)
    for (uint32_t i = 0; i < nchunks; i++) {
      const size_t pad = (size_t)(chunks[i].out_off % 16);
      emit_wave(DirectBytes{blocks[i] + pad - chunks[i].out_off}, Words<lane::DirectArray<uint64_t>>{{staging}}, chunks[i], d, prefix[i], totals[0]);
    }
    g.write(counts, 4, nchunks); g.write(prefix, 8, nchunks); g.write(totals, 8, 1 + (size_t)nframes); g.write(staging, 8, (size_t)big);
    for (uint8_t* b : blocks) free(b);
    free(staging); free(totals); free(prefix); free(counts); free(fstart); free(chunks);
  }
  f.close();
  g.close();
  printf("records_asan ok: %llu cases\n", (unsigned long long)cases);
  return 0;
}
#endif
