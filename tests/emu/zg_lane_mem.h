// zg_lane_mem.h — TEST-ONLY: the guarded memory the CPU harnesses of the lane and wave routines run over (tests/emu/zg_lane_*.cpp,
// tests/emu/zg_emu_seek*.cpp). A routine under test is a template over its accessors; a harness hands it the counted ones of this header, which
// count every access and every access outside what the routine may touch, or — in a stand-alone AddressSanitizer program — the direct ones,
// which check nothing, over heap blocks of exactly the size the routine may touch. This header knows no routine: where a routine wants members
// of other names (ld_d, frame, digest, begin, st16) the harness keeps a thin adapter over these. Not part of the product.
//
// What is in range. A read or an access names n >= 1 elements at index i (no accessor here has a form for n == 0) and is inside [lo, hi) when
// lo <= i < hi and n <= hi - i. So i == hi is outside whatever is asked for there: the one rule for every suite. (Two of the earlier private
// readers were written so that a read of no bytes at off == len would have passed; nothing ever issued one, and all eleven suites pass
// unchanged under this rule.)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

namespace lane {

constexpr int kFill = 0xEE;   // what memory nobody has written yet holds: guard bands, record slots, scratch

// One accessor's counts. n: accesses; bad: those outside (refused: a load gives 0, a store is dropped); forbidden: reads inside that touched a
// byte of the forbidden map; kept: elements stored; unaligned: multi-element stores at an address that is no multiple of their alignment.
struct Count { uint64_t n = 0, bad = 0, forbidden = 0, kept = 0, unaligned = 0; };

// ---- bytes of an entry ----------------------------------------------------------------------------------------------------------------------
struct Window { uint64_t lo, hi; };

// The entry as a lane may see it: the bytes of up to three windows [lo, hi), counted from the entry's first byte. forbidden (or null): a map of
// the entry, nonzero at bytes the routine has no business with (block bodies); a read of one is counted and served, so that the routine goes
// the way it goes on the device and the count is the finding. B: what ld1 returns (the kernels' readers give uint8_t or uint32_t).
template <class B = uint8_t> struct Reader {
  const uint8_t* p; Window win[3]; uint32_t nwin; const uint8_t* forbidden; Count* c;
  static Reader over(const uint8_t* p, uint64_t lo, uint64_t hi, Count* c, const uint8_t* forbidden = nullptr) {
    return Reader{p, {{lo, hi}, {0, 0}, {0, 0}}, 1, forbidden, c};
  }
  static Reader windows(const uint8_t* p, const uint64_t* lo_hi, uint32_t nwin, Count* c) {   // lo_hi: nwin <= 3 pairs
    Reader r{p, {{0, 0}, {0, 0}, {0, 0}}, nwin < 3 ? nwin : 3, nullptr, c};
    for (uint32_t w = 0; w < r.nwin; w++) r.win[w] = Window{lo_hi[2 * w], lo_hi[2 * w + 1]};
    return r;
  }
  bool ok(uint64_t off, uint64_t n) const {
    c->n++;
    for (uint32_t w = 0; w < nwin; w++) {
      if (off < win[w].lo || off >= win[w].hi || n > win[w].hi - off) continue;
      if (forbidden) for (uint64_t k = 0; k < n; k++) if (forbidden[off + k]) { c->forbidden++; break; }
      return true;
    }
    c->bad++;
    return false;
  }
  void get(uint64_t off, uint32_t* v, uint32_t words) const {   // zeros if refused
    memset(v, 0, 4 * words);
    if (ok(off, 4 * words)) memcpy(v, p + off, 4 * words);
  }
  B ld1(uint64_t off) const { return ok(off, 1) ? (B)p[off] : (B)0; }
  uint32_t ld4(uint64_t off) const { uint32_t v; get(off, &v, 1); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { uint32_t v[2]; get(off, v, 2); *a = v[0]; *b = v[1]; }
  void ld12(uint64_t off, uint32_t* a, uint32_t* b, uint32_t* s) const { uint32_t v[3]; get(off, v, 3); *a = v[0]; *b = v[1]; *s = v[2]; }
};

// No checks: what the kernel's reader does.
template <class B = uint8_t> struct Direct {
  const uint8_t* p;
  B ld1(uint64_t off) const { return p[off]; }
  uint32_t ld4(uint64_t off) const { uint32_t v; memcpy(&v, p + off, 4); return v; }
  void ld8(uint64_t off, uint32_t* a, uint32_t* b) const { memcpy(a, p + off, 4); memcpy(b, p + off + 4, 4); }
  void ld12(uint64_t off, uint32_t* a, uint32_t* b, uint32_t* s) const { ld8(off, a, b); memcpy(s, p + off + 8, 4); }
};

// ---- elements of an array -------------------------------------------------------------------------------------------------------------------
// Elements [lo, hi) of p: a lane's record range, an entry's pairs, the bytes of a chunk. ld_n / st_n move n elements at once; st_n also
// counts a store whose address is no multiple of `align` bytes (in range or not).
template <class T> struct Array {
  T* p; uint64_t lo, hi; Count* c;
  bool ok(uint64_t i, uint64_t n = 1) const { c->n++; if (i < lo || i >= hi || n > hi - i) { c->bad++; return false; } return true; }
  typename std::remove_const<T>::type ld(uint64_t i) const {
    typename std::remove_const<T>::type x;
    memset((void*)&x, 0, sizeof x);
    if (ok(i)) x = p[i];
    return x;
  }
  void st(uint64_t i, const T& x) const { if (ok(i)) { p[i] = x; c->kept++; } }
  void put(uint64_t i, const T& x) const { st(i, x); }
  void ld_n(uint64_t i, uint64_t n, void* to) const { memset(to, 0, n * sizeof(T)); if (ok(i, n)) memcpy(to, p + i, n * sizeof(T)); }
  void st_n(uint64_t i, uint64_t n, const void* from, uint64_t align) const {
    if (((uintptr_t)p + i * sizeof(T)) % align) c->unaligned++;
    if (ok(i, n)) { memcpy((void*)(p + i), from, n * sizeof(T)); c->kept += n; }
  }
};
template <class T> struct DirectArray {
  T* p;
  T ld(uint64_t i) const { return p[i]; }
  void st(uint64_t i, const T& x) const { p[i] = x; }
  void put(uint64_t i, const T& x) const { p[i] = x; }
  void ld_n(uint64_t i, uint64_t n, void* to) const { memcpy(to, p + i, n * sizeof(T)); }
  void st_n(uint64_t i, uint64_t n, const void* from, uint64_t) const { memcpy((void*)(p + i), from, n * sizeof(T)); }
};

// n elements between two bands of `guard` elements, every byte kFill. at(): the whole block, for an accessor whose range is [lo(), hi()).
template <class T> struct Guarded {
  std::vector<T> all; uint64_t guard, n;
  explicit Guarded(uint64_t n_, uint64_t guard_ = 4) : all(n_ + 2 * guard_), guard(guard_), n(n_) { memset((void*)all.data(), kFill, all.size() * sizeof(T)); }
  T* at() { return all.data(); }
  T* mid() { return all.data() + guard; }
  uint64_t lo() const { return guard; }
  uint64_t hi() const { return guard + n; }
  bool intact() const {   // both bands still hold kFill in every byte
    const uint8_t* a = (const uint8_t*)all.data();
    const uint8_t* b = (const uint8_t*)(all.data() + guard + n);
    for (size_t k = 0; k < guard * sizeof(T); k++) if (a[k] != kFill || b[k] != kFill) return false;
    return true;
  }
};

// The records zgk::seek_entry, zgt::seektab_entry and zgm::seekmany_find give (zgk::Seek), field by field: the padding does not count.
template <class S> bool same_seek(const S& a, const S& b) {
  return a.src_lo == b.src_lo && a.src_hi == b.src_hi && a.plain_lo == b.plain_lo && a.bound == b.bound && a.plain_seen == b.plain_seen &&
         a.status == b.status && a.frames_skipped == b.frames_skipped && a.frames_taken == b.frames_taken && a.nblocks == b.nblocks &&
         a.why == b.why && a.flags == b.flags;
}

#ifdef ZX_DEV   // (zg_simt.h was included first: the harness runs waves)
// One wave of n <= 64 lanes: every lane computes its record with f(), lane 0 stores its own through the routine's store function into a slot
// filled with kFill, and that slot is handed back in *out. False if a lane's record differs (same(a, b)) from lane 0's.
template <class Rec, class F, class St, class Eq> bool wave(uint32_t n, F f, St store, Eq same, Rec* out) {
  static Rec all[64];
  alignas(16) static Rec stored;   // (the records leave as 16-byte stores)
  if (n > 64) return false;
  memset((void*)&stored, kFill, sizeof stored);
  simt::run(n, [&]() {
    const Rec o = f();
    memcpy((void*)&all[zx_tid()], &o, sizeof o);
    if (zx_tid() == 0) store(&stored, o);
  });
  bool agree = true;
  for (uint32_t l = 1; l < n; l++) agree = agree && same(all[l], all[0]);
  memcpy((void*)out, &stored, sizeof stored);
  return agree;
}
#endif

// ---- the stand-alone programs ---------------------------------------------------------------------------------------------------------------
// A program with its own main (-D<NAME>_MAIN, AddressSanitizer linked statically) reads cases from argv[1] and may write records to argv[2].
// It ends with 0 and a line "<name>_asan ok: ..." on stdout, with kExitIO if a file cannot be opened, read or written, with kExitLanes if the
// lanes of a wave disagree; an access outside a block is AddressSanitizer's report and exit code.
enum { kExitIO = 2, kExitLanes = 3 };

struct CaseFile {
  FILE* f;
  CaseFile(const char* path, const char* mode) : f(path ? fopen(path, mode) : nullptr) { if (!f) exit(kExitIO); }
  // the next case's header: false at the end of the file
  bool next(void* hdr, size_t bytes) { return fread(hdr, bytes, 1, f) == 1; }
  void read(void* to, size_t size, size_t n) { if (n && fread(to, size, n, f) != n) exit(kExitIO); }
  // len bytes in a heap block of exactly len bytes: for len == 0 a block of size 0, never one byte that would hide an off-by-one
  uint8_t* block(uint64_t len) {
    uint8_t* e = (uint8_t*)malloc((size_t)len);
    if (len && !e) exit(kExitIO);
    read(e, 1, (size_t)len);
    return e;
  }
  // n records of 16 bytes' alignment in a block of exactly their size (one record's room where n == 0: aligned_alloc wants a size)
  template <class T> T* aligned(size_t n) {
    T* a = (T*)aligned_alloc(16, n ? n * sizeof(T) : 16);
    if (!a) exit(kExitIO);
    read(a, sizeof(T), n);
    return a;
  }
  void write(const void* from, size_t size, size_t n) { if (n && fwrite(from, size, n, f) != n) exit(kExitIO); }
  void close() { if (fclose(f)) exit(kExitIO); f = nullptr; }
};

}  // namespace lane
