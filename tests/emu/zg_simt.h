// zg_simt.h — TEST-ONLY: a small SIMT emulator for kernels written against the zx_* primitives (zg_huf.h, zg_flat1.h, zg_flat4.h,
// zg_exact.h, zg_inorder.h, zg_seqsize.h, zg_seektab.h, zg_seeksums.h, zg_idxsums.h, zg_seekmany.h, zg_records.h, zg_zxprobe.h). One workgroup
// at a time; every GPU thread is a fiber (ucontext) that runs the kernel body verbatim and yields at workgroup barriers
// and wave collectives; lanes of a wave are 64 consecutive threads. Deterministic (threads run in index order between
// synchronisation points), so a data race does not show as flakiness here — what it checks is the kernel's logic, against
// the oracle, before the same source is compiled for gfx950. Not part of the product.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>
#include <functional>
#include <vector>

namespace simt {

enum { RUN = 0, WAVE_WAIT = 1, WG_WAIT = 2, DONE = 3 };
struct Lane { ucontext_t ctx; char* stack = nullptr; int state = RUN; };
struct Machine {
  std::vector<Lane> lanes;
  ucontext_t sched;
  uint32_t cur = 0, T = 0;
  std::function<void()> body;
  std::vector<uint64_t> slot;      // collectives: one value per lane
  uint64_t barriers = 0;
};
inline Machine*& M() { static Machine* m = nullptr; return m; }

inline void trampoline() {
  Machine* m = M();
  m->body();
  m->lanes[m->cur].state = DONE;
  m->slot[m->cur] = 0;
  swapcontext(&m->lanes[m->cur].ctx, &m->sched);
}
inline void yield(int state) {
  Machine* m = M();
  m->lanes[m->cur].state = state;
  swapcontext(&m->lanes[m->cur].ctx, &m->sched);
}
// run `body` on T threads of one workgroup
inline void run(uint32_t T, const std::function<void()>& body) {
  Machine m;
  M() = &m;
  m.T = T; m.body = body;
  m.lanes.resize(T); m.slot.assign(T, 0);
  const size_t STK = 256 << 10;
  for (uint32_t i = 0; i < T; i++) {
    Lane& l = m.lanes[i];
    l.stack = (char*)malloc(STK);
    getcontext(&l.ctx);
    l.ctx.uc_stack.ss_sp = l.stack; l.ctx.uc_stack.ss_size = STK; l.ctx.uc_link = nullptr;
    makecontext(&l.ctx, (void (*)())trampoline, 0);
  }
  for (;;) {
    bool ran = false;
    for (uint32_t i = 0; i < T; i++)
      if (m.lanes[i].state == RUN) { m.cur = i; swapcontext(&m.sched, &m.lanes[i].ctx); ran = true; }
    bool released = false, all_done = true, all_wg = true, any_wg = false;
    for (uint32_t w = 0; w * 64 < T; w++) {
      bool ready = true, any = false;
      for (uint32_t l = w * 64; l < T && l < w * 64 + 64; l++) {
        const int s = m.lanes[l].state;
        if (s == WAVE_WAIT) any = true; else if (s != DONE) ready = false;
      }
      if (ready && any) { for (uint32_t l = w * 64; l < T && l < w * 64 + 64; l++) if (m.lanes[l].state == WAVE_WAIT) m.lanes[l].state = RUN; released = true; }
    }
    for (uint32_t i = 0; i < T; i++) {
      const int s = m.lanes[i].state;
      if (s != DONE) all_done = false;
      if (s == WG_WAIT) any_wg = true; else if (s != DONE) all_wg = false;
    }
    if (all_done) break;
    if (all_wg && any_wg) { for (uint32_t i = 0; i < T; i++) if (m.lanes[i].state == WG_WAIT) m.lanes[i].state = RUN; released = true; m.barriers++; }
    if (!ran && !released) { fprintf(stderr, "simt: deadlock (divergent barrier or collective)\n"); abort(); }
  }
  for (Lane& l : m.lanes) free(l.stack);
  M() = nullptr;
}

}  // namespace simt

// ---- the zx_* primitives on the emulator -----------------------------------------------------------------------------
// Each one states its DOMAIN: the arguments tests/zxprobe.py holds this definition, the one of zg_kernels.hip on an MI355X and a plain model
// against (tests/test_zxprobe_cpu.py, tests/test_gpu_zxprobe.py). Outside its domain a primitive aborts with a message: what the hardware does
// there is not known to this file, and a body that gets there is not tested by running here.
#define ZX_DEV static inline
#define ZX_OOB 0x80000000u   // as on the GPU (zg_kernels.hip): far outside every resource, and adding a few bytes to it does not wrap into one
#define ZX_FRESH(v) (v)
#define ZX_DOMAIN(ok, ...) do { if (!(ok)) { fprintf(stderr, "simt: outside the tested domain: " __VA_ARGS__); fprintf(stderr, "\n"); abort(); } } while (0)
struct ZxBuf { uint8_t* base; uint32_t bytes; };
static inline uint32_t zx_tid() { return simt::M()->cur; }
static inline void zx_barrier() { simt::yield(simt::WG_WAIT); }
static inline void zx_barrier_vm() { simt::yield(simt::WG_WAIT); }
// The wave collectives. Domain: any predicate or 32-bit value; lanes of the wave may have returned (a wave may be partial: the lanes a
// workgroup does not have count as returned). A returned lane's predicate counts as 0 and a shuffle from it reads 0 (ds_bpermute_b32 from a
// lane that is off in EXEC).
static inline unsigned long long zx_ballot(bool p) {
  simt::Machine* m = simt::M();
  const uint32_t me = m->cur, w0 = me & ~63u;
  m->slot[me] = p ? 1 : 0;
  simt::yield(simt::WAVE_WAIT);
  unsigned long long r = 0;
  for (uint32_t l = 0; l < 64 && w0 + l < m->T; l++) if (m->lanes[w0 + l].state != simt::DONE && m->slot[w0 + l]) r |= 1ull << l;
  simt::yield(simt::WAVE_WAIT);
  return r;
}
// what lane `src` (0 .. 63) of the caller's wave put into its slot; 0 if that lane has returned or the workgroup has no such thread
static inline uint32_t zx__lane(simt::Machine* m, uint32_t w0, uint32_t src) {
  const uint32_t i = w0 + src;
  return i < m->T && m->lanes[i].state != simt::DONE ? (uint32_t)m->slot[i] : 0u;
}
// zx_shfl_up(v, o): lane - o's value where lane >= o, else the caller's own (__shfl_up, width 64). Domain: 0 <= o <= 64.
static inline uint32_t zx_shfl_up(uint32_t v, int o) {
  simt::Machine* m = simt::M();
  const uint32_t me = m->cur, lane = me & 63u;
  ZX_DOMAIN(o >= 0 && o <= 64, "zx_shfl_up by %d", o);
  m->slot[me] = v;
  simt::yield(simt::WAVE_WAIT);
  const uint32_t r = (int)lane >= o ? zx__lane(m, me & ~63u, lane - (uint32_t)o) : v;
  simt::yield(simt::WAVE_WAIT);
  return r;
}
// the value lane l & 63 of the caller's wave holds (every lane of the wave calls it). Domain: 0 <= l < 128.
static inline uint32_t zx_shfl(uint32_t v, int l) {
  simt::Machine* m = simt::M();
  const uint32_t me = m->cur, w0 = me & ~63u;
  ZX_DOMAIN(l >= 0 && l < 128, "zx_shfl from lane %d", l);
  m->slot[me] = v;
  simt::yield(simt::WAVE_WAIT);
  const uint32_t r = zx__lane(m, w0, (uint32_t)l & 63u);
  simt::yield(simt::WAVE_WAIT);
  return r;
}
// the value of lane ^ x. Domain: 1 <= x <= 63 (from 64 on __shfl_xor hands a lane its own value where lane ^ x >= 64: no body needs it, no
// test holds this file to it)
static inline uint32_t zx_shfl_xor(uint32_t v, int x) {
  simt::Machine* m = simt::M();
  const uint32_t me = m->cur, w0 = me & ~63u;
  ZX_DOMAIN(x >= 1 && x <= 63, "zx_shfl_xor with mask %d", x);
  m->slot[me] = v;
  simt::yield(simt::WAVE_WAIT);
  const uint32_t r = zx__lane(m, w0, (me & 63u) ^ (uint32_t)x);
  simt::yield(simt::WAVE_WAIT);
  return r;
}
static inline bool zx_any(bool p) { return zx_ballot(p) != 0ull; }
// The wave scans on DPP (zg_kernels.hip). Domain: EVERY lane of a full wave is active — with a lane returned the call aborts (what a DPP move
// reads from a lane that is off in EXEC depends on bound_ctrl and the destination's old contents; the bodies never ask). The lane rules:
//   steps 0 .. 3   row_shr:1/2/4/8, inside the rows of 16 lanes: lane l reads l - 2^S where (l & 15) >= 2^S
//   step 4         row_bcast:15, row mask 0xA: the lanes of rows 1 and 3 read lane 15 of the row below
//   step 5         row_bcast:31, row mask 0xC: the lanes of rows 2 and 3 read lane 31
//   zx_shr1        wave_shr:1: lane l reads l - 1; lane 0 reads none
// A lane that reads none gets `fill` (bound_ctrl off: it keeps `old`).
template <int S> static inline bool zx_scan_takes(uint32_t lane) { return S < 4 ? (lane & 15u) >= (1u << S) : (lane & (S == 4 ? 16u : 32u)) != 0u; }
static inline uint32_t zx__dpp(uint32_t v, uint32_t fill, int src_of[64], const char* what) {
  simt::Machine* m = simt::M();
  const uint32_t me = m->cur, w0 = me & ~63u;
  m->slot[me] = v;
  simt::yield(simt::WAVE_WAIT);
  for (uint32_t l = 0; l < 64; l++) ZX_DOMAIN(w0 + l < m->T && m->lanes[w0 + l].state != simt::DONE, "%s with lane %u of the wave returned", what, l);
  const int src = src_of[me & 63u];
  const uint32_t r = src >= 0 ? (uint32_t)m->slot[w0 + (uint32_t)src] : fill;
  simt::yield(simt::WAVE_WAIT);
  return r;
}
template <int S> static inline uint32_t zx_scan_src(uint32_t v, uint32_t fill) {
  static_assert(S >= 0 && S < 6, "six steps");
  int src[64];
  for (int l = 0; l < 64; l++) src[l] = !zx_scan_takes<S>((uint32_t)l) ? -1 : S < 4 ? l - (1 << S) : S == 4 ? (l & ~15) - 1 : 31;
  return zx__dpp(v, fill, src, "zx_scan_src");
}
static inline uint32_t zx_scan_incl_add(uint32_t v) {
  v += zx_scan_src<0>(v, 0u); v += zx_scan_src<1>(v, 0u); v += zx_scan_src<2>(v, 0u); v += zx_scan_src<3>(v, 0u);
  v += zx_scan_src<4>(v, 0u); v += zx_scan_src<5>(v, 0u);
  return v;
}
static inline uint32_t zx_shr1(uint32_t v, uint32_t fill) {
  int src[64];
  for (int l = 0; l < 64; l++) src[l] = l - 1;
  return zx__dpp(v, fill, src, "zx_shr1");
}
// the lanes of a wave run one after the other here: what they wrote to LDS is complete for all of them behind this point
static inline void zx_wave_sync() { (void)zx_ballot(true); }
// The atomics. Domain: any value; any number of threads on one word for or, min, max and add (the result does not depend on their order), ONE
// contender per word for zx_cas_lds (which of several wins is the hardware's choice; here it would be the lowest thread).
static inline void zx_cas_lds(uint32_t* p, uint32_t cmp, uint32_t v) { if (*p == cmp) *p = v; }
// a no-op here: threads run one after the other up to the next collective or barrier, and every store has landed by then. What the
// kernels need from it — a round's copies visible to the lanes that read them after the next collective — holds by construction
static inline void zx_fence_block() {}
static inline void zx_syncthreads() { simt::yield(simt::WG_WAIT); }
static inline void zx_max_glb(uint32_t* p, uint32_t v) { if (v > *p) *p = v; }
// Global memory by pointer. Domain: zx_gst128 and zx_gld128 at multiples of 16 (else they abort), zx_gst32u at any address.
static inline void zx_gst128(void* p, const ZxU4& v) {
  if ((uintptr_t)p % 16) { fprintf(stderr, "simt: misaligned 16-byte global store\n"); abort(); }
  memcpy(p, &v, 16);
}
static inline void zx_gst32u(void* p, uint32_t v) { memcpy(p, &v, 4); }
static inline ZxU4 zx_gld128(const void* p) {
  if ((uintptr_t)p % 16) { fprintf(stderr, "simt: misaligned 16-byte global load\n"); abort(); }
  ZxU4 r; memcpy(&r, p, 16); return r;
}
static inline void zx_or_lds(uint32_t* p, uint32_t v) { *p |= v; }
static inline void zx_min_lds(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
static inline void zx_min_lds64(unsigned long long* p, unsigned long long v) { if (v < *p) *p = v; }
static inline void zx_min_glb(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
template <typename P> static inline ZxBuf zx_buf(P* base, uint32_t bytes) { ZxBuf b; b.base = (uint8_t*)base; b.bytes = bytes; return b; }
static inline ZxBuf zx_buf(decltype(nullptr), uint32_t) { ZxBuf b; b.base = nullptr; b.bytes = 0; return b; }
// Raw buffers: every dword (byte) of an access is range-checked by itself; out of range reads 0, writes nothing. A dword at offset off is in
// range exactly when off + 4 <= bytes, also where off is no multiple of 4 (zx_ld32 only). Domain: a resource of 0 .. 2^31 - 1 bytes (0 bytes
// over a null base included); offsets below 0xFFFFFFF0 — at and above it a wide access would wrap 2^32 in its later dwords, which no test
// runs on a GPU, so they abort; zx_ld8, zx_ld32 and zx_st8 at any byte offset, the others at offsets that make a dword-aligned ADDRESS
// (else they abort where the first dword is in range: the bodies promise it).
// One exception, for the one body that needs it: zx_ld32 at a MULTIPLE OF 4 is in the domain up to 0xFFFFFFFC. Its four bytes end at or below
// 2^32, so nothing in the access can wrap, and the offset is at or above every resource's size: it reads 0. S1c of zg_flat1.h fetches a root's
// parent word at 4 * (unit position of the parent), which is such an offset (0xFFFFFFF4 for a parent 3 bytes in front of the unit) for every
// parent in front of the unit. The probe cannot run it (its host rules stop every offset at 0x80000040); on the GPU it is held by every suite
// that decodes through the pointer-mode flatten against the oracle.
#define ZX_OFFSET(off) ZX_DOMAIN((off) < 0xFFFFFFF0u, "buffer offset 0x%08X", (unsigned)(off))
static inline uint32_t zx__dw(const ZxBuf& b, uint64_t off64) { const uint32_t off = (uint32_t)off64; uint32_t v = 0; if ((uint64_t)off + 4 <= b.bytes) memcpy(&v, b.base + off, 4); return v; }
static inline uint32_t zx_ld32(const ZxBuf& b, uint32_t off) { if (off & 3u) ZX_OFFSET(off); return zx__dw(b, off); }
#define ZX_ALIGNED(off, a) do { ZX_OFFSET(off); if ((off) != ZX_OOB && (off) < b.bytes && (((uintptr_t)b.base + (off)) % (a))) { fprintf(stderr, "simt: misaligned buffer access %u %% %d at %s:%d\n", (unsigned)(off), (int)(a), __FILE__, __LINE__); abort(); } } while (0)
static inline ZxU2 zx_ld64(const ZxBuf& b, uint32_t off) { ZX_ALIGNED(off, 4); ZxU2 r; r.x = zx__dw(b, off); r.y = zx__dw(b, (uint64_t)off + 4); return r; }
static inline ZxU3 zx_ld96(const ZxBuf& b, uint32_t off) { ZX_ALIGNED(off, 4); ZxU3 r; r.x = zx__dw(b, off); r.y = zx__dw(b, (uint64_t)off + 4); r.z = zx__dw(b, (uint64_t)off + 8); return r; }
static inline ZxU4 zx_ld128(const ZxBuf& b, uint32_t off) {
  ZX_ALIGNED(off, 4);
  ZxU4 r;
  r.x = zx__dw(b, off); r.y = zx__dw(b, (uint64_t)off + 4); r.z = zx__dw(b, (uint64_t)off + 8); r.w = zx__dw(b, (uint64_t)off + 12);
  return r;
}
static inline uint32_t zx_ld8(const ZxBuf& b, uint32_t off) { ZX_OFFSET(off); return off < b.bytes ? b.base[off] : 0u; }
static inline void zx_add_lds(uint32_t* p, uint32_t v) { *p += v; }
static inline void zx_st8(const ZxBuf& b, uint32_t off, uint32_t v) { ZX_OFFSET(off); if (off < b.bytes) b.base[off] = (uint8_t)v; }
static inline void zx_st32(const ZxBuf& b, uint32_t off, uint32_t v) { ZX_ALIGNED(off, 4); if ((uint64_t)off + 4 <= b.bytes) memcpy(b.base + off, &v, 4); }
// v_alignbit_b32: the low 32 bits of (hi:lo) >> (sh & 31). Domain: any sh.
static inline uint32_t zx_alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31u)); }
// packed 16-bit lanes: a - b per lane; 0xFFFF per lane whose signed value is negative. Domain: any values.
static inline uint32_t zx_pksub16(uint32_t a, uint32_t b) { return ((a - b) & 0xFFFFu) | (((a >> 16) - (b >> 16)) << 16); }
static inline uint32_t zx_pksign16(uint32_t a) { return ((a & 0x8000u) ? 0xFFFFu : 0u) | ((a & 0x80000000u) ? 0xFFFF0000u : 0u); }
