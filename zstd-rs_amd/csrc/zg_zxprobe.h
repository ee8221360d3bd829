// zg_zxprobe.h — the zx_* primitives, ONE per launch, so that their two definitions (zg_kernels.hip for gfx950, tests/emu/zg_simt.h for the CPU
// emulator) can be held against one plain model (tests/zxprobe.py) at each primitive's edges. Written against the zx_* primitives only, like
// the kernel bodies: zg_k_zxprobe (zg_kernels.hip, behind zgpu_debug_zx_probe) and tests/emu/zg_emu_zxprobe.cpp compile this same source.
//
// One workgroup of 64 or 256 threads. Thread t reads its operands a[0 .. 8) = in[8 t ...], applies the primitive `op` names and writes its
// results to o[0 .. 4) = out[4 t ...] (words it does not write keep what the caller put there). No loop over data, no pointer arithmetic on an
// operand: an address an operand chooses is an offset into the buffer resource [arena + res_off, + res_bytes) — which the hardware checks — or
// an index the HOST checked before the launch (zxp::args_ok, the same function in front of the GPU launch and the emulator's run).
//   collectives      a[0] != 0: the lane returns first. Then the primitive, then the store — in that order.
//   DPP              every lane active (the emulator aborts otherwise; the GPU is never asked).
//   raw buffers      a[0] != 0: the lane does nothing. a[1]: byte offset, a[2]: the value stored.
//   memory helpers   a[0] != 0: the lane skips the primitive (it still takes the barriers). a[1]: a byte index into the arena or a word of LDS.
//   publish          every lane writes its slot, synchronises, reads slot a[2]: pins that the primitive is there, cannot prove the absence of a race.
#ifndef ZG_ZXPROBE_TYPES
#define ZG_ZXPROBE_TYPES
#include <stdint.h>
#include <stddef.h>
#include "zg_types.h"

namespace zxp {
constexpr uint32_t kIn = 8, kOut = 4;          // operand and result words per thread
constexpr uint32_t kLdsWords = 64;             // words of LDS the atomics share (the publish cases: one per thread)
constexpr uint32_t kGuard = 256;               // bytes of arena on either side of the resource
constexpr uint32_t kArenaMax = 1u << 20;
constexpr uint32_t kOffEnd = 0x80000000u + 64u;   // buffer offsets stay below this: no wide access wraps 2^32
constexpr uint32_t kNullRes = 1u;              // flags: the resource is zx_buf(nullptr, 0) (res_off and res_bytes must be 0)
enum Op : uint32_t {
  kBallot = 0, kAny, kShfl, kShflUp, kShflXor, kShfl63, kScan64, kLane64, kXorSum64,
  kScanSrc0, kScanSrc1, kScanSrc2, kScanSrc3, kScanSrc4, kScanSrc5, kScanAdd, kShr1,
  kLd8, kLd32, kLd64, kLd96, kLd128, kSt8, kSt32,
  kAlignbit, kPkSub16, kPkSign16, kBfi,
  kGst32u, kGst128, kGld128,
  kOrLds, kMinLds, kMinLds64, kAddLds, kCasLds, kMinGlb, kMaxGlb,
  kPubWave, kPubBarrier, kPubBarrierVm, kPubFence,
  kOps
};

// What must hold before anything is launched: nothing an operand names lies outside the arena, no offset can wrap. No HIP call, no GPU.
inline bool args_ok(uint32_t op, uint32_t threads, uint32_t flags, uint32_t res_off, uint32_t res_bytes, const uint32_t* in, uint32_t arena_bytes) {
  if (op >= kOps || (threads != 64 && threads != 256) || !in || (flags & ~kNullRes)) return false;
  if (arena_bytes < 2 * kGuard || arena_bytes > kArenaMax || (arena_bytes & 15u)) return false;
  if (flags & kNullRes) { if (res_off || res_bytes) return false; }
  else if (res_off < kGuard || res_off > arena_bytes || res_bytes > arena_bytes - res_off || arena_bytes - res_off - res_bytes < kGuard) return false;
  for (uint32_t t = 0; t < threads; t++) {
    const uint32_t* a = in + (size_t)t * kIn;
    const uint32_t x = a[1];
    switch (op) {
      case kLd8: case kLd32: case kLd64: case kLd96: case kLd128: case kSt8: case kSt32:
        if (x >= kOffEnd) return false;
        break;
      case kGst32u: case kMinGlb: case kMaxGlb:
        if (x > arena_bytes - 4 || (op != kGst32u && (x & 3u))) return false;
        break;
      case kGst128: case kGld128:
        if (x > arena_bytes - 16 || (x & 15u)) return false;
        break;
      case kOrLds: case kMinLds: case kMinLds64: case kAddLds: case kCasLds:
        if (x >= kLdsWords) return false;
        break;
      case kPubWave:
        if (a[2] >= threads || (a[2] >> 6) != (t >> 6)) return false;
        break;
      case kPubBarrier:
        if (a[2] >= threads) return false;
        break;
      case kPubBarrierVm: case kPubFence:   // slot t is the arena's word t
        if (a[2] >= threads || arena_bytes < 4 * threads) return false;
        break;
      default: break;
    }
  }
  return true;
}
}  // namespace zxp
#endif  // ZG_ZXPROBE_TYPES

#if defined(ZX_DEV) && !defined(ZG_ZXPROBE_BODY)
#define ZG_ZXPROBE_BODY
#include "zg_flat1.h"     // zx_bfi
#include "zg_seektab.h"   // scan64, lane64
namespace zxp {

struct Lds { uint32_t w[256]; unsigned long long q[kLdsWords]; };

// ---- wave collectives ------------------------------------------------------------------------------------------------------------------
ZX_DEV void p_ballot(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const unsigned long long r = zx_ballot((a[1] & 1u) != 0u);
  o[0] = (uint32_t)r; o[1] = (uint32_t)(r >> 32);
}
ZX_DEV void p_any(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const bool r = zx_any((a[1] & 1u) != 0u);
  o[0] = r ? 1u : 0u;
}
ZX_DEV void p_shfl(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const uint32_t r = zx_shfl(a[1], (int)a[2]);
  o[0] = r;
}
ZX_DEV void p_shfl_up(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const uint32_t r = zx_shfl_up(a[1], (int)a[2]);
  o[0] = r;
}
ZX_DEV void p_shfl_xor(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const uint32_t r = zx_shfl_xor(a[1], (int)a[2]);
  o[0] = r;
}
// the wave's last lane by a constant, as the bodies ask for a wave total (zg_huf.h, zg_records.h, zg_inorder.h)
ZX_DEV void p_shfl63(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const uint32_t r = zx_shfl(a[1], 63);
  o[0] = r;
}
// the 64-bit idioms the bodies build from two calls: zg_seektab.h's scan64 and lane64, the butterfly sum of zg_seekmany.h
ZX_DEV void p_scan64(const uint32_t* a, uint32_t* o, uint32_t lane) {
  if (a[0]) return;
  const uint64_t r = zgt::scan64(((uint64_t)a[2] << 32) | a[1], lane);
  o[0] = (uint32_t)r; o[1] = (uint32_t)(r >> 32);
}
ZX_DEV void p_lane64(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const uint64_t r = zgt::lane64(((uint64_t)a[2] << 32) | a[1], a[3]);
  o[0] = (uint32_t)r; o[1] = (uint32_t)(r >> 32);
}
ZX_DEV void p_xorsum64(const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  uint64_t c0 = ((uint64_t)a[2] << 32) | a[1];
  for (int sh = 32; sh >= 1; sh >>= 1) c0 += ((uint64_t)zx_shfl_xor((uint32_t)(c0 >> 32), sh) << 32) | zx_shfl_xor((uint32_t)c0, sh);
  o[0] = (uint32_t)c0; o[1] = (uint32_t)(c0 >> 32);
}

// ---- DPP ---------------------------------------------------------------------------------------------------------------------------------
template <int S> ZX_DEV void p_scan_src(const uint32_t* a, uint32_t* o, uint32_t lane) {
  const uint32_t r = zx_scan_src<S>(a[1], a[2]);
  o[0] = r; o[1] = zx_scan_takes<S>(lane) ? 1u : 0u;
}
ZX_DEV void p_scan_add(const uint32_t* a, uint32_t* o) {
  const uint32_t r = zx_scan_incl_add(a[1]);
  o[0] = r;
}
ZX_DEV void p_shr1(const uint32_t* a, uint32_t* o) {
  const uint32_t r = zx_shr1(a[1], a[2]);
  o[0] = r;
}

// ---- raw buffers -------------------------------------------------------------------------------------------------------------------------
ZX_DEV void p_ld8(const ZxBuf& b, const uint32_t* a, uint32_t* o) { if (a[0]) return; o[0] = zx_ld8(b, a[1]); }
ZX_DEV void p_ld32(const ZxBuf& b, const uint32_t* a, uint32_t* o) { if (a[0]) return; o[0] = zx_ld32(b, a[1]); }
ZX_DEV void p_ld64(const ZxBuf& b, const uint32_t* a, uint32_t* o) { if (a[0]) return; const ZxU2 r = zx_ld64(b, a[1]); o[0] = r.x; o[1] = r.y; }
ZX_DEV void p_ld96(const ZxBuf& b, const uint32_t* a, uint32_t* o) { if (a[0]) return; const ZxU3 r = zx_ld96(b, a[1]); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
ZX_DEV void p_ld128(const ZxBuf& b, const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const ZxU4 r = zx_ld128(b, a[1]);
  o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
}
ZX_DEV void p_st8(const ZxBuf& b, const uint32_t* a) { if (a[0]) return; zx_st8(b, a[1], a[2]); }
ZX_DEV void p_st32(const ZxBuf& b, const uint32_t* a) { if (a[0]) return; zx_st32(b, a[1], a[2]); }

// ---- integer helpers ---------------------------------------------------------------------------------------------------------------------
ZX_DEV void p_alignbit(const uint32_t* a, uint32_t* o) { o[0] = zx_alignbit(a[1], a[2], a[3]); }
ZX_DEV void p_pksub16(const uint32_t* a, uint32_t* o) { o[0] = zx_pksub16(a[1], a[2]); }
ZX_DEV void p_pksign16(const uint32_t* a, uint32_t* o) { o[0] = zx_pksign16(a[1]); }
ZX_DEV void p_bfi(const uint32_t* a, uint32_t* o) { o[0] = zx_bfi(a[1], a[2], a[3]); }

// ---- memory helpers (a[1]: checked by the host against the arena / the LDS words) ----------------------------------------------------------
ZX_DEV void p_gst32u(uint8_t* arena, const uint32_t* a) { if (a[0]) return; zx_gst32u(arena + a[1], a[2]); }
ZX_DEV void p_gst128(uint8_t* arena, const uint32_t* a) {
  if (a[0]) return;
  ZxU4 v; v.x = a[2]; v.y = a[3]; v.z = a[4]; v.w = a[5];
  zx_gst128(arena + a[1], v);
}
ZX_DEV void p_gld128(const uint8_t* arena, const uint32_t* a, uint32_t* o) {
  if (a[0]) return;
  const ZxU4 r = zx_gld128(arena + a[1]);
  o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
}
// LDS word t < 64 starts as thread t's a[7] (the 64-bit words: a[6] low, a[7] high); barrier; the primitive; barrier; thread t reads word t & 63
template <int WHICH> ZX_DEV void p_lds(Lds& L, const uint32_t* a, uint32_t* o, uint32_t t) {
  if (t < kLdsWords) { L.w[t] = a[7]; L.q[t] = ((unsigned long long)a[7] << 32) | a[6]; }
  zx_syncthreads();
  if (!a[0]) {
    if (WHICH == kOrLds) zx_or_lds(&L.w[a[1]], a[2]);
    if (WHICH == kMinLds) zx_min_lds(&L.w[a[1]], a[2]);
    if (WHICH == kMinLds64) zx_min_lds64(&L.q[a[1]], ((unsigned long long)a[3] << 32) | a[2]);
    if (WHICH == kAddLds) zx_add_lds(&L.w[a[1]], a[2]);
    if (WHICH == kCasLds) zx_cas_lds(&L.w[a[1]], a[2], a[3]);
  }
  zx_syncthreads();
  if (WHICH == kMinLds64) { const unsigned long long r = L.q[t & (kLdsWords - 1)]; o[0] = (uint32_t)r; o[1] = (uint32_t)(r >> 32); }
  else o[0] = L.w[t & (kLdsWords - 1)];
}
ZX_DEV void p_min_glb(uint8_t* arena, const uint32_t* a) { if (a[0]) return; zx_min_glb((uint32_t*)(arena + a[1]), a[2]); }
ZX_DEV void p_max_glb(uint8_t* arena, const uint32_t* a) { if (a[0]) return; zx_max_glb((uint32_t*)(arena + a[1]), a[2]); }

// ---- publish: write the own slot, synchronise, read slot a[2] --------------------------------------------------------------------------
ZX_DEV void p_pub_wave(Lds& L, const uint32_t* a, uint32_t* o, uint32_t t) { L.w[t] = a[1]; zx_wave_sync(); o[0] = L.w[a[2]]; }
ZX_DEV void p_pub_barrier(Lds& L, const uint32_t* a, uint32_t* o, uint32_t t) { L.w[t] = a[1]; zx_barrier(); o[0] = L.w[a[2]]; }
ZX_DEV void p_pub_barrier_vm(uint8_t* arena, const uint32_t* a, uint32_t* o, uint32_t t) {
  volatile uint32_t* slots = (volatile uint32_t*)arena;
  slots[t] = a[1]; zx_barrier_vm(); o[0] = slots[a[2]];
}
ZX_DEV void p_pub_fence(uint8_t* arena, const uint32_t* a, uint32_t* o, uint32_t t) {
  volatile uint32_t* slots = (volatile uint32_t*)arena;
  slots[t] = a[1]; zx_fence_block(); zx_syncthreads(); o[0] = slots[a[2]];
}

// the workgroup's body: `op` and everything but in[] and out[] are the same for every thread
ZX_DEV void probe(uint32_t op, uint32_t flags, const uint32_t* in, uint32_t* out, uint8_t* arena, uint32_t res_off, uint32_t res_bytes, Lds& L) {
  const uint32_t t = zx_tid(), lane = t & 63u;
  const uint32_t* a = in + (size_t)t * kIn;
  uint32_t* o = out + (size_t)t * kOut;
  switch (op) {
    case kBallot: p_ballot(a, o); break;
    case kAny: p_any(a, o); break;
    case kShfl: p_shfl(a, o); break;
    case kShflUp: p_shfl_up(a, o); break;
    case kShflXor: p_shfl_xor(a, o); break;
    case kShfl63: p_shfl63(a, o); break;
    case kScan64: p_scan64(a, o, lane); break;
    case kLane64: p_lane64(a, o); break;
    case kXorSum64: p_xorsum64(a, o); break;
    case kScanSrc0: p_scan_src<0>(a, o, lane); break;
    case kScanSrc1: p_scan_src<1>(a, o, lane); break;
    case kScanSrc2: p_scan_src<2>(a, o, lane); break;
    case kScanSrc3: p_scan_src<3>(a, o, lane); break;
    case kScanSrc4: p_scan_src<4>(a, o, lane); break;
    case kScanSrc5: p_scan_src<5>(a, o, lane); break;
    case kScanAdd: p_scan_add(a, o); break;
    case kShr1: p_shr1(a, o); break;
    case kLd8: case kLd32: case kLd64: case kLd96: case kLd128: case kSt8: case kSt32: {
      ZxBuf b = zx_buf(nullptr, 0);
      if (!(flags & kNullRes)) b = zx_buf(arena + res_off, res_bytes);
      if (op == kLd8) p_ld8(b, a, o);
      else if (op == kLd32) p_ld32(b, a, o);
      else if (op == kLd64) p_ld64(b, a, o);
      else if (op == kLd96) p_ld96(b, a, o);
      else if (op == kLd128) p_ld128(b, a, o);
      else if (op == kSt8) p_st8(b, a);
      else p_st32(b, a);
      break;
    }
    case kAlignbit: p_alignbit(a, o); break;
    case kPkSub16: p_pksub16(a, o); break;
    case kPkSign16: p_pksign16(a, o); break;
    case kBfi: p_bfi(a, o); break;
    case kGst32u: p_gst32u(arena, a); break;
    case kGst128: p_gst128(arena, a); break;
    case kGld128: p_gld128(arena, a, o); break;
    case kOrLds: p_lds<kOrLds>(L, a, o, t); break;
    case kMinLds: p_lds<kMinLds>(L, a, o, t); break;
    case kMinLds64: p_lds<kMinLds64>(L, a, o, t); break;
    case kAddLds: p_lds<kAddLds>(L, a, o, t); break;
    case kCasLds: p_lds<kCasLds>(L, a, o, t); break;
    case kMinGlb: p_min_glb(arena, a); break;
    case kMaxGlb: p_max_glb(arena, a); break;
    case kPubWave: p_pub_wave(L, a, o, t); break;
    case kPubBarrier: p_pub_barrier(L, a, o, t); break;
    case kPubBarrierVm: p_pub_barrier_vm(arena, a, o, t); break;
    case kPubFence: p_pub_fence(arena, a, o, t); break;
    default: break;
  }
}
}  // namespace zxp
#endif  // ZX_DEV
