// zg_xxh64_dev.h — XXH64 of one byte range by one lane: the routine zg_k_xxh64 runs per lane (one lane per frame, zg_kernels.hip), written as
// plain C++ on uint64_t so that the same source also compiles with g++ (tests/test_xxh64_cpu.py checks it against the oracle's XXH64).
// Below it, the same hash by a quad of lanes (zg_k_xxh64q, one accumulator per lane; tests/test_xxh64_quad_cpu.py): the kernel for few long
// ranges, where one lane's rate is what a range costs.
// The full public algorithm with any seed: inputs shorter than 32 bytes, the 8 / 4 / 1-byte tail, the avalanche (what zg_xxh64.h's
// streaming hasher computes over the same bytes in one update()).
//
// Shape: the four accumulators stay in registers — four independent multiply chains per lane — and each 32-byte stripe arrives as two 16-byte
// loads. The source issues them two stripes ahead, but the compiler waits for every outstanding load at the top of the next iteration
// (s_waitcnt vmcnt(0)), so in effect one stripe's loads are in flight while one stripe is mixed: a lane is bound by load latency. Loads go to any byte address: gfx950 runs in unaligned access mode, and the
// 16-byte load of a misaligned stripe is one global_load_dwordx4 (the hardware splits it; every lane streams its own range, so the split
// halves hit the line the previous stripe brought in).
// gfx950 ISA of zg_k_xxh64 (hipcc -O3 --save-temps): the 16-byte loads are global_load_dwordx4; a multiply by a 64-bit constant is v_mad_u64_u32 +
// 2 v_mul_lo_u32 + v_add3_u32 (the low product and its two cross terms), the rotate v_lshlrev_b64 + v_lshrrev_b32 + v_or_b32, so one mix() is
// 11 VALU and a 32-byte stripe 44 VALU of mixing + ~10 of loop control and register moves (~54 per stripe, 1.7 per byte); 52 VGPRs, no scratch.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define ZG_XH_FN __host__ __device__ __forceinline__
#else
#define ZG_XH_FN static inline
#endif

namespace zgx {
constexpr uint64_t kP1 = 11400714785074694791ULL, kP2 = 14029467366897019727ULL, kP3 = 1609587929392839161ULL,
                   kP4 = 9650029242287828579ULL, kP5 = 2870177450012600261ULL;
ZG_XH_FN uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
ZG_XH_FN uint64_t mix(uint64_t acc, uint64_t in) { acc += in * kP2; acc = rotl(acc, 31); return acc * kP1; }
ZG_XH_FN uint64_t merge(uint64_t h, uint64_t v) { h ^= mix(0, v); return h * kP1 + kP4; }
ZG_XH_FN uint64_t ld64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
ZG_XH_FN uint32_t ld32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
struct Half { uint64_t a, b; };   // 16 bytes: one load
ZG_XH_FN Half ld128(const uint8_t* p) { Half h; memcpy(&h, p, 16); return h; }

// XXH64(p[0 .. len), seed)
ZG_XH_FN uint64_t xxh64(const uint8_t* p, uint64_t len, uint64_t seed) {
  const uint8_t* const end = p + len;
  uint64_t h;
  if (len >= 32) {
    uint64_t v0 = seed + kP1 + kP2, v1 = seed + kP2, v2 = seed, v3 = seed - kP1;
    const uint8_t* const stop = p + (len & ~(uint64_t)31);   // behind the last whole stripe
    // the loads of stripe k + 2 are issued while stripe k is mixed (never beyond the range: the tail is read below, word by word); the compiler
    // waits for them at the top of the next iteration, so one stripe's loads overlap one stripe's mixing
    Half x = ld128(p), y = ld128(p + 16), x2 = x, y2 = y;
    if (p + 32 < stop) { x2 = ld128(p + 32); y2 = ld128(p + 48); }
    for (;;) {
      const Half cx = x, cy = y;
      x = x2; y = y2;
      p += 32;
      if (p + 32 < stop) { x2 = ld128(p + 32); y2 = ld128(p + 48); }
      v0 = mix(v0, cx.a); v1 = mix(v1, cx.b); v2 = mix(v2, cy.a); v3 = mix(v3, cy.b);
      if (p >= stop) break;
    }
    h = rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
    h = merge(h, v0); h = merge(h, v1); h = merge(h, v2); h = merge(h, v3);
  } else {
    h = seed + kP5;
  }
  h += len;
  while (p + 8 <= end) { h ^= mix(0, ld64(p)); h = rotl(h, 27) * kP1 + kP4; p += 8; }
  if (p + 4 <= end) { h ^= (uint64_t)ld32(p) * kP1; h = rotl(h, 23) * kP2 + kP3; p += 4; }
  while (p < end) { h ^= (uint64_t)(*p) * kP5; h = rotl(h, 11) * kP1; p++; }
  h ^= h >> 33; h *= kP2; h ^= h >> 29; h *= kP3; h ^= h >> 32;
  return h;
}

// ---- one range by a QUAD of lanes (zg_k_xxh64q) -----------------------------------------------------------------------------------------
// XXH64 is serial per accumulator, but its four accumulators never meet before the merge: lane l of a quad owns v_l and reads word l (8 bytes)
// of every 32-byte stripe, so the quad's four loads of a stripe are 32 contiguous bytes and a lane's chain is one mix() per stripe, not four.
//   xxh64q_acc     lane l's accumulator after the last whole stripe (its seed value when len < 32: the lane then reads nothing)
//   xxh64q_finish  what lane 0 does once it holds all four (the kernel collects them by shuffle): the merge, the 8 / 4 / 1-byte tail, the
//                  avalanche. A range shorter than 32 bytes is this routine alone.
// Shape of the stripe loop: a ROUND is kQuadRound stripes. The loads of the next round (kQuadRound 8-byte loads per lane) are issued before
// the current round is mixed, into the other of two register buffers — the loop body is two rounds, a and b changing roles, so that no loaded
// value is copied across the back edge (the copy is what made the compiler wait for every load in the one-lane loop above), and the loop runs
// only while both of its loads are due, so that neither is conditional (a conditional load is a select, and a select is a copy again). A round is only
// loaded when it lies wholly in front of the last whole stripe's end: no lane reads a byte outside [p, p + len), prefetch included. The
// stripes behind the last round (fewer than kQuadRound) are read one at a time, and the tail by lane 0 in xxh64q_finish, word by word.
// gfx950 ISA of zg_k_xxh64q (hipcc -O3 --save-temps): every 8-byte load is one global_load_dwordx2 at any byte address (unaligned access mode,
// as above), 32 of them in the two-round loop body with constant offsets from one address register pair; the body's 32 mix() are 352 VALU
// (11 each, the same instructions as above) + 4 of loop control: 11.1 VALU per stripe and lane against ~54 in the one-lane loop, and the
// waits count the loads down (s_waitcnt vmcnt(31) .. vmcnt(16), one per mix) instead of draining them. With the loads of a round written
// conditionally (a first form of this loop) the compiler copied the buffers with v_mov_b64 behind an s_waitcnt vmcnt(0): the one-lane
// routine's problem again, and the reason for the loop's shape. 113 VGPRs (two buffers of 16 x 2), no scratch, no LDS allocation (the
// gather is 8 ds_bpermute_b32). Measured rates: LABNOTES.md "xxh64q".
#if defined(__clang__)
#define ZG_XH_UNROLL _Pragma("unroll")
#else
#define ZG_XH_UNROLL
#endif
constexpr uint32_t kQuadRound = 16;                    // stripes per round: 16 x 8 bytes per lane, 512 bytes per quad in flight
constexpr uint64_t kQuadRoundBytes = 32ull * kQuadRound;

ZG_XH_FN uint64_t xxh64q_acc(const uint8_t* p, uint64_t len, uint64_t seed, uint32_t l) {
  uint64_t v = l == 0 ? seed + kP1 + kP2 : l == 1 ? seed + kP2 : l == 2 ? seed : seed - kP1;
  const uint64_t stripes = len >> 5;
  uint64_t left = stripes / kQuadRound;                // whole rounds not yet mixed
  const uint8_t* q = p + 8u * l;                       // the lane's word of the stripe at hand
  const uint8_t* const stop = q + stripes * 32;        // the lane's word of the stripe behind the last whole one (not read)
  if (left) {
    uint64_t a[kQuadRound], b[kQuadRound];
    ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) a[j] = ld64(q + 32u * j);
    // a holds the round at q. While a round lies behind the next one, both loads of the body are unconditional: a and b are written by loads
    // only, never by a select or a copy, so the compiler counts the loads down (s_waitcnt vmcnt(N)) instead of waiting for all of them.
    for (; left >= 3; left -= 2) {
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) b[j] = ld64(q + kQuadRoundBytes + 32u * j);
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) v = mix(v, a[j]);
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) a[j] = ld64(q + 2 * kQuadRoundBytes + 32u * j);
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) v = mix(v, b[j]);
      q += 2 * kQuadRoundBytes;
    }
    if (left == 2) {
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) b[j] = ld64(q + kQuadRoundBytes + 32u * j);
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) v = mix(v, a[j]);
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) v = mix(v, b[j]);
      q += 2 * kQuadRoundBytes;
    } else {
      ZG_XH_UNROLL for (uint32_t j = 0; j < kQuadRound; j++) v = mix(v, a[j]);
      q += kQuadRoundBytes;
    }
  }
  for (; q < stop; q += 32) v = mix(v, ld64(q));
  return v;
}

// XXH64(p[0 .. len), seed) from the four accumulators of xxh64q_acc (ignored when len < 32)
ZG_XH_FN uint64_t xxh64q_finish(const uint8_t* p, uint64_t len, uint64_t seed, uint64_t v0, uint64_t v1, uint64_t v2, uint64_t v3) {
  const uint8_t* const end = p + len;
  uint64_t h;
  if (len >= 32) {
    h = rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
    h = merge(h, v0); h = merge(h, v1); h = merge(h, v2); h = merge(h, v3);
    p += len & ~(uint64_t)31;
  } else {
    h = seed + kP5;
  }
  h += len;
  while (p + 8 <= end) { h ^= mix(0, ld64(p)); h = rotl(h, 27) * kP1 + kP4; p += 8; }
  if (p + 4 <= end) { h ^= (uint64_t)ld32(p) * kP1; h = rotl(h, 23) * kP2 + kP3; p += 4; }
  while (p < end) { h ^= (uint64_t)(*p) * kP5; h = rotl(h, 11) * kP1; p++; }
  h ^= h >> 33; h *= kP2; h ^= h >> 29; h *= kP3; h ^= h >> 32;
  return h;
}
}  // namespace zgx
