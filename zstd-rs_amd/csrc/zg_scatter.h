// zg_scatter.h — zg_k_scatter: a submit's plaintext, which lies back to back in the batch output at offsets of any alignment, copied to
// destinations the caller owns (zgpu_decode_frames_device), one launch per submit. The chunk plan (host) and the routine a lane runs
// (device) are plain C++ behind two accessors, so that the same source also compiles with g++ (tests/test_scatter_cpu.py runs it lane by
// lane against a slice copy, with a reader that asserts every read stays inside the source and a writer that asserts every write stays
// inside the destination and every 16-byte store is aligned).
//
// Plan: one segment (src_off, dst, len) per frame; a segment is cut into chunks of at most `chunk` bytes whose inner boundaries lie on
// 16-byte boundaries of the DESTINATION, so only a segment's first chunk has head bytes and only its last one tail bytes. One workgroup of
// 256 threads takes a chunk (grid-stride over the chunk table, at most kMaxGroups workgroups).
// Body: head bytes up to the destination's 16-byte alignment (one byte per lane), then 16 bytes per lane and pass — a 16-byte load from the
// source at whatever alignment it has, a 16-byte store to an aligned destination address, four passes in flight per lane —, then the tail
// bytes. Loads never leave [src_off, src_off + len) — no padding behind the batch output is needed (it has kOutFront bytes in front and 64
// behind, zg_engine.cpp) — and stores never leave [dst, dst + len). Stores are plain: round 5 measured WRITE_SIZE 3.13x with nontemporal
// stores to unaligned addresses (LABNOTES.md), and a caller reads these bytes next.
// gfx950 ISA of zg_k_scatter (hipcc -O3 --save-temps): the body loop is 4 global_load_dwordx4 + 4 global_store_dwordx4 per iteration (gfx950
// runs in unaligned access mode: the load of a misaligned source is ONE global_load_dwordx4, as in zg_k_xxh64), its remainder loop one of
// each; head and tail are global_load_ubyte / global_store_byte; 38 VGPRs, no scratch, no LDS. (The writer stores through address space 1:
// through a generic pointer made from the table's integer the stores are flat_store_dwordx4.) Measured: 512 MiB in 187 us, 0.51 x the time
// of the 16 B/lane calibration copy on the same bytes; 16 / 64 / 256 KiB chunks measure the same (LABNOTES.md "decode_frames_device").
//
// zg_k_fill — the store half of the same problem: m byte regions of any length and alignment in ONE piece of the caller's device memory set to
// one byte (zgpu_gather_records_batch_indexed_device_src: the pad behind every row of a record batch). A region is a Seg whose src_off is
// unused; plan_chunks cuts the regions with kFillChunk, so inner chunk boundaries lie on 16-byte boundaries of the destination, only a
// region's first chunk has head bytes and only its last one tail bytes. fill_chunk is copy_chunk without the loads: head bytes up to the
// 16-byte boundary (one st1 per lane), st16 of the replicated byte at multiples of 16 — four in flight per lane —, tail bytes. Plain vector
// stores, no nontemporal ones (above), no atomics; the kernel reads its two tables and nothing else.
// Shape: ONE WAVE per chunk (kFillThreads = 64, a workgroup is a wave), grid-stride over the chunk table, at most kFillMaxGroups workgroups;
// kFillChunk = 4096 bytes is four passes of 64 lanes x 16 bytes. Why: a pad region is a fraction of a row — hundreds of bytes to a few KiB —,
// so a chunk rarely has more than 64 16-byte stores to hand out and three of a 256-thread workgroup's four waves would compute a head, a
// body count and a tail only to store nothing; with a wave per chunk the CUs hold four times as many chunks in flight. UNMEASURED as a
// comparison of shapes: LABNOTES.md "records_batch" has what was measured of this one. The host checks every region against
// [device_dst, device_dst + total) before the launch (zg_ranges.cpp).
// gfx950 ISA of zg_k_fill (hipcc -O3 --save-temps, the code object's metadata and the .s): 18 VGPRs, 32 SGPRs, no scratch (private segment 0),
// no spill, no LDS. Per chunk 1 global_load_dwordx4 (the 16-byte Chunk) and 1 global_load_dwordx2 (the region's dst); the head and the tail
// are 1 global_store_byte each, the body loop 4 global_store_dwordx4 per iteration and its remainder loop 1. No flat_*, no atomic.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

#if defined(__HIP__) || defined(__HIPCC__)
#define ZG_SC_FN __host__ __device__ __forceinline__
#else
#define ZG_SC_FN static inline
#endif

namespace zgs {

constexpr uint32_t kThreads = 256;           // lanes of the workgroup that takes a chunk
constexpr uint32_t kMaxGroups = 2048;        // workgroups of a launch (8 per CU on 256 CUs)
constexpr uint32_t kChunkDefault = 64u << 10;   // bytes per chunk: 16 passes of 256 lanes x 16 bytes (LABNOTES.md "decode_frames_device")
constexpr uint32_t kChunkMin = 4096;

constexpr uint32_t kFillThreads = 64;        // zg_k_fill: one wave takes a chunk
constexpr uint32_t kFillMaxGroups = 2048;    // zg_k_fill: workgroups (waves) of a launch
constexpr uint32_t kFillChunk = 4096;        // zg_k_fill: bytes per chunk, four passes of 64 lanes x 16 bytes

struct Seg { uint64_t src_off, dst, len; };       // dst: the destination's address (zg_k_fill: src_off is unused)
struct Chunk { uint32_t seg, len; uint64_t at; };   // bytes [at, at + len) of segment seg
struct alignas(16) V16 { uint64_t a, b; };

// chunk size the plan uses for a requested one: a multiple of 16, at least kChunkMin
static inline uint32_t chunk_bytes(uint32_t want) {
  if (want == 0) want = kChunkDefault;
  if (want < kChunkMin) want = kChunkMin;
  return want & ~15u;
}

// the chunks of segs[0 .. n), in order; every byte of every segment in exactly one chunk; dst + at of every chunk but a segment's first is
// a multiple of 16; no chunk is longer than chunk_bytes(chunk); segments of length 0 have none
static inline void plan_chunks(const Seg* segs, uint32_t n, uint32_t chunk, std::vector<Chunk>* out) {
  const uint64_t C = chunk_bytes(chunk);
  for (uint32_t s = 0; s < n; s++) {
    const uint64_t D = segs[s].dst, L = segs[s].len;
    for (uint64_t at = 0; at < L;) {
      uint64_t end = at + C;
      if (end >= L) end = L;
      else end -= (D + end) & 15;   // (C >= kChunkMin: end stays behind at)
      out->push_back(Chunk{s, (uint32_t)(end - at), at});
      at = end;
    }
  }
}

// What lane t of T does for the chunk [src, src + len) -> [dst, dst + len): R reads the source (ld1 / ld16 at any offset), W writes the
// destination (st1 at any address, st16 at multiples of 16 only).
template <class R, class W> ZG_SC_FN void copy_chunk(const R& r, const W& w, uint64_t src, uint64_t dst, uint32_t len, uint32_t t, uint32_t T) {
  uint32_t head = (uint32_t)((16 - (dst & 15)) & 15);
  if (head > len) head = len;
  if (t < head) w.st1(dst + t, r.ld1(src + t));
  const uint32_t nbody = (len - head) >> 4;
  const uint64_t s0 = src + head, d0 = dst + head;
  uint32_t k = t;
  for (; k + 3 * T < nbody; k += 4 * T) {   // four loads in flight per lane
    const V16 a = r.ld16(s0 + 16ull * k), b = r.ld16(s0 + 16ull * (k + T)), c = r.ld16(s0 + 16ull * (k + 2 * T)), d = r.ld16(s0 + 16ull * (k + 3 * T));
    w.st16(d0 + 16ull * k, a);
    w.st16(d0 + 16ull * (k + T), b);
    w.st16(d0 + 16ull * (k + 2 * T), c);
    w.st16(d0 + 16ull * (k + 3 * T), d);
  }
  for (; k < nbody; k += T) w.st16(d0 + 16ull * k, r.ld16(s0 + 16ull * k));
  const uint32_t done = head + (nbody << 4);   // (the tail is shorter than 16 bytes)
  if (t < len - done) w.st1(dst + done + t, r.ld1(src + done + t));
}

// What lane t of T does for the chunk [dst, dst + len) of a fill: W as above, `byte` into every byte. No byte is read.
template <class W> ZG_SC_FN void fill_chunk(const W& w, uint64_t dst, uint32_t len, uint8_t byte, uint32_t t, uint32_t T) {
  uint32_t head = (uint32_t)((16 - (dst & 15)) & 15);
  if (head > len) head = len;
  if (t < head) w.st1(dst + t, byte);
  const uint32_t nbody = (len - head) >> 4;
  const uint64_t d0 = dst + head, r = 0x0101010101010101ull * byte;
  const V16 v{r, r};
  uint32_t k = t;
  for (; k + 3 * T < nbody; k += 4 * T) {   // four stores in flight per lane
    w.st16(d0 + 16ull * k, v);
    w.st16(d0 + 16ull * (k + T), v);
    w.st16(d0 + 16ull * (k + 2 * T), v);
    w.st16(d0 + 16ull * (k + 3 * T), v);
  }
  for (; k < nbody; k += T) w.st16(d0 + 16ull * k, v);
  const uint32_t done = head + (nbody << 4);   // (the tail is shorter than 16 bytes)
  if (t < len - done) w.st1(dst + done + t, byte);
}

}  // namespace zgs
