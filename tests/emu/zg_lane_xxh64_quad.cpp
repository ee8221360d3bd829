// zg_lane_xxh64_quad.cpp — TEST-ONLY: the quad routine of zg_k_xxh64q (zstd-rs_amd/csrc/zg_xxh64_dev.h: xxh64q_acc, xxh64q_finish) for the
// CPU. tests/test_xxh64_quad_cpu.py builds this file (tests/lanesuite.py) as a shared library and holds it against the oracle's XXH64. It plays
// one quad: the lanes exchange nothing before the gather, so running them one after the other is what four lanes in lockstep compute. The
// routine reads through a plain pointer: there is no accessor to count. Not part of the product.
#include "zg_xxh64_dev.h"
extern "C" uint64_t quad_xxh64(const uint8_t* p, uint64_t n, uint64_t seed) {
  uint64_t v[4];
  for (uint32_t l = 0; l < 4; l++) v[l] = zgx::xxh64q_acc(p, n, seed, l);   // the four lanes of the quad
  return zgx::xxh64q_finish(p, n, seed, v[0], v[1], v[2], v[3]);            // lane 0, after the gather
}
extern "C" uint32_t quad_round() { return zgx::kQuadRound; }
