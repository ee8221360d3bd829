// zg_lane_xxh64.cpp — TEST-ONLY: the lane routine of zg_k_xxh64 (zstd-rs_amd/csrc/zg_xxh64_dev.h) for the CPU. tests/test_xxh64_cpu.py builds
// this file (tests/lanesuite.py) as a shared library and holds it against the oracle's XXH64. The routine reads through a plain pointer: there
// is no accessor to count. Not part of the product.
#include "zg_xxh64_dev.h"
extern "C" uint64_t lane_xxh64(const uint8_t* p, uint64_t n, uint64_t seed) { return zgx::xxh64(p, n, seed); }
