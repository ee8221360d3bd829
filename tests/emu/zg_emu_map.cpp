// TEST-ONLY: the symbolic offset history's map algebra (zg_dev.h: ZgHistMap, zg_map_apply, zg_map_compose, zg_sym_resolve) on the host.
// The harness's own decode (zg_emu.cpp, zg_emu_serial.h) steps the history serially with zg_hist_step and never composes maps; the
// kernels (zg_k_seqpost, zg_k_scan) compose them in the order their shuffles, LDS steps and carries give. This entry runs one string
// of (literal length zero or not, offset_value) both ways: serially on concrete slots, and as per-sequence maps folded under several
// bracketings (tests/test_repframes_cpu.py compares the serial side with its own statement of RFC 8878 3.1.1.5).
#include <stdint.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_dev.h"

namespace {

struct Rng {   // xorshift64*: the bracketings only have to be reproducible
  uint64_t s;
  uint32_t below(uint32_t n) {
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    return (uint32_t)(((s * 0x2545F4914F6CDD1Dull) >> 33) % n);
  }
};

// the map of sequences [a, b), split at random points down to runs of at most `leaf` sequences, which are stepped directly from
// the identity (a thread's own sequences in zg_k_seqpost); leaf == 1: every sequence is a map of its own
ZgHistMap tree(const std::vector<ZgHistMap>& m, const uint32_t* of, const uint8_t* ll, uint32_t a, uint32_t b, uint32_t leaf, Rng& r) {
  if (b - a <= leaf) {
    if (b - a == 1) return m[a];
    ZgHistMap x = zg_map_identity();
    for (uint32_t i = a; i < b; i++) zg_hist_step(of[i], ll[i], x.s[0], x.s[1], x.s[2]);
    return x;
  }
  const uint32_t mid = a + 1 + r.below(b - a - 1);
  const ZgHistMap L = tree(m, of, ll, a, mid, leaf, r), R = tree(m, of, ll, mid, b, leaf, r);
  return zg_map_compose(L, R);
}

}  // namespace

extern "C" {

void zgemu_map_apply(const uint32_t* a3, uint32_t v, uint32_t* out) { ZgHistMap A = {{a3[0], a3[1], a3[2]}}; *out = zg_map_apply(A, v); }
void zgemu_map_compose(const uint32_t* a3, const uint32_t* b3, uint32_t* out3) {
  ZgHistMap A = {{a3[0], a3[1], a3[2]}}, B = {{b3[0], b3[1], b3[2]}};
  const ZgHistMap r = zg_map_compose(A, B);
  out3[0] = r.s[0]; out3[1] = r.s[1]; out3[2] = r.s[2];
}
uint32_t zgemu_sym_resolve(uint32_t v, const uint32_t* h3) { return zg_sym_resolve(v, h3); }

// of[i]: offset_value as zg_k_seqpost hands it to zg_hist_step (1..3 repeat codes, else offset + 3); ll[i]: 0 or not; hist: the history
// in front of sequence 0. serial[4 * i ..]: the actual offset of sequence i and the three slots behind it, from zg_hist_step on
// concrete values. Returns 0 if, for every prefix [0, p), p = 1..n, the composed map under a left fold, a right fold and `ntrees`
// random trees (leaf runs of 1, and of up to 8 stepped directly) resolves to serial's slots, and the sequence's symbolic offset
// applied to the map in front of it resolves to serial's offset; else 1 + the first p that differs, with the bracketing in *which
// (0 left, 1 right, 2.. trees).
uint32_t zgemu_map_fold(const uint32_t* of, const uint8_t* ll, uint32_t n, const uint32_t* hist, uint64_t seed, uint32_t ntrees, uint32_t* serial, uint32_t* which) {
  uint32_t h[3] = {hist[0], hist[1], hist[2]};
  std::vector<ZgHistMap> m(n);
  std::vector<uint32_t> act(n);
  for (uint32_t i = 0; i < n; i++) {
    serial[4 * i] = zg_hist_step(of[i], ll[i], h[0], h[1], h[2]);
    serial[4 * i + 1] = h[0]; serial[4 * i + 2] = h[1]; serial[4 * i + 3] = h[2];
    ZgHistMap x = zg_map_identity();
    act[i] = zg_hist_step(of[i], ll[i], x.s[0], x.s[1], x.s[2]);
    m[i] = x;
  }
  Rng r{seed * 2654435761ull + 88172645463325252ull};
  auto same = [&](const ZgHistMap& M, uint32_t p) {   // M: the map of [0, p)
    for (int k = 0; k < 3; k++)
      if (zg_sym_resolve(M.s[k], hist) != (p ? serial[4 * (p - 1) + 1 + k] : hist[k])) return false;
    return p == n || zg_sym_resolve(zg_map_apply(M, act[p]), hist) == serial[4 * p];
  };
  ZgHistMap left = zg_map_identity();
  for (uint32_t p = 0; p <= n; p++) {
    if (p) left = zg_map_compose(left, m[p - 1]);
    if (!same(left, p)) { *which = 0; return 1 + p; }
    if (!p) continue;
    ZgHistMap right = m[p - 1];
    for (uint32_t i = p - 1; i-- > 0;) right = zg_map_compose(m[i], right);
    if (!same(right, p)) { *which = 1; return 1 + p; }
    for (uint32_t t = 0; t < ntrees; t++) {
      const ZgHistMap x = tree(m, of, ll, 0, p, t & 1 ? 1u + r.below(8) : 1u, r);
      if (!same(x, p)) { *which = 2 + t; return 1 + p; }
    }
  }
  return 0;
}

}
