// zg_idxsums.h — zg_k_idxsums: does a seek index HANDLE vouch for the frames that were decoded of one of its entries (ZGPU_DEVICE_VERIFY_SEEK_TABLE
// of zgpu_gather_ranges_indexed_device_src, for an entry whose handle holds sums)? The handle keeps, beside the pairs { C[k], D[k] } of every
// row, one uint32_t per row in device memory: the low 32 bits of XXH64 (seed 0) of that row's plaintext — left there by
// zgpu_seek_index_hash_device, which decodes and hashes every frame once, or by zgpu_seek_index_set_sums, the caller's promise. They are
// compared on the device with the digests the hash kernel left there: 32 bytes per group come back. The sibling of zg_seeksums.h, whose rule,
// Frame list, record and verdict (zgv::Frame, zgv::Sums, zgv::vouched) it uses unchanged; what differs is where the rows come from — the
// handle, not a table inside the entry: NO BYTE OF THE ENTRY IS READ. One WAVE per group, one launch per submit, on the engine's first stream
// behind the hash kernel. Written against the zx_* primitives behind two reader accessors: tests/test_idxsums_cpu.py runs this source with
// readers that count every access outside the windows below and compares every field with a model in Python (tests/idxsums.py). sums_pairs is
// the same rule in plain C++ over pairs and sums the host holds: the groups that are decoded alone (decode_alone_device).
//
// THE RULE is zg_seeksums.h's, with R_k = C[k] - C[first] and c_k = C[k + 1] - C[k] read straight from the pairs — the pairs ARE the prefix
// sums, the wave computes none — and sums[k] in the Checksum's place. A handle that holds sums always has one per row: kNoChecksums cannot
// arise. A skippable row holds 0 and is never looked at: no decoded zstd frame coincides with it.
//
// Inputs. Per group a Lane: where the entry's pair 0 and sum 0 lie in the handle's arrays, its row count, first, taken, and
// [frame_lo, frame_lo + frame_n), its slice of the submit's frame list (zgv::Frame; zg_seeksums.h says what is in it). The digests:
// Batch::hash_launch's output, 8 bytes per slot, still in device memory.
//
// first + taken > nrows: kRows; a slot at or behind the digest count: kList — a `why`, which the host makes ZGPU_E_INTERNAL with a last_error,
// never a stray access. Any why: every other field of the record is 0. The scan, 64 rows a step from `first`: lane l loads C[first + base + l],
// C[first + base + l + 1] and sums[first + base + l], with the next step's loads issued in front of this step's search; it binary-searches
// its group's slice for a frame that begins at R_k (loads of `begin` only), and at a hit loads the frame, checks the length (a c_k above
// 0xFFFFFFFF, or pairs that decrease, match no frame), loads the digest's low dword and compares. Three ballots and population counts
// accumulate coinciding, compared and differing frames; a find-first-set of the first step that differs gives first_bad, the entry's row
// (kNoRow: none). The record, 32 bytes, leaves lane 0 as two 16-byte stores through zgv::seeksums_store.
//
// What the wave reads: C of rows [first, first + taken] — the closing one included, 8 bytes of each pair, never D —; sums of rows
// [first, first + taken); its own slice of the frame list; the low dwords of the digests that slice names. Nothing of the rows in front or
// behind, nothing of another entry's rows.
//
// gfx950 ISA of zg_k_idxsums (hipcc -O3 --save-temps, the code object's metadata): 24 VGPRs, 54 SGPRs, no scratch (private segment 0), no LDS
// (group segment 0), no spills. The group's 48-byte Lane and the wave-uniform C[first] come in through scalar loads; per step 2 global_load_dwordx2 (C[k], C[k + 1]) and 1
// global_load_dword (sums[k]), the first step's in front of the loop and in the loop the next step's, issued in front of the search; per probe
// of the binary search 1 global_load_dwordx2 (a frame's begin), at the hit 1 global_load_dwordx4 (the Frame) and 1 global_load_dword (the
// digest's low half). No ds_bpermute_b32: there is no prefix sum and no carry. 3 s_bcnt1_i32_b64 and 1 s_ff1_i32_b64 for the counts and
// first_bad. The record leaves lane 0 as 2 global_store_dwordx4. Vector stores both.
//
// Included twice by zg_kernels.hip: through zg_kernels.h for the types, and behind the zx_* primitives (and zg_seeksums.h's wave part) for the
// wave routine.
#ifndef ZG_IDXSUMS_TYPES
#define ZG_IDXSUMS_TYPES
#include <stdint.h>
#include "zg_seeksums.h"

namespace zgh {

constexpr uint32_t kThreads = 64;   // lanes of a workgroup of zg_k_idxsums: one wave, one group

// pair0 / sum0: the index of the entry's pair 0 / sum 0 in the handle's arrays; nrows: the entry's rows (it has nrows + 1 pairs, nrows sums)
struct alignas(16) Lane { uint64_t pair0, sum0; uint32_t nrows, first, taken, frame_lo, frame_n, pad[3]; };
static_assert(sizeof(Lane) == 48, "handle checksum lanes");

// ---- the same rule over pairs and sums the HOST holds (groups decoded alone) ------------------------------------------------------------------
// c[0 .. taken]: C[first] .. C[first + taken]; sums[0 .. taken): the sums of rows [first, first + taken); fr[0 .. nfr): the group's frames;
// dig[0 .. ndig): their digests by slot. first + taken > nrows: nothing is looked at (the caller holds no such rows).
inline zgv::Sums sums_pairs(const uint64_t* c, const uint32_t* sums, uint32_t nrows, uint32_t first, uint32_t taken, const zgv::Frame* fr, uint32_t nfr,
                            const uint64_t* dig, uint32_t ndig) {
  if (!taken) return zgv::Sums{0, 0, 0, 0, 0, 0, 0, 0};
  if ((uint64_t)first + taken > nrows) return zgv::Sums{0, 0, 0, 0, 0, zgv::kRows, 0, 0};
  zgv::Sums o{taken, 0, 0, 0, zgv::kNoRow, 0, 0, 0};
  for (uint32_t k = 0; k < taken; k++) {
    const uint64_t at = c[k] - c[0], len = c[k + 1] - c[k];
    uint32_t lo = 0, hi = nfr;   // (pairs of a stale handle need not increase: every row searches on its own, as the wave's lanes do)
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (fr[mid].begin < at) lo = mid + 1; else hi = mid;
    }
    if (lo == nfr || fr[lo].begin != at || fr[lo].clen != len) continue;
    o.coinciding++;
    if (fr[lo].slot == zgv::kNotHashed) continue;
    if (fr[lo].slot >= ndig) return zgv::Sums{0, 0, 0, 0, 0, zgv::kList, 0, 0};
    o.compared++;
    if ((uint32_t)dig[fr[lo].slot] != sums[k]) { o.differing++; if (o.first_bad == zgv::kNoRow) o.first_bad = first + k; }
  }
  return o;
}

}  // namespace zgh
#endif  // ZG_IDXSUMS_TYPES

#if defined(ZX_DEV) && !defined(ZG_IDXSUMS_WAVE)
#define ZG_IDXSUMS_WAVE
namespace zgh {

// What the wave of one group does; every lane calls it and every lane gets the record. P reads the entry's rows in the handle: c(k) = C[k] for
// k <= nrows, sum(k) for k < nrows. F reads the group's slice of the frame list and the digests, as in zgv::seeksums_entry.
template <class P, class F> ZX_DEV zgv::Sums idxsums_group(const P& p, const F& f, uint32_t nrows, uint32_t first, uint32_t taken, uint32_t nfr, uint32_t ndig) {
  const uint32_t lane = zx_tid() & 63u;
  zgv::Sums o;
  o.rows = o.coinciding = o.compared = o.differing = o.first_bad = o.why = o.flags = o.pad = 0;
  if (!taken) return o;
  if ((uint64_t)first + taken > nrows) { o.why = zgv::kRows; return o; }
  const uint64_t c0 = p.c(first);
  uint64_t ck = 0, cn = 0;
  uint32_t s = 0, coinciding = 0, compared = 0, differing = 0, first_bad = zgv::kNoRow;
  bool bad_list = false;
  if (lane < taken) { ck = p.c((uint64_t)first + lane); cn = p.c((uint64_t)first + lane + 1); s = p.sum((uint64_t)first + lane); }
  for (uint32_t base = 0; base < taken; base += 64) {
    uint64_t nck = 0, ncn = 0;
    uint32_t ns = 0;
    if (base + 64 + lane < taken) {
      const uint64_t k = (uint64_t)first + base + 64 + lane;
      nck = p.c(k); ncn = p.c(k + 1); ns = p.sum(k);
    }
    const uint64_t rk = ck - c0, c = cn - ck;
    bool hit = false, cmp = false, diff = false, oob = false;
    if (base + lane < taken && nfr) {
      uint32_t lo = 0, hi = nfr;             // the first frame that begins at or behind R_k
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (f.begin(mid) < rk) lo = mid + 1; else hi = mid;
      }
      if (lo < nfr) {
        uint64_t fb;
        uint32_t fc, slot;
        f.frame(lo, &fb, &fc, &slot);
        hit = fb == rk && (uint64_t)fc == c;
        if (hit && slot != zgv::kNotHashed) {
          oob = slot >= ndig;
          cmp = !oob;
          if (cmp) diff = f.digest(slot) != s;
        }
      }
    }
    const unsigned long long mh = zx_ballot(hit), mc = zx_ballot(cmp), md = zx_ballot(diff);
    coinciding += (uint32_t)__builtin_popcountll(mh); compared += (uint32_t)__builtin_popcountll(mc); differing += (uint32_t)__builtin_popcountll(md);
    if (md && first_bad == zgv::kNoRow) first_bad = first + base + (uint32_t)__builtin_ctzll(md);
    if (zx_ballot(oob)) bad_list = true;
    ck = nck; cn = ncn; s = ns;
  }
  if (bad_list) o.why = zgv::kList;
  else { o.rows = taken; o.coinciding = coinciding; o.compared = compared; o.differing = differing; o.first_bad = first_bad; }
  return o;
}

}  // namespace zgh
#endif  // ZX_DEV
