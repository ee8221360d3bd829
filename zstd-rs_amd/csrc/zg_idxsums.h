// zg_idxsums.h — zg_k_idxsums: does a seek index HANDLE vouch for the frames that were decoded of one of its entries (ZGPU_DEVICE_VERIFY_SEEK_TABLE
// of zgpu_gather_ranges_indexed_device_src, for an entry whose handle holds sums)? The handle keeps, beside the pairs { C[k], D[k] } of every
// row, one uint32_t per row in device memory: the low 32 bits of XXH64 (seed 0) of that row's plaintext — left there by
// zgpu_seek_index_hash_device, which decodes and hashes every frame once, or by zgpu_seek_index_set_sums, the caller's promise. They are
// compared on the device with the digests the hash kernel left there: 32 bytes per group come back. The sibling of zg_seeksums.h, whose rule,
// Frame list, record and verdict (zgv::Frame, zgv::Sums, zgv::vouched) it uses unchanged; what differs is where the rows come from — the
// handle, not a table inside the entry: NO BYTE OF THE ENTRY IS READ. One WAVE per group, one launch per submit, on the engine's first stream
// behind the hash kernel. Written against the zx_* primitives behind two reader accessors: tests/test_idxsums_cpu.py runs this source with
// readers that count every access outside the windows below and compares every field with a model in Python (tests/idxsums.py). sums_pairs hands
// the pairs and sums the host holds to the host form of the rule (zgv::sums_host): the groups that are decoded alone (decode_alone_device).
//
// THE RULE is zg_seeksums.h's, in its code (zgv::sums_step, zgv::Tally, zgv::sums_host), with R_k = C[k] - C[first] and c_k = C[k + 1] - C[k]
// read straight from the pairs — the pairs ARE the prefix sums, the wave computes none — and sums[k] in the Checksum's place. A handle that
// holds sums always has one per row: kNoChecksums cannot arise. A skippable row holds 0 and is never looked at: no decoded zstd frame
// coincides with it.
//
// Inputs. Per group a Lane: where the entry's pair 0 and sum 0 lie in the handle's arrays, its row count, first, taken, and
// [frame_lo, frame_lo + frame_n), its slice of the submit's frame list (zgv::Frame; zg_seeksums.h says what is in it). The digests:
// Batch::hash_launch's output, 8 bytes per slot, still in device memory.
//
// first + taken > nrows: kRows; a slot at or behind the digest count: kList — a `why`, which the host makes ZGPU_E_INTERNAL with a last_error,
// never a stray access. Any why: every other field of the record is 0. The scan, 64 rows a step from `first`: lane l loads C[first + base + l],
// C[first + base + l + 1] and sums[first + base + l], with the next step's loads issued in front of this step's search; the row's step and the
// wave's tally are zg_seeksums.h's (zgv::sums_step, zgv::Tally: pairs that decrease give a c_k above 0xFFFFFFFF, which matches no frame). The
// record, 32 bytes, leaves lane 0 as two 16-byte stores through zgv::seeksums_store.
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
  return zgv::sums_host([&](uint32_t k, uint64_t* at, uint64_t* len, uint32_t* sum) { *at = c[k] - c[0]; *len = c[k + 1] - c[k]; *sum = sums[k]; },
                        true, first, taken, fr, nfr, dig, ndig);
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
  zgv::Sums o = zgv::sums_zero();
  if (!taken) return o;
  if ((uint64_t)first + taken > nrows) { o.why = zgv::kRows; return o; }
  const uint64_t c0 = p.c(first);
  uint64_t ck = 0, cn = 0;
  uint32_t s = 0;
  zgv::Tally t;
  if (lane < taken) { ck = p.c((uint64_t)first + lane); cn = p.c((uint64_t)first + lane + 1); s = p.sum((uint64_t)first + lane); }
  for (uint32_t base = 0; base < taken; base += 64) {
    uint64_t nck = 0, ncn = 0;
    uint32_t ns = 0;
    if (base + 64 + lane < taken) {
      const uint64_t k = (uint64_t)first + base + 64 + lane;
      nck = p.c(k); ncn = p.c(k + 1); ns = p.sum(k);
    }
    bool hit, cmp, diff, oob;
    zgv::sums_step(f, ck - c0, cn - ck, s, base + lane < taken, true, nfr, ndig, hit, cmp, diff, oob);
    zgv::tally_add(t, hit, cmp, diff, oob, first + base);
    ck = nck; cn = ncn; s = ns;
  }
  zgv::tally_record(t, taken, 0, o);
  return o;
}

}  // namespace zgh
#endif  // ZX_DEV
