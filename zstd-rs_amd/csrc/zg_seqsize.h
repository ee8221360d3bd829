// zg_seqsize.h — body of zg_k_seqsize: what a block's sequences ADD UP TO, and nothing else of them. Batch::measure (zg_engine.h) runs it in
// place of zg_k_seqpost where only the sizes of frames are wanted (zgpu_seek_index_measure_device): a block's output is Regenerated_Size
// of its literals plus the sum of its match lengths, and both sums need the codes of every sequence and the LL and ML extra-bit fields —
// no offset, no offset history, no position per sequence, no 12-byte record.
//
// One 256-thread workgroup per block of d.seq_blocks, ZG_SZ_S consecutive sequences per thread, like zg_k_seqpost; a block whose status is
// set is left alone. The block's three tables are staged in LDS in zg_k_seqpost's 16-bit form (symbol << 4 | state bits). A thread reads
// the 4-byte state records zg_k_seq left (ZG_RAW_LL / ML / OF), takes each sequence's bit count from the codes — the three extra-bit
// fields and, except on the block's last sequence, the three state updates —, and the counts become bit positions by zx_scan_incl_add and
// one cross-wave step, counted down from d.seq_out[b].pad exactly as zg_k_seqpost derives P[j]. The LL and ML fields of a sequence are
// adjacent, [q_ll, q_ll + xb_ll + xb_ml), at most 32 bits; they are read with zg_k_seqpost's load: three dwords from the dword-aligned address
// of the byte that holds bit q_ll, funnel-shifted. The load goes through a buffer resource over the dwords that hold the block's bitstream,
// so the kernel touches no byte zg_k_seqpost would not, whatever the records say. Σ ll and Σ ml are reduced over the block, pass by pass.
//
// Verdicts: those the sums decide. Literal lengths are non-negative, so a prefix of them exceeds a bound exactly when the total does:
//   ZG_EXE_NOT_ENOUGH_LITERALS  Σ ll > regen_size                  (sequence_execution.rs:14-19)
//   ZG_UNSUPPORTED              regen_size + Σ ml >= 2^31          (zg_k_seqpost's limit on a block's output)
// checked after every pass of 256 * ZG_SZ_S sequences (a pass adds less than 2^29 to either sum: no 32-bit sum wraps before it is checked),
// NOT_ENOUGH_LITERALS first. ZG_EXE_ZERO_OFFSET needs the offset history and is not seen here. Thread 0 leaves
// ZgBlockSeqOut{sum_ll, sum_ml, hist_end = the identity map's three tags, pad = 0}: zg_k_scan reads sum_ml and composes identities.
//
// Written against the zx_* primitives (zg_kernels.hip: gfx950 builtins; tests/emu/zg_emu_seqsize.cpp: the CPU emulator, with a bitstream
// reader that counts every dword it is asked for): tests/test_seqsize_cpu.py runs this source against the oracle's sequences.
//
// gfx950 ISA of zg_k_seqsize (hipcc -O3 --save-temps, wave64; .vgpr_count, .sgpr_count, .group_segment_fixed_size of the code object's
// metadata), by sequences per thread, with __launch_bounds__(256):
//   ZG_SZ_S = 4    53 VGPRs, 54 SGPRs     8 waves per SIMD
//   ZG_SZ_S = 8    80 VGPRs, 67 SGPRs     6 waves per SIMD: six workgroups per CU                        <- chosen
//   ZG_SZ_S = 16  143 VGPRs, 91 SGPRs     3 waves per SIMD
// each with 2964 bytes of LDS, .private_segment_fixed_size 0 and .vgpr_spill_count 0: no scratch, no spills. LDS never bounds occupancy
// (55 workgroups' worth per CU); the registers do. Eight sequences per thread are two 16-byte loads of records per thread and pass, one scan
// of bit counts per 512 sequences and two barriers per 2048 — half of what four cost per sequence — and eight independent chains of LDS
// lookups per thread, at 24 waves per CU. Forcing eight waves per SIMD on them (__launch_bounds__(256, 8): 64 VGPRs) spills 15 VGPRs to
// 40 bytes of scratch, so the kernel carries no second argument. Measured (LABNOTES.md "seek_index_measured"): 4 and 8 are equal within the
// spread of a measuring submit, of which this kernel is 4 to 6 % behind zg_k_seq; 8 is zg_k_seqpost's shape, and its seam tests serve both.
#pragma once
#include <stdint.h>
#include "zg_types.h"
#include "zg_dev.h"

#define ZG_SZ_T 256         // threads of a workgroup
#ifndef ZG_SZ_S
#define ZG_SZ_S 8           // consecutive sequences per thread and pass (a multiple of 4: records are read 16 bytes at a time)
#endif
// the dwords of a block's bitstream; ZG_SZ_LD96: how three of them are read (the CPU harness counts the reads)
#ifndef ZG_SZ_LD96
#define ZG_SZ_LD96(buf, off) zx_ld96(buf, off)
#endif

struct ZgSeqSizeLds {
  uint32_t wx[ZG_SZ_T / 64], wl[ZG_SZ_T / 64], wm[ZG_SZ_T / 64];   // per wave: bits, Σ ll, Σ ml of the pass
  uint32_t llb[36], mlb[53];                                       // base | extra bits << 24
  uint16_t t[ZG_FSE_SLOT_U32];                                     // per state: symbol << 4 | state bits
};

ZX_DEV void zg_seqsize_block(const ZgBatchDev& d, const uint32_t b, ZgSeqSizeLds& L) {
  const uint32_t t = zx_tid(), lane = t & 63u, wv = t >> 6;
  if (d.status[b]) return;                         // the bitstream (or a table) failed: nothing to add up
  const ZgBlock blk = d.blocks[b];
  {
    const int32_t sl[3] = {blk.ll_slot, blk.ml_slot, blk.of_slot};          // in the order of the slot layout (LL, ML, OF)
    const uint32_t offs[4] = {ZG_FSE_LL_OFF, ZG_FSE_ML_OFF, ZG_FSE_OF_OFF, ZG_FSE_SLOT_U32};
    for (int k = 0; k < 3; k++) {
      const uint32_t* g_t = d.fse_arena + (uint64_t)sl[k] * ZG_FSE_SLOT_U32;   // (the block passed zg_k_seq: all three slots are set)
      for (uint32_t i = offs[k] + t; i < offs[k + 1]; i += ZG_SZ_T) { const uint32_t v = g_t[i]; L.t[i] = (uint16_t)((ZG_FSE_SYM(v) << 4) | ZG_FSE_NB(v)); }
    }
  }
  if (t < 36) L.llb[t] = ZG_LL_BASE[t] | ((uint32_t)ZG_LL_BITS[t] << 24);
  if (t < 53) L.mlb[t] = ZG_ML_BASE[t] | ((uint32_t)ZG_ML_BITS[t] << 24);
  const uint32_t nseq = blk.nseq, regen = blk.regen_size;
  // the bitstream: [bs, bs + nbytes) of the submit's input, seen through the dwords that hold it (the first one begins up to 3 bytes in front)
  const uint32_t bits_off = d.aux[b].seq_bits_off;
  const uint8_t* bs = d.src + blk.src_off + bits_off;
  const uint32_t nbytes = blk.src_len > bits_off ? blk.src_len - bits_off : 0u;
  const uint32_t lead = (uint32_t)((uint64_t)bs & 3ull);
  const ZxBuf stream = zx_buf(bs - lead, (lead + nbytes + 3u) & ~3u);
  const ZxBuf raw = zx_buf(d.raw_arena + blk.seq_base, nseq * 4u);   // a record behind the last one reads as 0
  uint32_t pos_carry = d.seq_out[b].pad;           // bit position where the next pass's first sequence starts (left by zg_k_seq)
  uint32_t sum_ll = 0, sum_ml = 0, verdict = ZG_OK;
  zx_syncthreads();
  for (uint32_t i0 = 0; i0 < nseq; i0 += ZG_SZ_T * ZG_SZ_S) {
    const uint32_t ib = i0 + t * ZG_SZ_S;
    const uint32_t n = ib < nseq ? (nseq - ib < ZG_SZ_S ? nseq - ib : ZG_SZ_S) : 0u;
    uint32_t r[ZG_SZ_S];
#pragma unroll
    for (int j = 0; j < ZG_SZ_S; j += 4) {
      const ZxU4 v = zx_ld128(raw, (ib + (uint32_t)j) * 4u);
      r[j] = v.x; r[j + 1] = v.y; r[j + 2] = v.z; r[j + 3] = v.w;
    }
    // codes and bit counts from the recorded states: a sequence takes its three codes' extra bits and, unless it is the block's last
    // one, the three state updates. top[j]: bits between the thread's first sequence and the upper end of sequence j's ML field
    uint32_t vl[ZG_SZ_S], vm[ZG_SZ_S], top[ZG_SZ_S], tx = 0;
#pragma unroll
    for (int j = 0; j < ZG_SZ_S; j++) {
      const uint32_t e_of = L.t[ZG_FSE_OF_OFF + ZG_RAW_OF(r[j])], e_ml = L.t[ZG_FSE_ML_OFF + ZG_RAW_ML(r[j])], e_ll = L.t[ZG_FSE_LL_OFF + ZG_RAW_LL(r[j])];
      const uint32_t of_code = (e_of >> 4) & 31u, ml_code = e_ml >> 4, ll_code = e_ll >> 4;
      const bool have = (uint32_t)j < n;               // (a slot past the end takes no bits: its read below stays at the last position)
      vl[j] = have ? L.llb[ll_code < 36 ? ll_code : 0] : 0u;
      vm[j] = have ? L.mlb[ml_code < 53 ? ml_code : 0] : 0u;
      const uint32_t upd = ib + (uint32_t)j + 1u == nseq ? 0u : (e_of & 15u) + (e_ml & 15u) + (e_ll & 15u);
      top[j] = tx + (have ? of_code : 0u);
      tx += have ? of_code + (vl[j] >> 24) + (vm[j] >> 24) + upd : 0u;
    }
    const uint32_t sx = zx_scan_incl_add(tx);
    if (lane == 63) L.wx[wv] = sx;
    zx_syncthreads();
    uint32_t before = sx - tx, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < ZG_SZ_T / 64; w++) { const uint32_t wx = L.wx[w]; if (w < wv) before += wx; all += wx; }
    const uint32_t p0 = pos_carry - before;            // where the thread's first sequence starts
    pos_carry -= all;
    // values: the LL field is bits [q_ll, q_ll + xb_ll), the ML field lies on top of it
    uint32_t tl = 0, tm = 0;
#pragma unroll
    for (int j = 0; j < ZG_SZ_S; j++) {
      const uint32_t xb_ll = vl[j] >> 24, xb_ml = vm[j] >> 24;
      const uint32_t q_ll = p0 - top[j] - xb_ml - xb_ll;                  // >= 0 for every record zg_k_seq emitted
      const uint32_t at = lead + (q_ll >> 3);
      const ZxU3 w3 = ZG_SZ_LD96(stream, at & ~3u);                       // dword-aligned, as zg_k_seqpost loads it
      const uint32_t sh = (at & 3u) * 8u + (q_ll & 7u);                   // <= 31
      const uint32_t lo = zx_alignbit(w3.y, w3.x, sh), hi = zx_alignbit(w3.z, w3.y, sh);
      const uint32_t ll_add = lo & ((1u << xb_ll) - 1u);                  // xb_ll, xb_ml <= 16
      const uint32_t ml_add = zx_alignbit(hi, lo, xb_ll) & ((1u << xb_ml) - 1u);
      tl += (vl[j] & 0xFFFFFFu) + ll_add;                                 // (no sequence: base 0 and no bits)
      tm += (vm[j] & 0xFFFFFFu) + ml_add;
    }
    const uint32_t sl = zx_scan_incl_add(tl), sm = zx_scan_incl_add(tm);
    if (lane == 63) { L.wl[wv] = sl; L.wm[wv] = sm; }
    zx_syncthreads();
#pragma unroll
    for (uint32_t w = 0; w < ZG_SZ_T / 64; w++) { sum_ll += L.wl[w]; sum_ml += L.wm[w]; }
    if (sum_ll > regen) verdict = ZG_EXE_NOT_ENOUGH_LITERALS;
    else if ((uint64_t)regen + sum_ml >= (1ull << 31)) verdict = ZG_UNSUPPORTED;
    if (verdict) break;                                // (every thread holds the same sums)
  }
  if (t == 0) {
    ZgBlockSeqOut so;
    so.sum_ll = sum_ll; so.sum_ml = sum_ml;
    const ZgHistMap id = zg_map_identity();
    so.hist_end[0] = id.s[0]; so.hist_end[1] = id.s[1]; so.hist_end[2] = id.s[2];
    so.pad = 0;
    d.seq_out[b] = so;
    if (verdict) d.status[b] = verdict;   // (it was 0 above, and nobody else writes it while this kernel runs)
  }
}
