// zg_inorder.h — bodies of zg_k_lz, zg_k_sparse and zg_k_partial: the kernels that execute sequences IN ORDER (execute_sequences,
// sequence_execution.rs:5-54; DecodeBuffer::push / repeat, decode_buffer.rs:74-141), one batch of T sequences after the other.
// They share one rule, stated once in zg_retire: the matches of a batch are resolved in rounds, and a match is copied once every
// source byte it needs lies below the high-water mark, the lowest destination a pending match of the batch still has to write.
// What differs stays in the bodies: where positions come from, who checks the offsets, what an exhausted guard leads to.
// Written against the zx_* primitives like zg_exact.h: the same source runs under the CPU emulator (tests/test_inorder_cpu.py).
#pragma once
#include <stdint.h>
#include "zg_types.h"
#include "zg_dev.h"

ZG_HD void zg_lane_match_copy(uint8_t* dst, uint32_t off, uint32_t ml) {
  const uint8_t* src = dst - off;
  uint32_t k = 0;
  if (off >= 8) {
    for (; k + 8 <= ml; k += 8) ((zg_u64u*)(dst + k))->v = zg_ld64(src + k);
  }
  for (; k < ml; k++) dst[k] = src[k];  // also the overlapping case (offset < match length): periodic extension
}

// a lane's literal run: ll bytes at o, from index `at` of the block's literals (RLE literals: one byte, repeated)
ZG_HD void zg_lane_literals(uint8_t* o, const uint8_t* lit, bool lit_rle, uint32_t at, uint32_t ll) {
  if (lit_rle) { const uint8_t v = lit[0]; for (uint32_t k = 0; k < ll; k++) o[k] = v; }
  else { const uint8_t* s = lit + at; for (uint32_t k = 0; k < ll; k++) o[k] = s[k]; }
}

// inclusive scan of v over the caller's wave
ZX_DEV uint32_t zg_wave_scan(uint32_t v) {
  const uint32_t lane = zx_tid() & 63u;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = zx_shfl_up(v, o); if ((int)lane >= o) v += u; }
  return v;
}

// The rounds of one batch of T sequences, one per thread: `pending` is set for a thread that has a match of ml bytes to copy to
// frame_out + dpos from `off` bytes back; mdst is dpos relative to the block, which starts at out_base. Returns whether every match
// retired (every round retires the first pending match at least, so T rounds suffice; an exhausted guard is the caller's to report).
// T == 64: the batch is a wave, and a block-scope fence makes a round's copies visible to the lanes that copy from them next.
// T > 64: the per-wave minimum goes through wmin[T / 64] in LDS, and the workgroup barriers around it also make the copies visible
// to the other waves of the workgroup (same CU, shared L1).
template <int T>
ZX_DEV bool zg_retire(bool pending, const uint32_t mdst, const uint64_t dpos, const uint32_t off, const uint32_t ml, uint8_t* frame_out,
                      const uint64_t out_base, uint32_t* wmin) {
  const uint32_t t = zx_tid(), lane = t & 63u, wv = t >> 6;
  for (uint32_t guard = 0; guard <= (uint32_t)T; guard++) {
    uint32_t hwm = pending ? mdst : 0xFFFFFFFFu;              // the lowest destination a pending match of the batch still has to write
    for (int sh = 32; sh >= 1; sh >>= 1) { const uint32_t o = zx_shfl_xor(hwm, sh); hwm = o < hwm ? o : hwm; }
    if (T > 64) {
      if (lane == 0) wmin[wv] = hwm;
      zx_syncthreads();
      hwm = wmin[0];
      for (int w = 1; w < T / 64; w++) hwm = wmin[w] < hwm ? wmin[w] : hwm;
    }
    if (hwm == 0xFFFFFFFFu) return true;
    if (pending) {
      // source bytes that must already exist: [dpos - off, min(dpos - off + ml, dpos)). What lies in front of the frame (dictionary,
      // earlier submits) exists: src_end <= 0 needs nothing.
      const int64_t src_end = (int64_t)dpos - (int64_t)off + (int64_t)ml;
      const uint64_t need_end = ml < off ? (src_end > 0 ? (uint64_t)src_end : 0ull) : dpos;
      if (need_end <= out_base + hwm) { zg_lane_match_copy(frame_out + dpos, off, ml); pending = false; }
    }
    if (T > 64) zx_syncthreads(); else zx_fence_block();
  }
  return false;
}

template <int T>
struct ZgLzLds { uint32_t wmin[T / 64], so[T / 64], sl[T / 64], err, errblk; };   // zg_retire's minima; per wave: ll + ml and ll of the batch; the verdict

// zg_k_lz: a frame that left the flatten path (a block regenerating more than 128 KiB: not conforming), one workgroup. Positions are
// rebuilt from the exact fields of the records (ml, ll): a batch is scanned, every thread places its literal run and checks its offset.
template <int T>
ZX_DEV void zg_lz_frame(const ZgBatchDev& d, const uint32_t f, ZgLzLds<T>& L) {
  if (d.totals[2]) return;
  const uint32_t t = zx_tid(), lane = t & 63u, wv = t >> 6;
  const ZgFrame fr = d.frames[f];
  const ZgFrameOut fo = d.frame_out[f];
  if (fo.fast) return;
  uint8_t* frame_out = d.dst + fo.out_base;
  if (t == 0) { L.err = 0; L.errblk = 0; }
  zx_syncthreads();
  for (uint32_t bi = 0; bi < fo.good_blocks; bi++) {
    const uint32_t b = fr.first_block + bi;
    const ZgBlock* blk = &d.blocks[b];
    if (blk->btype != ZG_BT_COMPRESSED || blk->nseq == 0) continue;
    const uint32_t nseq = blk->nseq;
    const ZgBlockPos p = d.pos[b];
    const ZgBlockSeqOut so = d.seq_out[b];
    const ZgSeq* sq = d.seq_arena + blk->seq_base;
    const uint8_t* body = d.src + blk->src_off;
    const bool lit_rle = blk->lit_type == ZG_LT_RLE;
    const uint8_t* lit = blk->lit_type <= ZG_LT_RLE ? body + blk->lit_off : d.lit_arena + blk->lit_base;
    uint32_t carry_out = 0, carry_lit = 0;      // block-relative output position / literal index before the batch
    for (uint32_t s0 = 0; s0 < nseq; s0 += T) {
      const uint32_t i = s0 + t;
      bool pending = false;
      uint32_t off = 0, ml = 0, ll = 0, mdst = 0xFFFFFFFFu;
      if (i < nseq) {
        const ZgSeq q = sq[i];
        const uint32_t nx = i + 1 < nseq ? ZG_SEQ_LIT(sq[i + 1]) : so.sum_ll;
        ml = ZG_SEQ_ML(q); ll = (nx - ZG_SEQ_LIT(q)) & 0x1FFFFu;
        off = zg_sym_resolve(q.of, p.hist_init);
      }
      // exclusive scans of ll + ml and ll over the batch
      const uint32_t io = zg_wave_scan(ll + ml), il = zg_wave_scan(ll);
      if (lane == 63) { L.so[wv] = io; L.sl[wv] = il; }
      zx_syncthreads();
      uint32_t bo = carry_out, bl = carry_lit, to = carry_out, tl = carry_lit;
      for (uint32_t w = 0; w < (uint32_t)T / 64u; w++) { if (w < wv) { bo += L.so[w]; bl += L.sl[w]; } to += L.so[w]; tl += L.sl[w]; }
      uint64_t dpos = 0;  // frame-relative position of the match destination
      if (i < nseq) {
        mdst = bo + io - ml;
        dpos = p.out_base + mdst;
        zg_lane_literals(frame_out + dpos - ll, lit, lit_rle, bl + il - ll, ll);
        if (off == 0) zx_cas_lds(&L.err, 0u, (uint32_t)ZG_EXE_ZERO_OFFSET);
        else if ((uint64_t)off > dpos + fr.prior_reach + fr.dict_len || off >= ZG_OFF_HUGE - 2u) zx_cas_lds(&L.err, 0u, (uint32_t)(dpos + fr.prior_out <= fr.window_size ? ZG_EXE_DICT_TOO_SMALL : ZG_EXE_OFFSET_TOO_BIG));
        else pending = ml > 0;
      }
      carry_out = to; carry_lit = tl;
      zx_syncthreads();
      if (L.err) break;
      if (!zg_retire<T>(pending, mdst, dpos, off, ml, frame_out, p.out_base, L.wmin) && t == 0) L.err = ZG_INTERNAL;
      zx_syncthreads();
    }
    if (L.err) { if (t == 0) L.errblk = bi; break; }
    // trailing literals (sequence_execution.rs:40-44)
    const uint32_t rest = blk->regen_size - so.sum_ll;
    uint8_t* o = frame_out + p.out_base + ((uint64_t)so.sum_ll + so.sum_ml);
    if (lit_rle) zg_wg_fill(o, lit[0], rest, t, T);
    else zg_wg_copy(o, lit + so.sum_ll, rest, t, T);
    zx_syncthreads();
  }
  zx_syncthreads();
  if (t == 0 && L.err) {
    d.frame_out[f].status = L.err;
    d.frame_out[f].bad_block = L.errblk;
    d.frame_out[f].good_blocks = L.errblk;
  }
}

// zg_k_sparse: the matches of a frame that has hardly any (literal-heavy data: a sequence or two in one block out of twenty), one wave.
// zg_k_flatten has placed the literals and checked the offsets; what is left is a few hundred short copies, done in order (a match may
// copy from an earlier one) in the time of a few sweep launches — of which the frame would need one per unit.
ZX_DEV void zg_sparse_frame(const ZgBatchDev& d, const uint32_t f) {
  if (d.totals[2]) return;
  const uint32_t lane = zx_tid();
  const ZgFrame fr = d.frames[f];
  if (!fr.sparse) return;
  const ZgFrameOut fo = d.frame_out[f];
  if (!fo.fast) return;                                        // the in-order path has it
  const uint32_t stop = fo.err_packed == 0xFFFFFFFFu ? 0xFFFFFFFFu : fo.err_packed >> 8;   // zg_k_flatten found a sequence that cannot be executed: only the blocks in front of its block are executed
  uint8_t* frame_out = d.dst + fo.out_base;
  for (uint32_t e = 0; e < fr.seq_count; e++) {
    const uint32_t b = d.seq_blocks[fr.seq_first + e];
    const ZgBlockPos p = d.pos[b];
    if (!p.active || b - fr.first_block >= stop) break;
    const ZgBlock* blk = &d.blocks[b];
    const uint32_t nseq = blk->nseq;
    const ZgSeq* sq = d.seq_arena + blk->seq_base;
    for (uint32_t s0 = 0; s0 < nseq; s0 += 64) {
      const uint32_t i = s0 + lane;
      bool pending = false;
      uint32_t off = 0, ml = 0, mdst = 0xFFFFFFFFu;
      uint64_t dpos = 0;
      if (i < nseq) {
        const ZgSeq q = sq[i];
        ml = ZG_SEQ_ML(q); mdst = ZG_SEQ_MDST(q);
        off = zg_sym_resolve(q.of, p.hist_init);
        dpos = p.out_base + mdst;
        pending = ml > 0;
      }
      if (!zg_retire<64>(pending, mdst, dpos, off, ml, frame_out, p.out_base, nullptr)) { if (lane == 0) d.frame_out[f].status = ZG_INTERNAL; return; }
    }
  }
}

// zg_k_partial: what the reference's decode buffer holds of a block whose sequence EXECUTION failed, one wave. execute_sequences pushes a
// sequence's literals, then its match, and returns at the first sequence it cannot execute: what the ones in front of it wrote stays in
// the buffer (and that sequence's literals, unless it was the literals that ran out), where collect() / read() still find it after the
// Err. The fast path produces a block as a whole or not at all; for the ONE block that failed, of a frame decoded run by run, Batch::sync()
// runs this: sequences [0, nexec) of block b behind the bytes of the good blocks, plus the literals of sequence nexec when lits_of_next.
ZX_DEV void zg_partial_block(const ZgBatchDev& d, const uint32_t f, const uint32_t b, const uint32_t nexec, const uint32_t lits_of_next, const uint32_t limit) {
  const uint32_t lane = zx_tid();
  const ZgFrameOut fo = d.frame_out[f];
  const ZgBlockPos p = d.pos[b];
  const ZgBlock* blk = &d.blocks[b];
  uint8_t* frame_out = d.dst + fo.out_base;
  const ZgSeq* sq = d.seq_arena + blk->seq_base;
  const uint8_t* body = d.src + blk->src_off;
  const bool lit_rle = blk->lit_type == ZG_LT_RLE;
  const uint8_t* lit = blk->lit_type <= ZG_LT_RLE ? body + blk->lit_off : d.lit_arena + blk->lit_base;
  const uint32_t total = nexec + (lits_of_next ? 1u : 0u);          // sequences whose literals go out
  // Positions are rebuilt from the exact fields of the records, as in zg_lz_frame (a block beyond 128 KiB wraps the position fields): the
  // literal run of sequence i is what lies between the end of sequence i - 1 and its match, (mdst_i - mdst_(i-1) - ml_(i-1)) mod 2^17.
  // pass 0 only measures (the host has reserved `limit` bytes behind the run: more than that is not written at all), pass 1 executes.
  for (int pass = 0; pass < 2; pass++) {
    uint32_t carry = 0;                                              // block-relative end of the sequences in front of the batch
    for (uint32_t s0 = 0; s0 < total; s0 += 64) {
      const uint32_t i = s0 + lane;
      uint32_t off = 0, ml = 0, ll = 0, lp = 0;
      if (i < total) {
        const ZgSeq q = sq[i];
        uint32_t prev_end = 0;
        if (i) { const ZgSeq pq = sq[i - 1]; prev_end = ZG_SEQ_MDST(pq) + ZG_SEQ_ML(pq); }
        ll = (ZG_SEQ_MDST(q) - prev_end) & 0x1FFFFu;
        lp = ZG_SEQ_LIT(q);
        if (i < nexec) { ml = ZG_SEQ_ML(q); off = zg_sym_resolve(q.of, p.hist_init); }
      }
      const uint32_t io = zg_wave_scan(ll + ml);
      const uint32_t mdst = carry + io - ml;                         // where this sequence's match starts; its literals lie in front of it
      carry += zx_shfl(io, 63);
      if (pass == 0) continue;
      const uint64_t dpos = p.out_base + mdst;
      if (i < total) zg_lane_literals(frame_out + dpos - ll, lit, lit_rle, lp, ll);
      zx_fence_block();                                              // the literals are in place for the matches that copy from them
      (void)zg_retire<64>(i < nexec && ml > 0, mdst, dpos, off, ml, frame_out, p.out_base, nullptr);   // (an exhausted guard: the batch ends there)
    }
    if (pass == 0) {
      if (lane == 0) d.totals[5] = carry <= limit ? carry : 0xFFFFFFFFu;   // what the block leaves behind; 0xFFFFFFFF: more than was reserved, nothing written
      if (carry > limit) return;
    }
  }
}
