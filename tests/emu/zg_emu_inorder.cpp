// zg_emu_inorder.cpp — TEST-ONLY: runs the SOURCE of the in-order kernels (zstd-rs_amd/csrc/zg_inorder.h: zg_k_lz, zg_k_sparse,
// zg_k_partial and the retire routine they share) on the CPU through the SIMT emulator of zg_simt.h, on the intermediates the
// harness of zg_emu.cpp produced for a submit. tests/test_inorder_cpu.py compares the bytes and verdicts with the generators'
// plaintext and the oracle; the serial k_exec of zg_emu.cpp stays the model these bodies are compared against.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "../../zstd-rs_amd/csrc/zg_inorder.h"
#include "zg_emu_batch.h"

namespace {

// the device-side view of an EmuBatch after zgemu_decode*, as the engine lays it out: front pads, an output buffer of its own
// (0xAA where nothing was written), every frame as the scan left it — the serial model's execution verdicts taken back
struct Dev {
  std::vector<uint8_t> dst, lit;
  std::vector<ZgSeq> seqs;
  std::vector<ZgFrameOut> fout;
  uint32_t totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t total = 0;
  ZgBatchDev d;
  Dev(EmuBatch* e, uint64_t room_behind) {
    const zg::BatchBuilder& bb = e->bb;
    const uint32_t nb = (uint32_t)bb.blocks.size(), nf = (uint32_t)bb.frames.size();
    for (uint32_t f = 0; f < nf; f++) total = e->fout[f].out_base + e->fout[f].out_size > total ? e->fout[f].out_base + e->fout[f].out_size : total;
    dst.assign(256 + total + room_behind + 64, emufill::byte(0xAA));
    lit.assign(64 + e->lit.size() + 64, emufill::byte(0));
    memcpy(lit.data() + 64, e->lit.data(), e->lit.size());
    seqs.resize(e->seq.size() + 2);
    emufill::records(seqs);
    for (size_t i = 0; i < e->seq.size(); i++) {
      const EmuSeq& q = e->seq[i];
      seqs[i].of = q.of; seqs[i].w1 = ZG_SEQ_W1(q.mdst, q.ml); seqs[i].w2 = ZG_SEQ_W2(q.lit_start, q.ml);
    }
    fout.assign(e->fout.begin(), e->fout.begin() + nf);
    for (uint32_t f = 0; f < nf; f++) {
      const ZgFrame& fr = bb.frames[f];
      uint32_t good = 0;     // blocks the entropy stages (and the parser) accepted
      while (good < fr.nblocks && !bb.blocks[fr.first_block + good].host_status && !e->status[fr.first_block + good]) good++;
      ZgFrameOut& fo = fout[f];
      fo.good_blocks = fo.bad_block = good;
      fo.status = good < fr.nblocks ? (bb.blocks[fr.first_block + good].host_status ? bb.blocks[fr.first_block + good].host_status : e->status[fr.first_block + good]) : 0u;
      fo.fast = 1; fo.err_packed = 0xFFFFFFFFu;
    }
    memset(&d, 0, sizeof d);
    d.src = e->src; d.blocks = bb.blocks.data(); d.nblocks = nb; d.frames = bb.frames.data(); d.nframes = nf;
    d.lit_arena = lit.data() + 64; d.seq_arena = seqs.data(); d.seq_out = e->seqout.data(); d.pos = e->pos.data();
    d.frame_out = fout.data(); d.dst = dst.data() + 256; d.dst_cap = total; d.totals = totals;
    d.seq_blocks = bb.seq_blocks.data(); d.nseq_blocks = (uint32_t)bb.seq_blocks.size();
  }
};

// zg_k_lit on one block, by one thread: raw and RLE blocks and blocks without sequences
void lit_block(const ZgBatchDev& d, uint32_t b) {
  const ZgBlock& blk = d.blocks[b];
  if (!d.pos[b].active) return;
  uint8_t* out = d.dst + d.frame_out[blk.frame].out_base + d.pos[b].out_base;
  const uint8_t* body = d.src + blk.src_off;
  if (blk.btype == ZG_BT_RAW) zg_wg_copy(out, body, blk.regen_size, 0, 1);
  else if (blk.btype == ZG_BT_RLE) zg_wg_fill(out, body[0], blk.regen_size, 0, 1);
  else if (blk.nseq) return;
  else if (blk.lit_type == ZG_LT_RLE) zg_wg_fill(out, body[blk.lit_off], blk.regen_size, 0, 1);
  else zg_wg_copy(out, blk.lit_type == ZG_LT_RAW ? body + blk.lit_off : d.lit_arena + blk.lit_base, blk.regen_size, 0, 1);
}

}  // namespace

extern "C" {

// h: an EmuBatch after zgemu_decode*. Every frame is treated as having left the flatten path (fast = 0), as ZGPU_FORCE_INORDER does:
// zg_k_lit's blocks are put in place, then zg_lz_frame<256> runs on every frame. dst_out: [total output bytes] (0xAA: never
// written); per frame status_out and bad_out (frame-relative block) as the kernel leaves them in the frame's record.
int zgemu_inorder_lz(void* h, uint8_t* dst_out, uint32_t* status_out, uint32_t* bad_out) {
  EmuBatch* e = (EmuBatch*)h;
  Dev v(e, 0);
  for (ZgFrameOut& fo : v.fout) fo.fast = 0;
  for (uint32_t b = 0; b < v.d.nblocks; b++) lit_block(v.d, b);
  for (uint32_t f = 0; f < v.d.nframes; f++) {
    static ZgLzLds<256> L;
    simt::run(256, [&]() { zg_lz_frame<256>(v.d, f, L); });
    status_out[f] = v.fout[f].status; bad_out[f] = v.fout[f].bad_block;
  }
  memcpy(dst_out, v.dst.data() + 256, v.total);
  return 0;
}

// zg_sparse_frame on every frame the plan marks sparse: zg_k_lit's blocks and the literal runs of the other blocks are put in place
// first (on the GPU: zg_flat1_unit), the matches are the body's. Returns the number of sparse frames.
int zgemu_inorder_sparse(void* h, uint8_t* dst_out) {
  EmuBatch* e = (EmuBatch*)h;
  Dev v(e, 0);
  const ZgBatchDev& d = v.d;
  int nsparse = 0;
  for (uint32_t f = 0; f < d.nframes; f++) {
    nsparse += d.frames[f].sparse ? 1 : 0;
    // zg_k_flatten checks the offsets on the GPU; here the serial model has: its verdict stops the body in front of that block
    const ZgFrameOut& sf = e->fout[f];
    if (sf.status >= (uint32_t)ZG_EXE_NOT_ENOUGH_LITERALS && sf.status <= (uint32_t)ZG_EXE_DICT_TOO_SMALL) v.fout[f].err_packed = (sf.bad_block << 8) | sf.status;
  }
  for (uint32_t b = 0; b < d.nblocks; b++) {
    const ZgBlock& blk = d.blocks[b];
    lit_block(d, b);
    if (!d.pos[b].active || blk.btype != ZG_BT_COMPRESSED || !blk.nseq) continue;
    uint8_t* out = d.dst + d.frame_out[blk.frame].out_base + d.pos[b].out_base;
    const uint8_t* lit = blk.lit_type <= ZG_LT_RLE ? d.src + blk.src_off + blk.lit_off : d.lit_arena + blk.lit_base;
    const bool rle = blk.lit_type == ZG_LT_RLE;
    const EmuSeq* sq = e->seq.data() + blk.seq_base;
    const uint32_t sum_ll = e->seqout[b].sum_ll, sum_ml = e->seqout[b].sum_ml;
    for (uint32_t i = 0; i < blk.nseq; i++) {
      const uint32_t ll = (i + 1 < blk.nseq ? sq[i + 1].lit_start : sum_ll) - sq[i].lit_start;
      zg_lane_literals(out + sq[i].mdst - ll, lit, rle, sq[i].lit_start, ll);
    }
    zg_lane_literals(out + sum_ll + sum_ml, lit, rle, sum_ll, blk.regen_size - sum_ll);
  }
  for (uint32_t f = 0; f < d.nframes; f++) simt::run(64, [&]() { zg_sparse_frame(d, f); });
  memcpy(dst_out, v.dst.data() + 256, v.total);
  return nsparse;
}

// zg_partial_block on block b (batch index) of frame f: the bytes in front of the block are the serial model's, `room` bytes behind
// them are 0xAA. behind_out: [room] what lies behind the good blocks afterwards; *block_start: where they begin in the frame's
// output; *left: totals[5]. limit <= room.
int zgemu_inorder_partial(void* h, uint32_t f, uint32_t b, uint32_t nexec, uint32_t lits_of_next, uint32_t limit, uint32_t room,
                          uint8_t* behind_out, uint64_t* block_start, uint32_t* left) {
  EmuBatch* e = (EmuBatch*)h;
  if (f >= e->bb.frames.size() || b >= e->bb.blocks.size() || e->bb.blocks[b].frame != f || limit > room || nexec + (lits_of_next ? 1u : 0u) > e->bb.blocks[b].nseq) return -1;
  Dev v(e, room);
  const uint64_t at = v.fout[f].out_base + e->pos[b].out_base;
  memcpy(v.dst.data() + 256 + v.fout[f].out_base, e->dst.data() + v.fout[f].out_base, e->pos[b].out_base);
  simt::run(64, [&]() { zg_partial_block(v.d, f, b, nexec, lits_of_next, limit); });
  memcpy(behind_out, v.dst.data() + 256 + at, room);
  *block_start = e->pos[b].out_base; *left = v.totals[5];
  return 0;
}

// 1 + the sequence of block b that cannot be executed, as zg_k_seqpost's model or zgemu_exact left it (0: none)
uint32_t zgemu_block_pad(void* h, uint32_t b) { return ((EmuBatch*)h)->seqout[b].pad; }

}  // extern "C"
