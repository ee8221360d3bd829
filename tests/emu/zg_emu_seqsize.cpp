// zg_emu_seqsize.cpp — TEST-ONLY: runs the SOURCE of zg_k_seqsize (zstd-rs_amd/csrc/zg_seqsize.h) on the CPU through the SIMT emulator of
// zg_simt.h, one 256-thread workgroup per block with sequences, on what the stages in front of it leave: the host's parse
// (zg_host_parse.cpp), the FSE tables (zg_dev.h, as tests/emu/zg_emu.cpp builds them) and, in zg_k_seq's place, a serial follower of the
// three FSE states that packs every sequence's states with ZG_RAW_PACK and leaves the bit position of the first sequence in seq_out[b].pad.
// The bitstream is read through a hook (ZG_SZ_LD96) that counts every dword the kernel asks for and every dword it is served that lies
// outside the dwords holding the block's bitstream — what zg_k_seqpost's load may touch. tests/test_seqsize_cpu.py builds this file
// (tests/lanesuite.py; it is not in the Makefile's library) and compares every block's sums and status with the oracle's sequences.
// Not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../zstd-rs_amd/csrc/zg_types.h"
#include "zg_simt.h"
#include "zg_emu_serial.h"
#include "zg_emu_fill.h"
#include "../../zstd-rs_amd/csrc/zg_host_parse.h"

// the bitstream reader: counts[0] loads, [1] dwords served from outside [g_lo, g_hi), [2] dwords asked for that the resource refused (they
// read as 0: the second or third dword of a load near the stream's end), [3] those of them that were the FIRST dword of their load — the
// dword that holds bit q_ll, which lies inside the stream for every sequence zg_k_seq recorded
static uint64_t g_counts[4];
static uintptr_t g_lo, g_hi;
static inline ZxU3 sz_ld96(const ZxBuf& b, uint32_t off) {
  g_counts[0]++;
  for (uint32_t k = 0; k < 3; k++) {
    const uint64_t o = (uint64_t)off + 4 * k;
    if (o + 4 > b.bytes) { g_counts[2]++; g_counts[3] += k == 0; continue; }
    const uintptr_t a = (uintptr_t)b.base + (uintptr_t)o;
    if (a < g_lo || a + 4 > g_hi) g_counts[1]++;
  }
  return zx_ld96(b, off);
}
#define ZG_SZ_LD96(buf, off) sz_ld96(buf, off)
#include "../../zstd-rs_amd/csrc/zg_seqsize.h"

using namespace zg;

namespace {
// decode_all's walk, as tests/emu/zg_emu.cpp has it
int walk(const uint8_t* src, size_t len, BatchBuilder* bb) {
  size_t p = 0;
  static const uint32_t kHist[3] = {1, 4, 8};
  while (p < len) {
    FrameHeader h; size_t c; uint32_t sm = 0, sl = 0;
    int st = read_frame_header(src + p, len - p, &h, &c, &sm, &sl);
    if (st == ZG_SKIP_FRAME) { p += c; if ((size_t)sl > len - p) return ZG_FAILED_SKIP_FRAME; p += sl; continue; }
    if (st) return st;
    uint64_t w;
    if ((st = frame_window_size(h, &w))) return st;
    if (h.has_dict_id) return ZG_DICT_NOT_PROVIDED;
    p += c;
    bb->begin_frame(w, kHist, 0);
    for (;;) {
      if (len - p < 3) return ZG_FAILED_READ_BLOCK_HEADER;
      BlockHeader bh;
      if ((st = read_block_header(src + p, &bh))) return st;
      p += 3;
      if (len - p < bh.content_size) return ZG_FAILED_READ_BLOCK_BODY;
      st = bb->add_block(bh, src + p, p);
      p += bh.content_size;
      if (st) return st;
      if (bh.last) { if (h.content_checksum()) { if (len - p < 4) return ZG_FAILED_READ_CHECKSUM; p += 4; } break; }
    }
  }
  return ZG_OK;
}

// zg_k_seq's part: the states of every sequence, and where the first one starts. Returns the bitstream's status.
int follow(const uint8_t* bs, uint32_t bs_len, uint32_t nseq, const uint32_t* t_ll, unsigned ll_log, const uint32_t* t_of, unsigned of_log,
           const uint32_t* t_ml, unsigned ml_log, uint32_t* raw, uint32_t* first) {
  if (bs_len == 0 || bs[bs_len - 1] == 0) return ZG_SEQ_EXTRA_PADDING;
  int32_t P = (int32_t)(bs_len - 1) * 8 + (int32_t)(zg_hbit(bs[bs_len - 1]) - 1);
  P -= (int32_t)ll_log; uint32_t s_ll = zg_bits_at_z(bs, P, ll_log);
  P -= (int32_t)of_log; uint32_t s_of = zg_bits_at_z(bs, P, of_log);
  P -= (int32_t)ml_log; uint32_t s_ml = zg_bits_at_z(bs, P, ml_log);
  *first = (uint32_t)P;
  for (uint32_t i = 0; i < nseq; i++) {
    const uint32_t e_ll = t_ll[s_ll], e_of = t_of[s_of], e_ml = t_ml[s_ml];
    raw[i] = ZG_RAW_PACK(s_of, s_ml, s_ll);
    P -= (int32_t)(ZG_FSE_XB(e_of) + ZG_FSE_XB(e_ml) + ZG_FSE_XB(e_ll));
    if (i + 1 < nseq) {   // LL, ML, OF
      unsigned nb;
      nb = ZG_FSE_NB(e_ll); P -= (int32_t)nb; s_ll = ZG_FSE_BL(e_ll) + zg_bits_at_z(bs, P, nb);
      nb = ZG_FSE_NB(e_ml); P -= (int32_t)nb; s_ml = ZG_FSE_BL(e_ml) + zg_bits_at_z(bs, P, nb);
      nb = ZG_FSE_NB(e_of); P -= (int32_t)nb; s_of = ZG_FSE_BL(e_of) + zg_bits_at_z(bs, P, nb);
    }
    if (P < 0) return ZG_SEQ_NOT_ENOUGH_BYTES;
  }
  return P > 0 ? ZG_SEQ_EXTRA_BITS : ZG_OK;
}
}  // namespace

// what the harness says of one block with sequences, in the order of the submit's seq_blocks list
struct SzBlock { uint32_t frame, block, nseq, regen, front_status, status, sum_ll, sum_ml, hist[3], pad, nbytes, lead; };

// The frames of src decoded up to zg_k_seqsize, the copy of the input shifted by `shift` bytes (0 .. 3) against a 16-byte boundary. Returns the
// number of blocks with sequences (at most cap are written), or -(status) if the host's walk refuses the input; counts: the reader's four.
extern "C" int32_t sz_run(const uint8_t* src, uint64_t len, uint32_t shift, uint32_t cap, SzBlock* out, uint64_t* counts) {
  BatchBuilder bb;
  std::vector<uint8_t> store(len + 64 + 16 + 64 + 16, emufill::byte(0x5A));   // (the padding holds no zeros: a dword served from it would change a sum)
  uint8_t* base = store.data() + ((16 - ((uintptr_t)store.data() & 15u)) & 15u) + 64 + (shift & 3u);
  memcpy(base, src, len);
  const int wst = walk(base, len, &bb);
  if (wst) return -wst;
  bb.finish();
  const uint32_t nb = (uint32_t)bb.blocks.size(), nf = (uint32_t)bb.frames.size();
  const uint32_t nslots = nb + 1 + nf;
  std::vector<uint32_t> fse((size_t)nslots * ZG_FSE_SLOT_U32, emufill::word(0)), status(nb + 4, 0), raw(bb.seq_count + 8, emufill::word(0));
  std::vector<uint8_t> slot_log((size_t)nslots * 4, 0);
  std::vector<ZgBlockAux> aux(nb + 1);
  std::vector<ZgBlockSeqOut> seqout(nb + 1);
  memset(aux.data(), emufill::byte(0), aux.size() * sizeof(ZgBlockAux));         // (every field the kernel reads is written below: seq_bits_off for every block, log[] where a table is built)
  memset(seqout.data(), emufill::byte(0), seqout.size() * sizeof(ZgBlockSeqOut));   // (pad: written below for every block that runs)
  int16_t probs[256]; uint16_t counter[256];
  {   // the predefined tables (zg_k_ftab; tests/emu/zg_emu.cpp: k_tables)
    uint32_t* slot = fse.data() + (size_t)nb * ZG_FSE_SLOT_U32;
    for (int i = 0; i < 36; i++) probs[i] = ZG_LL_DEFAULT[i];
    zg_fse_build(probs, 36, 6, ZG_KIND_LL, slot + ZG_FSE_LL_OFF, counter);
    for (int i = 0; i < 29; i++) probs[i] = ZG_OF_DEFAULT[i];
    zg_fse_build(probs, 29, 5, ZG_KIND_OF, slot + ZG_FSE_OF_OFF, counter);
    for (int i = 0; i < 53; i++) probs[i] = ZG_ML_DEFAULT[i];
    zg_fse_build(probs, 53, 6, ZG_KIND_ML, slot + ZG_FSE_ML_OFF, counter);
    uint8_t* lg = slot_log.data() + (size_t)nb * 4; lg[0] = 6; lg[1] = 5; lg[2] = 6;
  }
  for (uint32_t b = 0; b < nb; b++) {
    const ZgBlock blk = bb.blocks[b];
    aux[b].seq_bits_off = blk.seq_off;
    if (blk.host_status || blk.btype != ZG_BT_COMPRESSED || !blk.nseq) continue;
    const uint8_t* body = base + blk.src_off;
    const uint8_t* p = body + blk.seq_off; uint32_t rem = blk.src_len - blk.seq_off;
    uint32_t* slot = fse.data() + (size_t)b * ZG_FSE_SLOT_U32;
    const int kinds[3] = {ZG_KIND_LL, ZG_KIND_OF, ZG_KIND_ML};
    const int modes[3] = {blk.seq_modes >> 6, (blk.seq_modes >> 4) & 3, (blk.seq_modes >> 2) & 3};
    const int max_log[3] = {9, 8, 9}, max_sym[3] = {35, 31, 52};
    const uint32_t offs[3] = {ZG_FSE_LL_OFF, ZG_FSE_OF_OFF, ZG_FSE_ML_OFF};
    int st = ZG_OK;
    for (int k = 0; k < 3 && !st; k++) {
      if (modes[k] == ZG_MODE_FSE) {
        int np, al; uint32_t used;
        st = zg_fse_read_probs(p, rem, max_log[k], max_sym[k], probs, &np, &al, &used);
        if (!st) st = zg_fse_build(probs, np, al, kinds[k], slot + offs[k], counter);
        if (!st) { aux[b].log[k] = (uint8_t)al; p += used; rem -= used; }
      } else if (modes[k] == ZG_MODE_RLE) {
        if (rem == 0 || p[0] > max_sym[k]) st = ZG_SEQ_RLE_BYTE;
        else { slot[offs[k]] = zg_fse_pack(kinds[k], 0, 0, p[0]); aux[b].log[k] = 0; p += 1; rem -= 1; }
      }
    }
    aux[b].seq_bits_off = (uint32_t)(p - body);
    uint8_t* lg = slot_log.data() + (size_t)b * 4; lg[0] = aux[b].log[0]; lg[1] = aux[b].log[1]; lg[2] = aux[b].log[2];
    status[b] = (uint32_t)st;
  }
  // zg_k_seq's part, then the kernel under test
  ZgBatchDev d;
  memset(&d, 0, sizeof d);
  d.src = base; d.src_len = len;
  d.blocks = bb.blocks.data(); d.nblocks = nb;
  d.frames = bb.frames.data(); d.nframes = nf;
  d.nslots = nslots;
  d.aux = aux.data(); d.slot_log = slot_log.data(); d.fse_arena = fse.data();
  d.status = status.data(); d.raw_arena = raw.data(); d.seq_out = seqout.data();
  d.seq_blocks = bb.seq_blocks.data(); d.nseq_blocks = (uint32_t)bb.seq_blocks.size();
  memset(g_counts, 0, sizeof g_counts);
  static ZgSeqSizeLds lds;
  int32_t n = 0;
  for (uint32_t b : bb.seq_blocks) {
    const ZgBlock blk = bb.blocks[b];
    const int32_t sl[3] = {blk.ll_slot, blk.of_slot, blk.ml_slot};
    const uint32_t offs[3] = {ZG_FSE_LL_OFF, ZG_FSE_OF_OFF, ZG_FSE_ML_OFF};
    const uint32_t* tp[3] = {nullptr, nullptr, nullptr}; unsigned lg[3] = {0, 0, 0};
    bool ok = status[b] == 0 && aux[b].seq_bits_off <= blk.src_len;
    for (int k = 0; k < 3; k++) {
      if (sl[k] < 0 || ((uint32_t)sl[k] < nb && status[sl[k]] != 0)) { ok = false; continue; }
      lg[k] = slot_log[(size_t)sl[k] * 4 + k];
      tp[k] = fse.data() + (size_t)sl[k] * ZG_FSE_SLOT_U32 + offs[k];
    }
    const uint32_t nbytes = ok ? blk.src_len - aux[b].seq_bits_off : 0;
    const uint8_t* bs = base + blk.src_off + aux[b].seq_bits_off;
    if (!ok && !status[b]) status[b] = ZG_FSE_UNINIT;
    if (ok) {
      uint32_t first = 0;
      status[b] = (uint32_t)follow(bs, nbytes, blk.nseq, tp[0], lg[0], tp[1], lg[1], tp[2], lg[2], raw.data() + blk.seq_base, &first);
      seqout[b].pad = first;
    }
    const uint32_t front = status[b];
    // the dwords that hold the bitstream: what zg_k_seqpost's load may touch of the input (its third dword may lie behind them, in the engine's padding)
    g_lo = (uintptr_t)bs & ~(uintptr_t)3;
    g_hi = ((uintptr_t)bs + nbytes + 3) & ~(uintptr_t)3;
    memset(&lds, emufill::byte(0xEE), sizeof lds);
    simt::run(ZG_SZ_T, [&]() { zg_seqsize_block(d, b, lds); });
    if ((uint32_t)n < cap) {
      SzBlock& o = out[n];
      o.frame = blk.frame; o.block = b - bb.frames[blk.frame].first_block; o.nseq = blk.nseq; o.regen = blk.regen_size;
      o.front_status = front; o.status = status[b];
      o.sum_ll = seqout[b].sum_ll; o.sum_ml = seqout[b].sum_ml;
      o.hist[0] = seqout[b].hist_end[0]; o.hist[1] = seqout[b].hist_end[1]; o.hist[2] = seqout[b].hist_end[2];
      o.pad = seqout[b].pad; o.nbytes = nbytes; o.lead = (uint32_t)((uintptr_t)bs & 3u);
    }
    n++;
  }
  memcpy(counts, g_counts, sizeof g_counts);
  return n;
}
extern "C" uint32_t sz_per_thread(void) { return ZG_SZ_S; }
extern "C" int sz_set_fill(int v) { const int was = emufill::g_fill; emufill::set(v); return was; }   // (zg_emu_fill.h)
