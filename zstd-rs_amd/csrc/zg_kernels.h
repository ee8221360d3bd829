// zg_kernels.h — launch interface of the gfx950 kernels (implemented in zg_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zg_types.h"
#include "zg_scatter.h"
#include "zg_dictfill.h"
#include "zg_walk.h"
#include "zg_index.h"
#include "zg_seek.h"
#include "zg_seektab.h"
#include "zg_seeksums.h"
#include "zg_idxsums.h"
#include "zg_seekmany.h"
#include "zg_seekidx.h"
#include "zg_records.h"
#include "zg_zxprobe.h"

// one launch of zg_k_sweep
// zg_k_sweep: threads per workgroup, groups of 4 output bytes a thread has in flight; a workgroup takes ZG_SW_BATCH bytes of a unit.
// (128 or 256 threads with 2 or 4 groups each measure the same; one group per thread, or several batches per workgroup, are
// slower. What matters more is that a launch has no workgroups that only come and go: see zg_launch_sweep.)
#ifndef ZG_SW_T
#define ZG_SW_T 256
#endif
#ifndef ZG_SW_B
#define ZG_SW_B 2
#endif
#define ZG_SW_BATCH (4u * ZG_SW_T * ZG_SW_B)
struct ZgSweepStep { uint32_t list_off, nunits, slices, pad; };
// measurement switches of the sweep (tools/dev/README.md): read from the environment ONCE, when an engine is created (zg::Tuning) —
// mode: ZGPU_SWEEP_MODE (timing experiments: wrong results), nbatch: batches per workgroup, group: steps whose heads share a launch,
// head_lds: unused LDS a head workgroup asks for (keeps the heads to a few workgroups per CU)
struct ZgSweepTuning { uint32_t mode = 0, nbatch = 0, group = 16, head_lds = 52u * 1024u, head_nbatch = 0; };   // nbatch 0: chosen by zg_launch_sweep

void zg_launch_reset(const ZgBatchDev& d, hipStream_t s);   // status words, table logs, totals (and d.dbg) to zero: the first kernel of a submit
void zg_launch_tables(const ZgBatchDev& d, hipStream_t s, int part);   // part 0: Huffman trees, part 1: FSE tables
void zg_launch_huf(const ZgBatchDev& d, hipStream_t s);
void zg_launch_seq(const ZgBatchDev& d, hipStream_t s, bool packed);   // packed: 16-bit table entries, three workgroups per CU (submits of more blocks than one round holds)
void zg_launch_seqpost(const ZgBatchDev& d, hipStream_t s);
void zg_launch_seqsize(const ZgBatchDev& d, hipStream_t s);   // in zg_launch_seqpost's place where a submit is only measured (zg_seqsize.h): the blocks' sums, no records
void zg_launch_merge(const ZgBatchDev& d, hipStream_t s);
void zg_launch_litfix(const ZgBatchDev& d, hipStream_t s);   // ZG_FLAG_LIT_DIRECT: literal verdicts found after the scan -> block and frame statuses
void zg_launch_scan(const ZgBatchDev& d, hipStream_t s, uint32_t max_frame_blocks);   // max_frame_blocks: of the submit's frames (picks the workgroup size)
void zg_launch_scan_sizes(const ZgBatchDev& d, hipStream_t s, uint32_t max_frame_blocks);   // zg_k_scan without zg_k_scanf: a submit that is only measured places no frame (Batch::measure)
void zg_launch_lit(const ZgBatchDev& d, hipStream_t s);
void zg_launch_flat(const ZgBatchDev& d, hipStream_t s, hipStream_t s2, hipEvent_t* ev, int flat4);   // s2, ev[2]: the direct units beside the pointer-mode ones
void zg_launch_sparse(const ZgBatchDev& d, hipStream_t s);   // the matches of frames marked sparse, in order (after zg_launch_flat)
bool zg_launch_sweep(const ZgBatchDev& d, hipStream_t s, const ZgSweepStep* steps, uint32_t nsteps, hipStream_t s2, hipEvent_t* evs, uint32_t nev,
                     uint32_t unit_bytes, uint32_t window_max, uint32_t window_min, const ZgSweepTuning& tn);   // s2 / evs: the side stream of the split sweep (nev == 0: one stream, step by step); returns whether it split
void zg_launch_lz(const ZgBatchDev& d, hipStream_t s);
void zg_launch_partial(const ZgBatchDev& d, hipStream_t s, uint32_t frame, uint32_t block, uint32_t nexec, bool lits_of_next, uint32_t limit);   // what the reference's buffer holds of a block whose sequence execution failed (Batch::sync, runs of one frame)
void zg_launch_exact(const ZgBatchDev& d, hipStream_t s, uint32_t drain_rule);   // zg_exact.h: the reference's DecodeBuffer bookkeeping, exactly (rare path, Batch::sync)
void zg_launch_calib(const void* src, void* dst, uint64_t bytes, hipStream_t s);
// zg_k_xxh64: XXH64 (seed 0) of byte ranges of a batch's output, one lane per range; out[slot] = digest. ranges are sorted by length, longest first
struct ZgHashRange { uint64_t off, len; uint32_t slot, pad; };
void zg_launch_xxh64(const uint8_t* base, const ZgHashRange* ranges, uint64_t* out, uint32_t n, hipStream_t s);
// zg_k_xxh64q: the same digests, four lanes per range (lane l owns accumulator l), 16 ranges per wave, one wave per workgroup. A range costs more
// wave-instructions this way (~17/16 of a lane's share per stripe against 54/64), so it is the kernel for launches whose ranges are too few to
// fill the chip, where the rate PER RANGE decides: zg_launch_xxh64 takes it for up to ZG_XXH64Q_MAX_RANGES ranges. That threshold comes from
// tools/dev/hash_ranges.py on an MI355X (LABNOTES.md "xxh64q": the quad kernel won on every workload measured, 1.35 x to 26 x). It is still 0:
// the launches of the existing calls are zg_k_xxh64 as before, and the quad kernel runs where it is asked for by name — zgpu_debug_hash_ranges,
// and Batch::hash_launch's quad_max_ranges, which the calls that carry ZGPU_DEVICE_VERIFY_SEEK_TABLE set (zg_frames.cpp: kTableQuadMaxRanges).
// zg_launch_xxh64_with: kernel 0 the rule above, 1 zg_k_xxh64, 4 zg_k_xxh64q (zgpu_debug_hash_ranges).
#define ZG_XXH64Q_RANGES 16u
#define ZG_XXH64Q_MAX_RANGES 0u
void zg_launch_xxh64_with(const uint8_t* base, const ZgHashRange* ranges, uint64_t* out, uint32_t n, hipStream_t s, int kernel);
// zg_k_scatter (zg_scatter.h): the chunks of the segments of a batch's output (base) to the segments' destinations, one workgroup per chunk
void zg_launch_scatter(const uint8_t* base, const zgs::Seg* segs, const zgs::Chunk* chunks, uint32_t nchunks, hipStream_t s);
// zg_k_gather (zg_walk.h): the same chunks the other way round — segments whose src_off is an ADDRESS in device memory of the caller (the entries
// of a submit of zgpu_decode_frames_device_src) copied to where the engine's kernels read the compressed bytes; dst: addresses in the engine's buffer
void zg_launch_gather(const zgs::Seg* segs, const zgs::Chunk* chunks, uint32_t nchunks, hipStream_t s);
// zg_k_dictfill (zg_dictfill.h): a dictionary's content and tables from the context's device copy to the gaps and carry slots of the frames that
// name it; segs hold addresses on both sides, chunks the plan of zgd::plan_fill
void zg_launch_dictfill(const zgd::Seg* segs, const zgs::Chunk* chunks, uint32_t nchunks, hipStream_t s);
// zg_k_walk (zg_walk.h): one lane per entry follows the entry's header chain; ends[i] = where lane i stopped and how many skeleton records it has.
// recs == nullptr: the count pass (nothing else is written); else lane i writes records lanes[i].first .. + lanes[i].limit of recs
void zg_launch_walk(const zgw::Lane* lanes, uint32_t n, zgw::End* ends, zgw::Rec* recs, hipStream_t s);
// zg_k_index (zg_index.h): one lane per entry follows the entry's header chain without touching a block body; entries[i] = the summary of lane i.
// recs == nullptr: the summary pass (nothing else is written); else lane i also writes frame records lanes[i].first .. + lanes[i].limit of recs
void zg_launch_index(const zgw::Lane* lanes, uint32_t n, zgi::Entry* entries, zgi::FrameRec* recs, hipStream_t s);
// zg_k_seek (zg_seek.h): one lane per entry selects the whole frames that hold a plaintext range of the entry, from frame and block headers alone;
// out[i] = the record of lane i. ONE launch for all n entries
void zg_launch_seek(const zgk::Lane* lanes, uint32_t n, zgk::Seek* out, hipStream_t s);
// zg_k_seektab (zg_seektab.h): one wave per entry answers the same from the seekable format's seek table at the entry's end; one 64-thread
// workgroup per entry, out[i] = entry i's record
void zg_launch_seektab(const zgt::Lane* lanes, uint32_t n, zgk::Seek* out, hipStream_t s);
// zg_k_seeksums (zg_seeksums.h): one wave per entry compares the Checksum fields of the entry's seek table with the digests the hash kernel wrote
// (digests[0 .. ndig), device memory) for the entry's slice of frames; one 64-thread workgroup per entry, out[i] = entry i's 32-byte record
void zg_launch_seeksums(const zgv::Lane* lanes, uint32_t n, const zgv::Frame* frames, const uint64_t* digests, uint32_t ndig, zgv::Sums* out, hipStream_t s);
// zg_k_idxsums (zg_idxsums.h): one wave per group compares the sums a seek index handle holds (pairs, sums: the handle's arrays in device memory)
// with the same digests for the group's slice of frames; one 64-thread workgroup per group, out[i] = group i's 32-byte record
void zg_launch_idxsums(const zgh::Lane* lanes, uint32_t n, const void* pairs, const uint32_t* sums, const zgv::Frame* frames, const uint64_t* digests,
                       uint32_t ndig, zgv::Sums* out, hipStream_t s);
// zg_seekmany.h: the seek tables of a few entries scanned once, many ranges answered from the prefix sums. locate: one lane per entry, out[i] =
// what entry i's table frame is. prefix: two launches over the nw chunks of work — zg_k_seekmany_total, then zg_k_seekmany_prefix — that fill
// pairs[], the scratch the host laid out. find: one lane per range, out[j] = range j's record
void zg_launch_seekmany_locate(const zgm::Ent* ents, uint32_t n, zgm::Loc* out, hipStream_t s);
void zg_launch_seekmany_prefix(const zgm::Work* work, uint32_t nw, zgm::Pair* pairs, hipStream_t s);
void zg_launch_seekmany_find(const zgm::Find* lanes, uint32_t m, const zgm::Pair* pairs, zgk::Seek* out, hipStream_t s);
// zg_k_seekidx_rows (zg_seekidx.h): one lane per entry follows the entry's header chain and stores the exclusive prefixes of its frame records
// into pairs[lanes[i].pre .. + lanes[i].limit]: the pairs zg_k_seekmany_find reads; out[i] = what lane i found
void zg_launch_seekidx_rows(const zgx::Lane* lanes, uint32_t n, zgm::Pair* pairs, zgx::Rows* out, hipStream_t s);
// zg_records.h: the record index's side pass over a synced submit's output `out` (one wave per chunk) and its lookup. count: counts[i] = the
// bytes of chunk i equal to d. scan (one workgroup): prefix[i] = the exclusive prefix of the counts, totals[0] = their sum, totals[1 + f] = the
// sum over the chunks [fstart[f], fstart[f + 1]) of frame f. emit: the value base + p + 1 of every such byte, in order, to
// staging[prefix[chunk] ...), never at or behind staging[total]. find: one lane per record range over the handle's offsets recs, out[j] = its answer
void zg_launch_recs_count(const uint8_t* out, const zgr::Chunk* chunks, uint32_t n, uint32_t d, uint32_t* counts, hipStream_t s);
void zg_launch_recs_scan(const uint32_t* counts, uint32_t nchunks, const uint32_t* fstart, uint32_t nframes, uint64_t* prefix, uint64_t* totals, hipStream_t s);
void zg_launch_recs_emit(const uint8_t* out, const zgr::Chunk* chunks, uint32_t n, uint32_t d, const uint64_t* prefix, uint64_t* staging, uint64_t total,
                         hipStream_t s);
void zg_launch_recs_find(const zgr::Find* lanes, uint32_t m, const uint64_t* recs, zgr::Found* out, hipStream_t s);
// zg_k_fill (zg_scatter.h): `byte` into the chunks of the regions segs[] (src_off unused), one wave per chunk
void zg_launch_fill(const zgs::Seg* segs, const zgs::Chunk* chunks, uint32_t nchunks, uint32_t byte, hipStream_t s);
// zg_k_zxprobe (zg_zxprobe.h): ONE zx_* primitive on one workgroup of `threads` (64 or 256) threads; in, out, arena: device memory whose
// every operand-named index the caller checked with zxp::args_ok
void zg_launch_zxprobe(uint32_t op, uint32_t threads, uint32_t flags, const uint32_t* in, uint32_t* out, uint8_t* arena, uint32_t res_off, uint32_t res_bytes, hipStream_t s);
