// zg_engine.h — one engine per (GPU, pair of HIP streams): device memory, upload of a parsed submit, the kernel
// pipeline, and result download. Host buffers never enter the kernels. The engine allocates its own device memory with the HIP runtime and
// knows nothing of torch; the one place where memory it does not own enters a kernel is Batch::scatter_launch, whose destinations are device
// pointers of the caller (a torch tensor's data_ptr(), say) that zgpu_decode_frames_device has checked against the runtime's allocations.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "zg_host_parse.h"
#include "zg_kernels.h"

namespace zg {

// Bytes allocated in front of every output buffer: zg_k_sweep fetches the source of output byte i of a 4-byte group as
// byte i of the dword that starts i bytes before it, so up to 3 bytes in front of the first output byte are touched.
constexpr size_t kOutFront = 256;

// ZGPU_POISON=<0..255> (development build only; Tuning::poison): every byte of device memory whose content the design does not define when a
// submit starts is filled with the value, in stream order in front of the first upload or kernel of the submit that touches the buffer —
// every DevBuf of the submit's Scratch over its whole cap (d_src's zero pads are issued behind the fill), the output with its front pad and
// what lies behind it, a frame's window outside [dictionary][have], the staging buffer, the carried table slots carry_mask says do not
// exist, a SidePass's buffer and the lane passes' buffers when they are reserved. Uploaded input, carried state, a seek index handle's pairs
// and sums, registered dictionaries and the caller's own memory are never touched. The value is the process's (the engine created last
// read it: a streaming decoder's worker engine fills with the same byte as the context's); bytes(): filled since the last submit was
// prepared (Engine::upload). Without ZG_DEV_SWITCHES every member is an empty inline function: the product contains none of this.
struct Poison {
#ifdef ZG_DEV_SWITCHES
  static int value();                                        // -1: off
  static void set(int v);
  static void fill(void* p, size_t n, hipStream_t s);        // in stream order on s
  static void fill_now(void* p, size_t n);                   // returns when the bytes are there (a buffer no stream has seen yet)
  static void begin_submit();
  static uint64_t bytes();
  static uint64_t scratch_cap;                               // the sum of the capacities of the last prepared submit's Scratch, as filled
#else
  static int value() { return -1; }
  static void fill(void*, size_t, hipStream_t) {}
  static void fill_now(void*, size_t) {}
  static void begin_submit() {}
  static uint64_t bytes() { return 0; }
#endif
};

// growable device buffer; a buffer that is grown again grows by at least half of its size (amortised reuse)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t n, bool keep = false, hipStream_t s = nullptr);
  void release();
  template <typename T> T* as() const { return (T*)p; }
};

// One timed pass beside or behind the decode: what Batch's side passes (below) and the engine's lane passes each need — ONE device buffer for the
// pass's tables and what it leaves, two events created with the first reserve, and n: what the pass in flight was launched over (0: none).
// Which stream a site uploads and launches on, where it waits and what it counts stay the site's: this holds only what every site repeated.
struct SidePass {
  DevBuf buf;
  hipEvent_t ev[2] = {nullptr, nullptr};
  uint32_t n = 0;
  size_t back = 0;                             // where what the kernel leaves begins in buf
  int reserve(size_t bytes);                   // the buffer and the events
  hipError_t upload(const void* a, size_t ab, const void* b, size_t bb, hipStream_t s) const;   // a to the front of buf, b (bb != 0) behind it
  hipError_t begin(hipStream_t s) const { return hipEventRecord(ev[0], s); }
  hipError_t end(hipStream_t s) const;         // the launch's hipGetLastError, then the second event
  hipError_t elapsed_us(uint64_t* us) const;   // the time between the two events, rounded to microseconds
  void release(int device = -1);               // device >= 0: made current in front of the free (a Batch may die on any thread)
  template <typename T> T* at(size_t off) const { return (T*)((uint8_t*)buf.p + off); }
};

// What one frame carries from one submit of its blocks to the next (the reference's DecoderScratch, scratch.rs:15-27):
// the decode window (a dictionary's content sits in front of it), the offset history, and the Huffman / FSE tables a
// later Treeless / Repeat block may decode with. The device holds [front pad][dictionary content][the last `have` bytes of
// the frame]; bytes the caller has drained and that no match may reach any more are dropped when the buffer is rebuilt.
struct FrameState {
  DevBuf d_out;
  uint64_t base = 0;             // dictionary content bytes in front of the frame bytes
  uint64_t have = 0;             // frame bytes on the device (the most recent ones)
  uint64_t produced = 0;         // frame bytes decoded so far
  uint32_t hist[3] = {1, 4, 8};  // scratch.rs:44
  uint64_t counted = 0;          // DecodeBuffer::total_output_counter so far (decode_buffer.rs:16): decides between the two "offset too far" errors
  DevBuf d_fse;                  // carried FSE tables, one arena slot (ZG_FSE_SLOT_U32 packed entries)
  DevBuf d_huf;                  // carried Huffman table (ZG_HUF_SLOT_U16 entries)
  DevBuf d_tmp;                  // make_room: staging for the undrained bytes when they are moved down over themselves
  uint8_t logs[4] = {0, 0, 0, 0};// accuracy logs LL, OF, ML of the carried FSE tables
  uint8_t huf_maxbits = 0;
  uint32_t carry_mask = 0;       // bit 0 Huffman, 1 LL, 2 OF, 3 ML: which tables exist
  uint64_t window_size = 0;
  uint8_t* out_ptr() const { return (uint8_t*)d_out.p + kOutFront; }   // first byte of [dictionary content][frame bytes]
  // Make room for `extra` more frame bytes. `keep` = frame bytes that must stay reachable (what the caller still holds
  // undrained: DecodeBuffer semantics, decode_buffer.rs:79-111,182-219); older bytes are dropped when the buffer is rebuilt.
  int make_room(uint64_t extra, uint64_t keep, hipStream_t s);
  int reserve_window(uint64_t payload, hipStream_t s);
  // would make_room(extra, keep) move or reallocate what the buffer holds? (a download of earlier bytes must not be in flight then)
  bool room_moves(uint64_t extra, uint64_t keep) const {
    if (keep > have) keep = have;
    if (base && keep < have && d_out.p) return true;
    return !d_out.p || kOutFront + base + have + extra + 64 > d_out.cap;
  }
  void reset();
  void release();
};

enum { ZG_T_TABLES = 0, ZG_T_HUF, ZG_T_SEQ, ZG_T_SEQPOST, ZG_T_SCAN, ZG_T_LIT, ZG_T_FLAT, ZG_T_SWEEP, ZG_T_LZ, ZG_T_TOTAL, ZG_T_COUNT };

// Device buffers and events of one submit in flight. Engines keep finished ones for reuse: a stream of submits (block runs
// of a streaming decoder, frames pulled from a work queue) allocates once.
struct Scratch {
  DevBuf d_src, d_blocks, d_frames, d_aux, d_fparsed, d_slot_log, d_fse, d_huf, d_hufmax, d_status, d_lit, d_seq, d_seqout, d_pos, d_frameout,
      d_dst, d_seqblocks, d_hufitems, d_hufgroups, d_totals, d_og, d_units, d_unitinfo, d_stepunits, d_swdesc, d_dbg, d_raw, d_unitlist;
  hipEvent_t ev[ZG_T_COUNT + 1] = {};
  hipEvent_t ev_up = nullptr;                     // a submit prepared beside another one: its uploads are done (Engine::upload side)
  hipEvent_t ev_huf[2] = {}, ev_fork = nullptr, ev_fork3 = nullptr;   // zg_k_huf runs on the engine's second stream beside zg_k_seq
  hipEvent_t ev_sw[80] = {};                      // split sweep: heads on the second stream (zg_launch_sweep)
  hipEvent_t ev_flat[2] = {};                     // the direct units' flatten on the second stream beside the pointer-mode units' (zg_launch_flat)
  bool have_events = false;
  template <class F> void each_buf(F f);          // every DevBuf above
  int init_events();
  void release();
  void release_but_output();
};

// Measurement and test switches (the ZGPU_* environment variables of tools/dev/README.md). The PRODUCT library (libzgpu.so) reads none of
// them: an environment variable must not be able to make a drop-in decoder slower, let alone wrong. The development build (make dev ->
// libzgpu_dev.so, -DZG_DEV_SWITCHES; what the tests that force a path and tools/dev load) reads them ONCE, when an engine is created:
// nothing on the submit path (prepare / run / sync, zg_launch_sweep) calls getenv. A test that wants a switch sets it before it creates
// its (development) context; a switch set afterwards is ignored (zgpu_debug_tuning shows what an engine took).
struct Tuning {
  bool dev_build = false;          // libzgpu_dev.so (-DZG_DEV_SWITCHES): the only build in which any of the switches below is read
  uint32_t unit_blocks = 0;        // ZGPU_UNIT_BLOCKS: blocks per flatten unit (0: chosen by BatchBuilder::finish)
  bool direct = true;              // ZGPU_DIRECT=0: no direct units
  uint32_t ramp_percent = 0;       // ZGPU_RAMP
  bool sparse_set = false;         // ZGPU_SPARSE_MAX given
  uint32_t sparse_max = 0;
  int lit_direct = -1;             // ZGPU_LIT_DIRECT: 0 never, 1 always, else the host's choice
  uint32_t direct_share10 = 0;     // ZGPU_DIRECT_SHARE (tenths, >= 10)
  bool debug_timers = false;       // ZGPU_DEBUG_TIMERS
  bool force_inorder = false;      // ZGPU_FORCE_INORDER=1
  uint32_t flat_mode = 0;          // ZGPU_FLAT_MODE (timing experiments)
  uint32_t sweep_w = 0;            // ZGPU_SWEEP_W
  bool overlap = true;             // ZGPU_OVERLAP=0
  bool no_sweep = false;           // ZGPU_DEBUG_NO_SWEEP
  bool sweep_split = true;         // ZGPU_SWEEP_SPLIT=0
  bool no_exact = false;           // ZGPU_DEBUG_NO_EXACT
  bool no_presize = false;         // ZGPU_PRESIZE=0
  int flat4 = -1;                  // ZGPU_FLAT4: how the direct units of a submit are flattened — -1 (default): chosen per submit from the number of
                                   // direct units (Batch::launch_phase2); 0: by the kernel of the pointer-mode units (one 1024-thread workgroup per
                                   // CU, round 4's form); 1 / 4 / 6: by zg_k_flatten4 with 1024 / 512 / 256 threads and 8 / 4 / 2 KiB tiles (2 / 4 / 8
                                   // workgroups per CU); 2, 3, 5, 7: other shapes (measurement)
  int flat_shape = 0;              // ZGPU_FLAT_T=512 -> 1
  int seq_packed = -1;             // ZGPU_SEQ_PACKED: zg_k_seq's table entries — -1 (default): packed (16 bits, three workgroups per CU) when the submit has more
                                   // blocks with sequences than one round holds, else unpacked; 0 / 1: never / always
  ZgSweepTuning sweep;             // ZGPU_SWEEP_MODE / _NB / _GROUP / _HEAD_LDS
  uint64_t measure_submit_bytes = 0; // ZGPU_MEASURE_SUBMIT_BYTES: input per measuring submit of zgpu_seek_index_measure_device (0: the input budget of the decode submits; tests force several)
  uint64_t frames_submit_bytes = 0;  // ZGPU_FRAMES_SUBMIT_BYTES: plaintext (and input) per submit of zgpu_decode_frames (0: the library's constant; tests force several submits)
  uint32_t scatter_chunk = 0;        // ZGPU_SCATTER_CHUNK: bytes per chunk of zg_k_scatter's plan (0: zgs::kChunkDefault; measurement of the chunk size)
  bool hash_device_max_set = false;  // ZGPU_HASH_DEVICE_MAX: longest frame zgpu_decode_frames hashes on the device (measurement of the threshold)
  uint64_t hash_device_max = 0;
  int poison = -1;                   // ZGPU_POISON=<0..255>: what memory no submit has defined holds (struct Poison above); -1: left as it is
  static Tuning from_env();
};

class Engine;

// What every lane pass of an engine adds to the statistics array it is handed (Engine::lane_pass); the arrays of zg_capi_int.h that a pass
// fills begin with these three slots.
enum { kPassLaunches = 0, kPassUs = 1, kPassBytes = 2 };

// One submit: parsed input + its device state. Created by Engine::prepare.
class Batch {
 public:
  ~Batch();
  BatchBuilder bb;
  std::vector<FrameInfo> info;
  std::vector<ZgFrameOut> frame_out;     // valid after run() (sizes) / sync() (final status)
  uint64_t total_out = 0;                // valid after run()
  float ms[ZG_T_COUNT] = {0};
  int parse_status = 0;                  // frame-layer error that stops decode_all (first failing frame's status)
  uint64_t src_len = 0;
  uint64_t keep_bytes = 0;               // streaming submits: frame bytes that must stay reachable on the device (FrameState::make_room)
  uint32_t drain_rule = 0;               // how the caller's surface drains the reference's DecodeBuffer inside this submit (zg_exact.h: ZG_DRAIN_*)
  bool far_seen = false;                 // a sequence set an offset beyond its frame's window (zg_k_seqpost); valid after sync()
  uint64_t declared_total = 0;           // sum of the frames' Frame_Content_Size when every frame of the submit declares one (else 0): the
  bool all_declared = false;             //   output can be sized before the run, and the LZ77 stages enqueued without waiting for the scan
  bool presized = false;                 // the last run() did that
  bool exact_ran = false;                // sync(): zg_k_exact replayed the reference's buffer bookkeeping for this submit (tests)
  // dictionary frames of a shared submit (zgpu_set_frames_shared_dicts; the walk marked them: ZgFrame::dict_len, FrameInfo::header.dict_id). The
  // caller hands over, per frame of the submit, the device image of its dictionary (content_len 0: the frame has none) before run(); run() then
  // launches zg_k_dictfill (zg_dictfill.h) twice: the tables into the frames' carry slots in front of the entropy stages, the contents into
  // the gaps in front of the frames' plaintext once the scan has placed them (the gaps' positions depend on the sizes of the frames in front).
  // Such a submit is never sized before the run. Every segment is checked against the engine's buffers before a launch.
  int set_frame_dicts(std::vector<zgd::DictImage> images);
  uint32_t dictfill_launches = 0;        // of the last run()
  uint64_t dictfill_bytes = 0;           //   bytes it replicated
  uint64_t dictfill_us = 0;              //   its kernels' time between HIP events (valid after sync())
  bool gather_launched = false;          // prepare_entries_device: zg_k_gather brought the compressed bytes (no entry had any: no launch)
  uint64_t gather_us = 0;                //   its time between two HIP events

  // Enqueue the kernel pipeline on the engine's streams. Two phases with one host round trip in between: the entropy
  // stages and the scan run first; the host reads the exact output size of every frame, sizes the output and the flatten
  // scratch to it, and then enqueues the LZ77 stages. Returns when the second phase is enqueued.
  int run();
  // In place of run() + sync(), for a caller that wants the frames' SIZES and nothing else (zgpu_seek_index_measure_device): zg_k_reset, the
  // FSE tables, zg_k_seq, zg_k_seqsize (zg_seqsize.h) where run() has zg_k_seqpost, zg_k_scan, and frame_out comes back — out_size and
  // status of every frame, as size_output() reads them. Nothing of the Huffman chain runs, no output and no flatten scratch is reserved, no
  // LZ77 stage follows: what those stages would find (a Huffman description or stream, an offset, a checksum) is not found. The stream is
  // drained on return. *phase1_us, if asked for: the kernels' time between two HIP events. A measured batch is not run afterwards.
  int measure(uint64_t* phase1_us = nullptr);
  // streaming submits: after sync(), fold this run into the frame's carried state (tables, history, produced bytes)
  int commit(FrameState* fs);
  uint32_t carry_mask_in = 0;            // streaming runs: the tables that existed when the run was parsed
  uint32_t carry_mask_after() const;
  bool wait_upload = false;              // prepared with side uploads: run() waits for them on the device
  bool saw_last_block = false;           // the run ended with the frame's last block
  int sync();                            // wait, download per-frame results, compute timings
  int size_output();                     // after the scan: read the frames' sizes, size output + flatten scratch exactly (one host round trip)
  int launch_phase2();                   // the LZ77 stages (and, for literal-heavy submits, the Huffman streams in front of them)
  void launch_sweep(bool split, hipStream_t main = nullptr);   // main: the stream of the chain of steps (default: the engine's first)
  bool split_sweep = false;              // the last run used the split sweep: sync() checks that it was entitled to
  bool synced = false;                   // sync() ran after the last run(): outputs may be read
  uint32_t sweep_mode = 0;               // of the last run: 0 plain chain of steps, 1 split, 2 split and then repeated as a plain chain (tests)
  bool lit_direct() const { return (dev.flags & ZG_FLAG_LIT_DIRECT) != 0u; }   // the last run decoded its Huffman literals after the scan (tests)
  int read_output(uint64_t off, uint8_t* dst, uint64_t n);   // D2H
  int read_output_async(uint64_t off, uint8_t* dst, uint64_t n, hipStream_t s);
  const uint8_t* device_output() const { return dev.dst; }
  // The side passes of a finished submit (after sync()). Each is a launch / wait pair over a SidePass of its own: launch checks what the kernel
  // will read against the arrays it uploads (a range, segment, slice or slot that leaves them: ZGPU_E_INTERNAL, nothing launched), uploads its
  // tables, and enqueues ONE kernel between two HIP events; wait waits for the kernel's stream and gives *kernel_us, the time between the
  // events, and what the kernel left. No launch (n == 0, no bytes): wait gives zeros. What differs:
  //  - hash: XXH64 (seed 0) of the output bytes of frames[0 .. n) as sync() left them ([out_base, out_base + out_size): a failed frame's good
  //    blocks), one lane or one quad of lanes per frame (zg_k_xxh64 / zg_k_xxh64q: zg_launch_xxh64 chooses), on the first stream; digest i is
  //    frames[i]'s. quad_max_ranges: up to this many frames the launch is zg_k_xxh64q's whatever zg_launch_xxh64 would choose (0: its choice;
  //    the calls that carry ZGPU_DEVICE_VERIFY_SEEK_TABLE hash few mid-sized frames per range, LABNOTES.md "xxh64q").
  //  - scatter: zg_k_scatter (zg_scatter.h) copies segs[0 .. n) of the output to their destinations — device memory of the CALLER, which it
  //    has checked (zgpu_decode_frames_device) — on the second stream, beside the hash kernel. chunk: bytes per chunk of the plan (0:
  //    zgs::kChunkDefault). *launched: whether there was a kernel.
  //  - the two compares, between hash_launch and hash_wait: zg_k_seeksums (zg_seeksums.h) compares the Checksum fields of the seek tables of
  //    lanes[0 .. n) — whole entries in device memory of the CALLER, which it has checked — with the digests the hash kernel writes, for
  //    frames[0 .. nframes) (a lane's slice; Frame::slot: the index of the frame in hash_launch's list); zg_k_idxsums (zg_idxsums.h) takes the
  //    rows from a seek index handle's arrays instead — pairs[0 .. npairs) of 16 bytes, sums[0 .. nsums), device memory the handle owns, against
  //    which every lane's rows are checked as well — and reads no byte of an entry. Tables on the second stream, the kernel on the first behind
  //    the hash kernel: no wait in between. A submit may launch both; compare_wait(by_handle) writes record i of that route's lanes[i], *bytes
  //    = what came back.
  int hash_launch(const uint32_t* frames, uint32_t n, uint32_t quad_max_ranges = 0);
  int hash_wait(uint64_t* out, uint64_t* kernel_us = nullptr);
  int scatter_launch(const zgs::Seg* segs, uint32_t n, uint32_t chunk);
  int scatter_wait(uint64_t* kernel_us, bool* launched);
  int seeksums_launch(const zgv::Lane* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes);
  int idxsums_launch(const zgh::Lane* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes, const void* pairs, uint64_t npairs,
                     const uint32_t* sums, uint64_t nsums);
  int compare_wait(bool by_handle, zgv::Sums* out, uint64_t* kernel_us, uint64_t* bytes);
  //  - records (zg_records.h), THREE kernels and one round trip in between, all on the first stream: records_launch uploads the chunk table
  //    (every chunk checked against the output) and the frames' first chunks fstart[0 .. nframes] and enqueues zg_k_recs_count and
  //    zg_k_recs_scan; records_sizes waits and brings back *total, the bytes equal to d in all chunks, and ftot[f], those of the chunks
  //    [fstart[f], fstart[f + 1]) (8 + 8 * nframes bytes); records_emit enqueues zg_k_recs_emit, which stores `total` 64-bit offsets in
  //    chunk order into staging — device memory of the caller with room for them —; records_wait waits for it. *kernel_us: count + scan, and
  //    the emit. No launch (no chunk): zeros.
  int records_launch(const zgr::Chunk* chunks, uint32_t nchunks, const uint32_t* fstart, uint32_t nframes, uint32_t d);
  int records_sizes(uint64_t* total, uint64_t* ftot, uint64_t* kernel_us, uint64_t* bytes);
  int records_emit(uint64_t* staging, uint64_t total);
  int records_wait(uint64_t* kernel_us);
  // after sync(): free everything but the plaintext (a finished submit that waits to be read: zgpu_pool_decode_all)
  void release_scratch();
  // intermediates, for parity tests
  int read_block_status(std::vector<uint32_t>* out);
  int read_literals(uint32_t block, std::vector<uint8_t>* out);
  int read_sequences(uint32_t block, std::vector<ZgSeq>* seqs, ZgBlockSeqOut* so, ZgBlockPos* pos);
  int read_fse_slot(uint32_t slot, std::vector<uint32_t>* entries, uint8_t logs[4]);
  int read_huf_slot(uint32_t slot, std::vector<uint16_t>* entries, int* max_bits);
  int read_debug(uint64_t out[1024]);
  int read_scratch(int what, uint64_t off, void* dst, uint64_t n);   // what: 0 flatten scratch (u32 per output byte), 1 ZgUnitInfo[]
  int unit_scratch_base(uint32_t unit, uint64_t* base);              // word index of a unit's first byte in the flatten scratch

 private:
  friend class Engine;
  Engine* eng = nullptr;
  Scratch* sc = nullptr;
  ZgBatchDev dev{};
  std::vector<ZgSweepStep> sweep_steps;
  uint64_t og_words = 0;
  bool ran = false;
  uint32_t epoch_ = 0;                   // runs of this batch so far (the flatten's per-unit flags carry it)
  FrameState* fs = nullptr;              // streaming submit: the frame state this run reads from / writes into
  // The side passes, one SidePass each (a new one: a name here, its launch and wait; ~Batch releases them all). What the buffers hold — hash: the
  // ranges, then the digests; scatter, the two dictfill parts (0: tables, 1: contents) and the gather: the segments, then the chunk table;
  // the compares: the lanes, the frame list, then the records; records: the chunk table, fstart, then counts, prefixes and totals.
  enum { kSideHash, kSideScatter, kSideTable, kSideHandle, kSideFill0, kSideFill1, kSideGather, kSideRecords, kSideCount };
  SidePass side_[kSideCount];
  struct { uint32_t nframes = 0, d = 0; size_t counts = 0, prefix = 0, totals = 0; bool emitted = false; } rec_;   // the records pass in flight: where its arrays lie
  template <class L, class Launch> int compare_launch(SidePass& p, const L* lanes, uint32_t n, const zgv::Frame* frames, uint32_t nframes, Launch launch);
  std::vector<zgd::DictImage> frame_dicts_;   // set_frame_dicts
  int dictfill_launch(int part);
  std::vector<zgs::Seg> gather_segs_;    // Engine::upload with a gather: the entries' segments and their chunks (the tables travel from here)
  std::vector<zgs::Chunk> gather_chunks_;
};

class Engine {
 public:
  static int create(int device, Engine** out);
  ~Engine();
  uint64_t max_window = kDefaultMaxWindow;
  // Walk `len` bytes of concatenated frames (decode_all semantics, frame_decoder.rs:541-577), upload everything.
  int prepare(const uint8_t* src, size_t len, Batch** out);
  // n independent entries that lie back to back in src (entry i at off[i], len[i] bytes): each is walked on its own with decode_all's rule
  // (parse_frames), its frames appended to ONE submit. walk[i] = the entry's walk status, its frames are [first_frame[i], first_frame[i + 1]).
  // dicts: the lookup the walk resolves Dictionary_IDs with (zg_host_parse.h; nullptr: a dictionary frame ends its entry's walk)
  int prepare_entries(const uint8_t* src, size_t len, const uint64_t* off, const uint64_t* elen, uint32_t n, Batch** out,
                      std::vector<int>* walk, std::vector<uint32_t>* first_frame, const DictLookup* dicts = nullptr);
  // The same for entries whose compressed bytes lie in DEVICE memory of the caller (zgpu_decode_frames_device_src, which has checked every range
  // against the runtime's allocations). walk_entries: zg_k_walk (zg_walk.h) follows the header chain of all n entries in two lane passes, count
  // and emit, and brings back the skeleton: entry i's records are sk->recs[sk->first[i] .. sk->first[i + 1]), sk->ends[i] where its lane
  // stopped. An entry of length 0 is not read; the emit pass is skipped when no entry has a record; a lane that stops elsewhere in the emit
  // pass than in the count pass (a source that changed meanwhile) is ZG_INTERNAL.
  // prepare_entries_device: entries idx[0 .. n) of that skeleton parsed with the host's one walk (parse_frames_skel) into ONE submit, as
  // prepare_entries does with bytes; off[j] = where entry idx[j] lies in the submit's input (back to back, total bytes). The compressed bytes
  // reach the engine's source buffer by ONE zg_k_gather launch instead of the H2D copy; everything behind that is shared.
  struct DevEntry { uint64_t src, len; };
  struct Skeleton { std::vector<zgw::Rec> recs; std::vector<uint64_t> first; std::vector<zgw::End> ends; };
  int walk_entries(const DevEntry* e, uint32_t n, Skeleton* sk, uint64_t* stats);
  int prepare_entries_device(const DevEntry* e, const Skeleton& sk, const uint32_t* idx, const uint64_t* off, uint32_t n, size_t total, Batch** out,
                             std::vector<int>* walk, std::vector<uint32_t>* first_frame, const DictLookup* dicts = nullptr);
  // The lane passes: ONE launch over n lanes whose records come back to the host (lane_pass below is the one routine behind all of them, and
  // behind walk_entries' two). Every pass adds to stats[kPassLaunches], stats[kPassUs] (the kernel's time between two HIP events) and
  // stats[kPassBytes] (bytes downloaded); n == 0 is no pass at all, not even a hipSetDevice.
  // index_pass — what such entries hold, from their headers alone (zgpu_frames_index_device / zgpu_frames_table_device): zg_k_index
  // (zg_index.h). first == nullptr: the summary pass, out[i] = entry i's summary. Else the emit pass: sum = the summaries of the summary
  // pass, first[i] .. first[i + 1] (their prefix sum, n + 1 slots) the frame records lane i may write of recs[0 .. first[n]); out = what this
  // pass says about every entry (the caller compares). An entry of length 0 is not read.
  int index_pass(const DevEntry* e, uint32_t n, const uint64_t* first, const zgi::Entry* sum, zgi::Entry* out, zgi::FrameRec* recs, uint64_t* stats);
  // seek_pass — which whole frames of such entries hold a plaintext range (zgpu_frames_seek_device / zgpu_decode_ranges_device_src): zg_k_seek
  // (zg_seek.h), out[i] = lane i's record (64 bytes per lane come back). A lane of length 0 is not read.
  int seek_pass(const zgk::Lane* lanes, uint32_t n, zgk::Seek* out, uint64_t* stats);
  // seektab_pass — the same from the seekable format's seek table at each entry's end (zgpu_frames_seek_table_device /
  // zgpu_decode_ranges_seek_table_device_src): zg_k_seektab (zg_seektab.h), a wave per entry.
  int seektab_pass(const zgt::Lane* lanes, uint32_t n, zgk::Seek* out, uint64_t* stats);
  // seekmany_pass — m ranges over ne such entries, each table scanned ONCE (zgpu_frames_seek_table_many_device /
  // zgpu_gather_ranges_seek_table_device_src; zg_seekmany.h): a locate pass (one lane per entry; 32 bytes per entry come back, from which the
  // prefix scratch and the grids are sized), the two prefix launches, a find pass (one lane per range; out[j] = range j's record). ranges[j].entry
  // indexes e; a range of rlen 0 reads nothing. The scratch — 16 * (nframes + 1) bytes of prefixes per entry with a usable table, plus its
  // chunk totals — lives for the call; ZG_NOMEM if it cannot be had. locate's three kPass* slots go to stats, the rest to *more.
  struct ManyRange { uint64_t begin, rlen; uint32_t entry; };
  struct ManyStats { uint64_t prefix_launches = 0, prefix_us = 0, find_launches = 0, find_us = 0, scratch_bytes = 0; };
  int seekmany_pass(const DevEntry* e, uint32_t ne, const ManyRange* ranges, uint32_t m, zgk::Seek* out, uint64_t* stats, ManyStats* more);
  // The two halves of seekmany_pass, for a caller that keeps the pairs (zgpu_seek_index, zg_ranges.cpp). seekmany_prefixes: the locate pass
  // and the two prefix launches; loc[i] = what locate found of entry i, pre[i] = the index of its pair 0 in *scratch (usable tables only),
  // *npairs = the pairs of prefixes at the front of *scratch (the chunk totals lie behind them); the caller releases *scratch.
  // seekmany_find: ONE find launch over m lanes the caller laid out on `pairs`; its download is added to stats[kPassBytes] (stats may be null).
  int seekmany_prefixes(const DevEntry* e, uint32_t ne, zgm::Loc* loc, uint64_t* pre, DevBuf* scratch, uint64_t* npairs, uint64_t* stats, ManyStats* more);
  int seekmany_find(const zgm::Find* lanes, uint32_t m, const zgm::Pair* pairs, zgk::Seek* out, uint64_t* stats, ManyStats* more);
  // seekidx_rows_pass — the same pairs from the header chain of entries that declare their sizes (zg_seekidx.h): zg_k_seekidx_rows, one lane
  // per entry, stores into pairs[lanes[i].pre .. + lanes[i].limit] (device memory of the caller); out[i] = what lane i found.
  int seekidx_rows_pass(const zgx::Lane* lanes, uint32_t n, zgm::Pair* pairs, zgx::Rows* out, uint64_t* stats);
  // records_find — m record ranges looked up in a seek index handle's record offsets (zg_records.h): zg_k_recs_find, one lane per range, ONE
  // launch; recs: the handle's array (device memory the handle owns; the caller checked every lane's rpre + nrec against it), out[j] = lane
  // j's 24-byte answer.
  int records_find(const zgr::Find* lanes, uint32_t m, const uint64_t* recs, zgr::Found* out, uint64_t* stats);
  // fill_pass — `byte` into the n regions (zgs::Seg, src_off unused) of device memory the CALLER checked, region by region, against the one
  // piece they lie in (zg_scatter.h: zg_k_fill): the regions and their chunk table go up, ONE launch between two HIP events, the stream is
  // drained. stats[kPassBytes] counts the bytes FILLED (nothing comes back). Regions of length 0 only: no pass at all.
  int fill_pass(const zgs::Seg* regions, uint32_t n, uint32_t byte, uint64_t* stats);
  // hash_ranges_pass — XXH64 of ranges[0 .. n) of base (device memory the caller has checked) by the hash kernel `kernel` chooses
  // (zg_launch_xxh64_with); digests[i] is ranges[i]'s (zgpu_debug_hash_ranges).
  int hash_ranges_pass(const uint8_t* base, const ZgHashRange* ranges, uint32_t n, int kernel, uint64_t* digests, uint64_t* stats);
  // Same for a run of blocks of ONE frame that starts at a block header (the FrameDecoder mirror parsed the frame
  // header itself). *consumed = bytes of the run (block headers, bodies, checksum).
  // max_blocks: 0 = up to the last block of the frame. fs carries the frame's state across calls; keep = frame bytes
  // that must stay reachable (FrameState::make_room).
  // side: the run in front (of the same frame) is still on the GPU — this run's bytes and tables travel on the upload stream beside it and its run()
  // waits for them; carry_mask_now: the tables that will exist when it starts (Batch::carry_mask_after of the run in front), fs->carry_mask if null
  int prepare_run(const uint8_t* src, size_t len, FrameState* fs, bool has_checksum, uint32_t max_blocks, uint64_t keep, Batch** out, size_t* consumed,
                  bool side = false, const uint32_t* carry_mask_now = nullptr);
  // Same for blocks whose 3-byte headers the CALLER parsed (the thin boundary: ruzstd keeps read_block_header,
  // block_decoder.rs:201-247): hb[i] describes Block_Content i inside src. The run ends with the first block marked last.
  struct HostBlock { uint64_t src_off; uint32_t src_len; uint32_t raw_rle_size; uint8_t type; uint8_t last; };
  int prepare_blocks(const uint8_t* src, size_t len, const HostBlock* hb, size_t n, FrameState* fs, uint64_t keep, Batch** out);
  hipStream_t stream() const { return stream_; }
  hipStream_t copy_stream() const { return stream2_; }
  hipStream_t download_stream() const { return stream3_; }
  hipStream_t download_stream2() const { return stream5_; }  // the second half of a large download (two copy engines instead of one: zg_stream.cpp)
  hipStream_t upload_stream() const { return stream4_; }     // uploads of a run that is prepared while the run in front is on the GPU (prepare_run side = true)
   // D2H of a finished submit while the next one runs (zgpu_pool_decode_all): nothing else uses it then
  int device() const { return device_; }
  int compute_units() const { return cus_; }
  const Tuning& tuning() const { return tn_; }
  std::string last_error;

 private:
  friend class Batch;
  int device_ = 0;
  int cus_ = 256;                // compute units of the device (MI355X: 256)
  Tuning tn_;                    // the ZGPU_* switches as they were when the engine was created
  bool no_presize_ = false;      // (ZGPU_PRESIZE=0: measurement / tests) never size the output before the run
  int flat_shape_ = 0;           // zg_k_flatten shape: 0 = 1024 threads x 16 KiB tiles (one workgroup per CU), 1 = 512 x 8 KiB (two)
  hipStream_t stream_ = nullptr, stream2_ = nullptr, stream3_ = nullptr, stream4_ = nullptr, stream5_ = nullptr;   // stream3_: the flatten, when the sweep chain runs beside it
  std::vector<Scratch*> free_;   // finished submits' buffers, for reuse
  Scratch* acquire();
  void recycle(Scratch* s);
  int fail(hipError_t e, const char* what);
  // One lane pass on the first stream: t's buffers reserved (they and its two events are reused by a second pass of the same call; LaneTmp is a
  // SidePass with the two download buffers), lane_bytes of lanes uploaded and the stream synchronised (the lane array is pageable), event,
  // launch(t, stream), hipGetLastError, event, out — and
  // extra, the second array of an emit pass, if it has a host side — downloaded, the stream synchronised, the three kPass* slots of stats added to.
  struct LaneTmp;
  struct Down { void* host = nullptr; size_t bytes = 0; };   // bytes of a device array (LaneTmp::out / extra) that come back to host
  template <class Launch> int lane_pass(LaneTmp& t, const void* lanes, size_t lane_bytes, Down out, Down extra, uint64_t* stats, Launch launch);
  struct GatherPlan { const DevEntry* e; const uint32_t* idx; const uint64_t* off; uint32_t n; };
  // g: the len bytes come from device memory, entry g->idx[j] to offset g->off[j], by one zg_k_gather launch (src is not looked at)
  int upload(Batch* b, const uint8_t* src, size_t len, Batch** out, bool side = false, const GatherPlan* g = nullptr);
};

// (parse_frames, split_frames and plaintext_bound: zg_host_parse.h)
int parse_block_run(const uint8_t* src, size_t len, uint64_t window, bool has_checksum, const uint32_t hist[3], uint32_t carry_mask,
                    uint32_t max_blocks, BatchBuilder* bb, std::vector<FrameInfo>* info, size_t* consumed, bool* saw_last);

}  // namespace zg
