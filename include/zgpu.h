/*
 * zgpu.h — C ABI of the MI355X-native zstd block-decode engine (libzgpu.so).
 *
 * This is the drop-in boundary for the reference's block-decode path. The reference (KillingSpark/zstd-rs,
 * crate ruzstd 0.9.1) has no FFI of its own; the seam this library replaces is
 *     BlockDecoder::decode_block_content          ruzstd/src/decoding/block_decoder.rs:39-95
 * as called from FrameDecoder::decode_blocks        ruzstd/src/decoding/frame_decoder.rs:338-340
 * and FrameDecoder::decode_from_to                  ruzstd/src/decoding/frame_decoder.rs:495-501,
 * together with the state it mutates (DecoderScratch, ruzstd/src/decoding/scratch.rs:15-27).
 * Because one launch per block would be ~7.6 K launches for enwik9, the ABI is batched: the host walks the
 * 3-byte block headers and hands over whole runs of blocks (INTEGRATION.md shows the Rust-side binding).
 *
 * All functions return 0 on success or a positive zgpu status (values below); nothing throws or unwinds across
 * the boundary; pointers are plain host pointers unless a name says "device". There is no CPU fallback: without
 * a usable gfx950 device zgpu_ctx_create fails with ZGPU_E_HIP.
 */
#ifndef ZGPU_H
#define ZGPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Status codes: leaves of the reference's error enums (ruzstd/src/decoding/errors.rs). */
enum zgpu_status {
  ZGPU_OK = 0,
  ZGPU_E_SKIP_FRAME = 1,              /* ReadFrameHeaderError::SkipFrame                errors.rs (frame.rs:15-23) */
  ZGPU_E_BAD_MAGIC = 2,               /* ReadFrameHeaderError::BadMagicNumber */
  ZGPU_E_HEADER_READ = 3,             /* ReadFrameHeaderError::*ReadError */
  ZGPU_E_WINDOW_TOO_BIG_SPEC = 4,     /* FrameHeaderError::WindowTooBig */
  ZGPU_E_WINDOW_TOO_SMALL = 5,        /* FrameHeaderError::WindowTooSmall */
  ZGPU_E_WINDOW_SIZE_TOO_BIG = 6,     /* FrameDecoderError::WindowSizeTooBig */
  ZGPU_E_DICT_NOT_PROVIDED = 7,       /* FrameDecoderError::DictNotProvided */
  ZGPU_E_NOT_INITIALIZED = 8,         /* FrameDecoderError::NotYetInitialized */
  ZGPU_E_FAILED_READ_BLOCK_HEADER = 9,
  ZGPU_E_FAILED_READ_BLOCK_BODY = 10,
  ZGPU_E_FAILED_READ_CHECKSUM = 11,
  ZGPU_E_TARGET_TOO_SMALL = 12,
  ZGPU_E_FAILED_SKIP_FRAME = 13,
  ZGPU_E_RESERVED_BLOCK = 20,         /* BlockHeaderReadError::FoundReservedBlock */
  ZGPU_E_BLOCK_SIZE_TOO_LARGE = 21,   /* BlockSizeError::BlockSizeTooLarge */
  ZGPU_E_MALFORMED_SECTION_HEADER = 22, /* DecompressBlockError::MalformedSectionHeader */
  ZGPU_E_LITERALS_HEADER = 23,        /* LiteralsSectionParseError */
  ZGPU_E_SEQUENCES_HEADER = 24,       /* SequencesHeaderParseError */
  ZGPU_E_LIT_UNINIT_HUF = 30,         /* DecompressLiteralsError::UninitializedHuffmanTable */
  ZGPU_E_LIT_MISSING_JUMP = 31,
  ZGPU_E_LIT_MISSING_BYTES = 32,
  ZGPU_E_LIT_EXTRA_PADDING = 33,
  ZGPU_E_LIT_BITSTREAM_MISMATCH = 34,
  ZGPU_E_LIT_COUNT_MISMATCH = 35,
  ZGPU_E_HUF_TABLE = 36,              /* HuffmanTableError::* */
  ZGPU_E_FSE_TABLE = 40,              /* FSETableError::* */
  ZGPU_E_FSE_UNINIT = 41,             /* FSEDecoderError::TableIsUninitialized */
  ZGPU_E_SEQ_MISSING_MODE = 42,
  ZGPU_E_SEQ_RLE_BYTE = 43,
  ZGPU_E_SEQ_EXTRA_PADDING = 44,
  ZGPU_E_SEQ_UNSUPPORTED_OFFSET = 45,
  ZGPU_E_SEQ_NOT_ENOUGH_BYTES = 46,
  ZGPU_E_SEQ_EXTRA_BITS = 47,
  ZGPU_E_EXE_NOT_ENOUGH_LITERALS = 50, /* ExecuteSequencesError::NotEnoughBytesForSequence */
  ZGPU_E_EXE_ZERO_OFFSET = 51,
  ZGPU_E_EXE_OFFSET_TOO_BIG = 52,     /* DecodeBufferError::OffsetTooBig */
  ZGPU_E_EXE_DICT_TOO_SMALL = 53,
  ZGPU_E_DICT_DECODE = 60,
  /* No counterpart in the reference, which never enforces a Content_Checksum (libzstd does: its checksum_wrong). Only an entry of
   * zgpu_decode_frames_device / zgpu_decode_frames_device_src called with ZGPU_DEVICE_VERIFY gets it: the entry decoded, and the XXH64 of a
   * frame's plaintext differs from the checksum stored in the frame. */
  ZGPU_E_CHECKSUM_MISMATCH = 70,
  /* No counterpart in the reference, which never compares a frame's length with its Frame_Content_Size (libzstd does: its corruption_detected /
   * srcSize_wrong). Only an entry of zgpu_decode_ranges_device_src gets it: a frame of the selection declares a size and decoded to another
   * length, so the plaintext coordinates the range was asked in do not hold. */
  ZGPU_E_CONTENT_SIZE_MISMATCH = 71,
  /* No counterpart in the reference, which knows no seekable format. Only an entry of zgpu_frames_seek_table_device /
   * zgpu_decode_ranges_seek_table_device_src gets it: the entry does not end in a usable seek table; zgpu_seek.why (ZGPU_SEEKTAB_*) says why. */
  ZGPU_E_SEEK_TABLE = 72,
  /* No counterpart in the reference (libzstd's seekable reader has it: its corruption_detected on a frame checksum). Only an entry of
   * zgpu_decode_ranges_seek_table_device_src called with ZGPU_DEVICE_VERIFY_SEEK_TABLE gets it: the entry decoded, and its seek table does not
   * vouch for the bytes — a frame's XXH64 differs from the table's Checksum, a decoded frame matches no table row, or the table has no checksums. */
  ZGPU_E_SEEK_CHECKSUM_MISMATCH = 73,
  /* No counterpart in the reference. Only an entry of a zgpu_seek_index, and the ranges that name it, get it: the entry's header chain yields
   * no index; zgpu_seek_index_info.why says why — a ZGPU_CHAIN_* reason (the chain broke), ZGPU_INDEX_UNSIZED (a zstd frame declares no
   * Frame_Content_Size) or ZGPU_SEEKTAB_TOO_LARGE (more than 2^27 rows). */
  ZGPU_E_FRAME_INDEX = 74,
  /* Input the reference tolerates but this engine rejects. No conforming encoder produces any of it:
   *  - offsets >= 2^30 (offset codes 30, 31) while >= 1 GiB of the frame is held undrained (FrameDecoder::decode_blocks(All) on a
   *    frame beyond 1 GiB that nobody reads from): ZGPU_E_UNSUPPORTED. With less than 1 GiB held — always the case in decode_all
   *    and the streaming decoder — such an offset fails in the reference too, and with the same error here;
   *  - a block that regenerates >= 2^31 bytes: ZGPU_E_UNSUPPORTED.
   * (Round 5 listed a third case: decode_all on a frame WITH a dictionary that holds more than 1 MiB of raw / RLE output in front of a
   *  match that starts in the dictionary — the reference has drained bytes inside that call, frame_decoder.rs:560-563, and splices the
   *  dictionary's tail with the oldest byte it still holds, which one submit that keeps every byte in place cannot serve. zgpu_decode_all
   *  now decodes such a frame a second time on the reference's own schedule, rounds of UptoBytes(1 MiB) + read(), and returns its bytes.)
   * (Rounds 2-4 listed another case here: a match that starts in the dictionary and continues BEHIND bytes the caller has drained — the
   *  reference splices the dictionary's tail with the oldest byte it still holds, decode_buffer.rs:159-163. Since round 5 the device
   *  window of a frame with a dictionary is laid out like the reference's buffer, [dictionary content][undrained bytes], and the match
   *  yields the reference's bytes.)
   * Blocks regenerating more than 128 KiB (beyond Block_Maximum_Size) are decoded, by the in-order kernel, and fail with the
   * reference's own error leaf (the exact buffer bookkeeping of zg_exact.h covers them since round 4). */
  ZGPU_E_UNSUPPORTED = 80,
  ZGPU_E_INTERNAL = 90,               /* where the reference would panic */
  ZGPU_E_NOMEM = 91,
  ZGPU_E_HIP = 92,                    /* HIP runtime error / no device */
  ZGPU_E_BAD_ARG = 93
};

typedef struct zgpu_ctx zgpu_ctx;         /* one per (GPU, HIP stream); not thread-safe, may move between threads */
typedef struct zgpu_batch zgpu_batch;     /* one submit: a run of whole frames, parsed and resident on the device */
typedef struct zgpu_decoder zgpu_decoder; /* mirror of ruzstd's FrameDecoder for one frame at a time */

/* ---- context -------------------------------------------------------------------------------------------
 * Threads. Distinct contexts, and everything made from them, may be used from distinct threads at once. One context together with its
 * decoders, streams, batches and seek indexes is one thread's at a time: no two calls on any of them may overlap, and the library takes no
 * lock for them. Between calls these objects may change threads, and they may be destroyed on any thread. What the process shares — the
 * caches behind the streams — is locked inside the library; zgpu_release_caches must be called only while no stream is in a call. */
int zgpu_ctx_create(int device_id, zgpu_ctx** out);                 /* ~ FrameDecoder::new  frame_decoder.rs:158 */
void zgpu_ctx_destroy(zgpu_ctx*);
void zgpu_set_max_window_size(zgpu_ctx*, uint64_t max_window_size); /* frame_decoder.rs:175 (clamped to the format maximum) */
uint64_t zgpu_max_window_size(const zgpu_ctx*);                     /* frame_decoder.rs:180 */
const char* zgpu_last_error(const zgpu_ctx*);
const char* zgpu_status_name(int status);

/* ---- FrameDecoder::decode_all (frame_decoder.rs:541-577) -------------------------------------------------
 * src holds concatenated frames (skippable frames are skipped); the plaintext of all frames is written back to
 * back into dst. ZGPU_E_TARGET_TOO_SMALL if it does not fit. H2D + kernels + D2H.
 * An input with several defects returns the error the reference meets FIRST in stream order (it decodes block by block,
 * frame_decoder.rs:319-375): a defect inside a block comes before a header further back that cannot be read, a block's
 * literals before its sequences, an earlier stream / sequence before a later one — whichever of them the engine's stages
 * find first. */
int zgpu_decode_all(zgpu_ctx*, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, size_t* written);
/* decode_all_to_vec (frame_decoder.rs:591-610): the library sizes the output (exactly: the size of every frame is known on
 * the host before the LZ77 stages run). *out is malloc'ed; release it with zgpu_free. */
int zgpu_decode_all_alloc(zgpu_ctx*, const uint8_t* src, size_t len, uint8_t** out, size_t* written);
void zgpu_free(void*);

/* ---- decode_all over many independent buffers in few submits --------------------------------------------------------------
 * One zgpu_decode_all call lasts as long as one block's sequence chain plus its launches and copies (~1.6 ms host to host for a 128 KiB frame)
 * whatever it holds; a caller with many small buffers hands them over together. Entry i is srcs[i] (lens[i] bytes: frames back to back, skippable
 * frames allowed — what decode_all takes), its plaintext goes to dsts[i] (caps[i] bytes). Entries are walked one by one and their frames decoded
 * together in submits of at most 512 MiB of plaintext (an entry is never split); results[i] is what zgpu_decode_all of entry i ALONE would give
 * — it does not depend on the other entries or on their order. The return value reports engine failures only (BAD_ARG, NOMEM, HIP). */
typedef struct {
  uint64_t written;              /* bytes written to dsts[i]; 0 unless status == 0 */
  int32_t status;                /* what zgpu_decode_all(ctx, srcs[i], lens[i], dsts[i], caps[i], &w) returns */
  uint32_t nframes;              /* frames decoded in the entry (skippable frames not counted); 0 unless status == 0 */
  /* the content checksums, reported, never enforced (the reference checks them neither in decode_all nor in its CLI): 0 unless status == 0 */
  uint32_t checksums;            /* of those frames, the ones that carry a Content_Checksum */
  uint32_t checksum_mismatches;  /* of those, the ones whose XXH64 (seed 0, low 32 bits) of the decoded bytes differs from it */
  uint32_t checksum_from_data;   /* the entry's first frame: FrameDecoder::get_checksum_from_data (frame_decoder.rs:254), 0 if absent */
  uint32_t calculated_checksum;  /* the entry's first frame: get_calculated_checksum (frame_decoder.rs:263-270); 0 if the entry has no frame */
} zgpu_entry_result;
/* Submits hold at most 512 MiB of plaintext (bounded from the headers) and 512 MiB of input. A submit's frames are hashed on the device (one lane
 * per frame) when an estimate says that beats the host's copy threads (up to 16) — many short frames —, else on the host, from the bytes that come
 * back anyway. (An Unsupported / Internal verdict of the one-submit path is decoded again alone; should the checksums of such an entry not be
 * computable, it reports its frames with checksums = checksum_mismatches = checksum_from_data = calculated_checksum = 0.) */
int zgpu_decode_frames(zgpu_ctx*, const uint8_t* const* srcs, const size_t* lens, uint32_t n, uint8_t* const* dsts, const size_t* caps,
                       zgpu_entry_result* results);
/* An upper bound of the plaintext of src (concatenated frames) from frame and block headers only — a frame's declared content size when smaller,
 * 128 KiB per compressed block; the walk stops where a header cannot be read. What zgpu_decode_frames cuts its submits by; a caller may size
 * caps[i] with it. Host only. */
uint64_t zgpu_plaintext_bound(const uint8_t* src, size_t len);
/* diagnostics: the submits the context's last zgpu_decode_frames / zgpu_decode_frames_device / zgpu_decode_frames_device_src call ran */
uint32_t zgpu_debug_frames_submits(const zgpu_ctx*);

/* ---- the same, with the plaintext left in device memory the caller owns ------------------------------------------------------
 * For callers that want the plaintext ON the GPU (compressed shards headed for tensors, columnar pages headed for a GPU query): no download,
 * no host copy, no upload of the caller's own. srcs are HOST pointers (compressed input that is already device-resident: the call below).
 * device_dsts[i] is device memory on the context's device (a hipMalloc'ed
 * block or any part of one, e.g. a torch tensor's data_ptr()), caps[i] bytes, at any alignment.
 *  - results[i].r.status / .written / .nframes are what zgpu_decode_frames reports for the same entries: what zgpu_decode_all of entry i ALONE
 *    returns, independent of the other entries and of their order. On status 0 the first `written` bytes of device_dsts[i] are the plaintext.
 *    No byte of a FAILED entry's destination is written, and no byte at or behind device_dsts[i] + written ever is.
 *  - Before any kernel is launched every destination is checked with the HIP runtime (hipPointerGetAttributes, hipMemGetAddressRange): device
 *    memory (not host, not managed), on the context's device, [dst, dst + caps[i]) inside ONE allocation. An entry that fails the check gets
 *    ZGPU_E_BAD_ARG and takes no part in any launch; the other entries are unaffected. (caps[i] == 0: nothing is written, nothing is checked.)
 *    A wrong pointer becomes a status, never a GPU fault.
 *  - The call returns after the engine's streams are synchronised: every later operation on any stream sees the bytes. The caller guarantees
 *    that nothing in flight touches the destinations during the call (memory of a stream-ordered allocator: synchronise that stream first).
 *    Overlapping destinations are undefined.
 *  - Submits are cut as zgpu_decode_frames cuts them (512 MiB of plaintext bound and of input; zgpu_debug_frames_submits counts them). A submit's
 *    plaintext lies back to back in the engine's output; ONE kernel launch per submit (zg_k_scatter) copies the frames of every successful entry
 *    to their destinations.
 *  - Entries the one-submit path does not serve — dictionary frames while dictionaries are registered, Unsupported / Internal verdicts — are
 *    decoded again alone, as by zgpu_decode_frames, into a host buffer and then copied to the destination with one H2D (rare; correct first).
 *  - Checksums: the bytes never reach the host, so frames are hashed on the device only (zg_k_xxh64, one lane per frame, ~226 MB/s per lane;
 *    zg_k_xxh64q, four lanes per frame and ~1.1 - 1.4 GB/s per frame, is the choice of the calls that carry ZGPU_DEVICE_VERIFY_SEEK_TABLE only:
 *    LABNOTES.md "xxh64q").
 *    r.checksums counts the frames that carry a Content_Checksum, r.checksum_mismatches only those among the HASHED frames; the rest are
 *    counted in checksums_unverified. By default nothing fails on a mismatch, as in the reference, and the scatter runs beside the hash: a
 *    corrupted frame's bytes are in the destination when the caller reads the counter. (Entries decoded alone are hashed on the host,
 *    whatever their length.)
 *  - ZGPU_DEVICE_VERIFY (flags bit 1) makes a mismatch the entry's verdict, as libzstd does. Every frame that carries a Content_Checksum is
 *    then hashed, whatever its length (hash_max_bytes == 0 means NO limit under this flag; a nonzero value still bounds what is hashed, and
 *    longer frames pass, counted in checksums_unverified; frames without a checksum are hashed as without the flag). An entry that would have
 *    had status 0 and holds a hashed frame whose low 32 digest bits differ from its stored checksum gets ZGPU_E_CHECKSUM_MISMATCH instead:
 *    written = nframes = 0 like any failed entry, and NO byte of its destination is written — a submit's digests are waited for before its
 *    scatter list is built. r.checksums and r.checksum_mismatches of such an entry are still filled (all its frames that carry a checksum /
 *    those that failed), so the caller sees which count failed; every other field is 0. The verdict ranks behind all others: a decode
 *    error, a walk error, TARGET_TOO_SMALL and BAD_ARG are reported exactly as without the flag. Other entries are unaffected, in any order.
 *    Entries decoded alone are hashed on the host and compared before their one H2D, with the same verdict. What it costs: the scatter no
 *    longer overlaps the hash, and a frame is hashed at a lane group's rate — one lane's today: a 64 MiB frame takes ~0.3 s, tens of
 *    milliseconds even with four lanes —, hidden only when many frames are hashed side by side (LABNOTES.md "xxh64q"); a nonzero
 *    hash_max_bytes bounds it.
 *    Bit 1 together with bit 0 is a contradiction: the call returns ZGPU_E_BAD_ARG and launches nothing. */
#define ZGPU_DEVICE_NO_HASH 1u
#define ZGPU_DEVICE_VERIFY 2u
#define ZGPU_DEVICE_VERIFY_SEEK_TABLE 4u   /* the two decode calls that have a seek table only — zgpu_decode_ranges_seek_table_device_src (see there) and
                                              zgpu_gather_ranges_seek_table_device_src; ZGPU_E_BAD_ARG on every other call */
typedef struct {
  uint64_t hash_max_bytes;   /* frames whose plaintext is at most this long are hashed on the device; longer ones are not hashed.
                                0: default 4 MiB — except under ZGPU_DEVICE_VERIFY, where 0 means no limit for frames that carry a checksum */
  uint32_t flags;            /* bit 0 (ZGPU_DEVICE_NO_HASH): hash no frame at all; bit 1 (ZGPU_DEVICE_VERIFY): a checksum mismatch fails the
                                entry with ZGPU_E_CHECKSUM_MISMATCH and nothing of it is written; bit 2 (ZGPU_DEVICE_VERIFY_SEEK_TABLE): the seek table's
                                checksums are enforced (the calls that have a seek table only), hash_max_bytes == 0 means no limit */
  uint32_t pad;
} zgpu_device_opts;
typedef struct {
  zgpu_entry_result r;            /* exactly the fields and meanings of zgpu_decode_frames, except as said above */
  uint32_t checksums_unverified;  /* frames that carry a Content_Checksum and were not hashed (too long / hashing off) */
  uint32_t first_hashed;          /* 1 if r.calculated_checksum is the first frame's real XXH64, 0 if it was not hashed (then 0) */
} zgpu_device_entry_result;
int zgpu_decode_frames_device(zgpu_ctx*, const uint8_t* const* srcs, const size_t* lens, uint32_t n, void* const* device_dsts, const size_t* caps,
                              const zgpu_device_opts* opts_or_null, zgpu_device_entry_result* results);
/* diagnostics: the context's last zgpu_decode_frames_device call — out[0] submits, [1] scatter launches, [2] bytes scattered, [3] scatter kernel
 * microseconds (HIP events), [4] frames hashed, [5] frames not hashed, [6] entries that were decoded alone, [7] entries failed by
 * ZGPU_DEVICE_VERIFY, [8] hash kernel microseconds (HIP events, summed over the submits). Returns how many were written. */
int zgpu_debug_frames_device_stats(const zgpu_ctx*, uint64_t* out, int n);
/* measurement and tests: XXH64 (seed 0) of n ranges [device_base + offs[i], + lens[i]) of the caller's device memory by the hash kernels of
 * the calls above. kernel 0: the library's choice for n ranges, 1: zg_k_xxh64 (one lane per range), 4: zg_k_xxh64q (four lanes per range).
 * [device_base, device_base + max(offs[i] + lens[i])) passes the pointer check that device sources pass, before anything is launched: else
 * ZGPU_E_BAD_ARG. No lane reads a byte outside its range. The ranges are sorted longest first internally, as the engine sorts a submit's
 * frames; digests[i] belongs to range i in the caller's order. zgpu_debug_hash_ranges_us: the kernel's time in the last call (HIP events). */
int zgpu_debug_hash_ranges(zgpu_ctx*, const void* device_base, const uint64_t* offs, const uint64_t* lens, uint32_t n, int kernel,
                           uint64_t* digests);
uint64_t zgpu_debug_hash_ranges_us(const zgpu_ctx*);
/* tests: ONE of the primitives the kernel bodies are written against (zstd-rs_amd/csrc/zg_zxprobe.h names them: op, the operand words in[8 t ..]
 * of thread t, the result words out[4 t ..]) on one workgroup of `threads` threads, so that the CPU emulator the suites run those bodies on can be
 * held against the hardware. out[] goes up as the caller filled it and comes back with the words the threads wrote; arena_in goes up as the
 * kernel's memory arena and comes back whole in arena_out. The buffer resource is [res_off, res_off + res_bytes) of the arena, or with flags = 1
 * (res_off = res_bytes = 0) a resource of 0 bytes over a null base. Refused with ZGPU_E_BAD_ARG before any HIP call: threads other than 64 or
 * 256; an arena below 512 bytes, above 1 MiB or no multiple of 16; a resource with less than 256 bytes of arena on either side; a buffer offset
 * at or above 0x80000040; an index of a global store, load or atomic outside the arena or misaligned for its width; an LDS word >= 64. */
int zgpu_debug_zx_probe(zgpu_ctx*, uint32_t op, uint32_t threads, uint32_t flags, uint32_t res_off, uint32_t res_bytes, const uint32_t* in,
                        uint32_t* out, const uint8_t* arena_in, uint8_t* arena_out, uint32_t arena_bytes);

/* ---- the same, with the compressed input in device memory too ------------------------------------------------------------------
 * For callers whose compressed bytes are in HBM already (a GPUDirect / RDMA read, a torch tensor loaded from a sharded checkpoint, the output of
 * an earlier GPU stage): no download of the caller's, no staging copy, no upload. device_srcs[i] is device memory on the context's device,
 * lens[i] bytes at any alignment; everything else is zgpu_decode_frames_device.
 *  - results[i] equals, field for field, what zgpu_decode_frames_device reports for a host copy of the same bytes with the same destinations
 *    and options, and so do the destination bytes. Every guarantee of that call holds: entries are isolated and their order does not matter,
 *    nothing of a failed entry and nothing at or behind dst + written is written, submits are cut the same way (zgpu_debug_frames_submits gives
 *    the same count), the hash rule is the same, the engine's streams are synchronised on return.
 *  - The host still owns every verdict, the table lineage and the launch plan. It reads a skeleton instead of the bytes: one lane per entry
 *    follows the header chain on the device (zg_k_walk, two launches for the whole call) and 32 bytes per frame header, block and checksum
 *    come back; the host's one parse runs over those records. A submit's entries reach the engine's input buffer by ONE kernel launch
 *    (zg_k_gather).
 *  - Every source passes the check the destinations pass, before anything is launched: device memory (not host, not managed), on the
 *    context's device, [src, src + lens[i]) inside ONE allocation; else that entry gets ZGPU_E_BAD_ARG and the others are unaffected.
 *    lens[i] == 0: nothing is checked, nothing is read.
 *  - The library never writes to a source and no lane reads a byte outside [src, src + lens[i]), not even inside the same allocation: an
 *    entry may end flush with its allocation. A source that overlaps a destination is undefined. The caller guarantees that nothing in
 *    flight writes the sources during the call.
 *  - Entries the one-submit path does not serve (dictionary frames while dictionaries are registered, Unsupported / Internal verdicts) are
 *    downloaded, one D2H each, and decoded alone as by zgpu_decode_frames_device (rare; correct first). */
int zgpu_decode_frames_device_src(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, void* const* device_dsts,
                                  const size_t* caps, const zgpu_device_opts* opts_or_null, zgpu_device_entry_result* results);
/* diagnostics: the context's last zgpu_decode_frames_device_src call — out[0] walk launches, [1] walk kernel microseconds (HIP events), [2] skeleton
 * bytes downloaded, [3] gather launches, [4] gather kernel microseconds, [5] input bytes that crossed to the host (entries decoded alone only).
 * zgpu_debug_frames_device_stats is filled by that call as well. Returns how many were written. */
int zgpu_debug_frames_device_src_stats(const zgpu_ctx*, uint64_t* out, int n);

/* ---- dictionary frames inside the shared submits of the three calls above ---------------------------------------------------------------------
 * Dictionaries are how many small buffers are compressed well (one trained dictionary, thousands of short records), and by default every entry
 * that holds a dictionary frame is decoded alone: a submit per frame at least, a D2H of the entry for device-resident sources.
 * zgpu_set_frames_shared_dicts(ctx, 1): dictionary frames whose id is registered (zgpu_add_dict) join the shared submits of zgpu_decode_frames,
 * zgpu_decode_frames_device and zgpu_decode_frames_device_src. 0 (the default): they are decoded alone, as before — every call then behaves byte
 * for byte and counter for counter as it did without the switch.
 *  - The contract of each call is unchanged: results[i] is what zgpu_decode_all of entry i ALONE returns; entries are isolated and their order
 *    does not matter; nothing of a failed entry and nothing at or behind dst + written is written; the hash rule and the synchronisation on
 *    return are the same. With device-resident sources no byte of a shared entry's input crosses to the host.
 *  - In the submit's output a dictionary frame takes [gap of the dictionary's content length][its plaintext]; the dictionary's one device copy
 *    per context (uploaded at first use, freed with the context, replaced when zgpu_add_dict replaces the dictionary) is replicated into the
 *    gaps and into the frames' table slots by zg_k_dictfill: two launches per submit that holds dictionary frames — the tables in front of the
 *    entropy stages, the contents once the frames' sizes have placed the gaps.
 *  - The submit cut counts a dictionary frame's content length towards the 512 MiB plaintext budget, so zgpu_debug_frames_submits may differ
 *    from the same call with the switch off. zgpu_plaintext_bound, and with it the room a caller needs, does not change.
 *  - Still decoded alone, with today's answers: an entry with a frame whose id is not registered (ZGPU_E_DICT_NOT_PROVIDED — or, if the
 *    window is refused first, ZGPU_E_WINDOW_SIZE_TOO_BIG), a dictionary without content, and an entry whose shared verdict is Unsupported /
 *    Internal: a match into the dictionary behind a drain that falls inside decode_all (more than 1 MiB of one frame in front of it). */
void zgpu_set_frames_shared_dicts(zgpu_ctx*, int on);
int zgpu_frames_shared_dicts(const zgpu_ctx*);
/* diagnostics: the context's last zgpu_decode_frames / _device / _device_src call — out[0] dictionary frames decoded inside shared submits (of
 * entries that succeeded), [1] zg_k_dictfill launches, [2] dictionary bytes replicated (contents and tables), [3] fill kernel microseconds
 * (HIP events), [4] entries with a dictionary frame that still went alone. All 0 with the switch off. Returns how many were written. */
int zgpu_debug_frames_dict_stats(const zgpu_ctx*, uint64_t* out, int n);

/* ---- what device-resident compressed input holds: bounds and frame tables without a download -----------------------------------------------
 * zgpu_decode_frames_device_src needs caps[i], and zgpu_plaintext_bound reads host memory. These calls answer the sizing question — and how many
 * frames an entry has, where they start, which declare a content size, name a dictionary or carry a checksum — for entries that lie in device
 * memory, from frame and block headers alone: one lane per entry follows the header chain on the device (zg_k_index) and reads three bytes per
 * block, never a block body; a fixed-size summary per entry (and, for the table, a record per frame) comes back, no byte of the input does.
 *  - Sources pass the check of zgpu_decode_frames_device_src before anything is launched; an entry that fails gets ZGPU_E_BAD_ARG in
 *    entries[i].status, every other field 0, and the others are unaffected. lens[i] == 0 is neither checked nor read.
 *  - No lane reads a byte outside [src, src + lens[i]) — an entry may end flush with its allocation — and nothing is written to a source. The
 *    caller guarantees that nothing in flight writes the sources during the call.
 *  - The calls return with the engine's streams synchronised; the return value reports engine failures only. Results do not depend on the order
 *    of the entries.
 *  - What the index says agrees with what a decode reports: for an entry whose zgpu_decode_frames_device_src status is 0, nframes equals
 *    r.nframes and r.written <= bound. */
/* why a header chain ended (zgpu_entry_index.why): no verdict — a decode of the entry decides its status */
enum {
  ZGPU_CHAIN_END = 0,                 /* the chain reached the end of the entry */
  ZGPU_CHAIN_SHORT_HEADER = 1,        /* a frame header that is not all there */
  ZGPU_CHAIN_BAD_MAGIC = 2,
  ZGPU_CHAIN_SKIP_PAST_END = 3,       /* a skippable frame's length leads past the entry */
  ZGPU_CHAIN_SHORT_BLOCK_HEADER = 4,  /* fewer than 3 bytes left where a block header is due */
  ZGPU_CHAIN_RESERVED_BLOCK = 5,
  ZGPU_CHAIN_BLOCK_TOO_LARGE = 6,     /* Block_Size above 128 KiB */
  ZGPU_CHAIN_BODY_PAST_END = 7,
  ZGPU_CHAIN_SHORT_CHECKSUM = 8
};
typedef struct {
  uint64_t bound;       /* == zgpu_plaintext_bound of a host copy of the entry, always */
  uint64_t chain_end;   /* offset in the entry at which the header chain ended */
  uint32_t status;      /* 0, or ZGPU_E_BAD_ARG: the source failed the pointer check (then every other field is 0) */
  uint32_t nframes;     /* zstd frames whose header the chain read (skippable frames not counted) */
  uint32_t nskippable;
  uint32_t nblocks;     /* block headers read, over all frames */
  uint32_t why;         /* why the chain ended: ZGPU_CHAIN_*; 0 = it reached the end of the entry */
  uint32_t flags;       /* of the zstd frames counted in nframes (all 0 if there is none) — bit 0: every one declares Frame_Content_Size;
                           bit 1: some frame names a dictionary id; bit 2: some frame carries a Content_Checksum; bit 3: every frame is
                           complete (last block seen, checksum all there) */
} zgpu_entry_index;
typedef struct {
  uint64_t src_begin, src_end;   /* the frame's bytes in its entry; src_end = where the chain left it */
  uint64_t bound;                /* this frame's share of the entry's bound */
  uint64_t frame_content_size;   /* 0 if absent */
  uint64_t window_size;          /* as zgpu_frame_info.window_size; 0 for a skippable frame or an unreadable header */
  uint32_t entry, nblocks;
  uint32_t dict_id;              /* 0 if absent */
  uint32_t flags;                /* bit 0 skippable, bit 1 has Frame_Content_Size, bit 2 has Content_Checksum, bit 3 complete, bit 4 single segment */
  uint32_t header_status;        /* what read_frame_header says about the header bytes: 0, ZGPU_E_SKIP_FRAME, or its error */
  uint32_t skip_magic;           /* skippable frames: the magic (the low nibble is the caller's), else 0 */
} zgpu_frame_index;
/* entries[i] for every entry; one launch, 48 bytes per entry come back, no byte of the input does */
int zgpu_frames_index_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, zgpu_entry_index* entries);
/* the same plus a frame table: frames[0 .. *nframes_out), entry by entry in input order, frame_first[i] .. frame_first[i + 1] are entry i's
 * (frame_first has n + 1 slots): its zstd frames and skippable frames in order, tiling [0, chain_end), and — where the chain ended at a frame
 * header it could not read — one last record for that header (src_begin == src_end, header_status says what is wrong with it). Two launches:
 * the summaries, a prefix sum on the host, then every lane writes its own records (64 bytes each come back). frames_cap too small:
 * ZGPU_E_TARGET_TOO_SMALL, *nframes_out = the count needed, entries[] and frame_first[] are still filled (one launch). */
int zgpu_frames_table_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, zgpu_entry_index* entries,
                             uint64_t* frame_first, zgpu_frame_index* frames, size_t frames_cap, size_t* nframes_out);
/* diagnostics of the context's last index / table call: out[0] launches, [1] kernel microseconds (HIP events), [2] bytes downloaded,
 * [3] input bytes that crossed to the host (always 0). Returns how many were written. */
int zgpu_debug_frames_index_stats(const zgpu_ctx*, uint64_t* out, int n);

/* ---- byte ranges of device-resident multi-frame entries ------------------------------------------------------------------------------------
 * Shards and columnar pages are cut into many independent frames so that a part of one can be read. zgpu_decode_ranges_device_src writes
 * plaintext bytes [begin, begin + len) of entry i to device_dsts[i] and decodes only the frames that hold them: one lane per entry follows the
 * header chain on the device (zg_k_seek: three bytes per block, never a block body, ONE launch for the whole call, 64 bytes per entry come back
 * and no byte of the input), and the whole frames it selects, (src + src_lo, src_hi - src_lo), go through the machinery of
 * zgpu_decode_frames_device_src — walk, submits cut by the selection's bound, gather, decode, hash, one scatter launch per submit whose segments
 * are clipped to the range. zgpu_frames_seek_device is the selection alone.
 *  - Plaintext coordinates are DECLARED coordinates: the offset of a frame is the sum of the Frame_Content_Size fields in front of it (from the
 *    anchor on). The rule, one definition (zg_seek.h): from p = anchor_src, pos = anchor_plain — a skippable frame is passed over (in front of
 *    the selection while nothing is taken, inside it afterwards); a zstd frame that declares a size fcs, with nothing taken yet and
 *    pos + fcs <= begin, is skipped (pos += fcs); any other frame is taken (the first sets src_lo and plain_lo = pos; a sized frame adds its fcs
 *    to pos, an unsized one makes the selection open-ended); behind a taken frame the chain stops with src_hi = p once the selection is not
 *    open-ended and pos >= begin + len (saturating). An open-ended selection runs to the end of the chain: an unsized frame and everything
 *    behind it is decoded. Where the chain breaks (why != 0), in a skipped or a taken frame, src_hi = lens[i] and, if nothing was taken, src_lo
 *    = the broken frame's begin: the decode of those bytes then reports what zgpu_decode_all reports for them. The end of the entry with
 *    nothing taken (the range lies behind the plaintext) sets bit 2, and the decode call answers status 0, written 0.
 *  - What random access means: frames in front of the range are never decoded, so a defect in their bodies or checksums is NOT seen; a
 *    skipped frame whose declared size is false shifts the coordinates of everything behind it, silently; frames behind the range are not
 *    read at all. A TAKEN frame that declares a size and decodes to another length fails its entry with ZGPU_E_CONTENT_SIZE_MISMATCH — behind
 *    a decode error, a walk error and BAD_ARG, in front of TARGET_TOO_SMALL and of the checksum verdict of ZGPU_DEVICE_VERIFY. The check is
 *    per frame, and the order is one — decode and walk, size, TARGET_TOO_SMALL, checksum — for every entry: with or without dictionary
 *    frames, in a shared submit or decoded alone (an entry's status does not depend on zgpu_set_frames_shared_dicts).
 *    (In the library that order is written once: zstd-rs_amd/csrc/zg_entry.h, for the entries of a submit and for those decoded alone.)
 *  - results[i].d is zgpu_decode_frames_device_src's result for the selection, except: written is the CLIPPED count — the bytes of
 *    [begin - plain_lo, begin - plain_lo + len) that the taken frames' concatenation has — and ZGPU_E_TARGET_TOO_SMALL is decided by that
 *    count against caps[i], not by the decoded size; nframes counts the frames decoded. The destination holds exactly those bytes.
 *  - Anchors: a caller that reads many ranges of one entry indexes it once (zgpu_frames_table_device), keeps the table, and starts each chain
 *    at a frame boundary in front of begin: anchor_src = that frame's src_begin, anchor_plain = the declared sizes in front of it. Nothing in
 *    front of anchor_src is read. An anchor is the caller's promise; a wrong one shifts the coordinates like a false size.
 *  - Guarantees that carry over: entries are isolated and their order does not matter; no byte of a failed entry's destination is written and
 *    no byte at or behind dst + written; the hash rule and ZGPU_DEVICE_VERIFY act on the taken frames, hashed whole in the engine's output
 *    (a corrupted checksum in a skipped frame is not seen); every source and destination passes the pointer check before anything is
 *    launched; no lane reads a byte outside [src, src + lens[i]), in front of anchor_src, or inside a block body; streams are synchronised
 *    on return. Entries decoded alone (dictionary frames with the shared switch off, Unsupported / Internal verdicts) download only
 *    [src_lo, src_hi) and upload only the clipped bytes. zgpu_debug_frames_submits / _device_stats / _device_src_stats / _dict_stats are
 *    filled as by zgpu_decode_frames_device_src. */
typedef struct {
  uint64_t begin, len;          /* plaintext bytes [begin, begin + len) of the entry (saturating); len == 0: nothing of the entry is checked, read
                                   or written (its lane reads no byte), the record is all zeros */
  uint64_t anchor_src;          /* a frame boundary of the entry at which the header chain starts (0: its first byte) ... */
  uint64_t anchor_plain;        /* ... and the plaintext offset of that boundary (0 with anchor_src 0). From a cached zgpu_frames_table_device. */
} zgpu_range;
typedef struct {                /* 64 bytes: what one lane found; also what the decode call acted on */
  uint64_t src_lo, src_hi;      /* the bytes of the entry that are decoded: whole frames (skippable frames between them included) */
  uint64_t plain_lo;            /* plaintext offset, in the entry's coordinates, of the first byte the frame at src_lo yields */
  uint64_t bound;               /* == zgpu_plaintext_bound of a host copy of [src_lo, src_hi) */
  uint64_t plain_seen;          /* declared plaintext offset where the chain stopped */
  uint32_t status;              /* 0 or ZGPU_E_BAD_ARG (pointer check, anchor_src > lens[i], anchor_plain > begin): then every other field 0 */
  uint32_t frames_skipped, frames_taken, nblocks;   /* zstd frames (skippable frames are not counted; a frame in which the chain broke counts as
                                   taken); nblocks: block headers read, skipped and taken frames together */
  uint32_t why;                 /* ZGPU_CHAIN_*: why the chain ended, 0 if it stopped because the range was covered or the entry ended */
  uint32_t flags;               /* bit 0 open-ended (an unsized frame was taken), bit 1 the chain broke, bit 2 nothing taken: the range lies behind the plaintext */
} zgpu_seek;
typedef struct { zgpu_device_entry_result d; zgpu_seek seek; } zgpu_range_result;
/* out[i] for every entry; one launch, 64 bytes per entry come back, no byte of the input does */
int zgpu_frames_seek_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges, zgpu_seek* out);
int zgpu_decode_ranges_device_src(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges,
                                  void* const* device_dsts, const size_t* caps, const zgpu_device_opts* opts_or_null, zgpu_range_result* results);
/* diagnostics of the context's last seek / ranges call: out[0] seek launches, [1] seek kernel microseconds (HIP events), [2] bytes downloaded by
 * the seek (64 * n), [3] input bytes that crossed to the host (entries decoded alone only), [4] frames skipped, [5] frames decoded, [6] plaintext
 * bytes decoded, [7] bytes written to destinations ([3], [5] - [7]: 0 after zgpu_frames_seek_device). [5] and [6] are work done, not bytes
 * delivered: an entry that decoded and then failed a later check (size, TARGET_TOO_SMALL, checksum) is counted, and every entry is counted
 * once, in its submit or alone. ZGPU_DEVICE_VERIFY_SEEK_TABLE: [8] checksum-compare launches (zg_k_seeksums, one per submit that holds
 * such entries), [9] their kernel microseconds (HIP events), [10] bytes they brought back (32 per entry), [11] frames compared, [12] entries
 * failed by the flag. A caller that asks for 8 gets what it always got. Returns how many were written. */
int zgpu_debug_ranges_stats(const zgpu_ctx*, uint64_t* out, int n);

/* ---- byte ranges through the seek table of zstd's seekable format ------------------------------------------------------------------------------
 * Files written for random access (libzstd's contrib/seekable_format, t2sz, shard and columnar writers) are compressed as a stream, so their
 * frames usually declare no Frame_Content_Size: zgpu_decode_ranges_device_src then takes the first frame, is open-ended and decodes the whole
 * entry. Such files carry the index themselves: ONE skippable frame at the entry's end, the seek table (all fields little-endian) —
 *    Skippable_Magic 0x184D2A5E | Frame_Size = nframes * es + 9 | nframes x { Compressed_Size u32, Decompressed_Size u32 [, Checksum u32] } |
 *    Number_Of_Frames u32 (<= 0x8000000) | Seek_Table_Descriptor u8 (bit 7 Checksum_Flag; bits 6..2 reserved, 0; bits 1..0 ignored) | 0x8F92EAB1
 * es = 8, or 12 with checksums. Entry k describes the k-th frame of the entry (a skippable frame is entered with decompressed size 0); it lies
 * at source offset C_k, the compressed sizes in front of it, and yields plaintext [D_k, D_k + d_k), D_k the decompressed sizes in front of it.
 * zgpu_frames_seek_table_device reads that table on the device, one WAVE per entry (zg_k_seektab, ONE launch for the whole call: coalesced loads,
 * two wave-wide prefix sums, a ballot; no frame or block header is touched, 64 bytes per entry come back and no byte of the input), and
 * zgpu_decode_ranges_seek_table_device_src runs the selections through the machinery of zgpu_decode_ranges_device_src.
 *  - Plaintext coordinates are the TABLE's coordinates, not declared ones. The rule, one definition (zg_seektab.h), end = begin + len saturating:
 *    first = the smallest k with D_k + d_k > begin; last = the smallest k >= first with D_k + d_k >= end, else nframes - 1. The record: src_lo =
 *    C_first, src_hi = C_last + c_last, plain_lo = D_first, plain_seen = D_last + d_last, bound = plain_seen - plain_lo — what the table
 *    promises, not zgpu_plaintext_bound of the bytes —, frames_skipped = first, frames_taken = last - first + 1 (table entries, zero-size ones
 *    included), nblocks = 0, flags 0. No first (the range lies behind the plaintext): flags bit 2, src_lo = src_hi = C_n, plain_lo = plain_seen
 *    = D_n, frames_skipped = nframes, frames_taken = 0, and the decode call answers status 0, written 0. For an entry whose frames all declare
 *    their true size this selects the bytes zgpu_frames_seek_device selects.
 *  - A table that is not usable: status = ZGPU_E_SEEK_TABLE, why = ZGPU_SEEKTAB_*, every other field 0; in the decode call the entry fails with
 *    that status, is not read further and not written. The checks, in order: the entry is shorter than 17 bytes or does not end in the seekable
 *    magic (NONE); reserved descriptor bits (RESERVED_BITS); more than 0x8000000 frames, or a table larger than the entry (TOO_LARGE); no
 *    skippable magic or another Frame_Size where the table frame must begin (BAD_FRAME); compressed sizes that lead past the table frame's begin
 *    (PAST_TABLE). The wave reads bytes of the table frame only, nothing in front of it and nothing at or behind lens[i]: an entry may end flush
 *    with its allocation, and the table may begin at any alignment.
 *  - A range with anchor_src != 0 or anchor_plain != 0 gets ZGPU_E_BAD_ARG in its record: the table is the index, there is nothing to anchor.
 *  - The decode call decodes (src + src_lo, src_hi - src_lo) as zgpu_decode_ranges_device_src decodes its selections — walk, submits cut by the
 *    walk's bound, gather, decode, hash, clipped scatter, entries that go alone — and results[i] means the same, with one more check: an entry
 *    whose taken frames decode to another total than the table promises (plain_seen - plain_lo) fails with ZGPU_E_CONTENT_SIZE_MISMATCH, in
 *    the rank that verdict has (behind a decode or walk error, in front of TARGET_TOO_SMALL and the checksum verdict), in a shared submit and
 *    alone. The check is on the entry's total: two lies that cancel out go unseen (one frame yields 10 bytes fewer than its table entry says
 *    and the next 10 more). A frame that declares a Frame_Content_Size is still held to it, per frame.
 *  - A false table is a status, never a fault: compressed sizes that put src_lo inside a frame give what zgpu_decode_all reports for those
 *    bytes, and every access stays inside the entry. Frames in front of the range are not decoded, so a false size in their table entries
 *    shifts the coordinates silently.
 *  - The table's own Checksum fields — the low 32 bits of XXH64 (seed 0) of each frame's plaintext, the only integrity information of files
 *    whose frames carry no Content_Checksum — are enforced by ZGPU_DEVICE_VERIFY_SEEK_TABLE (flags bit 2; without it they are not read, and
 *    ZGPU_DEVICE_VERIFY acts on frames that carry a Content_Checksum, as in the other calls). The comparison runs on the device (zg_k_seeksums,
 *    one wave per entry, one launch per submit behind the hash kernel; 32 bytes per entry come back, no byte of the table). The rule, one
 *    definition (zg_seeksums.h). For an entry whose selection is table rows [first, first + taken), with R_k = C_k - C_first:
 *      - a decoded zstd frame COINCIDES with row k if it begins at selection offset R_k and is c_k bytes long;
 *      - a frame that coincides with a row and was hashed is COMPARED: the low 32 bits of its digest against the row's Checksum;
 *      - rows that no decoded zstd frame coincides with are not looked at: skippable frames entered with size 0, and rows outside the
 *        selection. A false checksum in a skipped frame's row is not seen, exactly as a false size there shifts the coordinates silently;
 *      - the entry fails with ZGPU_E_SEEK_CHECKSUM_MISMATCH if any compared frame differs, if any decoded zstd frame coincides with no row
 *        (nothing vouches for such a frame), or if the table carries no checksums (Checksum_Flag clear);
 *      - an entry of which no zstd frame is decoded (a range of length 0, nothing taken, skippable frames only) is not looked at at all.
 *    Every decoded zstd frame of such an entry is hashed, with or without a Content_Checksum: hash_max_bytes == 0 means NO limit under this
 *    flag; a nonzero value still bounds what is hashed, and longer frames pass uncompared, as under ZGPU_DEVICE_VERIFY. The verdict ranks
 *    last: behind decode and walk errors, ZGPU_E_CONTENT_SIZE_MISMATCH, ZGPU_E_TARGET_TOO_SMALL and ZGPU_E_CHECKSUM_MISMATCH. A failed entry
 *    has written = nframes = 0 and NO byte of its destination is written (the verdict comes before the scatter list is built); r.checksums is
 *    the frames compared, r.checksum_mismatches those that differ, checksums_unverified the decoded frames not compared (no coinciding row,
 *    not hashed, or no checksums in the table), every other field 0; results[i].seek stays the selection's record. Other entries are
 *    unaffected, in any order and with zgpu_set_frames_shared_dicts on or off: entries decoded alone get the same verdict on the host, from
 *    the footer and rows [first, first + taken) (counted in the input bytes that crossed to the host), before their one H2D. A table that
 *    changed between the seek and the compare fails the CALL with ZGPU_E_INTERNAL. The flag may be combined with ZGPU_DEVICE_VERIFY; with
 *    ZGPU_DEVICE_NO_HASH, or on any other call that takes zgpu_device_opts, the call returns ZGPU_E_BAD_ARG and launches nothing.
 *  - Everything else carries over from zgpu_decode_ranges_device_src: isolation and order independence, no byte of a failed entry and no byte at
 *    or behind dst + written is written, the pointer checks before any launch, streams synchronised on return, and the same diagnostics
 *    (zgpu_debug_ranges_stats, zgpu_debug_frames_submits, _device_stats, _device_src_stats, _dict_stats). */
enum {                                /* zgpu_seek.why of an entry with status ZGPU_E_SEEK_TABLE */
  ZGPU_SEEKTAB_NONE = 16,
  ZGPU_SEEKTAB_RESERVED_BITS = 17,
  ZGPU_SEEKTAB_TOO_LARGE = 18,
  ZGPU_SEEKTAB_BAD_FRAME = 19,
  ZGPU_SEEKTAB_PAST_TABLE = 20
};
int zgpu_frames_seek_table_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges, zgpu_seek* out);
int zgpu_decode_ranges_seek_table_device_src(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_range* ranges,
                                             void* const* device_dsts, const size_t* caps, const zgpu_device_opts* opts_or_null,
                                             zgpu_range_result* results);

/* ---- many byte ranges of few seekable entries, each frame decoded once ---------------------------------------------------------------------------
 * A data loader pulls hundreds of records out of each of a few large seekable shards that sit in device memory. The calls above take one range
 * per entry: every range scans its entry's table again, a frame that holds ten records is decoded ten times, and a frame's plaintext can reach
 * only one destination. These two calls take n entries and m ranges, each range naming its entry (ranges[j].entry < n, pad = 0):
 *  - every entry that a range of nonzero length names is located once (zg_k_seekmany_locate, one lane per entry; 32 bytes per entry come back,
 *    no byte of a table) and its table is scanned ONCE into 64-bit exclusive prefix sums C[k], D[k], k = 0 .. nframes, in device scratch of
 *    16 * (nframes + 1) bytes per entry (two launches, one wave per chunk of 2048 rows; ZGPU_E_NOMEM if the scratch cannot be had);
 *  - every range finds its rows by binary search on D, one lane per range (zg_k_seekmany_find, one launch). zg_seekmany.h has the kernels.
 * Selection. out[j], and results[j].seek, is the full record zgpu_frames_seek_table_device returns for (entry, begin, len) of range j — the
 * rule above, one definition (zg_seektab.h): ZGPU_E_SEEK_TABLE and every why, ZGPU_SEEKTAB_PAST_TABLE decided per range from its own
 * C_last + c_last > tab. A range of length 0 gives a record of zeros and reads no byte. A range with entry >= n or pad != 0 gets ZGPU_E_BAD_ARG
 * in its record, as does one whose entry or (gather call, caps[j] > 0) destination is not device memory of this context's device; the other
 * ranges are unaffected. An entry that no range of nonzero length names is neither checked nor read.
 * Groups (the gather call). Of the ranges of ONE entry with status 0 and frames_taken > 0, those whose row intervals [frames_skipped,
 * frames_skipped + frames_taken) share at least one row belong to one group, transitively. A group's rows are the union [gfirst, glast] of its
 * ranges' intervals, and the group is decoded ONCE, exactly as zgpu_decode_ranges_seek_table_device_src decodes a selection of those rows:
 * (src + C_gfirst, C_{glast + 1} - C_gfirst) is walked, cut into submits (a group is never split), gathered, decoded and hashed; it promises
 * D_{glast + 1} - D_gfirst bytes; a frame that declares a size is held to it; dictionary frames and entries that go alone are served as there
 * (a group that goes alone downloads its selection once, and every range's clipped bytes are uploaded to that range's destination).
 * RANGES THAT SHARE A FRAME SHARE THE FATE OF EVERY FRAME OF THEIR GROUP: a defect in any frame of [gfirst, glast] fails every range of the
 * group, also those that take no byte of that frame. The verdict of range j, in the rank order of the calls above:
 *   1. the group's decode or walk error, or ZGPU_E_CONTENT_SIZE_MISMATCH (the group's total against the table's promise, declared sizes per frame);
 *   2. ZGPU_E_TARGET_TOO_SMALL, by the range's OWN clipped count against its OWN caps[j]: a range that is too small does not disturb the
 *      other ranges of its group;
 *   3. the group's ZGPU_E_CHECKSUM_MISMATCH under ZGPU_DEVICE_VERIFY;
 *   4. the group's ZGPU_E_SEEK_CHECKSUM_MISMATCH under ZGPU_DEVICE_VERIFY_SEEK_TABLE (rows [gfirst, glast] of the entry's table).
 * written is the range's own clipped count; nframes and the checksum fields are the group's. A range that is alone in its group gets, field
 * for field and byte for byte, what zgpu_decode_ranges_seek_table_device_src gives for it.
 * Carried over: groups are isolated from each other, and the order of ranges and of entries does not matter; no byte of a failed range's
 * destination is written, and none at or behind dst + written; every source and every destination with caps[j] > 0 and len > 0 is checked
 * against the runtime's allocations before any launch; no lane reads outside [tab, lens[i]) of an entry during the selection, nor outside
 * [src, src + lens[i]) at any time; the streams are synchronised on return; destinations that overlap each other or a source are undefined;
 * all three option flags are accepted, with the contradictions they have on zgpu_decode_ranges_seek_table_device_src.
 * Diagnostics: zgpu_debug_ranges_stats appends out[13] groups decoded, [14] prefix launches, [15] their microseconds (HIP events), [16] find
 * launches, [17] their microseconds, [18] bytes of prefix scratch; out[0] - [2] are the locate pass (32 * entries + 64 * m bytes come
 * back). [5] and [6], frames decoded and plaintext bytes decoded, count each GROUP once: a frame that ten ranges share is counted once. A
 * caller that asks for 13 gets what it always got.
 * Out of scope: a sibling for host sources, several GPUs, isolation of single rows inside a group. (A prefix handle cached across calls, and
 * entries that declare sizes instead of carrying a table: zgpu_seek_index, below.) */
typedef struct { uint64_t begin, len; uint32_t entry, pad; } zgpu_entry_range;   /* plaintext [begin, begin + len) of entry `entry` */
int zgpu_frames_seek_table_many_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, const zgpu_entry_range* ranges,
                                       uint32_t m, zgpu_seek* out /* m */);
int zgpu_gather_ranges_seek_table_device_src(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                             const zgpu_entry_range* ranges, uint32_t m, void* const* device_dsts /* m */,
                                             const size_t* caps /* m */, const zgpu_device_opts* opts_or_null, zgpu_range_result* results /* m */);

/* ---- seek index handles: index a shard once, seek and gather any number of times -----------------------------------------------------------
 * A zgpu_seek_index holds, per entry, the 64-bit exclusive prefix sums C[k], D[k], k = 0 .. nrows, of the entry's rows in DEVICE memory:
 * row k is the entry's k-th frame (zstd or skippable), c_k its compressed bytes, d_k its plaintext bytes. The two calls above compute these
 * pairs from a seek table and throw them away on return; the handle keeps them, and can also build them for entries WITHOUT a seek table
 * whose frames declare their Frame_Content_Size (what ZSTD_compress writes): the common shard of one frame per record.
 * Building (zgpu_seek_index_create_device). Every entry with lens[i] > 0 passes the pointer check of the device-source calls before any
 * launch; one that fails has status ZGPU_E_BAD_ARG in its info, the others are unaffected; the return value reports engine failures only
 * (ZGPU_E_NOMEM, ZGPU_E_HIP, ZGPU_E_INTERNAL: nothing is left behind, *out = NULL).
 *  - ZGPU_INDEX_SEEK_TABLE: the locate, total and prefix passes of zg_seekmany.h; the pairs and what locate found (tab, nrows) are kept. An
 *    unusable table: ZGPU_E_SEEK_TABLE, why = ZGPU_SEEKTAB_*.
 *  - ZGPU_INDEX_DECLARED: the summary pass of zgpu_frames_index_device, then zg_k_seekidx_rows (zg_seekidx.h), one lane per entry: every frame
 *    record of the header chain is a row, d_k = its declared Frame_Content_Size (the 2-byte form's + 256 included; 0 for a skippable frame;
 *    a seek table at the entry's end is one more skippable row). Indexable: the chain reached the entry's end and every zstd frame declares
 *    a size. Else ZGPU_E_FRAME_INDEX with why = the ZGPU_CHAIN_* reason, ZGPU_INDEX_UNSIZED, or ZGPU_SEEKTAB_TOO_LARGE (more than 2^27
 *    rows). An entry of length 0 is a valid index without rows. The host accepts the pairs only where C[nrows] == lens[i]; an input that
 *    changed between the two passes is ZGPU_E_INTERNAL, never a store outside the entry's pairs.
 *  - ZGPU_INDEX_AUTO: the table is tried; an entry whose table answer is ZGPU_SEEKTAB_NONE, and only that one, is indexed by its chain. A
 *    table that is present and malformed stays an error. info.kind says what an entry was indexed by.
 * The handle owns 16 * (nrows + 1) bytes of device memory per indexed entry and the per-entry host records. No byte of an entry comes back
 * to the host. It stores no source pointer: an index describes bytes, not an address. It belongs to one context and is destroyed before it.
 * Selection (zgpu_frames_seek_indexed_device): ONE zg_k_seekmany_find launch over the handle's pairs; no byte of any entry is read. out[j] is
 * the record of zg_seektab.h's rule applied to the entry's rows: for a table-kind entry all 64 bytes of what
 * zgpu_frames_seek_table_many_device returns (ZGPU_SEEKTAB_PAST_TABLE decided per range against the kept tab); for a declared-kind entry tab
 * is the entry's length — PAST_TABLE cannot arise — and src_lo, src_hi, plain_lo, plain_seen and flag bit 2 equal what
 * zgpu_frames_seek_device answers for the range with anchor 0 (frames_skipped / frames_taken count ROWS, skippable frames included, and
 * bound is the declared promise plain_seen - plain_lo). A range that names an entry the index refused gets that entry's status and why, every
 * other field 0; entry >= entries or pad != 0: ZGPU_E_BAD_ARG; a length of 0: a record of zeros. A handle of another context fails the call
 * with ZGPU_E_BAD_ARG.
 * Gather (zgpu_gather_ranges_indexed_device_src): n must be the handle's entry count (else ZGPU_E_BAD_ARG). An entry that a range of nonzero
 * length names must pass the pointer check and have lens[i] == info.len, else the ranges that name it get ZGPU_E_BAD_ARG and the others are
 * unaffected; the pointer may differ from the one the index was built from. Behind the selection it IS
 * zgpu_gather_ranges_seek_table_device_src — one routine —: groups by shared rows, each decoded once; the promise D[glast + 1] - D[gfirst]
 * held against the group's total, declared sizes per frame; fate sharing within a group; ZGPU_E_TARGET_TOO_SMALL per range; the rank order
 * of verdicts; dictionary frames; ZGPU_DEVICE_VERIFY; no byte of a failed range's destination written, none at or behind dst + written; the
 * streams synchronised on return. ZGPU_DEVICE_VERIFY_SEEK_TABLE works for ranges of table-kind entries (the rows are read from the entry at
 * verify time); a range of a declared-kind entry under that flag gets ZGPU_E_BAD_ARG in its result: there is no table to enforce
 * (unless the handle holds the entry's sums: seek index checksums, below).
 * RANDOM ACCESS here means: a call costs one find launch plus the decode of the frames its ranges touch; nothing in front of them is read.
 * THE INDEX IS THE CALLER'S PROMISE that the entry's bytes have not changed since it was built. A stale index is a status, never a fault:
 * every record is held against lens[i] on the host (src_lo <= src_hi <= lens[i]) before anything is gathered, the bytes then go through the
 * bounded device walk, and the range gets what zgpu_decode_all reports for those bytes, or ZGPU_E_CONTENT_SIZE_MISMATCH.
 * Diagnostics: zgpu_seek_index_stats — [0] launches of the build, [1] their microseconds (HIP events), [2] bytes downloaded, [3] device bytes
 * held, [4] rows, [5] input bytes that crossed to the host (always 0). zgpu_debug_ranges_stats after an indexed call: [0] - [2], [14], [15]
 * and [18] are 0 (no locate, no prefix pass), [16] is 1 when any range has nonzero length, [13], [5], [6] count groups and their frames once.
 * Entries whose frames declare no size are indexed by measuring them: zgpu_seek_index_measure_device, below.
 * Out of scope: updating an index in place, host sources, several GPUs, sharing one handle between contexts. */
typedef struct zgpu_seek_index zgpu_seek_index;        /* belongs to one zgpu_ctx; destroy it before the context; its context's thread rule (context section) */
enum { ZGPU_INDEX_SEEK_TABLE = 0, ZGPU_INDEX_DECLARED = 1, ZGPU_INDEX_AUTO = 2 };
#define ZGPU_INDEX_UNSIZED 32u                         /* zgpu_seek_index_info.why: a zstd frame declares no Frame_Content_Size */
typedef struct {
  uint64_t len;          /* bytes of the entry the index was built from */
  uint64_t compressed;   /* C[nrows] */
  uint64_t plaintext;    /* D[nrows] */
  uint32_t status;       /* 0, ZGPU_E_BAD_ARG (pointer check), ZGPU_E_SEEK_TABLE, ZGPU_E_FRAME_INDEX; != 0: nrows = compressed = plaintext = 0 */
  uint32_t why;          /* ZGPU_SEEKTAB_* | ZGPU_CHAIN_* (the chain broke) | ZGPU_INDEX_UNSIZED | ZGPU_INDEX_UNMEASURED | ZGPU_INDEX_DICT */
  uint32_t kind;         /* ZGPU_INDEX_SEEK_TABLE, ZGPU_INDEX_DECLARED or ZGPU_INDEX_MEASURED: what this entry was indexed by */
  uint32_t nrows;
} zgpu_seek_index_info;
int zgpu_seek_index_create_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, uint32_t kind, zgpu_seek_index** out);
void zgpu_seek_index_destroy(zgpu_seek_index*);
uint32_t zgpu_seek_index_entries(const zgpu_seek_index*);
int zgpu_seek_index_info_of(const zgpu_seek_index*, uint32_t i, zgpu_seek_index_info* out);
int zgpu_seek_index_stats(const zgpu_seek_index*, uint64_t* out, int n);
int zgpu_frames_seek_indexed_device(zgpu_ctx*, const zgpu_seek_index*, const zgpu_entry_range* ranges, uint32_t m, zgpu_seek* out /* m */);
int zgpu_gather_ranges_indexed_device_src(zgpu_ctx*, const zgpu_seek_index*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                          const zgpu_entry_range* ranges, uint32_t m, void* const* device_dsts /* m */,
                                          const size_t* caps /* m */, const zgpu_device_opts* opts_or_null, zgpu_range_result* results /* m */);

/* ---- seek index by measuring: entries whose frames declare no size and that carry no seek table ----------------------------------------------
 * A shard of frames written by a streaming compressor (ZSTD_compressStream with ZSTD_e_end per record, zstd reading a pipe, a stream writer
 * that flushes a frame per record, files joined with cat) has no Frame_Content_Size and no seek table: ZGPU_INDEX_DECLARED refuses it with
 * ZGPU_INDEX_UNSIZED, ZGPU_INDEX_SEEK_TABLE with ZGPU_SEEKTAB_NONE, and every range call decodes everything behind the first frame it takes.
 * zgpu_seek_index_measure_device indexes such entries by MEASURING them on the device, once: a frame's plaintext length is the sum of its
 * blocks' lengths — a raw or RLE block: Block_Size; a compressed block without sequences: Regenerated_Size of its literals; a compressed
 * block with sequences: Regenerated_Size + the sum of its match lengths — and those sums need the FSE tables, the sequence bitstream and the
 * LL and ML extra bits, but no Huffman stream, no byte of LZ77 execution and no output buffer.
 * The call returns the same kind of handle under the same rules as zgpu_seek_index_create_device: every entry with lens[i] > 0 passes the
 * pointer check before any launch; one that fails has ZGPU_E_BAD_ARG in its info and the others are unaffected; the return value reports
 * engine failures only, nothing is left behind on failure (*out = NULL), the streams are drained on return, an entry of length 0 is a valid
 * index without rows, and no byte of an entry comes back to the host (frame records and skeleton records do).
 *  - mode ZGPU_MEASURE_ALL: every entry is measured, whatever it declares or carries. ZGPU_MEASURE_UNSIZED: every entry is first indexed as
 *    ZGPU_INDEX_AUTO indexes it, and only an entry that AUTO refuses with ZGPU_E_FRAME_INDEX / ZGPU_INDEX_UNSIZED is measured; a malformed
 *    table or a broken chain stays the error it is. Any other mode: ZGPU_E_BAD_ARG.
 *  - Rows of a measured entry: the frame records of its header chain, exactly as for the declared kind — c_k the frame's bytes; a skippable
 *    frame, or a seek table at the end, is a row with d_k = 0 — but d_k of a zstd frame is its MEASURED size. A declared Frame_Content_Size
 *    is not consulted: a frame that lies about it fails later, per frame, in the gather, as it does today. info.kind =
 *    ZGPU_INDEX_MEASURED, tab = lens[i] (ZGPU_SEEKTAB_PAST_TABLE cannot arise), info.plaintext = D[nrows]; D saturates at 2^64 - 1.
 *  - Refusals (ZGPU_E_FRAME_INDEX, kind ZGPU_INDEX_MEASURED, nrows = compressed = plaintext = 0), in this order: the chain does not reach
 *    the entry's end (why = the ZGPU_CHAIN_* reason); more than 2^27 rows (ZGPU_SEEKTAB_TOO_LARGE); a frame names a dictionary id
 *    (ZGPU_INDEX_DICT); the measuring of a frame ends in a status (ZGPU_INDEX_UNMEASURED): a header the host's parse refuses, an FSE table
 *    description, the sequence bitstream, a block whose literal lengths add up to more than its literals (NotEnoughLiterals), a block
 *    that regenerates 2^31 bytes or more (Unsupported). zgpu_last_error names the first such entry, its frame (counted in zstd frames) and
 *    zgpu_status_name of the status. An entry that fails never disturbs another, in any order.
 *  - How: the summary pass and the frame records of zgpu_frames_table_device; runs of whole frames then go through the machinery of the
 *    device-source calls (zg_k_walk's skeleton, the host's one parse, zg_k_gather) in submits cut at frame boundaries at the input budget of
 *    the decode submits — a frame is never split, one above the budget is a submit of its own, and no plaintext budget applies: nothing is
 *    produced —, and every submit runs zg_k_reset, the FSE tables, zg_k_seq, zg_k_seqsize (zg_seqsize.h) and zg_k_scan; the sizes come back
 *    per frame, the host builds the pairs and uploads them in one copy.
 * WHAT MEASURING DOES NOT SEE: Huffman tree descriptions and Huffman streams; offsets (too far, zero); content checksums. An entry with
 * such a defect IS indexed, with the sizes its headers, tables and sequences give. The defect surfaces when the frame is decoded, as a status
 * of the ranges whose group holds that frame. AN INDEX IS A PROMISE ABOUT SIZES, NOT A VERDICT ON THE BYTES.
 * Using a measured index: zgpu_frames_seek_indexed_device and zgpu_gather_ranges_indexed_device_src, unchanged — one find launch over the
 * pairs; a group's promise D[glast + 1] - D[gfirst] is held against the decoded total (ZGPU_E_CONTENT_SIZE_MISMATCH on a stale index); a range
 * of a measured-kind entry under ZGPU_DEVICE_VERIFY_SEEK_TABLE gets ZGPU_E_BAD_ARG, as a declared-kind entry's does — until the handle holds the
 * entry's sums (zgpu_seek_index_hash_device, below, which also sees what measuring does not).
 * zgpu_seek_index_export_seek_table writes entry `entry`'s rows, of whatever kind, as ONE seekable-format skippable frame into HOST memory
 * (it is meant for a file), so that the entry never needs measuring again:
 *    0x184D2A5E | Frame_Size = 8 * nrows + 9 | nrows x { c_k u32, d_k u32 } | Number_Of_Frames | descriptor 0 (no checksums) | 0x8F92EAB1
 * 17 + 8 * nrows bytes; the entry's 16 * (nrows + 1) bytes of pairs are downloaded, nothing else. For a declared- or measured-kind entry,
 * the entry's bytes followed by the exported frame are an entry whose ZGPU_INDEX_SEEK_TABLE index has the same nrows, C and D.
 * ZGPU_E_BAD_ARG: a null handle or `written`, entry out of range, an entry whose info has a status, host_dst == NULL with cap > 0.
 * ZGPU_E_TARGET_TOO_SMALL with *written = the size needed: cap too small (host_dst == NULL with cap == 0 asks for the size).
 * ZGPU_E_SEEK_TABLE: some c_k or d_k exceeds 0xFFFFFFFF — the format cannot say it —, and nothing is written.
 * Diagnostics: zgpu_seek_index_stats appends [6] measuring submits, [7] their phase-1 microseconds (HIP events), [8] zstd frames measured;
 * [0] - [2] include the measuring call's lane passes and gathers, [5] stays 0 (records are not input bytes). A caller that asks for 6
 * gets what it always got.
 * Out of scope: frames that name a dictionary id, updating an index in place, host sources, several
 * GPUs, cutting one frame's measuring over submits, ZGPU_INDEX_AUTO falling through to measuring (it would change an existing answer). */
enum { ZGPU_INDEX_MEASURED = 3 };        /* zgpu_seek_index_info.kind only; not accepted by zgpu_seek_index_create_device */
#define ZGPU_INDEX_UNMEASURED 33u        /* info.why: a frame of the entry could not be measured (its headers or its sequence stage fail) */
#define ZGPU_INDEX_DICT 34u              /* info.why: a frame of the entry names a dictionary id (out of scope, above) */
enum { ZGPU_MEASURE_ALL = 0, ZGPU_MEASURE_UNSIZED = 1 };
int zgpu_seek_index_measure_device(zgpu_ctx*, const void* const* device_srcs, const size_t* lens, uint32_t n, uint32_t mode, zgpu_seek_index** out);
int zgpu_seek_index_export_seek_table(const zgpu_seek_index*, uint32_t entry, uint8_t* host_dst, size_t cap, size_t* written);

/* ---- seek index checksums: hash a shard once, enforce on every gather ---------------------------------------------------------------------------
 * A handle may hold, beside its pairs, ONE uint32_t PER ROW in device memory: the low 32 bits of XXH64 (seed 0) of that row's plaintext; a
 * skippable row holds 0 and is never looked at. The array — 4 bytes per row of every indexed entry — is allocated when the first entry of the
 * handle gets sums; a handle that never gets any holds what it always held. Every entry has a state: 0 none, 1 hashed
 * (zgpu_seek_index_hash_device), 2 set by the caller (zgpu_seek_index_set_sums). zgpu_seek_index_info is unchanged; the state is read with
 * zgpu_seek_index_sums_of.
 * zgpu_seek_index_hash_device decodes every zstd frame of every chosen entry ONCE, hashes its plaintext on the device and keeps the sums in
 * the handle. No plaintext is delivered: there is no destination. THIS PASS SEES WHAT MEASURING DOES NOT SEE — Huffman tree descriptions and
 * Huffman streams, offsets, content checksums: every frame goes through the whole decode, and a frame that carries a Content_Checksum is
 * held against it. An entry that passes is known good, not merely measured.
 *  - n must be the handle's entry count and the handle this context's (else ZGPU_E_BAD_ARG). which_or_null[i] == 0 leaves entry i untouched;
 *    NULL chooses every entry. An entry the index refused is skipped: its sums record carries the index's status. A chosen entry must pass
 *    the pointer check of the device-source calls and have lens[i] == info.len, else its record is ZGPU_E_BAD_ARG; the others are unaffected.
 *  - Runs. The entry's pairs come down (16 bytes a row) and its rows are cut into runs of consecutive rows: a run closes in front of a zstd
 *    row (d_k > 0) when it already holds one and its plaintext, with that row, would exceed run_bytes (0: 64 MiB); skippable rows join the
 *    run in progress; a single frame above the limit is a run of its own. Each run is one selection [C[k0], C[k1]) of the machinery of the
 *    gather calls, decoded under the promise D[k1] - D[k0] — a stale index is ZGPU_E_CONTENT_SIZE_MISMATCH — with every decoded zstd frame
 *    hashed on the device, whatever its length; a frame whose own Content_Checksum disagrees fails its run with ZGPU_E_CHECKSUM_MISMATCH.
 *    Dictionary frames and entries that go alone are served as in the gather calls. A frame is mapped to its row by the rule of
 *    ZGPU_DEVICE_VERIFY_SEEK_TABLE: it begins at C[k] - C[k0] and is C[k + 1] - C[k] bytes long; a decoded zstd frame that coincides with
 *    no row is ZGPU_E_CONTENT_SIZE_MISMATCH. The sums reach the handle in one copy per stretch of chosen entries (NULL: one copy).
 *  - ALL OR NOTHING PER ENTRY: if any run of an entry ends in a status the entry keeps NO sums — earlier ones are dropped, state 0 —, its
 *    record carries that status and [row_lo, row_hi), the rows of the first failing run in row order, and zgpu_last_error names the entry,
 *    the run and zgpu_status_name. A failing entry does not disturb another. The return value reports engine failures only; on such a
 *    failure no entry's state has changed. The streams are drained on return. Hashing an entry again replaces its sums.
 * zgpu_seek_index_set_sums uploads nrows sums the caller kept (its own metadata, a checksummed table): the caller's promise, as an anchor is.
 * zgpu_seek_index_read_sums downloads an entry's sums (*nrows = info.nrows; cap_rows below that: ZGPU_E_TARGET_TOO_SMALL, nothing written).
 * ZGPU_E_BAD_ARG: a null argument, entry out of range, an entry the index refused, nrows != info.nrows, reading an entry without sums.
 * Enforcing: under ZGPU_DEVICE_VERIFY_SEEK_TABLE, zgpu_gather_ranges_indexed_device_src applies one rule — AN ENTRY WHOSE HANDLE HOLDS SUMS IS
 * VOUCHED FOR BY THE HANDLE; ANY OTHER ENTRY IS TREATED AS BEFORE (a table-kind entry reads its table; a declared- or measured-kind entry
 * gets ZGPU_E_BAD_ARG). The rule of the flag carries over word for word with sums[k] in the Checksum's place, R_k = C[k] - C[gfirst] and
 * c_k = C[k + 1] - C[k] from the pairs: every decoded zstd frame of such a group is hashed (hash_max_bytes == 0: no limit), the comparison
 * runs on the device (zg_k_idxsums, zg_idxsums.h: one wave per group, one launch per submit behind the hash kernel, no byte of the entry
 * read, 32 bytes per group back; a submit that holds groups of both routes launches both compare kernels), the verdict
 * ZGPU_E_SEEK_CHECKSUM_MISMATCH ranks last, falls on every range of the group, and no byte of a failed range's destination is written.
 * checksums / checksum_mismatches / checksums_unverified of a failed range and zgpu_debug_ranges_stats [8] - [12] mean what they mean for a
 * table. Groups decoded alone get the same verdict on the host from rows [gfirst, glast] of pairs and sums. With the flag a changed byte
 * inside a frame — which changes no size, and which a gather without the flag delivers with status 0: the index is a promise about sizes —
 * fails the group.
 * zgpu_seek_index_export_seek_table_ex: flags == 0 is zgpu_seek_index_export_seek_table; ZGPU_EXPORT_CHECKSUMS writes
 *    0x184D2A5E | Frame_Size = 12 * nrows + 9 | nrows x { c_k u32, d_k u32, sums[k] u32 } | Number_Of_Frames | descriptor 0x80 | 0x8F92EAB1
 * 17 + 12 * nrows bytes, for an entry that has sums (else, or with unknown flag bits, ZGPU_E_BAD_ARG); the size query,
 * ZGPU_E_TARGET_TOO_SMALL and ZGPU_E_SEEK_TABLE as above. The entry's bytes followed by that frame are an entry whose ZGPU_INDEX_SEEK_TABLE
 * index has the same rows and which passes ZGPU_DEVICE_VERIFY_SEEK_TABLE by its table.
 * Diagnostics: zgpu_seek_index_stats appends [9] decode submits of the hash passes, [10] their hash kernels' microseconds (HIP events), [11]
 * zstd frames hashed, [12] bytes of sums held (0 until an entry gets sums; [3] is unchanged), [13] runs cut. A caller that asks for 9 gets
 * what it always got.
 * Out of scope: sums for single rows of an entry, updating in place, host sources, several GPUs. */
typedef struct {
  uint32_t status;       /* of the last zgpu_seek_index_hash_device that chose the entry (0; the index's status; ZGPU_E_BAD_ARG; the failing run's) */
  uint32_t state;        /* 0 none, 1 hashed, 2 set by the caller */
  uint32_t row_lo, row_hi;   /* status != 0 from a run: its rows */
  uint64_t frames;       /* zstd frames hashed (state 1) */
  uint64_t bytes;        /* plaintext bytes hashed (state 1) */
} zgpu_seek_index_sums;
#define ZGPU_EXPORT_CHECKSUMS 1u
int zgpu_seek_index_hash_device(zgpu_ctx*, zgpu_seek_index*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                const uint8_t* which_or_null, uint64_t run_bytes);
int zgpu_seek_index_set_sums(zgpu_seek_index*, uint32_t entry, const uint32_t* sums, uint32_t nrows);
int zgpu_seek_index_read_sums(const zgpu_seek_index*, uint32_t entry, uint32_t* dst, uint32_t cap_rows, uint32_t* nrows);
int zgpu_seek_index_sums_of(const zgpu_seek_index*, uint32_t i, zgpu_seek_index_sums* out);
int zgpu_seek_index_export_seek_table_ex(const zgpu_seek_index*, uint32_t entry, uint32_t flags, uint8_t* host_dst, size_t cap, size_t* written);

/* ---- record index: gather delimited records of indexed shards by number -----------------------------------------------------------------------
 * Every call above speaks in plaintext BYTE offsets. A shard of text (one document per line) is asked for by record NUMBER. A handle may hold,
 * beside its pairs and sums, the RECORD OFFSETS of an entry in device memory, and two calls take record numbers in front of the indexed gather.
 * Definitions, for an indexed entry with plaintext P of length L = info.plaintext and a delimiter byte d (0 .. 255):
 *  - a record is a maximal run of bytes ending in d; the delimiter belongs to the record it ends;
 *  - if L > 0 and P[L - 1] != d, the bytes behind the last delimiter are one more record, the OPEN TAIL;
 *  - R is the number of records (L == 0: R == 0); the entry's offsets are O[0 .. R], 64 bits each: O[0] = 0, O[r] the position just behind
 *    the r-th delimiter, O[R] = L; O is strictly increasing; record r is plaintext [O[r], O[r + 1]);
 *  - records ignore frame and row boundaries: a record may straddle frames, runs and submits; skippable rows contribute nothing.
 * A RECORD INDEX, LIKE THE PAIRS, IS A PROMISE ABOUT BYTES, NOT A VERDICT: offsets that no longer describe the shard (a stale index, a wrong
 * zgpu_seek_index_set_records) deliver the wrong bytes with status 0. Only the handle's sums under ZGPU_DEVICE_VERIFY_SEEK_TABLE catch a shard
 * that changed.
 * zgpu_seek_index_records_device decodes every zstd frame of every chosen entry ONCE, as zgpu_seek_index_hash_device does, finds every byte
 * equal to `delimiter` on the device and keeps the offsets in the handle; nothing is delivered. The argument rules are that call's: n must be
 * the handle's entry count and the handle this context's (else ZGPU_E_BAD_ARG); which_or_null chooses entries; an entry the index refused is
 * skipped and its record carries the index's status; a chosen entry whose pointer check fails or whose lens[i] != info.len gets
 * ZGPU_E_BAD_ARG in its record and keeps what it held; delimiter > 255 is ZGPU_E_BAD_ARG for the whole call. Runs are cut by the same rule
 * (run_bytes, 0: 64 MiB) and each run is one selection decoded under its promise D[k1] - D[k0] (a stale index: ZGPU_E_CONTENT_SIZE_MISMATCH);
 * dictionary frames and entries that go alone are served as in the gather calls (an entry decoded alone is searched on the host, by the same
 * definition). No frame is hashed. ALL OR NOTHING PER ENTRY: if any run ends in a status the entry keeps no offsets (state 0), its record
 * names the first failing run's rows and zgpu_last_error names entry, run and status; a failing entry does not disturb another. The return
 * value reports engine failures only, and such a failure leaves the whole handle as it was. The streams are drained on return. Running the
 * pass on an entry again, with the same or another delimiter, replaces its offsets.
 * On the device, per submit, behind the submit's verdicts (zg_records.h): zg_k_recs_count — one wave per chunk of 4096 plaintext bytes of
 * one decoded frame, 16-byte loads, the ragged head and tail byte by byte, a population count per chunk —, zg_k_recs_scan — the exclusive
 * prefix of the counts, the submit's total and the frames' totals, which come back to the host (8 + 8 bytes per frame: the one round trip
 * per submit) and size the submit's staging —, zg_k_recs_emit — the same chunks, a wave-level prefix of the lanes' counts, every offset stored
 * once, already in the entry's coordinates. The staging buffers live until every run has its verdict; then the handle's array — 8 bytes per
 * offset, R + 1 per entry — is allocated anew and filled by device-to-device copies in row order, O[0] = 0 in front and O[R] = L appended
 * for an open tail. PEAK EXTRA DEVICE MEMORY IS TWICE THE FINAL ARRAY, beside the array a repeated pass replaces.
 * zgpu_seek_index_read_records downloads O[first .. min(first + cap, R + 1)) of an entry into host memory, *n = how many (host_dst == NULL
 * with cap == 0 asks for R + 1 in *n). zgpu_seek_index_set_records uploads offsets the caller kept (a sidecar file): offsets[0] == 0, strictly
 * increasing, offsets[nrecords] == info.plaintext (so nrecords == 0 needs info.plaintext == 0), the delimiter in the low bits of `delimiter`
 * and ZGPU_RECORDS_OPEN_TAIL in its top bit if the last record ends in no delimiter (the call cannot see the bytes; what
 * zgpu_seek_index_records_of reports as flags bit 0 is that bit) — else ZGPU_E_BAD_ARG, and nothing changes. State 2 is the caller's promise.
 * ZGPU_E_BAD_ARG: a null argument, an entry out of range, an entry the index refused, reading an entry without records.
 * zgpu_seek_index_record_ranges_device turns m record ranges into byte ranges with ONE zg_k_recs_find launch, one lane per range; nothing of
 * any entry is read. [first, first + count) is clipped to [0, R) as byte ranges clip to the plaintext (the sum saturates): first >= R or
 * count == 0 gives { begin = O[min(first, R)], len = 0 }; else begin = O[first], len = O[last + 1] - O[first], and with ZGPU_RECORDS_STRIP
 * len is one less unless the last record taken is the open tail. status[j], decided on the host before the launch, in this order: entry out
 * of range or unknown flag bits: ZGPU_E_BAD_ARG; the index's own status for a refused entry; ZGPU_E_BAD_ARG for an entry without records.
 * A range with a status has out[j] = { 0, 0, entry, 0 }; a failing range never disturbs another.
 * zgpu_gather_records_indexed_device_src is that lookup followed by zgpu_gather_ranges_indexed_device_src on the byte ranges: the same
 * groups, verdict order, per-range destinations and options (ZGPU_E_TARGET_TOO_SMALL is the range's own; ZGPU_DEVICE_VERIFY and
 * ZGPU_DEVICE_VERIFY_SEEK_TABLE by the handle's sums; no byte of a failed range's destination is written). A range whose lookup failed
 * carries that status in results[j].d.r.status and the gather skips it. The cost over the byte gather: one launch and 24 * m bytes back.
 * Diagnostics: zgpu_seek_index_stats appends [14] decode submits of the record passes, [15] the microseconds of count + scan + emit (HIP
 * events), [16] chunks scanned, [17] records held, [18] bytes of offsets held, [19] bytes that came back from the side pass. A caller that
 * asks for 14 gets what it always got. zgpu_debug_ranges_stats appends [19] record find launches, [20] their microseconds, [21] bytes back.
 * Out of scope: host sources, several GPUs, multi-byte delimiters, length-prefixed records, hashing and record finding in one decode, offsets
 * narrower than 64 bits, the lookup fused into the gather's find kernel, updating in place. */
typedef struct {
  uint32_t status;      /* of the last zgpu_seek_index_records_device that chose the entry (0; the index's status; ZGPU_E_BAD_ARG; the failing run's) */
  uint32_t state;       /* 0 none, 1 found by the pass, 2 set by the caller */
  uint32_t delimiter;
  uint32_t flags;       /* bit 0: open tail */
  uint64_t nrecords;
  uint32_t row_lo, row_hi;   /* status != 0 from a run: its rows */
} zgpu_seek_index_records;
typedef struct { uint64_t first, count; uint32_t entry, flags; } zgpu_record_range;   /* records [first, first + count) of entry `entry` */
#define ZGPU_RECORDS_STRIP 1u   /* zgpu_record_range.flags: drop the final delimiter of the last record taken (an open tail has none) */
#define ZGPU_RECORDS_OPEN_TAIL 0x80000000u   /* zgpu_seek_index_set_records' delimiter word: the last record ends in no delimiter */
int zgpu_seek_index_records_device(zgpu_ctx*, zgpu_seek_index*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                   const uint8_t* which_or_null, uint32_t delimiter, uint64_t run_bytes);
int zgpu_seek_index_records_of(const zgpu_seek_index*, uint32_t i, zgpu_seek_index_records* out);
int zgpu_seek_index_read_records(const zgpu_seek_index*, uint32_t entry, uint64_t first, uint64_t* host_dst, uint64_t cap, uint64_t* n);
int zgpu_seek_index_set_records(zgpu_seek_index*, uint32_t entry, const uint64_t* offsets /* nrecords + 1 */, uint64_t nrecords, uint32_t delimiter);
int zgpu_seek_index_record_ranges_device(zgpu_ctx*, const zgpu_seek_index*, const zgpu_record_range* recs, uint32_t m,
                                         zgpu_entry_range* out /* m */, uint32_t* status /* m */);
int zgpu_gather_records_indexed_device_src(zgpu_ctx*, const zgpu_seek_index*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                           const zgpu_record_range* recs, uint32_t m, void* const* device_dsts /* m */,
                                           const size_t* caps /* m */, const zgpu_device_opts* opts_or_null, zgpu_range_result* results /* m */);

/* ---- record batches: gather records into one padded or packed tensor ---------------------------------------------------------------------------
 * zgpu_gather_records_indexed_device_src delivers m separate destinations, which the caller sizes with a lookup of its own. A training step
 * consumes ONE tensor: PADDED — uint8[m, width], every row a record followed by the pad byte, plus lengths[m] — or PACKED — the records back to
 * back plus offsets[m + 1] (the cu_seqlens form). zgpu_gather_records_batch_indexed_device_src writes either, layered on the calls above:
 * 1. LOOKUP. The record lookup exactly as in zgpu_seek_index_record_ranges_device: one zg_k_recs_find launch, 24 bytes per range,
 *    ZGPU_RECORDS_STRIP and the status rules. len_j: the range's byte length, 0 where the lookup gave a status or the range is empty.
 *    host_record_bytes[j] = len_j (HOST memory), before any truncation.
 * 2. LAYOUT, on the host from the lookup alone, before anything is decoded (zg_records.h: plan_rows). want_j = len_j, or min(len_j, width)
 *    under ZGPU_BATCH_TRUNCATE with width > 0; rows_truncated counts the rows that were cut. Padded: at_j = j * width, slot_j = width,
 *    total = m * width. Packed: at_j = want_0 + ... + want_{j-1}, slot_j = want_j, total = at_m. Every sum and product is checked: a layout
 *    that does not fit in 64 bits is ZGPU_E_BAD_ARG.
 * 3. ARGUMENTS. ZGPU_E_BAD_ARG for the whole call, with nothing written: a null batch, results or info; a handle of another context; n other
 *    than the handle's entry count; an unknown layout, unknown flag bits, reserved != 0; pad_byte > 255; padded with width == 0; packed with
 *    width != 0 and no ZGPU_BATCH_TRUNCATE; device_lengths or device_offsets not 8-byte aligned; device_lengths (m slots), device_offsets
 *    (m + 1 slots) or, when 0 < total <= cap, [device_dst, device_dst + total) not device memory of the context's device inside one
 *    allocation (the check of the other device-sink calls); options the gather refuses. All of these are found before anything is launched,
 *    but for a packed batch's device_dst and a packed sum that overflows, which need the lookup (it reads the handle and writes nothing of
 *    the caller's). A wrong pointer is a status, never a GPU fault.
 * 4. THE BATCH DOES NOT FIT (total > cap): info->total holds the need, every range whose lookup succeeded gets ZGPU_E_TARGET_TOO_SMALL (the
 *    others keep the lookup's status), nothing behind the lookup is launched, NOTHING IN DEVICE MEMORY IS WRITTEN, the two arrays included,
 *    and the call returns ZGPU_OK. cap == 0 with device_dst == NULL is therefore the size query.
 * 5. GATHER. Else the byte ranges (entry, begin_j, want_j) go through zgpu_gather_ranges_indexed_device_src with destination
 *    device_dst + at_j and capacity slot_j: groups, fate sharing, verdict order, the three option flags, entries decoded alone and results[j]
 *    are that call's, field for field. A truncated range asks for fewer bytes, so the frames behind the cut are neither selected nor
 *    decoded. Without ZGPU_BATCH_TRUNCATE a padded row with len_j > width is that call's own ZGPU_E_TARGET_TOO_SMALL for that row alone. A
 *    range whose lookup failed keeps the lookup's status, as in zgpu_gather_records_indexed_device_src.
 * 6. FINISH, behind the gather's verdicts. final_j = results[j].d.r.written if the row's status is 0, else 0. ONE zg_k_fill launch
 *    (zg_scatter.h: a ragged fill of m regions, one wave per chunk, plain vector stores) writes pad_byte into [at_j + final_j, at_j + slot_j)
 *    of every row: a failed row is all pad in both layouts, and in the packed layout its slot keeps its place. device_lengths[j] = final_j,
 *    device_offsets[j] = at_j, device_offsets[m] = total, by host-to-device copies on the engine's stream. The streams are drained on return.
 *    ON ZGPU_OK WITH total <= cap EVERY BYTE OF [device_dst, device_dst + total) IS EITHER A RECORD'S BYTE OR THE PAD BYTE: no result depends
 *    on memory the call never wrote. No byte at or behind device_dst + total is written, and none outside the arrays' m and m + 1 slots.
 *    info: total, bytes_filled (pad bytes written), rows_ok, rows_failed (rows with a status), rows_truncated.
 * 7. m == 0: total = 0, device_offsets[0] = 0 if the array is given, no launch.
 * The call adds no status code. Diagnostics: zgpu_debug_ranges_stats appends [22] fill launches, [23] their microseconds (HIP events), [24]
 * bytes filled, [25] bytes uploaded into the two arrays. A caller that asks for 22 gets what it always got.
 * Out of scope: the fill fused into the scatter's chunks, record numbers that live in device memory, host sources, several GPUs, element
 * types other than bytes. */
#define ZGPU_BATCH_PADDED   0u
#define ZGPU_BATCH_PACKED   1u
#define ZGPU_BATCH_TRUNCATE 1u          /* zgpu_record_batch.flags */
typedef struct {
  void*     device_dst;  uint64_t cap;  /* the batch: ONE piece of device memory, any alignment */
  uint64_t* device_lengths;             /* m values, or NULL */
  uint64_t* device_offsets;             /* m + 1 values, or NULL */
  uint64_t* host_record_bytes;          /* m values in HOST memory, or NULL: each range's length before any truncation */
  uint64_t  width;                      /* padded: bytes per row, > 0; packed: 0, or with TRUNCATE the most bytes taken of one range */
  uint32_t  layout, flags, pad_byte, reserved;
} zgpu_record_batch;
typedef struct { uint64_t total, bytes_filled; uint32_t rows_ok, rows_failed, rows_truncated, pad; } zgpu_record_batch_info;
int zgpu_gather_records_batch_indexed_device_src(zgpu_ctx*, const zgpu_seek_index*, const void* const* device_srcs, const size_t* lens, uint32_t n,
                                                 const zgpu_record_range* recs, uint32_t m, const zgpu_record_batch* batch,
                                                 const zgpu_device_opts* opts_or_null, zgpu_range_result* results /* m */,
                                                 zgpu_record_batch_info* info);

/* ---- the same over several GPUs: frames are independent, a host-side work queue shards them (no collective) -------
 * One worker thread + one engine (HIP streams, device buffers) per GPU inside the library. Replaces the frame loop of
 * FrameDecoder::decode_all (frame_decoder.rs:541-577), which decodes the frames of a buffer one after the other. */
typedef struct zgpu_pool zgpu_pool;                   /* one thread's at a time, like a context; distinct pools may run on distinct threads at once */
int zgpu_pool_create(int n_gpus /* <= 0: all visible */, zgpu_pool** out);
int zgpu_pool_create_on(const int* devices, int n, zgpu_pool** out);   /* explicit device ids (e.g. {LOCAL_RANK} in a one-process-per-GPU job) */
void zgpu_pool_destroy(zgpu_pool*);
int zgpu_pool_num_gpus(const zgpu_pool*);
/* decode_all over the pool: the buffer is cut into frames on the host, jobs (runs of frames, >= 32 MiB of input) are queued
 * largest first and pulled by two engines per GPU, so that the upload of one job, the kernels of another and the download of a
 * third overlap (pass pinned host memory for src and dst to get real DMA overlap); plaintext back to back in input order, first
 * error in input order wins. Device memory is proportional to the jobs in flight when the frames declare their content size. */
int zgpu_pool_decode_all(zgpu_pool*, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, size_t* written);
/* The plan of the queue, host only (no GPU touched): longest-processing-time-first order of n jobs by cost and the worker
 * each job goes to when n_workers workers pull in that order with time proportional to cost; load_out[w] = sum of w's costs. */
int zgpu_pool_plan(const uint64_t* cost, uint32_t n, uint32_t n_workers, uint32_t* order_out, uint32_t* worker_out, uint64_t* load_out);
/* device-resident form (bench / roofline): stage n entries (each one frame, or a run of frames) — LPT assignment over the GPUs, one
 * resident submit per GPU — then run passes over them; outputs stay in HBM. What the HOST reads must be readable in every entry —
 * frame headers, block headers, whole bodies, the literals / sequences section headers of every block (a GPU's entries are parsed as one
 * concatenation, with decode_all's rule that the first such error ends the walk): an entry that fails there fails the call — with that
 * error, or with the one its bytes yield once the next entry's follow them (a truncated entry runs into its neighbour) — and nothing stays staged. What the DEVICE finds (table descriptions, bitstreams, sequence execution) is per entry:
 * zgpu_pool_frame gives the status of the entry's first failing frame and the size of all its frames, zgpu_pool_read their bytes. */
int zgpu_pool_stage(zgpu_pool*, const uint8_t* const* frames, const size_t* lens, uint32_t n);
int zgpu_pool_run(zgpu_pool*, float* gpu_ms /* [num_gpus] kernel pipeline ms per GPU */, float* wall_ms);
/* per-kernel times of GPU g's last pass (ms, the order of zgpu_batch_timings), summed over its resident jobs, and what they hold */
int zgpu_pool_timings(const zgpu_pool*, uint32_t g, float* ms, int n, uint64_t* plain_bytes, uint64_t* comp_bytes, uint32_t* nblocks, uint32_t* njobs);
/* the LZ77 plan of GPU g's resident jobs after a run: out[0..6] = units, direct units, units without sequences, pointer-mode units,
 * sweep steps, plaintext bytes of the pointer-mode units, of the direct units (n >= 7) */
int zgpu_pool_plan_stats(const zgpu_pool*, uint32_t g, uint64_t* out, int n);
int zgpu_pool_frame(zgpu_pool*, uint32_t i, int* gpu, uint64_t* out_size, uint32_t* status);
int zgpu_pool_read(zgpu_pool*, uint32_t i, uint8_t* dst, size_t cap, size_t* written);

/* ---- staged form of the same path, for device-resident runs (bench / roofline) ----------------------------
 * (Content checksums: the reference feeds XXH64 as bytes are DRAINED (decode_buffer.rs:223-227,290,301), and output that stays in HBM is never
 *  drained. XXH64 is serial in 32-byte stripes — one 1 GB frame is 31 M dependent steps, ~0.5 s on a GPU lane against ~50 ms on a host core — so
 *  a long frame is hashed where its bytes reach the host (zgpu_decoder_* / zgpu_frame_* / zgpu_streaming_*). Many short frames are the case one
 *  lane per frame fills the chip with: zgpu_batch_checksums hashes every frame of a synced batch on the device, and zgpu_decode_frames below reports
 *  the checksums of the frames it decodes. zgpu_frame_info.checksum is the value stored in the frame; neither surface fails on a mismatch.) */
typedef struct {
  uint64_t src_begin, src_end;   /* byte range of the frame in the input */
  uint64_t window_size;          /* FrameHeader::window_size  frame.rs:116-139 */
  uint64_t frame_content_size;   /* FrameHeader::frame_content_size (0 if absent) */
  uint64_t out_base, out_size;   /* where the frame's plaintext sits in the batch output (after sync) */
  uint32_t nblocks;
  uint32_t status;               /* first error of the frame, 0 if none */
  uint32_t bad_block;            /* frame-relative index of the failing block */
  uint32_t has_checksum;         /* Content_Checksum flag + value read from the data (frame_decoder.rs:347-359) */
  uint32_t checksum;
  uint32_t pad;
} zgpu_frame_info;

/* parse the frame/block/section headers on the host and upload: after this the compressed bytes and the block
 * table are resident in HBM. Returns the frame-layer status of the walk (0, or the error decode_all would return);
 * *out is valid unless the status is ZGPU_E_NOMEM / ZGPU_E_HIP. */
int zgpu_batch_prepare(zgpu_ctx*, const uint8_t* src, size_t len, zgpu_batch** out);
int zgpu_batch_run(zgpu_batch*);                                     /* enqueue the kernels (async on the ctx stream) */
/* (*total_out = the bytes of all frames as the block walk sized them: a frame that FAILED keeps its place — its out_size in
 * zgpu_batch_frame_info ends with its last good block, the frames behind it stay where they are, total_out is not shrunk.) */
int zgpu_batch_sync(zgpu_batch*, uint64_t* total_out, uint32_t* first_bad_frame /* UINT32_MAX if none */, uint32_t* its_status);
uint32_t zgpu_batch_num_frames(const zgpu_batch*);
uint32_t zgpu_batch_num_blocks(const zgpu_batch*);
uint64_t zgpu_batch_compressed_size(const zgpu_batch*);
int zgpu_batch_frame_info(const zgpu_batch*, uint32_t frame, zgpu_frame_info* out);
int zgpu_batch_read(zgpu_batch*, uint64_t offset, uint8_t* dst, uint64_t n);   /* D2H of plaintext bytes (waits for the run like zgpu_batch_sync) */
/* after zgpu_batch_sync: out[f] = XXH64 (seed 0, all 64 bits) of frame f's output bytes as zgpu_batch_frame_info describes them — a frame that failed:
 * the bytes of its good blocks — computed on the device, one lane per frame (zg_k_xxh64). n = zgpu_batch_num_frames, else ZGPU_E_BAD_ARG. */
int zgpu_batch_checksums(zgpu_batch*, uint64_t* out, uint32_t n);
const void* zgpu_batch_output_device(const zgpu_batch*);            /* device pointer of the plaintext (no copy); valid after zgpu_batch_sync */
/* kernel times of the last run in ms, measured with HIP events on the ctx stream:
 * [0] tables [1] huffman [2] sequence chains [3] sequence post-processing [4] scan [5] literals/raw/rle [6] flatten
 * [7] sweep [8] in-order fallback [9] whole pipeline. Returns how many were written. */
int zgpu_batch_timings(const zgpu_batch*, float* ms, int n);
void zgpu_batch_destroy(zgpu_batch*);

/* intermediates of a batch, for parity tests against the oracle (blocks are numbered across the whole batch) */
typedef struct {
  uint32_t btype, lit_type, nstreams, seq_modes;
  uint32_t regen_size, nseq, frame, status;
  int32_t huf_slot, ll_slot, of_slot, ml_slot;
  uint32_t sum_ll, sum_ml;
  uint32_t hist_init[3];
  uint32_t active;
  uint64_t out_base;
} zgpu_block_info;
typedef struct { uint32_t of, ml, mdst, lit_start; } zgpu_seq;   /* of: resolved offset or symbolic (see zg_dev.h) */
int zgpu_batch_block_info(zgpu_batch*, uint32_t block, zgpu_block_info* out);
int zgpu_batch_block_literals(zgpu_batch*, uint32_t block, uint8_t* dst, size_t cap, size_t* n);
int zgpu_batch_block_sequences(zgpu_batch*, uint32_t block, zgpu_seq* dst, size_t cap, size_t* n);
/* diagnostics: cycle counters accumulated by the kernels when ZGPU_DEBUG_TIMERS is set (all zero otherwise) */
int zgpu_batch_debug_timers(zgpu_batch*, uint64_t out[1024]);
/* diagnostics for the parity tests of the LZ77 stage: the units a submit was cut into, and raw reads of the flatten
 * scratch (what = 0: one u32 effective offset per output byte of a unit, at scratch_base + position; 1: per-unit sizes) */
uint32_t zgpu_batch_num_units(const zgpu_batch*);
uint32_t zgpu_batch_debug_sweep_mode(const zgpu_batch*);   /* after sync: 0 plain chain of sweep steps, 1 split (tails / heads), 2 split, then repeated plain */
uint32_t zgpu_batch_debug_lit_direct(const zgpu_batch*);   /* after run: 1 the last run decoded its Huffman literals after the position scan (ZG_FLAG_LIT_DIRECT), 0 beside the sequences */
int zgpu_batch_unit(zgpu_batch*, uint32_t unit, uint32_t* first_block, uint32_t* nblocks, uint64_t* scratch_base);
int zgpu_batch_debug_scratch(zgpu_batch*, int what, uint64_t off, void* dst, uint64_t n);
/* diagnostics: runs kernels with known traffic per access pattern (16 B/lane copy, 4 B/lane copy, random 4- and 8-byte
 * reads) to calibrate the profiler's HBM byte counters */
int zgpu_debug_calibrate(zgpu_ctx*, uint64_t bytes);
/* diagnostics: the measurement / test switches the context's engine took when it was created. The product library reads NO environment
 * variable (every value is its default, out[0] = 0); libzgpu_dev.so (built with -DZG_DEV_SWITCHES, loaded by tests and tools/dev only) reads
 * the ZGPU_* variables of tools/dev/README.md once, at zgpu_ctx_create. out[0] development build, [1] ZGPU_UNIT_BLOCKS, [2] ZGPU_SEQ_PACKED,
 * [3] ZGPU_FLAT4, [4] ZGPU_RAMP, [5] ZGPU_SWEEP_W, [6] ZGPU_FLAT_T shape, [7] ZGPU_FORCE_INORDER. Returns how many were written. */
int zgpu_debug_tuning(const zgpu_ctx*, uint32_t* out, int n);
int zgpu_batch_fse_slot(zgpu_batch*, uint32_t slot, uint32_t* entries /* 1280 */, uint8_t logs[4]);
int zgpu_batch_huf_slot(zgpu_batch*, uint32_t slot, uint16_t* entries /* 2048 */, int* max_bits);

/* ---- FrameDecoder mirror (frame_decoder.rs:80-627): one frame at a time ---------------------------------- */
enum { ZGPU_STRAT_ALL = 0, ZGPU_STRAT_UPTO_BLOCKS = 1, ZGPU_STRAT_UPTO_BYTES = 2 };  /* BlockDecodingStrategy :96-100 */
/* add_dict (frame_decoder.rs:224-227) with Dictionary::decode_dict (dictionary.rs:45-126): raw = a zstd dictionary file */
int zgpu_add_dict(zgpu_ctx*, const uint8_t* raw, size_t len, uint32_t* id_out);
int zgpu_decoder_create(zgpu_ctx*, zgpu_decoder** out);
void zgpu_decoder_destroy(zgpu_decoder*);
/* init/reset (:190-221): parses a frame header from src; *consumed = header bytes. ZGPU_E_SKIP_FRAME fills skip_*. */
int zgpu_decoder_init(zgpu_decoder*, const uint8_t* src, size_t len, size_t* consumed, uint32_t* skip_magic, uint32_t* skip_len);
/* decode_blocks (:309-377): src continues where the previous call stopped; *consumed = bytes taken (on success: an Err of the reference
 * carries neither a count nor "finished", and the two outputs mean nothing then). The call does not look at an earlier "finished": bytes
 * handed over behind the frame's end are read as further blocks, as by the reference. After an error the decoder answers like the
 * reference's — blocks_decoded counts the blocks in front of the failing one, bytes_read_from_source their bytes plus the failing block's
 * header when it was its body that failed (:325-341), frame_finished is set by a last block whose checksum then is not there (:347-357),
 * and a block whose sequence EXECUTION fails (ZGPU_E_EXE_*) leaves behind what it had written before it failed — the output of the
 * sequences in front of the failing one, and that one's literals unless it was the literals that ran out (sequence_execution.rs:6-52) —
 * where collect() / read() still find it. (The same holds for zgpu_frame_* and zgpu_streaming_*; a frame of a many-frame submit,
 * zgpu_batch_* / zgpu_pool_*, ends with its last good block.) */
int zgpu_decoder_decode_blocks(zgpu_decoder*, const uint8_t* src, size_t len, size_t* consumed, int strat, size_t n, int* frame_finished);
/* force_dict (:229-243): use a registered dictionary although the frame header names none; like the reference, at any
 * time (tables, offset history and dictionary content are replaced for the blocks that follow) */
int zgpu_decoder_force_dict(zgpu_decoder*, uint32_t dict_id);
/* decode_from_to (:439-529): consumes only whole blocks of src, then drains into dst; *read_out / *written_out as the
 * reference's (usize, usize). May be called without init: it then parses the frame header from src itself. */
int zgpu_decoder_decode_from_to(zgpu_decoder*, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, size_t* read_out, size_t* written_out);
size_t zgpu_decoder_can_collect(const zgpu_decoder*);                /* :410-424 */
size_t zgpu_decoder_collect(zgpu_decoder*, uint8_t* dst, size_t cap);/* :381-389 */
size_t zgpu_decoder_read(zgpu_decoder*, uint8_t* dst, size_t cap);   /* impl Read :615-627 */
/* collect_to_writer (:395-407): what collect() would return goes to the writer (returns the bytes it took, io::Write::write) */
typedef size_t (*zgpu_write_fn)(void* user, const uint8_t* data, size_t n);
int zgpu_decoder_collect_to_writer(zgpu_decoder*, zgpu_write_fn write, void* user, size_t* written);
int zgpu_decoder_is_finished(const zgpu_decoder*);                   /* :284-294 */
uint64_t zgpu_decoder_blocks_decoded(const zgpu_decoder*);           /* :297 */
uint64_t zgpu_decoder_bytes_read_from_source(const zgpu_decoder*);   /* :273 */
uint64_t zgpu_decoder_content_size(const zgpu_decoder*);             /* :246 */
int zgpu_decoder_checksum_from_data(const zgpu_decoder*, uint32_t* out); /* :254 — returns 1 if present */
uint32_t zgpu_decoder_calculated_checksum(const zgpu_decoder*);      /* :263-270 XXH64 seed 0, low 32 bits */
void zgpu_decoder_set_hash(zgpu_decoder*, int on);                    /* ruzstd's `hash` cargo feature (default on): 0 = no XXH64 of the bytes handed out */
/* decode_blocks(UptoBytes(n)) decodes at least `bytes` per call (what UptoBytes(max(n, bytes)) gives in the reference): one submit lasts
 * as long as one block's sequence chain whatever it holds, so small requests are served from large submits. 0 (default): exactly n. */
void zgpu_decoder_set_read_ahead(zgpu_decoder*, uint64_t bytes);
uint64_t zgpu_decoder_device_bytes(const zgpu_decoder*);             /* device memory the frame holds now (window + carried tables): bounded by the window, not by the frame */

/* ---- the thin boundary: host-parsed block tables -----------------------------------------------------------------------
 * For a caller that keeps ruzstd's own header parse — read_frame_header (ruzstd/src/decoding/frame.rs:6-85) and
 * read_block_header (block_decoder.rs:201-247) — and hands the Block_Content of whole runs of blocks to the device: exactly the
 * seam of BlockDecoder::decode_block_content (block_decoder.rs:39-95) as FrameDecoder::decode_blocks calls it
 * (frame_decoder.rs:319-375), batched. INTEGRATION.md section 2 shows the Rust side. One zgpu_frame = one frame in flight
 * (DecoderScratch, scratch.rs:15-27, lives on the device behind it); several may exist per context. */
typedef struct zgpu_frame zgpu_frame;
typedef struct {
  uint64_t src_off;        /* offset of Block_Content in the src of the submit */
  uint32_t src_len;        /* Block_Content bytes: Block_Size for raw and compressed blocks, 1 for RLE blocks (block_decoder.rs:249-283) */
  uint32_t raw_rle_size;   /* raw / RLE blocks: decompressed size (= Block_Size); compressed blocks: 0 */
  uint8_t type;            /* 0 raw, 1 RLE, 2 compressed (blocks/block.rs:31-44) */
  uint8_t last;            /* Last_Block flag */
  uint8_t pad[6];
} zgpu_block;
/* FrameDecoderState::new/reset (frame_decoder.rs:103-134) from the header fields the caller parsed. dict_id_or_0 names a
 * dictionary registered with zgpu_add_dict (init_from_dict, scratch.rs:70-78); ZGPU_E_DICT_NOT_PROVIDED / ZGPU_E_WINDOW_SIZE_TOO_BIG
 * as the reference (:137-145, :212-219). content_size_or_0 is a hint only. */
int zgpu_frame_begin(zgpu_ctx*, uint64_t window_size, uint64_t content_size_or_0, uint32_t dict_id_or_0, zgpu_frame** out);
void zgpu_frame_end(zgpu_frame*);
/* decode_block_content x nblocks. src is copied to the device before this returns; the kernels run on the context's
 * streams. Blocks of a frame depend on each other: a second submit first waits for the one in flight. The run ends with the
 * first block marked last. */
int zgpu_blocks_submit(zgpu_frame*, const uint8_t* src, size_t src_len, const zgpu_block* blocks, size_t nblocks);
/* wait for the submit in flight. *first_bad_block = frame-relative index (counted over all submits) of the first block that
 * failed, SIZE_MAX if none; *its_status = its DecompressBlockError leaf (the zgpu_status values above). Blocks in front of
 * it are decoded and readable, like the reference's — and, like there, what the failing block itself had written when its sequence
 * execution failed (see zgpu_decoder_decode_blocks). The return value only reports engine failures (HIP, memory). */
int zgpu_sync(zgpu_frame*, size_t* first_bad_block, int32_t* its_status);
/* can_collect / read (decode_buffer.rs:182-219, frame_decoder.rs:381-424): while the frame is unfinished the last window_size
 * bytes stay back. frame_finished: the caller has submitted the last block (it reads the flag itself). */
size_t zgpu_available(const zgpu_frame*, int frame_finished);
int zgpu_read(zgpu_frame*, uint8_t* dst, size_t cap, int frame_finished, size_t* n);      /* D2H happened at zgpu_sync; this drains */
int zgpu_device_output(zgpu_frame*, const void** dptr, size_t* len);   /* the frame's most recent bytes as they sit in HBM (no copy) */
uint32_t zgpu_frame_checksum(const zgpu_frame*);         /* XXH64 (seed 0) of the bytes read so far, low 32 bits (frame_decoder.rs:263-270) */
uint64_t zgpu_frame_blocks_decoded(const zgpu_frame*);   /* frame_decoder.rs:297 */

/* ---- StreamingDecoder mirror (ruzstd/src/decoding/streaming_decoder.rs:40-156): io::Read over one frame ----------------
 * The reference decodes lazily — read(buf) runs decode_blocks(UptoBytes(missing)) until buf.len() bytes can be collected (:134-150),
 * one block per call for the 8 KiB reader std::io::copy is (cli/src/main.rs:142-144). A GPU submit lasts as long as one block's sequence
 * chain whatever it holds, so this mirror READS AHEAD: it pulls whole runs of blocks from the source, decodes run k + 1 while run k
 * travels to a pinned host ring and the reader drains run k - 1 (zg_stream.h), bounded by a budget whatever the frame's length.
 * What io::Read shows stays the reference's:
 *   - the same bytes; read() returns cap bytes unless the frame ends first, 0 at the end of the frame;
 *   - an error of block b surfaces in the read() call in which the reference would have decoded b (a run decoded ahead is only taken
 *     when no block of it failed and no sequence set an offset beyond the window — else it is dropped and the stream continues block
 *     by block from the state the reference would be in);
 *   - nothing behind the frame's last block (+ checksum) is taken from the source.
 * What differs, because blocks are decoded before the reader asks: the source is consumed earlier (by whole runs), and
 * zgpu_decoder_blocks_decoded / zgpu_decoder_bytes_read_from_source of the decoder behind the stream count what has been decoded, which
 * runs ahead of what read() has returned. zgpu_stream_opts.read_ahead_bytes = 1 switches all of that off (the reference's schedule).
 * Engine errors (ZGPU_E_HIP, ZGPU_E_NOMEM, ZGPU_E_INTERNAL from the engine — not a block's verdict, which stays the reference's) end the
 * stream: the first one is kept, the read() that meets it returns it with *n == 0, and so does every later read(), without touching the
 * engine or the source again. Bytes that were decoded and had reached the host before it are still handed out by the reads they can serve
 * in full, so every byte a read() returns is the frame's plaintext at its position and the calculated checksum is the XXH64 of exactly the
 * bytes returned; a read() that fails returns none, whatever it had written to dst. The stream's threads are gone and its ring is released
 * when that read() returns; zgpu_streaming_destroy is all that is left to do. Two things are NOT errors and stay invisible: when the worker
 * thread's side cannot be set up — the engine refuses (no device memory for the larger window) or there is no pinned memory for the ring or a
 * staging buffer — the stream goes on decoding on the caller's thread. Host memory that cannot be got inside a read() (ZGPU_E_NOMEM
 * from the library's own buffers) ends the stream in the same way. */
typedef struct zgpu_streaming zgpu_streaming;         /* its context's thread rule (context section): one thread at a time, any thread between calls */
typedef size_t (*zgpu_read_fn)(void* user, uint8_t* dst, size_t n);   /* io::Read::read of the source: 0 = end of input */
typedef struct {
  uint64_t read_ahead_bytes;   /* plaintext that may be decoded ahead of the reader = size of the pinned host ring. 0: default (512 MiB, and
                                  never less than the frame's window + 2 MiB); 1: no read-ahead at all */
  uint32_t no_checksum;        /* 1: ruzstd built without its `hash` feature — no XXH64 of the bytes handed out (one core hashes ~10-20 GB/s:
                                  with the checksum on, a hasher thread keeps it off the reader's path, but it bounds the stream) */
  uint32_t copy_threads;       /* helper threads that copy reads of 512 KiB and more out of the ring. 0: default (3); 0xFFFFFFFF: none */
  uint64_t pipe_after_bytes;   /* a frame is decoded on the caller's thread (runs of 8, 32, 128 ... blocks) until this much is decoded, or
                                  its header declares more than this; then a worker thread takes over. 0: default (32 MiB) */
  uint32_t first_run_blocks;   /* 0: default (8) */
  uint32_t pad;
} zgpu_stream_opts;
int zgpu_streaming_create(zgpu_ctx*, zgpu_read_fn read, void* user, zgpu_streaming** out);   /* new (:51-58): reads the frame header */
int zgpu_streaming_create_ex(zgpu_ctx*, zgpu_read_fn read, void* user, const zgpu_stream_opts* opts_or_null, zgpu_streaming** out);
/* the source is memory (Rust: StreamingDecoder<&[u8], _>, what the reference's benches and fuzz targets use): blocks are uploaded from where
 * they lie, nothing is copied on the host. src must stay valid until the stream is destroyed; pinned memory is DMA'd directly. */
int zgpu_streaming_create_slice(zgpu_ctx*, const uint8_t* src, size_t len, const zgpu_stream_opts* opts_or_null, zgpu_streaming** out);
size_t zgpu_streaming_source_position(const zgpu_streaming*);   /* slice sources: bytes of src taken so far (runs ahead of the reader) */
void zgpu_streaming_destroy(zgpu_streaming*);
/* get_ref / get_mut (:66-85): the decoder behind the stream — its accessors (is_finished, the checksums, the counters), can_collect / collect /
 * read (they hand out what the stream has buffered). decode_blocks / decode_from_to on it return ZGPU_E_BAD_ARG: the stream feeds it.
 * collect / read return byte counts and cannot report an error: behind a stream that an engine error has ended they return 0,
 * can_collect is 0 and is_finished stays 0 — zgpu_decoder_stream_error tells that state from a frame that merely has nothing buffered. */
zgpu_decoder* zgpu_streaming_decoder(zgpu_streaming*);
int zgpu_decoder_stream_error(const zgpu_decoder*);   /* the engine error that ended the stream this decoder is behind; 0: none, or no stream */
/* read (:119-155): *n = bytes written to dst (0 = end of frame). A nonzero return that is an engine error is final (see above): every
 * later call returns the same code and *n == 0. */
int zgpu_streaming_read(zgpu_streaming*, uint8_t* dst, size_t cap, size_t* n);
/* std::io::copy(&mut decoder, &mut writer) with a buffer of buf_size bytes (the reference's CLI: 8 KiB, cli/src/main.rs:142-144);
 * write == NULL is io::sink(). *total = bytes copied: what the writer got before the call ended, also when it returns an error. Behind
 * an engine error the stream is over; calling again returns the same code and *total == 0. */
int zgpu_streaming_copy(zgpu_streaming*, size_t buf_size, zgpu_write_fn write, void* user, uint64_t* total);
/* A stream that used a worker thread leaves its engine (streams, device buffers sized to its runs; at most two per device) and its pinned ring /
 * staging memory (at most 3 GiB) to the next stream of the process: allocating them is what a short-lived stream would otherwise spend its time on.
 * This returns all of that to the runtime. It must be called only while no stream of the process, on any thread, is in a call. */
void zgpu_release_caches(void);
/* diagnostics: out[0] mode now (0 runs on the caller's thread, 1 worker thread + ring, 2 block by block), [1] runs decoded ahead and
 * taken, [2] runs decoded ahead and dropped, [3] host bytes held (buffer + ring); [4..11] microseconds — worker thread: waiting for a run
 * from the reader, decoding (parse + upload + kernels), waiting for the previous run's download, commit, waiting for room in the ring; reader:
 * waiting for bytes, copying reads of 1 MiB and more out of the ring, taking runs from the source. Returns how many were written. */
int zgpu_streaming_stats(const zgpu_streaming*, uint64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif
