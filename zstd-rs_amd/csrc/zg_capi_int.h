// zg_capi_int.h — what the translation units behind include/zgpu.h share: the context, the dictionaries, the FrameDecoder mirror's
// state. Internal (not installed): the C ABI sees these as opaque types.
#pragma once
#include <map>
#include <string>
#include <vector>
#include "../../include/zgpu.h"
#include "zg_engine.h"
#include "zg_xxh64.h"
#include "zg_entry.h"

struct ZgDict {   // Dictionary (decoding/dictionary.rs:12-37), tables in the engine's packed formats
  uint32_t id = 0;
  std::vector<uint32_t> fse;   // one FSE arena slot
  uint8_t logs[4] = {0, 0, 0, 0};
  std::vector<uint16_t> huf;
  uint8_t huf_maxbits = 0;
  uint32_t hist[3] = {1, 4, 8};
  std::vector<uint8_t> content;
};
struct ZgDictDev {   // a dictionary's one device copy per context (zg_dictfill.h: DictImage), uploaded when a shared submit first needs it
  zg::DevBuf buf;
  zgd::DictImage im{};
};
// The slots of the context's statistics arrays, each under the key zgpu.py reports it by (include/zgpu.h: the zgpu_debug_*_stats getters).
// The arrays an engine pass is handed begin with its three slots (zg_engine.h: kPassLaunches, kPassUs, kPassBytes).
enum { kDictStatFramesShared = 0, kDictStatFillLaunches, kDictStatBytesReplicated, kDictStatFillUs, kDictStatEntriesAlone, kDictStatCount };
enum { kDevStatSubmits = 0, kDevStatScatterLaunches, kDevStatBytesScattered, kDevStatScatterUs, kDevStatFramesHashed, kDevStatFramesNotHashed,
       kDevStatEntriesAlone, kDevStatEntriesFailedVerify, kDevStatHashUs, kDevStatCount };
enum { kSrcStatWalkLaunches = 0, kSrcStatWalkUs, kSrcStatSkeletonBytes, kSrcStatGatherLaunches, kSrcStatGatherUs, kSrcStatInputBytesToHost, kSrcStatCount };
enum { kIndexStatLaunches = 0, kIndexStatKernelUs, kIndexStatBytesDownloaded, kIndexStatInputBytesToHost, kIndexStatCount };
enum { kRangeStatSeekLaunches = 0, kRangeStatSeekUs, kRangeStatSeekBytesDownloaded, kRangeStatInputBytesToHost, kRangeStatFramesSkipped,
       kRangeStatFramesDecoded, kRangeStatPlaintextDecoded, kRangeStatBytesWritten,
       // ZGPU_DEVICE_VERIFY_SEEK_TABLE (zg_seeksums.h): zg_k_seeksums launches, their time, the bytes they brought back, frames compared, entries failed
       kRangeStatCompareLaunches, kRangeStatCompareUs, kRangeStatCompareBytesDownloaded, kRangeStatFramesCompared, kRangeStatEntriesFailedTable, kRangeStatCount };
// what zgpu_debug_ranges_stats appends behind the slots above (out[13] ...): the calls that take many ranges per entry (zg_seekmany.h)
enum { kManyStatGroupsDecoded = 0, kManyStatPrefixLaunches, kManyStatPrefixUs, kManyStatFindLaunches, kManyStatFindUs, kManyStatPrefixScratchBytes,
       kManyStatCount };
// and behind those (out[19] ...): the lookup of the calls that take record numbers (zg_records.h) — zg_k_recs_find launches, their microseconds
// (HIP events), the bytes they brought back (24 per range)
enum { kRecFindStatLaunches = 0, kRecFindStatUs, kRecFindStatBytesDownloaded, kRecFindStatCount };
// and behind those (out[22] ...): the finish of a record batch (zg_scatter.h: zg_k_fill) — fill launches, their microseconds (HIP events), bytes
// filled, bytes uploaded into the batch's two arrays
enum { kBatchStatFillLaunches = 0, kBatchStatFillUs, kBatchStatBytesFilled, kBatchStatBytesUploaded, kBatchStatCount };
static_assert(kBatchStatFillLaunches == zg::kPassLaunches && kBatchStatFillUs == zg::kPassUs && kBatchStatBytesFilled == zg::kPassBytes,
              "the array handed to Engine::fill_pass");
static_assert(kSrcStatWalkLaunches == zg::kPassLaunches && kSrcStatWalkUs == zg::kPassUs && kSrcStatSkeletonBytes == zg::kPassBytes &&
              kIndexStatLaunches == zg::kPassLaunches && kIndexStatKernelUs == zg::kPassUs && kIndexStatBytesDownloaded == zg::kPassBytes &&
              kRangeStatSeekLaunches == zg::kPassLaunches && kRangeStatSeekUs == zg::kPassUs && kRangeStatSeekBytesDownloaded == zg::kPassBytes,
              "the arrays handed to Engine::walk_entries, index_pass and seek_pass / seektab_pass");

struct zgpu_ctx {
  zg::Engine* eng = nullptr;
  std::map<uint32_t, ZgDict> dicts;   // FrameDecoder::dicts (frame_decoder.rs:82)
  std::map<uint32_t, zg::DictFacts> dict_facts;   // what the walk of a shared submit is told of each (zgpu_add_dict keeps it in step with dicts)
  std::map<uint32_t, ZgDictDev> dict_dev;         // freed with the context; an entry goes when zgpu_add_dict replaces its dictionary
  bool frames_shared_dicts = false;               // zgpu_set_frames_shared_dicts
  uint32_t frames_submits = 0;        // submits the last zgpu_decode_frames call ran (zgpu_debug_frames_submits)
  // of the last call of their family (zg_frames_int.h: reset_stats says which call owns which)
  uint64_t frames_dict_stats[kDictStatCount] = {};        // zgpu_decode_frames* and the decode_ranges calls (zgpu_debug_frames_dict_stats)
  uint64_t frames_device_stats[kDevStatCount] = {};       // the calls with a device sink (zgpu_debug_frames_device_stats)
  uint64_t frames_device_src_stats[kSrcStatCount] = {};   // the calls with device sources (zgpu_debug_frames_device_src_stats)
  uint64_t frames_index_stats[kIndexStatCount] = {};      // zgpu_frames_index_device / zgpu_frames_table_device (zgpu_debug_frames_index_stats)
  uint64_t ranges_stats[kRangeStatCount] = {};            // the seek and decode_ranges calls (zgpu_debug_ranges_stats)
  uint64_t ranges_many_stats[kManyStatCount] = {};        //   the slots behind them (zgpu_frames_seek_table_many_device, zgpu_gather_ranges_seek_table_device_src)
  uint64_t ranges_rec_stats[kRecFindStatCount] = {};      //   and behind those (zgpu_seek_index_record_ranges_device, zgpu_gather_records_indexed_device_src)
  uint64_t ranges_batch_stats[kBatchStatCount] = {};      //   and behind those (zgpu_gather_records_batch_indexed_device_src)
  uint64_t hash_ranges_us = 0;                          // kernel time of the last zgpu_debug_hash_ranges call (HIP events)
  std::string err;
};

// A seek index (include/zgpu.h: zgpu_seek_index): the pairs { C[k], D[k] } of every indexed entry in device memory, and per entry where they
// lie and what the selection needs besides. No source pointer: offsets only.
enum { kSeekIdxStatLaunches = 0, kSeekIdxStatKernelUs, kSeekIdxStatBytesDownloaded, kSeekIdxStatDeviceBytes, kSeekIdxStatRows, kSeekIdxStatInputBytesToHost,
       // zgpu_seek_index_measure_device: measuring submits (Batch::measure), their phase-1 microseconds (HIP events), zstd frames measured
       kSeekIdxStatMeasureSubmits, kSeekIdxStatMeasureUs, kSeekIdxStatFramesMeasured, kSeekIdxStatCount };
// what zgpu_seek_index_stats appends behind the slots above (out[9] ...): zgpu_seek_index_hash_device, summed over its calls — decode submits, the
// hash kernels' microseconds (HIP events), zstd frames hashed —; the bytes of sums the handle holds now (0 until an entry gets sums); the
// runs the passes cut
enum { kSumStatHashSubmits = 0, kSumStatHashUs, kSumStatFramesHashed, kSumStatSumsBytes, kSumStatHashRuns, kSumStatCount };
// and behind those (out[14] ...): zgpu_seek_index_records_device, summed over its calls — decode submits, the microseconds of zg_k_recs_count,
// _scan and _emit (HIP events), chunks scanned, bytes the side pass brought back (totals, open-tail probes) —; what the handle holds now:
// records, bytes of offsets
enum { kRecStatSubmits = 0, kRecStatUs, kRecStatChunks, kRecStatRecordsHeld, kRecStatOffsetBytes, kRecStatBytesDownloaded, kRecStatCount };
static_assert(kSeekIdxStatLaunches == zg::kPassLaunches && kSeekIdxStatKernelUs == zg::kPassUs && kSeekIdxStatBytesDownloaded == zg::kPassBytes,
              "the array handed to the passes of the build");
struct zgpu_seek_index {
  zgpu_ctx* ctx = nullptr;
  zg::DevBuf pairs;                      // 16 * (nrows + 1) bytes per indexed entry, back to back
  uint64_t npairs = 0;                   // pairs of all indexed entries
  // pre: the index of the entry's pair 0; tab: where its table frame begins (declared kind: len); spre: the index of its sum 0; sums: what
  // zgpu_seek_index_sums_of answers (state 0: the handle vouches for nothing of it)
  // rpre: the index of the entry's O[0] in recs (recs.state != 0); recs: what zgpu_seek_index_records_of answers
  struct Ent { zgpu_seek_index_info info; uint64_t pre, tab, spre; zgpu_seek_index_sums sums; uint64_t rpre = 0; zgpu_seek_index_records recs = {}; };
  std::vector<Ent> ents;
  zg::DevBuf sums;                       // 4 bytes per row of every indexed entry, in the pairs' order; allocated when the first entry gets sums
  uint64_t nsums = 0;                    // rows of all indexed entries
  uint64_t stats[kSeekIdxStatCount] = {};
  uint64_t sums_stats[kSumStatCount] = {};
  zg::DevBuf recs;                       // the record offsets (zg_records.h): 8 * (nrecords + 1) bytes per entry that has records, in entry order
  uint64_t nrec_slots = 0;               // offsets of all such entries
  uint64_t rec_stats[kRecStatCount] = {};
};

namespace zg { class StreamCore; }

// ---- FrameDecoder mirror (frame_decoder.rs:80-627) ---------------------------------------------------------------------------
struct zgpu_decoder {
  zgpu_ctx* ctx = nullptr;
  bool has_state = false;
  zg::FrameHeader fh;
  uint64_t window_size = 0;
  bool frame_finished = false;
  uint64_t block_counter = 0, bytes_read = 0;
  bool has_checksum = false;
  uint32_t checksum = 0;
  uint32_t using_dict = 0;
  zg::FrameState fs;             // device side of DecoderScratch
  std::vector<uint8_t> buf;      // decoded, not yet drained bytes (DecodeBuffer, decode_buffer.rs:9-17)
  size_t head = 0;
  zg::Xxh64 hash;
  bool hash_on = true;           // ruzstd's `hash` cargo feature (default on): XXH64 of the drained bytes (decode_buffer.rs:42,223-227)
  size_t held() const { return buf.size() - head; }
  uint32_t drain_rule = 0;       // how the surface driving this decoder drains the reference's DecodeBuffer inside one run (zg_exact.h: ZG_DRAIN_*)
  uint64_t read_ahead = 0;       // zgpu_decoder_set_read_ahead: decode_blocks(UptoBytes(n)) decodes at least this many bytes per call (0: exactly the reference's n)
  zg::StreamCore* stream = nullptr;   // the streaming decoder that drives this decoder (zg_stream.h): while it reads ahead, the counters and the
                                      // buffered bytes live there and the accessors below ask it
};

// (zg_capi.cpp) DecodeBuffer::drain_to (decode_buffer.rs:256-314) on the mirror's host buffer; DecoderScratch::init_from_dict (scratch.rs:70-78)
size_t zg_dec_drain(zgpu_decoder* d, size_t n, uint8_t* dst);
int zg_apply_dict(zgpu_decoder* d, const ZgDict& dict);

// (zg_stream.cpp) what the decoder behind a streaming decoder answers while the stream owns its buffered bytes and counters
bool zg_stream_is_finished(const zg::StreamCore* c);
size_t zg_stream_can_collect(const zg::StreamCore* c);
uint64_t zg_stream_blocks_decoded(const zg::StreamCore* c);
uint64_t zg_stream_bytes_read(const zg::StreamCore* c);
bool zg_stream_checksum_from_data(const zg::StreamCore* c, uint32_t* out);
uint32_t zg_stream_calculated_checksum(zg::StreamCore* c);
uint64_t zg_stream_host_bytes(const zg::StreamCore* c);
int zg_stream_error(const zg::StreamCore* c);                          // the engine error that ended the stream (0: none)
size_t zg_stream_take(zg::StreamCore* c, uint8_t* dst, size_t n);   // n <= can_collect: bytes that are buffered already

// (zg_capi.cpp) FrameDecoder::decode_all frame by frame through the FrameDecoder mirror (the path of dictionary frames); frames, if given, collects
// the facts of every frame it decoded (zg_entry.h): bytes [begin, begin + clen) of src, what it yielded, what it declares, its Content_Checksum
// and the low 32 bits of the XXH64 of what it yielded — the decoder hashes what is drained: every frame is hashed, its slot is its index
int zg_decode_all_per_frame(zgpu_ctx* c, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, size_t* written, std::vector<zge::Frame>* frames);
// (zg_stream.cpp) the process-wide cache of pinned host blocks the streams use; nullptr if none can be had
void* zg_pinned_get(size_t n);
void zg_pinned_put(void* p);
