"""ctypes binding of libzgpu.so (include/zgpu.h) + thin Python mirrors of the reference's decoder surface.

Names follow ruzstd (FrameDecoder, StreamingDecoder, decode_all, decode_blocks, collect ...). There is no CPU path:
if libzgpu.so is missing or no gfx950 device is usable, construction raises.
"""
import ctypes as C
import os
import struct
from array import array

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZGPU_LIB") or os.path.join(HERE, "libzgpu.so")   # ZGPU_LIB: a profiling build (tools/dev)
# the development build (-DZG_DEV_SWITCHES): the only library that reads the ZGPU_* measurement / test switches. Tests that force a path
# and tools/dev ask for it explicitly (Context(dev=True)); the product library ignores the environment.
DEV_LIB_PATH = os.path.join(HERE, "libzgpu_dev.so")
_LIB = None
_DEV_LIB = None

STRAT_ALL, STRAT_UPTO_BLOCKS, STRAT_UPTO_BYTES = 0, 1, 2
E_SKIP_FRAME = 1
E_WINDOW_SIZE_TOO_BIG = 6
E_DICT_NOT_PROVIDED = 7
E_FAILED_READ_BLOCK_HEADER, E_FAILED_READ_BLOCK_BODY, E_FAILED_READ_CHECKSUM = 9, 10, 11
E_TARGET_TOO_SMALL = 12
E_FAILED_SKIP_FRAME = 13
E_RESERVED_BLOCK, E_BLOCK_SIZE_TOO_LARGE = 20, 21
E_CHECKSUM_MISMATCH = 70    # decode_frames_device / decode_frames_device_src with verify=True only (no counterpart in the reference)
E_SEEK_TABLE = 72              # the seek-table calls only: the entry does not end in a usable seek table (Seek.why: SEEKTAB_*)
SEEKTAB_NONE, SEEKTAB_RESERVED_BITS, SEEKTAB_TOO_LARGE, SEEKTAB_BAD_FRAME, SEEKTAB_PAST_TABLE = 16, 17, 18, 19, 20
E_CONTENT_SIZE_MISMATCH = 71   # decode_ranges_device_src only: a taken frame decoded to another length than it declares (no counterpart in the reference)
E_SEEK_CHECKSUM_MISMATCH = 73  # decode_ranges_seek_table_device_src with verify_table=True only: the entry decoded, and its seek table does not vouch for the bytes
E_FRAME_INDEX = 74             # a SeekIndex entry, and the ranges that name it: the header chain yields no index (SeekIndexInfo.why: CHAIN_* reason, INDEX_UNSIZED)
INDEX_SEEK_TABLE, INDEX_DECLARED, INDEX_AUTO = 0, 1, 2   # zgpu_seek_index_create_device's kind
INDEX_UNSIZED = 32             # SeekIndexInfo.why: a zstd frame declares no Frame_Content_Size
_INDEX_KINDS = {"seek_table": INDEX_SEEK_TABLE, "declared": INDEX_DECLARED, "auto": INDEX_AUTO}
INDEX_MEASURED = 3             # SeekIndexInfo.kind only (Context.seek_index_measured): the entry's frames were measured on the device
INDEX_UNMEASURED = 33          # SeekIndexInfo.why: a frame of the entry could not be measured (its headers or its sequence stage fail)
INDEX_DICT = 34                # SeekIndexInfo.why: a frame of the entry names a dictionary id
MEASURE_ALL, MEASURE_UNSIZED = 0, 1   # zgpu_seek_index_measure_device's mode
E_UNSUPPORTED = 80
E_HIP = 92
E_BAD_ARG = 93

# The statistics getters: the C function each reads and the keys of its slots, in the order of the enumerators that are named after them
# (csrc/zg_capi_int.h: kDictStat*, kDevStat*, kSrcStat*, kIndexStat*, kRangeStat*). _read_stats reads through it.
_TIMING_KEYS = ("tables", "huf", "seq", "seqpost", "scan", "lit", "flat", "sweep", "lz", "total")   # csrc/zg_engine.h: ZG_T_*
_STATS = {
    "Context.frames_dict_stats": ("zgpu_debug_frames_dict_stats", C.c_uint64,
                                  ("frames_shared", "fill_launches", "bytes_replicated", "fill_us", "entries_alone")),
    "Context.frames_device_stats": ("zgpu_debug_frames_device_stats", C.c_uint64,
                                    ("submits", "scatter_launches", "bytes_scattered", "scatter_us", "frames_hashed", "frames_not_hashed",
                                     "entries_alone", "entries_failed_verify", "hash_us")),
    "Context.frames_device_src_stats": ("zgpu_debug_frames_device_src_stats", C.c_uint64,
                                        ("walk_launches", "walk_us", "skeleton_bytes", "gather_launches", "gather_us", "input_bytes_to_host")),
    "Context.frames_index_stats": ("zgpu_debug_frames_index_stats", C.c_uint64,
                                   ("launches", "kernel_us", "bytes_downloaded", "input_bytes_to_host")),
    "Context.ranges_stats": ("zgpu_debug_ranges_stats", C.c_uint64,
                             ("seek_launches", "seek_us", "seek_bytes_downloaded", "input_bytes_to_host", "frames_skipped", "frames_decoded",
                              "plaintext_decoded", "bytes_written",
                              "compare_launches", "compare_us", "compare_bytes_downloaded", "frames_compared", "entries_failed_table")),
    "SeekIndex.stats": ("zgpu_seek_index_stats", C.c_uint64,
                        ("launches", "kernel_us", "bytes_downloaded", "device_bytes", "rows", "input_bytes_to_host",
                         "measure_submits", "measure_us", "frames_measured")),
    # the same getter asked for the slots zgpu_seek_index_hash_device appends (csrc/zg_capi_int.h: kSeekIdxStatHash*)
    "SeekIndex.sums_stats": ("zgpu_seek_index_stats", C.c_uint64,
                             ("launches", "kernel_us", "bytes_downloaded", "device_bytes", "rows", "input_bytes_to_host",
                              "measure_submits", "measure_us", "frames_measured",
                              "hash_submits", "hash_us", "frames_hashed", "sums_bytes", "hash_runs")),
    # the same getter asked for the slots zgpu_seek_index_records_device appends behind those (csrc/zg_capi_int.h: kRecStat*)
    "SeekIndex.records_stats": ("zgpu_seek_index_stats", C.c_uint64,
                                ("launches", "kernel_us", "bytes_downloaded", "device_bytes", "rows", "input_bytes_to_host",
                                 "measure_submits", "measure_us", "frames_measured",
                                 "hash_submits", "hash_us", "frames_hashed", "sums_bytes", "hash_runs",
                                 "records_submits", "records_us", "records_chunks", "records_held", "records_offset_bytes",
                                 "records_bytes_downloaded")),
    "Context.tuning": ("zgpu_debug_tuning", C.c_uint32,
                       ("dev_build", "unit_blocks", "seq_packed", "flat4", "ramp_percent", "sweep_w", "flat_shape", "force_inorder",
                        "poison", "poisoned_lo", "poisoned_hi", "scratch_cap_lo", "scratch_cap_hi")),
    "Pool.plan_stats": ("zgpu_pool_plan_stats", C.c_uint64,
                        ("units", "direct_units", "noseq_units", "pointer_units", "sweep_steps", "pointer_bytes", "direct_bytes")),
    "CStreamingDecoder.stats": ("zgpu_streaming_stats", C.c_uint64,
                                ("mode", "runs", "dropped", "host_bytes", "us_worker_idle", "us_run", "us_land", "us_commit", "us_ring_full",
                                 "us_reader_wait", "us_reader_copy", "us_pull", "us_prepare", "us_kernels") + tuple("k_" + k for k in _TIMING_KEYS)),
}


def _read_stats(L, getter, *handle, slots=None, counted=True):
    """What getter's C function (_STATS) writes for handle, under the table's keys. slots: how many to ask for (default: all). counted: the
    function returns how many slots it filled, and the dict holds those; else it returns a status, raised unless 0."""
    fn, ctype, keys = _STATS[getter]
    a = (ctype * len(keys))()
    k = getattr(L, fn)(*handle, a, len(keys) if slots is None else slots)
    if not counted:
        if k:
            raise ZgpuError(k)
        k = len(keys)
    return dict(zip(keys[:k], a[:k]))


class EntryResultC(C.Structure):
    _fields_ = [("written", C.c_uint64), ("status", C.c_int32), ("nframes", C.c_uint32), ("checksums", C.c_uint32),
                ("checksum_mismatches", C.c_uint32), ("checksum_from_data", C.c_uint32), ("calculated_checksum", C.c_uint32)]


class EntryResult:
    """One entry of Context.decode_frames (zgpu_entry_result): status is what decode_all of the entry alone returns; data its plaintext
    (None unless status == 0); the checksum fields are reported, never enforced."""
    __slots__ = ("status", "data", "written", "nframes", "checksums", "checksum_mismatches", "checksum_from_data", "calculated_checksum")

    def __repr__(self):
        return "EntryResult(status=%d, written=%d, nframes=%d, checksums=%d, mismatches=%d)" % (
            self.status, self.written, self.nframes, self.checksums, self.checksum_mismatches)


class DeviceOptsC(C.Structure):
    """zgpu_device_opts (include/zgpu.h)"""
    _fields_ = [("hash_max_bytes", C.c_uint64), ("flags", C.c_uint32), ("pad", C.c_uint32)]


class DeviceEntryResultC(C.Structure):
    _fields_ = [("r", EntryResultC), ("checksums_unverified", C.c_uint32), ("first_hashed", C.c_uint32)]


class DeviceEntryResult:
    """One entry of Context.decode_frames_device (zgpu_device_entry_result): the fields of EntryResult without data — on status 0 the first
    `written` bytes of the entry's destination are the plaintext — plus checksums_unverified (frames with a Content_Checksum that were not
    hashed) and first_hashed (whether calculated_checksum is the first frame's real XXH64)."""
    __slots__ = ("status", "written", "nframes", "checksums", "checksum_mismatches", "checksum_from_data", "calculated_checksum",
                 "checksums_unverified", "first_hashed")

    def __repr__(self):
        return "DeviceEntryResult(status=%d, written=%d, nframes=%d, checksums=%d, mismatches=%d, unverified=%d)" % (
            self.status, self.written, self.nframes, self.checksums, self.checksum_mismatches, self.checksums_unverified)


# why a header chain ended (zgpu_entry_index.why, ZGPU_CHAIN_*)
(CHAIN_END, CHAIN_SHORT_HEADER, CHAIN_BAD_MAGIC, CHAIN_SKIP_PAST_END, CHAIN_SHORT_BLOCK_HEADER, CHAIN_RESERVED_BLOCK, CHAIN_BLOCK_TOO_LARGE,
 CHAIN_BODY_PAST_END, CHAIN_SHORT_CHECKSUM) = range(9)


class EntryIndexC(C.Structure):
    """zgpu_entry_index (include/zgpu.h)"""
    _fields_ = [("bound", C.c_uint64), ("chain_end", C.c_uint64), ("status", C.c_uint32), ("nframes", C.c_uint32), ("nskippable", C.c_uint32),
                ("nblocks", C.c_uint32), ("why", C.c_uint32), ("flags", C.c_uint32)]


class FrameIndexC(C.Structure):
    """zgpu_frame_index (include/zgpu.h)"""
    _fields_ = [("src_begin", C.c_uint64), ("src_end", C.c_uint64), ("bound", C.c_uint64), ("frame_content_size", C.c_uint64),
                ("window_size", C.c_uint64), ("entry", C.c_uint32), ("nblocks", C.c_uint32), ("dict_id", C.c_uint32), ("flags", C.c_uint32),
                ("header_status", C.c_uint32), ("skip_magic", C.c_uint32)]


class EntryIndex:
    """One entry of Context.frames_index_device (zgpu_entry_index): bound is plaintext_bound of the entry's bytes; status is 0, or E_BAD_ARG for
    a source that failed the pointer check (every other field is 0 then). flags: all_sized (every frame declares its content size), any_dict,
    any_checksum, all_complete — of the nframes zstd frames, all False if there is none."""
    __slots__ = ("bound", "chain_end", "status", "nframes", "nskippable", "nblocks", "why", "flags", "all_sized", "any_dict", "any_checksum",
                 "all_complete")

    def __init__(self, c):
        for k in ("bound", "chain_end", "status", "nframes", "nskippable", "nblocks", "why", "flags"):
            setattr(self, k, int(getattr(c, k)))
        self.all_sized, self.any_dict = bool(self.flags & 1), bool(self.flags & 2)
        self.any_checksum, self.all_complete = bool(self.flags & 4), bool(self.flags & 8)

    def __repr__(self):
        return "EntryIndex(status=%d, bound=%d, nframes=%d, nskippable=%d, nblocks=%d, chain_end=%d, why=%d, flags=%#x)" % (
            self.status, self.bound, self.nframes, self.nskippable, self.nblocks, self.chain_end, self.why, self.flags)


class FrameIndex:
    """One frame of Context.frames_table_device (zgpu_frame_index): [src_begin, src_end) in entry `entry`, its share of the entry's bound, and
    what its header says. header_status is 0 for a zstd frame, E_SKIP_FRAME for a skippable one, else the error of a header the chain could
    not read (the entry's last record then, src_begin == src_end)."""
    __slots__ = ("src_begin", "src_end", "bound", "frame_content_size", "window_size", "entry", "nblocks", "dict_id", "flags", "header_status",
                 "skip_magic", "skippable", "has_content_size", "has_checksum", "complete", "single_segment")

    def __init__(self, c):
        for k in ("src_begin", "src_end", "bound", "frame_content_size", "window_size", "entry", "nblocks", "dict_id", "flags", "header_status",
                  "skip_magic"):
            setattr(self, k, int(getattr(c, k)))
        f = self.flags
        self.skippable, self.has_content_size, self.has_checksum = bool(f & 1), bool(f & 2), bool(f & 4)
        self.complete, self.single_segment = bool(f & 8), bool(f & 16)

    def __repr__(self):
        return "FrameIndex(entry=%d, [%d, %d), bound=%d, nblocks=%d, header_status=%d, flags=%#x)" % (
            self.entry, self.src_begin, self.src_end, self.bound, self.nblocks, self.header_status, self.flags)


class RangeC(C.Structure):
    """zgpu_range (include/zgpu.h)"""
    _fields_ = [("begin", C.c_uint64), ("len", C.c_uint64), ("anchor_src", C.c_uint64), ("anchor_plain", C.c_uint64)]


class EntryRangeC(C.Structure):
    """zgpu_entry_range (include/zgpu.h)"""
    _fields_ = [("begin", C.c_uint64), ("len", C.c_uint64), ("entry", C.c_uint32), ("pad", C.c_uint32)]


class SeekC(C.Structure):
    """zgpu_seek (include/zgpu.h)"""
    _fields_ = [("src_lo", C.c_uint64), ("src_hi", C.c_uint64), ("plain_lo", C.c_uint64), ("bound", C.c_uint64), ("plain_seen", C.c_uint64),
                ("status", C.c_uint32), ("frames_skipped", C.c_uint32), ("frames_taken", C.c_uint32), ("nblocks", C.c_uint32),
                ("why", C.c_uint32), ("flags", C.c_uint32)]


class RangeResultC(C.Structure):
    """zgpu_range_result (include/zgpu.h)"""
    _fields_ = [("d", DeviceEntryResultC), ("seek", SeekC)]


class SeekIndexInfoC(C.Structure):
    """zgpu_seek_index_info (include/zgpu.h)"""
    _fields_ = [("len", C.c_uint64), ("compressed", C.c_uint64), ("plaintext", C.c_uint64), ("status", C.c_uint32), ("why", C.c_uint32),
                ("kind", C.c_uint32), ("nrows", C.c_uint32)]


class SeekIndexInfo:
    """One entry of a SeekIndex (zgpu_seek_index_info): len, the entry's bytes when it was indexed; compressed = C[nrows], plaintext = D[nrows];
    status 0, E_BAD_ARG, E_SEEK_TABLE or E_FRAME_INDEX with why (SEEKTAB_*, a CHAIN_* reason, INDEX_UNSIZED, INDEX_UNMEASURED, INDEX_DICT); kind
    INDEX_SEEK_TABLE, INDEX_DECLARED or INDEX_MEASURED: what the entry was indexed by; nrows, its rows (frames, skippable ones included)."""
    __slots__ = FIELDS = ("len", "compressed", "plaintext", "status", "why", "kind", "nrows")

    def __init__(self, c):
        for k in self.FIELDS:
            setattr(self, k, int(getattr(c, k)))

    def __repr__(self):
        return "SeekIndexInfo(status=%d, why=%d, kind=%d, nrows=%d, len=%d, compressed=%d, plaintext=%d)" % (
            self.status, self.why, self.kind, self.nrows, self.len, self.compressed, self.plaintext)


class SeekIndexSumsC(C.Structure):
    """zgpu_seek_index_sums (include/zgpu.h)"""
    _fields_ = [("status", C.c_uint32), ("state", C.c_uint32), ("row_lo", C.c_uint32), ("row_hi", C.c_uint32), ("frames", C.c_uint64),
                ("bytes", C.c_uint64)]


SUMS_NONE, SUMS_HASHED, SUMS_SET = 0, 1, 2   # SeekIndexSums.state
EXPORT_CHECKSUMS = 1                         # zgpu_seek_index_export_seek_table_ex's flags


class SeekIndexSums:
    """What a SeekIndex knows of one entry's sums (zgpu_seek_index_sums): state SUMS_NONE, SUMS_HASHED or SUMS_SET; status of the last
    SeekIndex.hash that chose the entry (0, the index's status, E_BAD_ARG, or the failing run's with its rows [row_lo, row_hi)); frames and
    bytes: the zstd frames and plaintext bytes hashed."""
    __slots__ = FIELDS = ("status", "state", "row_lo", "row_hi", "frames", "bytes")

    def __init__(self, c):
        for k in self.FIELDS:
            setattr(self, k, int(getattr(c, k)))

    def __repr__(self):
        return "SeekIndexSums(status=%d, state=%d, rows=[%d, %d), frames=%d, bytes=%d)" % (
            self.status, self.state, self.row_lo, self.row_hi, self.frames, self.bytes)


class SeekIndexRecordsC(C.Structure):
    """zgpu_seek_index_records (include/zgpu.h)"""
    _fields_ = [("status", C.c_uint32), ("state", C.c_uint32), ("delimiter", C.c_uint32), ("flags", C.c_uint32), ("nrecords", C.c_uint64),
                ("row_lo", C.c_uint32), ("row_hi", C.c_uint32)]


class RecordRangeC(C.Structure):
    """zgpu_record_range (include/zgpu.h)"""
    _fields_ = [("first", C.c_uint64), ("count", C.c_uint64), ("entry", C.c_uint32), ("flags", C.c_uint32)]


class RecordBatchC(C.Structure):
    """zgpu_record_batch (include/zgpu.h)"""
    _fields_ = [("device_dst", C.c_void_p), ("cap", C.c_uint64), ("device_lengths", C.c_void_p), ("device_offsets", C.c_void_p),
                ("host_record_bytes", C.POINTER(C.c_uint64)), ("width", C.c_uint64), ("layout", C.c_uint32), ("flags", C.c_uint32),
                ("pad_byte", C.c_uint32), ("reserved", C.c_uint32)]


class RecordBatchInfoC(C.Structure):
    """zgpu_record_batch_info (include/zgpu.h)"""
    _fields_ = [("total", C.c_uint64), ("bytes_filled", C.c_uint64), ("rows_ok", C.c_uint32), ("rows_failed", C.c_uint32),
                ("rows_truncated", C.c_uint32), ("pad", C.c_uint32)]


class RecordBatchInfo:
    """What Context.gather_records_batch says of the batch it wrote (zgpu_record_batch_info): total — the bytes the layout needs —,
    bytes_filled — pad bytes written —, rows_ok, rows_failed (rows with a status), rows_truncated."""
    __slots__ = FIELDS = ("total", "bytes_filled", "rows_ok", "rows_failed", "rows_truncated")

    def __init__(self, c):
        for k in self.FIELDS:
            setattr(self, k, int(getattr(c, k)))

    def __repr__(self):
        return "RecordBatchInfo(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k in self.FIELDS)


BATCH_PADDED, BATCH_PACKED = 0, 1                    # zgpu_record_batch.layout
BATCH_TRUNCATE = 1                                   # zgpu_record_batch.flags
_BATCH_LAYOUTS = {"padded": BATCH_PADDED, "packed": BATCH_PACKED}
RECORDS_NONE, RECORDS_FOUND, RECORDS_SET = 0, 1, 2   # SeekIndexRecords.state
RECORDS_STRIP = 1                                    # zgpu_record_range.flags
RECORDS_OPEN_TAIL = 0x80000000                       # zgpu_seek_index_set_records' delimiter word


class SeekIndexRecords:
    """What a SeekIndex knows of one entry's record offsets (zgpu_seek_index_records): state RECORDS_NONE, RECORDS_FOUND or RECORDS_SET;
    status of the last SeekIndex.records that chose the entry (0, the index's status, E_BAD_ARG, or the failing run's with its rows
    [row_lo, row_hi)); delimiter; flags bit 0 (open_tail): the last record ends in no delimiter; nrecords."""
    __slots__ = FIELDS = ("status", "state", "delimiter", "flags", "nrecords", "row_lo", "row_hi")

    def __init__(self, c):
        for k in self.FIELDS:
            setattr(self, k, int(getattr(c, k)))

    @property
    def open_tail(self):
        return bool(self.flags & 1)

    def __repr__(self):
        return "SeekIndexRecords(status=%d, state=%d, delimiter=%d, flags=%d, nrecords=%d, rows=[%d, %d))" % (
            self.status, self.state, self.delimiter, self.flags, self.nrecords, self.row_lo, self.row_hi)


class Seek:
    """One entry of Context.frames_seek_device (zgpu_seek): the whole frames [src_lo, src_hi) of the entry that hold the range, the plaintext
    offset plain_lo of the first of them, bound = plaintext_bound of those bytes. flags: open_ended (an unsized frame was taken: everything
    behind it is decoded too), broken (the header chain broke: why says how), nothing (the range lies behind the plaintext)."""
    __slots__ = ("src_lo", "src_hi", "plain_lo", "bound", "plain_seen", "status", "frames_skipped", "frames_taken", "nblocks", "why", "flags",
                 "open_ended", "broken", "nothing")
    FIELDS = __slots__[:11]

    def __init__(self, c):
        for k in self.FIELDS:
            setattr(self, k, int(getattr(c, k)))
        self.open_ended, self.broken, self.nothing = bool(self.flags & 1), bool(self.flags & 2), bool(self.flags & 4)

    def key(self):
        return tuple(getattr(self, k) for k in self.FIELDS)

    def __repr__(self):
        return "Seek(status=%d, src=[%d, %d), plain_lo=%d, bound=%d, skipped=%d, taken=%d, nblocks=%d, why=%d, flags=%#x)" % (
            self.status, self.src_lo, self.src_hi, self.plain_lo, self.bound, self.frames_skipped, self.frames_taken, self.nblocks, self.why,
            self.flags)


def anchor_before(frames, offset, entry=0):
    """The anchor nearest in front of plaintext offset `offset` of entry `entry`, from the FrameIndex records of Context.frames_table_device:
    (anchor_src, anchor_plain) of the last frame boundary whose declared plaintext offset is <= offset, with every zstd frame in front of it
    declaring its content size (behind an unsized frame no offset is known, so no later boundary is an anchor). (0, 0) if there is none."""
    best, plain = (0, 0), 0
    for f in frames:
        if f.entry != entry:
            continue
        if plain <= offset:
            best = (f.src_begin, plain)
        if f.header_status != 0:
            if f.header_status == E_SKIP_FRAME:
                continue
            break
        if not f.has_content_size or not f.complete:
            break
        plain += f.frame_content_size
        if plain > offset:
            break
    return best


def seek_table_frame(csizes, dsizes, checksums=None):
    """The seek table of zstd's seekable format for frames of csizes[k] compressed and dsizes[k] decompressed bytes (a skippable frame is
    entered with dsize 0): the skippable frame that, appended behind those frames, makes an entry seekable for
    Context.decode_ranges_seek_table_device_src. checksums[k]: the low 32 bits of the XXH64 (seed 0) of frame k's plaintext; None: the table
    carries none. Host only."""
    n = len(csizes)
    if len(dsizes) != n or (checksums is not None and len(checksums) != n):
        raise ValueError("seek_table_frame: one size pair (and one checksum) per frame")
    if n > 0x8000000:
        raise ValueError("seek_table_frame: more than 0x8000000 frames")
    es = 8 if checksums is None else 12
    out = [struct.pack("<II", 0x184D2A5E, n * es + 9)]
    for k in range(n):
        out.append(struct.pack("<II", int(csizes[k]), int(dsizes[k])))
        if checksums is not None:
            out.append(struct.pack("<I", int(checksums[k]) & 0xFFFFFFFF))
    out.append(struct.pack("<IBI", n, 0 if checksums is None else 0x80, 0x8F92EAB1))
    return b"".join(out)


def plaintext_bound(buf):
    """zgpu_plaintext_bound: an upper bound of the plaintext of concatenated frames from frame and block headers only (a frame's declared
    content size when smaller; a compressed block counts 128 KiB); the walk stops where a header cannot be read. Decode_frames' default
    capacity and what it cuts its submits by. Host only (no GPU touched)."""
    b = bytes(buf)
    return load_library().zgpu_plaintext_bound(b, len(b))


class FrameInfo(C.Structure):
    _fields_ = [("src_begin", C.c_uint64), ("src_end", C.c_uint64), ("window_size", C.c_uint64), ("frame_content_size", C.c_uint64),
                ("out_base", C.c_uint64), ("out_size", C.c_uint64), ("nblocks", C.c_uint32), ("status", C.c_uint32),
                ("bad_block", C.c_uint32), ("has_checksum", C.c_uint32), ("checksum", C.c_uint32), ("pad", C.c_uint32)]


class BlockInfo(C.Structure):
    _fields_ = [("btype", C.c_uint32), ("lit_type", C.c_uint32), ("nstreams", C.c_uint32), ("seq_modes", C.c_uint32),
                ("regen_size", C.c_uint32), ("nseq", C.c_uint32), ("frame", C.c_uint32), ("status", C.c_uint32),
                ("huf_slot", C.c_int32), ("ll_slot", C.c_int32), ("of_slot", C.c_int32), ("ml_slot", C.c_int32),
                ("sum_ll", C.c_uint32), ("sum_ml", C.c_uint32), ("hist_init", C.c_uint32 * 3), ("active", C.c_uint32),
                ("out_base", C.c_uint64)]


class Seq(C.Structure):
    _fields_ = [("of", C.c_uint32), ("ml", C.c_uint32), ("mdst", C.c_uint32), ("lit_start", C.c_uint32)]


class Block(C.Structure):
    """zgpu_block: one host-parsed Block_Header (include/zgpu.h, the thin boundary)"""
    _fields_ = [("src_off", C.c_uint64), ("src_len", C.c_uint32), ("raw_rle_size", C.c_uint32), ("type", C.c_uint8), ("last", C.c_uint8),
                ("pad", C.c_uint8 * 6)]


class StreamOpts(C.Structure):
    """zgpu_stream_opts (include/zgpu.h)"""
    _fields_ = [("read_ahead_bytes", C.c_uint64), ("no_checksum", C.c_uint32), ("copy_threads", C.c_uint32), ("pipe_after_bytes", C.c_uint64),
                ("first_run_blocks", C.c_uint32), ("pad", C.c_uint32)]


NO_READ_AHEAD = 1

EXPORTS = [
    "zgpu_seek_index_create_device", "zgpu_seek_index_destroy", "zgpu_seek_index_entries", "zgpu_seek_index_info_of", "zgpu_seek_index_stats",
    "zgpu_frames_seek_indexed_device", "zgpu_gather_ranges_indexed_device_src",
    "zgpu_seek_index_measure_device", "zgpu_seek_index_export_seek_table",
    "zgpu_seek_index_hash_device", "zgpu_seek_index_set_sums", "zgpu_seek_index_read_sums", "zgpu_seek_index_sums_of",
    "zgpu_seek_index_export_seek_table_ex",
    "zgpu_seek_index_records_device", "zgpu_seek_index_records_of", "zgpu_seek_index_read_records", "zgpu_seek_index_set_records",
    "zgpu_seek_index_record_ranges_device", "zgpu_gather_records_indexed_device_src", "zgpu_gather_records_batch_indexed_device_src",
    "zgpu_frames_seek_table_many_device", "zgpu_gather_ranges_seek_table_device_src",
    "zgpu_frames_seek_table_device", "zgpu_decode_ranges_seek_table_device_src",
    "zgpu_frames_seek_device", "zgpu_decode_ranges_device_src", "zgpu_debug_ranges_stats",
    "zgpu_frames_index_device", "zgpu_frames_table_device", "zgpu_debug_frames_index_stats",
    "zgpu_decode_frames_device_src", "zgpu_debug_frames_device_src_stats",
    "zgpu_decode_frames_device", "zgpu_debug_frames_device_stats", "zgpu_debug_hash_ranges", "zgpu_debug_hash_ranges_us", "zgpu_debug_zx_probe",
    "zgpu_set_frames_shared_dicts", "zgpu_frames_shared_dicts", "zgpu_debug_frames_dict_stats",
    "zgpu_decode_frames", "zgpu_batch_checksums", "zgpu_plaintext_bound", "zgpu_debug_frames_submits",
    "zgpu_ctx_create", "zgpu_ctx_destroy", "zgpu_set_max_window_size", "zgpu_max_window_size", "zgpu_last_error", "zgpu_status_name",
    "zgpu_decode_all", "zgpu_batch_prepare", "zgpu_batch_run", "zgpu_batch_sync", "zgpu_batch_num_frames", "zgpu_batch_num_blocks",
    "zgpu_batch_compressed_size", "zgpu_batch_frame_info", "zgpu_batch_read", "zgpu_batch_output_device", "zgpu_batch_timings",
    "zgpu_batch_destroy", "zgpu_batch_block_info", "zgpu_batch_block_literals", "zgpu_batch_block_sequences", "zgpu_batch_fse_slot",
    "zgpu_batch_huf_slot", "zgpu_batch_debug_timers", "zgpu_batch_num_units", "zgpu_batch_debug_sweep_mode", "zgpu_batch_debug_lit_direct", "zgpu_batch_unit", "zgpu_batch_debug_scratch", "zgpu_debug_calibrate", "zgpu_add_dict", "zgpu_decoder_force_dict",
    "zgpu_decoder_decode_from_to", "zgpu_decoder_create", "zgpu_decoder_destroy", "zgpu_decoder_init", "zgpu_decoder_decode_blocks",
    "zgpu_decoder_can_collect", "zgpu_decoder_collect", "zgpu_decoder_read", "zgpu_decoder_is_finished", "zgpu_decoder_blocks_decoded",
    "zgpu_decoder_bytes_read_from_source", "zgpu_decoder_content_size", "zgpu_decoder_checksum_from_data",
    "zgpu_decoder_calculated_checksum", "zgpu_decode_all_alloc", "zgpu_free", "zgpu_decoder_collect_to_writer", "zgpu_streaming_create",
    "zgpu_streaming_destroy", "zgpu_streaming_decoder", "zgpu_streaming_read", "zgpu_pool_create", "zgpu_pool_create_on", "zgpu_pool_destroy",
    "zgpu_pool_num_gpus", "zgpu_pool_decode_all", "zgpu_pool_plan", "zgpu_pool_stage", "zgpu_pool_run", "zgpu_pool_frame", "zgpu_pool_read", "zgpu_pool_timings", "zgpu_pool_plan_stats",
    "zgpu_frame_begin", "zgpu_frame_end", "zgpu_blocks_submit", "zgpu_sync", "zgpu_available", "zgpu_read", "zgpu_device_output",
    "zgpu_frame_checksum", "zgpu_frame_blocks_decoded", "zgpu_decoder_device_bytes", "zgpu_debug_tuning",
    "zgpu_streaming_create_ex", "zgpu_streaming_create_slice", "zgpu_streaming_source_position", "zgpu_streaming_copy", "zgpu_streaming_stats",
    "zgpu_decoder_set_hash", "zgpu_decoder_set_read_ahead", "zgpu_release_caches", "zgpu_decoder_stream_error",
]
WRITE_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)
READ_FN = C.CFUNCTYPE(C.c_size_t, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)


def load_library(dev=False):
    """Load libzgpu.so (dev=True: libzgpu_dev.so) and declare the prototypes. Does not touch the GPU."""
    global _LIB, _DEV_LIB
    if dev:
        if _DEV_LIB is None:
            if not os.path.exists(DEV_LIB_PATH):
                raise RuntimeError("libzgpu_dev.so is not built (run __graft_entry__.build())")
            _DEV_LIB = _declare(C.CDLL(DEV_LIB_PATH))
        return _DEV_LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libzgpu.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    _LIB = _declare(C.CDLL(LIB_PATH))
    return _LIB


def _declare(L):
    vp, sz, u8p = C.c_void_p, C.c_size_t, C.c_char_p
    P = C.POINTER
    L.zgpu_ctx_create.argtypes = [C.c_int, P(vp)]
    L.zgpu_ctx_destroy.argtypes = [vp]
    L.zgpu_set_max_window_size.argtypes = [vp, C.c_uint64]
    L.zgpu_max_window_size.argtypes = [vp]
    L.zgpu_max_window_size.restype = C.c_uint64
    L.zgpu_last_error.argtypes = [vp]
    L.zgpu_last_error.restype = C.c_char_p
    L.zgpu_status_name.argtypes = [C.c_int]
    L.zgpu_status_name.restype = C.c_char_p
    L.zgpu_decode_all.argtypes = [vp, u8p, sz, vp, sz, P(sz)]
    L.zgpu_batch_prepare.argtypes = [vp, u8p, sz, P(vp)]
    L.zgpu_batch_run.argtypes = [vp]
    L.zgpu_batch_sync.argtypes = [vp, P(C.c_uint64), P(C.c_uint32), P(C.c_uint32)]
    L.zgpu_batch_num_frames.argtypes = [vp]
    L.zgpu_batch_num_frames.restype = C.c_uint32
    L.zgpu_batch_num_blocks.argtypes = [vp]
    L.zgpu_batch_num_blocks.restype = C.c_uint32
    L.zgpu_batch_compressed_size.argtypes = [vp]
    L.zgpu_batch_compressed_size.restype = C.c_uint64
    L.zgpu_batch_frame_info.argtypes = [vp, C.c_uint32, P(FrameInfo)]
    L.zgpu_batch_read.argtypes = [vp, C.c_uint64, vp, C.c_uint64]
    L.zgpu_batch_checksums.argtypes = [vp, P(C.c_uint64), C.c_uint32]
    L.zgpu_decode_frames.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(vp), P(sz), P(EntryResultC)]
    L.zgpu_decode_frames_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(vp), P(sz), P(DeviceOptsC), P(DeviceEntryResultC)]
    L.zgpu_debug_frames_device_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_debug_hash_ranges.argtypes = [vp, vp, P(C.c_uint64), P(C.c_uint64), C.c_uint32, C.c_int, P(C.c_uint64)]
    L.zgpu_debug_hash_ranges_us.argtypes = [vp]
    L.zgpu_debug_hash_ranges_us.restype = C.c_uint64
    L.zgpu_debug_zx_probe.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32), vp, vp, C.c_uint32]
    L.zgpu_decode_frames_device_src.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(vp), P(sz), P(DeviceOptsC), P(DeviceEntryResultC)]
    L.zgpu_debug_frames_device_src_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_frames_index_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(EntryIndexC)]
    L.zgpu_frames_table_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(EntryIndexC), P(C.c_uint64), P(FrameIndexC), sz, P(sz)]
    L.zgpu_debug_frames_index_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_frames_seek_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(RangeC), P(SeekC)]
    L.zgpu_decode_ranges_device_src.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(RangeC), P(vp), P(sz), P(DeviceOptsC), P(RangeResultC)]
    L.zgpu_debug_ranges_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_frames_seek_table_device.argtypes = L.zgpu_frames_seek_device.argtypes
    L.zgpu_decode_ranges_seek_table_device_src.argtypes = L.zgpu_decode_ranges_device_src.argtypes
    L.zgpu_frames_seek_table_many_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(EntryRangeC), C.c_uint32, P(SeekC)]
    L.zgpu_gather_ranges_seek_table_device_src.argtypes = [vp, P(vp), P(sz), C.c_uint32, P(EntryRangeC), C.c_uint32, P(vp), P(sz), P(DeviceOptsC),
                                                           P(RangeResultC)]
    L.zgpu_seek_index_create_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, C.c_uint32, P(vp)]
    L.zgpu_seek_index_measure_device.argtypes = [vp, P(vp), P(sz), C.c_uint32, C.c_uint32, P(vp)]
    L.zgpu_seek_index_export_seek_table.argtypes = [vp, C.c_uint32, C.c_char_p, sz, P(sz)]
    L.zgpu_seek_index_export_seek_table_ex.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_char_p, sz, P(sz)]
    L.zgpu_seek_index_hash_device.argtypes = [vp, vp, P(vp), P(sz), C.c_uint32, C.c_char_p, C.c_uint64]
    L.zgpu_seek_index_set_sums.argtypes = [vp, C.c_uint32, P(C.c_uint32), C.c_uint32]
    L.zgpu_seek_index_read_sums.argtypes = [vp, C.c_uint32, P(C.c_uint32), C.c_uint32, P(C.c_uint32)]
    L.zgpu_seek_index_sums_of.argtypes = [vp, C.c_uint32, P(SeekIndexSumsC)]
    L.zgpu_seek_index_records_device.argtypes = [vp, vp, P(vp), P(sz), C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint64]
    L.zgpu_seek_index_records_of.argtypes = [vp, C.c_uint32, P(SeekIndexRecordsC)]
    L.zgpu_seek_index_read_records.argtypes = [vp, C.c_uint32, C.c_uint64, P(C.c_uint64), C.c_uint64, P(C.c_uint64)]
    L.zgpu_seek_index_set_records.argtypes = [vp, C.c_uint32, P(C.c_uint64), C.c_uint64, C.c_uint32]
    L.zgpu_seek_index_record_ranges_device.argtypes = [vp, vp, P(RecordRangeC), C.c_uint32, P(EntryRangeC), P(C.c_uint32)]
    L.zgpu_gather_records_indexed_device_src.argtypes = [vp, vp, P(vp), P(sz), C.c_uint32, P(RecordRangeC), C.c_uint32, P(vp), P(sz), P(DeviceOptsC),
                                                         P(RangeResultC)]
    L.zgpu_gather_records_batch_indexed_device_src.argtypes = [vp, vp, P(vp), P(sz), C.c_uint32, P(RecordRangeC), C.c_uint32, P(RecordBatchC),
                                                               P(DeviceOptsC), P(RangeResultC), P(RecordBatchInfoC)]
    L.zgpu_seek_index_destroy.argtypes = [vp]
    L.zgpu_seek_index_destroy.restype = None
    L.zgpu_seek_index_entries.argtypes = [vp]
    L.zgpu_seek_index_entries.restype = C.c_uint32
    L.zgpu_seek_index_info_of.argtypes = [vp, C.c_uint32, P(SeekIndexInfoC)]
    L.zgpu_seek_index_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_frames_seek_indexed_device.argtypes = [vp, vp, P(EntryRangeC), C.c_uint32, P(SeekC)]
    L.zgpu_gather_ranges_indexed_device_src.argtypes = [vp, vp, P(vp), P(sz), C.c_uint32, P(EntryRangeC), C.c_uint32, P(vp), P(sz), P(DeviceOptsC),
                                                        P(RangeResultC)]
    L.zgpu_set_frames_shared_dicts.argtypes = [vp, C.c_int]
    L.zgpu_set_frames_shared_dicts.restype = None
    L.zgpu_frames_shared_dicts.argtypes = [vp]
    L.zgpu_debug_frames_dict_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_plaintext_bound.argtypes = [u8p, sz]
    L.zgpu_plaintext_bound.restype = C.c_uint64
    L.zgpu_debug_frames_submits.argtypes = [vp]
    L.zgpu_debug_frames_submits.restype = C.c_uint32
    L.zgpu_batch_output_device.argtypes = [vp]
    L.zgpu_batch_output_device.restype = vp
    L.zgpu_batch_timings.argtypes = [vp, P(C.c_float), C.c_int]
    L.zgpu_batch_destroy.argtypes = [vp]
    L.zgpu_batch_block_info.argtypes = [vp, C.c_uint32, P(BlockInfo)]
    L.zgpu_batch_block_literals.argtypes = [vp, C.c_uint32, vp, sz, P(sz)]
    L.zgpu_batch_block_sequences.argtypes = [vp, C.c_uint32, P(Seq), sz, P(sz)]
    L.zgpu_batch_fse_slot.argtypes = [vp, C.c_uint32, P(C.c_uint32), P(C.c_uint8)]
    L.zgpu_batch_huf_slot.argtypes = [vp, C.c_uint32, P(C.c_uint16), P(C.c_int)]
    L.zgpu_batch_debug_timers.argtypes = [vp, P(C.c_uint64)]
    L.zgpu_batch_num_units.argtypes = [vp]
    L.zgpu_batch_num_units.restype = C.c_uint32
    L.zgpu_batch_debug_sweep_mode.argtypes = [vp]
    L.zgpu_batch_debug_sweep_mode.restype = C.c_uint32
    L.zgpu_batch_debug_lit_direct.argtypes = [vp]
    L.zgpu_batch_debug_lit_direct.restype = C.c_uint32
    L.zgpu_batch_unit.argtypes = [vp, C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]
    L.zgpu_batch_debug_scratch.argtypes = [vp, C.c_int, C.c_uint64, vp, C.c_uint64]
    L.zgpu_debug_calibrate.argtypes = [vp, C.c_uint64]
    L.zgpu_frame_begin.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, P(vp)]
    L.zgpu_frame_end.argtypes = [vp]
    L.zgpu_blocks_submit.argtypes = [vp, u8p, sz, P(Block), sz]
    L.zgpu_sync.argtypes = [vp, P(sz), P(C.c_int32)]
    L.zgpu_available.argtypes = [vp, C.c_int]
    L.zgpu_available.restype = sz
    L.zgpu_read.argtypes = [vp, vp, sz, C.c_int, P(sz)]
    L.zgpu_device_output.argtypes = [vp, P(vp), P(sz)]
    L.zgpu_frame_checksum.argtypes = [vp]
    L.zgpu_frame_checksum.restype = C.c_uint32
    L.zgpu_frame_blocks_decoded.argtypes = [vp]
    L.zgpu_frame_blocks_decoded.restype = C.c_uint64
    L.zgpu_decoder_device_bytes.argtypes = [vp]
    L.zgpu_decoder_device_bytes.restype = C.c_uint64
    L.zgpu_decoder_create.argtypes = [vp, P(vp)]
    L.zgpu_add_dict.argtypes = [vp, u8p, sz, P(C.c_uint32)]
    L.zgpu_decoder_force_dict.argtypes = [vp, C.c_uint32]
    L.zgpu_decoder_decode_from_to.argtypes = [vp, u8p, sz, vp, sz, P(sz), P(sz)]
    L.zgpu_decoder_destroy.argtypes = [vp]
    L.zgpu_decoder_init.argtypes = [vp, u8p, sz, P(sz), P(C.c_uint32), P(C.c_uint32)]
    L.zgpu_decoder_decode_blocks.argtypes = [vp, u8p, sz, P(sz), C.c_int, sz, P(C.c_int)]
    L.zgpu_decoder_can_collect.argtypes = [vp]
    L.zgpu_decoder_can_collect.restype = sz
    L.zgpu_decoder_collect.argtypes = [vp, vp, sz]
    L.zgpu_decoder_collect.restype = sz
    L.zgpu_decoder_read.argtypes = [vp, vp, sz]
    L.zgpu_decoder_read.restype = sz
    L.zgpu_decoder_is_finished.argtypes = [vp]
    for nm in ("zgpu_decoder_blocks_decoded", "zgpu_decoder_bytes_read_from_source", "zgpu_decoder_content_size"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = C.c_uint64
    L.zgpu_decoder_checksum_from_data.argtypes = [vp, P(C.c_uint32)]
    L.zgpu_decoder_calculated_checksum.argtypes = [vp]
    L.zgpu_decoder_calculated_checksum.restype = C.c_uint32
    L.zgpu_decode_all_alloc.argtypes = [vp, u8p, sz, P(vp), P(sz)]
    L.zgpu_free.argtypes = [vp]
    L.zgpu_decoder_collect_to_writer.argtypes = [vp, WRITE_FN, vp, P(sz)]
    L.zgpu_streaming_create.argtypes = [vp, READ_FN, vp, P(vp)]
    L.zgpu_streaming_destroy.argtypes = [vp]
    L.zgpu_streaming_decoder.argtypes = [vp]
    L.zgpu_streaming_decoder.restype = vp
    L.zgpu_streaming_read.argtypes = [vp, vp, sz, P(sz)]
    L.zgpu_pool_create.argtypes = [C.c_int, P(vp)]
    L.zgpu_pool_create_on.argtypes = [P(C.c_int), C.c_int, P(vp)]
    L.zgpu_pool_destroy.argtypes = [vp]
    L.zgpu_pool_num_gpus.argtypes = [vp]
    L.zgpu_pool_decode_all.argtypes = [vp, u8p, sz, vp, sz, P(sz)]
    L.zgpu_pool_plan.argtypes = [P(C.c_uint64), C.c_uint32, C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_uint64)]
    L.zgpu_pool_stage.argtypes = [vp, P(C.c_char_p), P(sz), C.c_uint32]
    L.zgpu_pool_run.argtypes = [vp, P(C.c_float), P(C.c_float)]
    L.zgpu_pool_frame.argtypes = [vp, C.c_uint32, P(C.c_int), P(C.c_uint64), P(C.c_uint32)]
    L.zgpu_pool_read.argtypes = [vp, C.c_uint32, vp, sz, P(sz)]
    L.zgpu_pool_timings.argtypes = [vp, C.c_uint32, P(C.c_float), C.c_int, P(C.c_uint64), P(C.c_uint64), P(C.c_uint32), P(C.c_uint32)]
    L.zgpu_pool_plan_stats.argtypes = [vp, C.c_uint32, P(C.c_uint64), C.c_int]
    L.zgpu_debug_tuning.argtypes = [vp, P(C.c_uint32), C.c_int]
    L.zgpu_streaming_create_ex.argtypes = [vp, READ_FN, vp, P(StreamOpts), P(vp)]
    L.zgpu_streaming_create_slice.argtypes = [vp, vp, sz, P(StreamOpts), P(vp)]
    L.zgpu_streaming_source_position.argtypes = [vp]
    L.zgpu_streaming_source_position.restype = sz
    L.zgpu_streaming_copy.argtypes = [vp, sz, vp, vp, P(C.c_uint64)]
    L.zgpu_streaming_stats.argtypes = [vp, P(C.c_uint64), C.c_int]
    L.zgpu_decoder_set_hash.argtypes = [vp, C.c_int]
    L.zgpu_decoder_set_read_ahead.argtypes = [vp, C.c_uint64]
    L.zgpu_decoder_stream_error.argtypes = [vp]
    return L


class ZgpuError(Exception):
    def __init__(self, status, what=""):
        self.status = status
        name = load_library().zgpu_status_name(status).decode()
        super().__init__("%s (status %d) %s" % (name, status, what))


# ---- marshalling of the calls that take parallel lists, one element per entry ---------------------------------------------------------------
def _ptr_array(ptrs):
    """void*[max(n, 1)] of n addresses (integers); 0 is NULL"""
    return (C.c_void_p * max(len(ptrs), 1)).from_buffer_copy(array("Q", ptrs if len(ptrs) else (0,)))   # (one copy of 64-bit words: no Python loop)


def _size_array(sizes):
    """size_t[max(n, 1)] of n sizes (integers)"""
    return (C.c_size_t * max(len(sizes), 1)).from_buffer_copy(array("Q", sizes if len(sizes) else (0,)))


def _one_per(method, n, *lists):
    """every list (None: not given) holds one element for each of the call's n entries"""
    for x in lists:
        if x is not None and len(x) != n:
            raise ValueError("%s: %d entries, but a parallel list of %d elements" % (method, n, len(x)))


DEVICE_NO_HASH, DEVICE_VERIFY, DEVICE_VERIFY_SEEK_TABLE = 1, 2, 4   # zgpu_device_opts.flags


def _opts(hash_max, no_hash, verify, verify_table=False):
    return DeviceOptsC(int(hash_max), (DEVICE_NO_HASH if no_hash else 0) | (DEVICE_VERIFY if verify else 0) |
                       (DEVICE_VERIFY_SEEK_TABLE if verify_table else 0), 0)


# what _results makes of an array of each record: the record's fields in the order of _fields_ as a struct format — a zgpu_range_result begins with
# its zgpu_device_entry_result (.d), the zgpu_seek behind it is passed over — and the class of the Python object
_RESULT_RECORDS = {EntryResultC: ("<QiIIIII", EntryResult), DeviceEntryResultC: ("<QiIIIIIII", DeviceEntryResult),
                   RangeResultC: ("<QiIIIIIII64x", DeviceEntryResult)}


def _results(res, n):
    """The first n records of a ctypes array of zgpu_entry_result (as EntryResult objects, data left to the caller), zgpu_device_entry_result or
    zgpu_range_result (as DeviceEntryResult objects): every field as it stands, whatever the status. The array is read in one pass over its
    memory: one ctypes access per field costs more than the rest of the conversion."""
    fmt, cls = _RESULT_RECORDS[res._type_]
    out = []
    for v in struct.iter_unpack(fmt, memoryview(res).cast("B")[:n * C.sizeof(res._type_)]):
        e = cls()
        e.written, e.status, e.nframes, e.checksums, e.checksum_mismatches, e.checksum_from_data, e.calculated_checksum = v[:7]
        if cls is DeviceEntryResult:
            e.checksums_unverified, e.first_hashed = v[7:]
        out.append(e)
    return out


def _slots(caps):
    """(offs, total): slots of caps[i] bytes back to back, each on a 256-byte boundary"""
    offs, total = [], 0
    for c in caps:
        offs.append(total)
        total += (int(c) + 255) & ~255
    return offs, total


class Context:
    """One engine per GPU (zgpu_ctx)."""

    def __init__(self, device=0, dev=False):
        self.L = load_library(dev)
        h = C.c_void_p()
        st = self.L.zgpu_ctx_create(device, C.byref(h))
        if st:
            raise ZgpuError(st, "zgpu_ctx_create: no usable MI355X/HIP device — the engine has no CPU path")
        self.h = h
        self.device = device
        self._indexes = []   # the SeekIndex handles that are still open: closed before the context

    def close(self):
        if getattr(self, "h", None):
            for ix in list(getattr(self, "_indexes", ())):
                ix.close()
            self.L.zgpu_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def tuning(self):
        """the switches this context's engine took when it was created (zgpu_debug_tuning): all defaults in the product library"""
        d = _read_stats(self.L, "Context.tuning", self.h)
        for k in ("seq_packed", "flat4", "poison"):
            if d.get(k, 0) >= 1 << 31:
                d[k] -= 1 << 32
        # ZGPU_POISON (-1: not set), the bytes filled for the last prepared submit and the capacity of its scratch buffers (development build)
        for k in ("poisoned", "scratch_cap"):
            d[k + "_bytes"] = d.pop(k + "_lo", 0) | d.pop(k + "_hi", 0) << 32
        return d

    def set_max_window_size(self, n):
        self.L.zgpu_set_max_window_size(self.h, n)

    def max_window_size(self):
        return self.L.zgpu_max_window_size(self.h)

    def add_dict(self, raw):
        """FrameDecoder::add_dict (frame_decoder.rs:224-227); returns the dictionary id"""
        did = C.c_uint32()
        st = self.L.zgpu_add_dict(self.h, raw, len(raw), C.byref(did))
        if st:
            raise ZgpuError(st)
        return did.value

    def decode_all(self, src, cap):
        """FrameDecoder::decode_all (frame_decoder.rs:541-577). Returns the plaintext or raises ZgpuError."""
        w = C.c_size_t()
        try:                                   # no zero-fill, one copy: matters for GB-sized outputs
            import numpy as np
            arr = np.empty(max(cap, 1), dtype=np.uint8)
            st = self.L.zgpu_decode_all(self.h, src, len(src), arr.ctypes.data_as(C.c_void_p), cap, C.byref(w))
            if st:
                raise ZgpuError(st)
            return arr[:w.value].tobytes()
        except ImportError:
            buf = C.create_string_buffer(max(cap, 1))
            st = self.L.zgpu_decode_all(self.h, src, len(src), buf, cap, C.byref(w))
            if st:
                raise ZgpuError(st)
            return buf.raw[:w.value]

    def decode_all_to_vec(self, src):
        """FrameDecoder::decode_all_to_vec (frame_decoder.rs:591-610): the library sizes the output"""
        out, n = C.c_void_p(), C.c_size_t()
        st = self.L.zgpu_decode_all_alloc(self.h, src, len(src), C.byref(out), C.byref(n))
        if st:
            raise ZgpuError(st)
        try:
            return C.string_at(out, n.value)
        finally:
            self.L.zgpu_free(out)

    def prepare(self, src):
        return Batch(self, src)

    def _check(self, st, what=None):
        """the one error path of the calls below: a status other than 0 raises with the context's last error (or the fixed text `what`)"""
        if st:
            raise ZgpuError(st, self.L.zgpu_last_error(self.h).decode() if what is None else what)

    def last_error(self):
        """zgpu_last_error: the text the engine left last (seek_index_measured names there the first frame it could not measure)"""
        return self.L.zgpu_last_error(self.h).decode()

    def _stats(self, getter, slots=None):
        return _read_stats(self.L, "Context." + getter, self.h, slots=slots)

    def decode_frames(self, entries, caps=None):
        """zgpu_decode_frames: many independent buffers (bytes, or (address, length) of memory the caller keeps alive), each what decode_all
        takes, in few submits. caps: bytes of room per entry (default: plaintext_bound of the entry). Returns one EntryResult per entry, which is
        what decode_all of that entry alone would give, plus the content checksums of its frames."""
        import numpy as np
        n = len(entries)
        srcs, lens, keep = self._entries(entries)
        if caps is None:
            caps = self._bounds(srcs, lens, n)
        offs = [0] + (np.cumsum(np.asarray(caps, dtype=np.uint64)).tolist() if n else [])
        out = np.empty(max(offs[-1], 1), dtype=np.uint8)
        base = out.ctypes.data
        res = (EntryResultC * max(n, 1))()
        self._check(self.L.zgpu_decode_frames(self.h, srcs, lens, n, _ptr_array([base + o for o in offs[:n]]), _size_array(caps), res))
        outl = _results(res, n)
        for o, e in zip(offs, outl):
            e.data = out[o:o + e.written].tobytes() if e.status == 0 else None
        return outl

    def frames_submits(self):
        """submits the last decode_frames / decode_frames_device call ran (zgpu_debug_frames_submits)"""
        return self.L.zgpu_debug_frames_submits(self.h)

    def set_frames_shared_dicts(self, on):
        """zgpu_set_frames_shared_dicts: True — dictionary frames whose id is registered (add_dict) join the shared submits of decode_frames,
        decode_frames_device and decode_frames_device_src; False (the default) — their entries are decoded alone, as before."""
        self.L.zgpu_set_frames_shared_dicts(self.h, 1 if on else 0)

    def frames_shared_dicts(self):
        return bool(self.L.zgpu_frames_shared_dicts(self.h))

    def frames_dict_stats(self):
        """the last decode_frames / decode_frames_device / decode_frames_device_src call (zgpu_debug_frames_dict_stats)"""
        return self._stats("frames_dict_stats")

    @staticmethod
    def _entries(entries):
        """(srcs, lens, what keeps them alive) of entries: bytes, or (address, length) of memory the caller keeps alive"""
        ptrs, lens, keep = [], [], []
        for e in entries:
            if isinstance(e, tuple):
                ptrs.append(e[0])
                lens.append(e[1])
            else:
                b = C.c_char_p(bytes(e))                   # (no copy of a bytes object)
                keep.append(b)
                ptrs.append(C.cast(b, C.c_void_p).value)
                lens.append(len(e))
        return _ptr_array(ptrs), _size_array(lens), keep

    def _bounds(self, srcs, lens, n):
        return [self.L.zgpu_plaintext_bound(C.cast(C.c_void_p(srcs[i]), C.c_char_p), lens[i]) for i in range(n)]

    def decode_frames_device(self, entries, ptrs, caps, hash_max=0, no_hash=False, verify=False):
        """zgpu_decode_frames_device: decode_frames with the plaintext left in DEVICE memory the caller owns. ptrs[i] is the address of caps[i]
        bytes on this context's device (any alignment; a torch tensor's data_ptr()); the library checks every one with the HIP runtime before it
        launches anything, and a pointer that is not such memory gives that entry E_BAD_ARG. Nothing in flight may touch the destinations during
        the call; when it returns, the bytes are there for every stream. hash_max: frames up to this many bytes are hashed on the device
        (0: 4 MiB), longer ones are counted in checksums_unverified; no_hash: hash nothing. verify (ZGPU_DEVICE_VERIFY): an entry that decodes
        but holds a hashed frame whose XXH64 differs from its Content_Checksum gets E_CHECKSUM_MISMATCH, written = nframes = 0, and no byte of
        its destination is written (checksums / checksum_mismatches still say which count failed); hash_max=0 then means no limit for frames
        that carry a checksum. verify with no_hash raises E_BAD_ARG. Returns one DeviceEntryResult per entry."""
        n = len(entries)
        _one_per("decode_frames_device", n, ptrs, caps)
        srcs, lens, keep = self._entries(entries)
        res = (DeviceEntryResultC * max(n, 1))()
        st = self.L.zgpu_decode_frames_device(self.h, srcs, lens, n, _ptr_array(ptrs), _size_array(caps),
                                              C.byref(_opts(hash_max, no_hash, verify)), res)
        del keep
        self._check(st)
        return _results(res, n)

    def frames_device_stats(self, verify=False):
        """the last decode_frames_device call (zgpu_debug_frames_device_stats). verify=True: with the two fields of verification as well —
        entries_failed_verify (out[7]) and hash_us (out[8], the hash kernel's time, HIP events)."""
        return self._stats("frames_device_stats", 9 if verify else 7)

    def hash_ranges(self, ptr, offs, lens, kernel=0):
        """zgpu_debug_hash_ranges: XXH64 (seed 0) of the ranges [ptr + offs[i], + lens[i]) of device memory by the hash kernels of the device
        calls. kernel 0: the library's choice, 1: zg_k_xxh64 (one lane per range), 4: zg_k_xxh64q (four lanes per range). ptr must be device
        memory of this context's device that holds every range (else E_BAD_ARG, nothing launched). Returns the digests in the caller's order;
        hash_ranges_us() is the kernel's time in that call."""
        n = len(offs)
        _one_per("hash_ranges", n, lens)
        o, ln, out = (C.c_uint64 * max(n, 1))(*offs), (C.c_uint64 * max(n, 1))(*lens), (C.c_uint64 * max(n, 1))()
        self._check(self.L.zgpu_debug_hash_ranges(self.h, int(ptr) or None, o, ln, n, int(kernel), out), "zgpu_debug_hash_ranges")
        return out[:n]

    def hash_ranges_us(self):
        return int(self.L.zgpu_debug_hash_ranges_us(self.h))

    def zx_probe(self, op, threads, flags, res_off, res_bytes, in_words, out_words, arena):
        """zgpu_debug_zx_probe: one zx_* primitive (zg_zxprobe.h) on one workgroup. in_words: 8 per thread, out_words: 4 per thread as they go up,
        arena: bytes. Returns (the result words, the arena afterwards, the operand words as the call left them)."""
        a, o = (C.c_uint32 * len(in_words))(*in_words), (C.c_uint32 * len(out_words))(*out_words)
        src, dst = C.create_string_buffer(bytes(arena), len(arena)), C.create_string_buffer(len(arena))
        self._check(self.L.zgpu_debug_zx_probe(self.h, op, threads, flags, res_off, res_bytes, a, o, src, dst, len(arena)), "zgpu_debug_zx_probe")
        assert src.raw == bytes(arena)
        return list(o), dst.raw, list(a)

    def decode_frames_device_src(self, src_ptrs, lens, dst_ptrs, caps, hash_max=0, no_hash=False, verify=False):
        """zgpu_decode_frames_device_src: decode_frames_device with the compressed input in DEVICE memory too. src_ptrs[i] is the address of
        lens[i] bytes on this context's device (any alignment), dst_ptrs[i] of caps[i] bytes; sources pass the same check as destinations
        (a pointer that is not such memory gives that entry E_BAD_ARG), are never written, and no byte outside [src, src + len) is read.
        Nothing in flight may write the sources or touch the destinations during the call. Results are those of decode_frames_device on a
        host copy of the same bytes, verify included. Returns one DeviceEntryResult per entry."""
        n = len(src_ptrs)
        _one_per("decode_frames_device_src", n, lens, dst_ptrs, caps)
        res = (DeviceEntryResultC * max(n, 1))()
        self._check(self.L.zgpu_decode_frames_device_src(self.h, _ptr_array(src_ptrs), _size_array(lens), n, _ptr_array(dst_ptrs), _size_array(caps),
                                                         C.byref(_opts(hash_max, no_hash, verify)), res))
        return _results(res, n)

    def frames_device_src_stats(self):
        """the last decode_frames_device_src call (zgpu_debug_frames_device_src_stats)"""
        return self._stats("frames_device_src_stats")

    def frames_index_device(self, src_ptrs, lens):
        """zgpu_frames_index_device: what entries in DEVICE memory hold, from frame and block headers alone. src_ptrs[i] is the address of
        lens[i] bytes on this context's device (any alignment; checked like the sources of decode_frames_device_src: a pointer that is not
        such memory gives that entry E_BAD_ARG). One kernel launch, 48 bytes per entry come back, no byte of the input does. Returns one
        EntryIndex per entry; .bound is plaintext_bound of the entry: room enough for decode_frames_device_src."""
        n = len(src_ptrs)
        _one_per("frames_index_device", n, lens)
        ents = (EntryIndexC * max(n, 1))()
        self._check(self.L.zgpu_frames_index_device(self.h, _ptr_array(src_ptrs), _size_array(lens), n, ents))
        return [EntryIndex(c) for c in ents[:n]]

    def frames_table_device(self, src_ptrs, lens, room=None):
        """zgpu_frames_table_device: frames_index_device plus one FrameIndex per frame (zstd or skippable) of every entry. Returns
        (entries, frame_first, frames): frames[frame_first[i]:frame_first[i + 1]] are entry i's, in order. room: records to make room for in the
        first call (default: two per entry); a table that turns out too small is sized by a second call."""
        n = len(src_ptrs)
        _one_per("frames_table_device", n, lens)
        srcs, lena = _ptr_array(src_ptrs), _size_array(lens)
        ents = (EntryIndexC * max(n, 1))()
        first = (C.c_uint64 * (n + 1))()
        need = C.c_size_t(0)
        cap = max(int(room) if room is not None else 2 * n, 1)
        for _ in range(2):
            frames = (FrameIndexC * cap)()
            st = self.L.zgpu_frames_table_device(self.h, srcs, lena, n, ents, first, frames, cap, C.byref(need))
            if st != E_TARGET_TOO_SMALL:
                break
            cap = need.value
        self._check(st)
        return [EntryIndex(c) for c in ents[:n]], first[:], [FrameIndex(c) for c in frames[:need.value]]

    def frames_index_stats(self):
        """the last frames_index_device / frames_table_device call (zgpu_debug_frames_index_stats)"""
        return self._stats("frames_index_stats")

    @staticmethod
    def _ranges(ranges, anchors):
        n = len(ranges)
        rg = (RangeC * max(n, 1))()
        for i in range(n):
            a = anchors[i] if anchors is not None and anchors[i] is not None else (0, 0)
            rg[i] = RangeC(int(ranges[i][0]), int(ranges[i][1]), int(a[0]), int(a[1]))
        return rg

    def _seek_call(self, what, m, *args):
        """the body of every seek call: zgpu_<what>(context, *args, out) gives one Seek per range, m of them. args: what lies between the
        context and the records — the sources and lengths with n, or the index handle, then the marshalled ranges, with m where the call
        counts them on their own"""
        out = (SeekC * max(m, 1))()
        self._check(getattr(self.L, "zgpu_" + what)(self.h, *args, out))
        return [Seek(c) for c in out[:m]]

    def _decode_call(self, what, m, args, dst_ptrs, caps, opts, batch=None, tail=()):
        """the body of every range-decode and gather call: zgpu_<what>(context, *args, destinations, capacities, options, results) gives
        (results, seeks), m of each. args: as _seek_call takes them. batch: the call's ONE destination, a RecordBatchC, in place of the m
        destinations and capacities; tail: what the call takes behind the results"""
        res = (RangeResultC * max(m, 1))()
        dest = (_ptr_array(dst_ptrs), _size_array(caps)) if batch is None else (C.byref(batch),)
        self._check(getattr(self.L, "zgpu_" + what)(self.h, *args, *dest, C.byref(opts), res, *tail))
        return _results(res, m), [Seek(res[j].seek) for j in range(m)]

    def _frames_seek(self, what, src_ptrs, lens, ranges, anchors):
        """the two seek calls with one range per entry (anchors: None for the seek-table form)"""
        n = len(src_ptrs)
        _one_per(what, n, lens, ranges, anchors)
        return self._seek_call(what, n, _ptr_array(src_ptrs), _size_array(lens), n, self._ranges(ranges, anchors))

    def _decode_ranges(self, what, src_ptrs, lens, ranges, anchors, dst_ptrs, caps, opts):
        """the two range-decode calls with one range per entry (anchors: None for the seek-table form)"""
        n = len(src_ptrs)
        _one_per(what, n, lens, ranges, anchors, dst_ptrs, caps)
        return self._decode_call(what, n, (_ptr_array(src_ptrs), _size_array(lens), n, self._ranges(ranges, anchors)), dst_ptrs, caps, opts)

    def frames_seek_device(self, src_ptrs, lens, ranges, anchors=None):
        """zgpu_frames_seek_device: which whole frames of entries in DEVICE memory hold plaintext bytes [begin, begin + len) of them, from
        frame and block headers alone. ranges[i] = (begin, len); anchors[i] = (anchor_src, anchor_plain) or None: a frame boundary of the entry
        at which the header chain starts and its plaintext offset (anchor_before gives one from a cached frames_table_device). One kernel
        launch, 64 bytes per entry come back, no byte of the input does. Returns one Seek per entry."""
        return self._frames_seek("frames_seek_device", src_ptrs, lens, ranges, anchors)

    def decode_ranges_device_src(self, src_ptrs, lens, ranges, dst_ptrs, caps, anchors=None, hash_max=0, no_hash=False, verify=False):
        """zgpu_decode_ranges_device_src: plaintext bytes ranges[i] = (begin, len) of entry i (device memory, as decode_frames_device_src takes
        it) written to dst_ptrs[i] (caps[i] bytes of device memory); only the frames that hold the range are decoded. Frames in front of the
        range are never decoded (a defect in them is not seen, a false declared size in them shifts the coordinates); frames behind it are
        not read. Returns (results, seeks): one DeviceEntryResult per entry — written is the clipped count, E_CONTENT_SIZE_MISMATCH a taken
        frame that decoded to another length than it declares — and the Seek record the call acted on."""
        return self._decode_ranges("decode_ranges_device_src", src_ptrs, lens, ranges, anchors, dst_ptrs, caps, _opts(hash_max, no_hash, verify))

    def frames_seek_table_device(self, src_ptrs, lens, ranges):
        """zgpu_frames_seek_table_device: frames_seek_device answered from the seekable format's seek table at each entry's end (seek_table_frame
        writes one), one wave per entry: no frame or block header is read, frames need not declare a size. Returns one Seek per entry, in the
        table's coordinates; an entry without a usable table has status E_SEEK_TABLE and why SEEKTAB_*."""
        return self._frames_seek("frames_seek_table_device", src_ptrs, lens, ranges, None)

    def decode_ranges_seek_table_device_src(self, src_ptrs, lens, ranges, dst_ptrs, caps, hash_max=0, no_hash=False, verify=False,
                                            verify_table=False):
        """zgpu_decode_ranges_seek_table_device_src: decode_ranges_device_src with the selection taken from each entry's seek table. Only the
        frames the table names for the range are decoded, whether or not they declare a size. Returns (results, seeks) as
        decode_ranges_device_src does; E_SEEK_TABLE: no usable table, E_CONTENT_SIZE_MISMATCH: the taken frames decoded to another total than
        the table promises. verify_table (ZGPU_DEVICE_VERIFY_SEEK_TABLE): the table's Checksum fields are enforced on the device — every
        decoded frame is hashed (hash_max=0: no limit) and compared with the row it coincides with; an entry with a frame that differs, a frame
        that coincides with no row, or a table without checksums gets E_SEEK_CHECKSUM_MISMATCH, written = nframes = 0 and no byte of its
        destination is written (checksums: frames compared, checksum_mismatches: those that differ, checksums_unverified: decoded frames not
        compared). verify_table with no_hash raises E_BAD_ARG."""
        return self._decode_ranges("decode_ranges_seek_table_device_src", src_ptrs, lens, ranges, None, dst_ptrs, caps,
                                   _opts(hash_max, no_hash, verify, verify_table))

    @staticmethod
    def _entry_ranges(ranges):
        """zgpu_entry_range[max(m, 1)] of m triples (entry, begin, len); a fourth element, if given, is the record's pad (tests)"""
        m = len(ranges)
        rg = (EntryRangeC * max(m, 1))()
        for j, r in enumerate(ranges):
            rg[j] = EntryRangeC(int(r[1]), int(r[2]), int(r[0]), int(r[3]) if len(r) > 3 else 0)
        return rg

    def frames_seek_table_many_device(self, src_ptrs, lens, ranges):
        """zgpu_frames_seek_table_many_device: frames_seek_table_device for MANY ranges over few entries. ranges[j] = (entry, begin, len) names
        its entry, an index into src_ptrs. Every entry's table is scanned once into prefix sums on the device and every range is a binary
        search in them. Returns one Seek per range, each equal to what frames_seek_table_device gives for that entry and range; a range whose
        entry is out of range gets E_BAD_ARG in its record, the others are unaffected."""
        n, m = len(src_ptrs), len(ranges)
        _one_per("frames_seek_table_many_device", n, lens)
        return self._seek_call("frames_seek_table_many_device", m, _ptr_array(src_ptrs), _size_array(lens), n, self._entry_ranges(ranges), m)

    def gather_ranges_seek_table_device_src(self, src_ptrs, lens, ranges, dst_ptrs, caps, hash_max=0, no_hash=False, verify=False,
                                            verify_table=False):
        """zgpu_gather_ranges_seek_table_device_src: plaintext bytes ranges[j] = (entry, begin, len) of seekable entries in device memory,
        range j to dst_ptrs[j] (caps[j] bytes of device memory). The tables are scanned once, and ranges of one entry whose table rows overlap
        form a group whose frames are decoded ONCE, however many ranges take bytes of them. Ranges that share a frame share the fate of every
        frame of their group (a decode error, a size that differs from the table's promise, a checksum verdict); E_TARGET_TOO_SMALL is each
        range's own. A range alone in its group gets what decode_ranges_seek_table_device_src gives for it. The options are that call's.
        Returns (results, seeks): one DeviceEntryResult and one Seek per range."""
        n, m = len(src_ptrs), len(ranges)
        _one_per("gather_ranges_seek_table_device_src", n, lens)
        _one_per("gather_ranges_seek_table_device_src", m, dst_ptrs, caps)
        return self._decode_call("gather_ranges_seek_table_device_src", m, (_ptr_array(src_ptrs), _size_array(lens), n, self._entry_ranges(ranges), m),
                                 dst_ptrs, caps, _opts(hash_max, no_hash, verify, verify_table))

    # the slots zgpu_debug_ranges_stats appends behind _STATS["Context.ranges_stats"] (csrc/zg_capi_int.h: kManyStat*, an enumeration of its own)
    GATHER_STATS = ("groups_decoded", "prefix_launches", "prefix_us", "find_launches", "find_us", "prefix_scratch_bytes")

    def gather_ranges_stats(self):
        """ranges_stats(verify_table=True) of the last call plus the slots zgpu_debug_ranges_stats appends for the calls that take many ranges
        per entry (out[13] ...): groups_decoded, prefix_launches, prefix_us, find_launches, find_us (HIP events), prefix_scratch_bytes.
        frames_decoded and plaintext_decoded count each group once."""
        keys = _STATS["Context.ranges_stats"][2] + self.GATHER_STATS
        a = (C.c_uint64 * len(keys))()
        k = self.L.zgpu_debug_ranges_stats(self.h, a, len(keys))
        return dict(zip(keys[:k], a[:k]))

    def seek_index(self, src_ptrs, lens, kind="auto"):
        """zgpu_seek_index_create_device: a SeekIndex over entries in DEVICE memory — per entry the prefix sums of its rows, built once on the
        device and kept there. kind: "seek_table" (the entry's seek table), "declared" (its header chain: every frame declares its size),
        "auto" (the table, and the chain for an entry that has none). An entry that cannot be indexed has a status in index.infos[i]; the
        others are unaffected. Close it (or the context) when done; it also is a context manager."""
        n = len(src_ptrs)
        _one_per("seek_index", n, lens)
        h = C.c_void_p()
        self._check(self.L.zgpu_seek_index_create_device(self.h, _ptr_array(src_ptrs), _size_array(lens), n, _INDEX_KINDS[kind], C.byref(h)))
        return SeekIndex(self, h)

    def seek_index_tensors(self, tensors, kind="auto"):
        """seek_index on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding shard i. The index
        describes the bytes, not the tensor: a copy of the shard elsewhere is served by the same index."""
        self._tensor_check(tensors, "seek_index_tensors")
        return self.seek_index([t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors], kind)

    def seek_index_measured(self, src_ptrs, lens, only_unsized=False):
        """zgpu_seek_index_measure_device: a SeekIndex over entries in DEVICE memory whose frames declare no size and that carry no seek table
        (what a streaming compressor writes) — every frame's plaintext length is MEASURED on the device, once: block sizes, literal sizes and
        the sums of match lengths, without a Huffman stream, an LZ77 byte or an output buffer. only_unsized: every entry is indexed as
        seek_index(kind="auto") indexes it, and only those it refuses as INDEX_UNSIZED are measured; else every entry is measured. An entry
        that cannot be measured has E_FRAME_INDEX in index.infos[i] (why: a CHAIN_* reason, SEEKTAB_TOO_LARGE, INDEX_DICT, INDEX_UNMEASURED —
        last_error names the frame). Measuring does not see Huffman, offset or checksum defects: those surface when the frame is decoded —
        in a gather, or once for the whole shard in SeekIndex.hash.
        The index serves frames_seek_indexed_device and gather_ranges_indexed_device_src like any other; export_seek_table writes it out."""
        n = len(src_ptrs)
        _one_per("seek_index_measured", n, lens)
        h = C.c_void_p()
        self._check(self.L.zgpu_seek_index_measure_device(self.h, _ptr_array(src_ptrs), _size_array(lens), n,
                                                          MEASURE_UNSIZED if only_unsized else MEASURE_ALL, C.byref(h)))
        return SeekIndex(self, h)

    def seek_index_measured_tensors(self, tensors, only_unsized=False):
        """seek_index_measured on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding shard i."""
        self._tensor_check(tensors, "seek_index_measured_tensors")
        return self.seek_index_measured([t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors], only_unsized)

    def _index_handle(self, index, what):
        if not isinstance(index, SeekIndex) or not index.h:
            raise ValueError("%s: an open SeekIndex" % what)
        return index.h

    def frames_seek_indexed_device(self, index, ranges):
        """zgpu_frames_seek_indexed_device: one Seek per range (entry, begin, len) from the index alone — one find launch, no byte of any entry
        is read. A table-kind entry answers what frames_seek_table_many_device answers; a declared-kind entry what frames_seek_device answers
        in src_lo, src_hi, plain_lo, plain_seen and `nothing` (frames_skipped / frames_taken count rows, skippable frames included). A range
        of an entry the index refused carries that entry's status and why."""
        m = len(ranges)
        return self._seek_call("frames_seek_indexed_device", m, self._index_handle(index, "frames_seek_indexed_device"), self._entry_ranges(ranges), m)

    def gather_ranges_indexed_device_src(self, index, src_ptrs, lens, ranges, dst_ptrs, caps, hash_max=0, no_hash=False, verify=False,
                                         verify_table=False):
        """zgpu_gather_ranges_indexed_device_src: gather_ranges_seek_table_device_src with the selection taken from a SeekIndex — one find
        launch plus the decode, no locate and no prefix pass. src_ptrs / lens name the index's entries (all of them; an entry's length must
        be the one it was indexed at, its address may differ). Everything behind the selection is that call: groups decoded once, fate
        sharing, E_TARGET_TOO_SMALL per range, the options. verify_table: an entry whose index holds sums (SeekIndex.hash / set_sums) is
        vouched for by the index, of whatever kind; else a table-kind entry reads its table and a range of a declared- or measured-kind
        entry gets E_BAD_ARG. A stale index ends in a status per range, never in a fault. Returns (results, seeks), one of each per range."""
        n, m = len(src_ptrs), len(ranges)
        _one_per("gather_ranges_indexed_device_src", n, lens)
        _one_per("gather_ranges_indexed_device_src", m, dst_ptrs, caps)
        return self._decode_call("gather_ranges_indexed_device_src", m,
                                 (self._index_handle(index, "gather_ranges_indexed_device_src"), _ptr_array(src_ptrs), _size_array(lens), n,
                                  self._entry_ranges(ranges), m), dst_ptrs, caps, _opts(hash_max, no_hash, verify, verify_table))

    @staticmethod
    def _record_ranges(recs):
        """zgpu_record_range[max(m, 1)] of m triples (entry, first, count); a fourth element, if given, is the record's flags (RECORDS_STRIP)"""
        m = len(recs)
        rg = (RecordRangeC * max(m, 1))()
        for j, r in enumerate(recs):
            rg[j] = RecordRangeC(int(r[1]), int(r[2]), int(r[0]), int(r[3]) if len(r) > 3 else 0)
        return rg

    def record_ranges(self, index, recs):
        """zgpu_seek_index_record_ranges_device: recs[j] = (entry, first, count[, flags]) — records [first, first + count) of entry `entry`
        of a SeekIndex that holds its record offsets (SeekIndex.records / set_records) — as plaintext byte ranges, by ONE find launch over
        the index's offsets; nothing of any entry is read. The records are clipped to those the entry has; flags RECORDS_STRIP drops the
        final delimiter of the last record taken. Returns (ranges, statuses): ranges[j] = (entry, begin, len), what
        gather_ranges_indexed_device_src takes; statuses[j] E_BAD_ARG for an entry out of range, unknown flags or an entry without records,
        the index's status for an entry it refused."""
        m = len(recs)
        out, status = (EntryRangeC * max(m, 1))(), (C.c_uint32 * max(m, 1))()
        self._check(self.L.zgpu_seek_index_record_ranges_device(self.h, self._index_handle(index, "record_ranges"), self._record_ranges(recs), m, out,
                                                                status), "zgpu_seek_index_record_ranges_device")
        return [(int(o.entry), int(o.begin), int(o.len)) for o in out[:m]], list(status[:m])

    def gather_records_indexed_device_src(self, index, src_ptrs, lens, recs, dst_ptrs, caps, hash_max=0, no_hash=False, verify=False,
                                          verify_table=False):
        """zgpu_gather_records_indexed_device_src: gather_ranges_indexed_device_src by record NUMBER — recs[j] = (entry, first, count[, flags])
        as record_ranges takes them, record range j to dst_ptrs[j] (caps[j] bytes of device memory). The lookup is one launch and 24 bytes
        per range; everything behind it is that call: groups decoded once, fate sharing, E_TARGET_TOO_SMALL per range, the options. A range
        whose lookup failed carries that status and nothing of it is gathered. Returns (results, seeks), one of each per range."""
        n, m = len(src_ptrs), len(recs)
        _one_per("gather_records_indexed_device_src", n, lens)
        _one_per("gather_records_indexed_device_src", m, dst_ptrs, caps)
        return self._decode_call("gather_records_indexed_device_src", m,
                                 (self._index_handle(index, "gather_records_indexed_device_src"), _ptr_array(src_ptrs), _size_array(lens), n,
                                  self._record_ranges(recs), m), dst_ptrs, caps, _opts(hash_max, no_hash, verify, verify_table))

    # the slots zgpu_debug_ranges_stats appends behind GATHER_STATS (csrc/zg_capi_int.h: kRecFindStat*)
    RECORD_STATS = ("record_find_launches", "record_find_us", "record_find_bytes_downloaded")

    # and behind RECORD_STATS (csrc/zg_capi_int.h: kBatchStat*)
    BATCH_STATS = ("batch_fill_launches", "batch_fill_us", "batch_bytes_filled", "batch_bytes_uploaded")

    def gather_records_batch(self, index, src_ptrs, lens, recs, dst_ptr, cap, layout="padded", width=0, pad=0, truncate=False, lengths_ptr=0,
                             offsets_ptr=0, hash_max=0, no_hash=False, verify=False, verify_table=False):
        """zgpu_gather_records_batch_indexed_device_src: gather_records_indexed_device_src into ONE piece of device memory, dst_ptr of cap
        bytes. layout "padded": row j is the width bytes at dst_ptr + j * width, its record followed by the byte `pad`; "packed": the
        records back to back (width: 0, or with truncate the most bytes taken of one record). truncate: a record longer than width is cut to
        width — the frames behind the cut are not decoded — where it otherwise gets E_TARGET_TOO_SMALL (padded). lengths_ptr / offsets_ptr
        (device memory, 8-byte aligned, or 0): m lengths — 0 for a row with a status, which is all pad — and m + 1 offsets. A batch that
        needs more than cap bytes writes nothing: every row gets E_TARGET_TOO_SMALL and info.total is the need (cap=0, dst_ptr=0: the
        size query). Returns (results, seeks, info, record_bytes): a RecordBatchInfo and every range's byte length before truncation."""
        n, m = len(src_ptrs), len(recs)
        _one_per("gather_records_batch", n, lens)
        rb, info = (C.c_uint64 * max(m, 1))(), RecordBatchInfoC()
        batch = RecordBatchC(dst_ptr or None, int(cap), lengths_ptr or None, offsets_ptr or None, rb, int(width), _BATCH_LAYOUTS[layout],
                             BATCH_TRUNCATE if truncate else 0, int(pad), 0)
        res, seeks = self._decode_call("gather_records_batch_indexed_device_src", m,
                                       (self._index_handle(index, "gather_records_batch"), _ptr_array(src_ptrs), _size_array(lens), n,
                                        self._record_ranges(recs), m), None, None, _opts(hash_max, no_hash, verify, verify_table),
                                       batch=batch, tail=(C.byref(info),))
        return res, seeks, RecordBatchInfo(info), list(rb[:m])

    def gather_records_batch_tensors(self, index, tensors, recs, width=None, pad=0, truncate=False, hash_max=0, no_hash=False, verify=False,
                                     verify_table=False):
        """gather_records_batch on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding shard i,
        index a SeekIndex over these shards that holds their record offsets — index once, then ONE call per step. width given: the padded
        batch, (uint8[m, width], int64 lengths[m], results). width None: the packed batch, (uint8[total], int64 offsets[m + 1], int64
        lengths[m], results) — one call with cap = 0 asks for the size, a second one writes. A row with a status is all `pad` and has
        length 0. torch is imported here, not by `import zgpu`."""
        import torch
        self._tensor_check(tensors, "gather_records_batch_tensors")
        ptrs, lens = [t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors]
        m, dev = len(recs), torch.device("cuda", self.device)
        opts = dict(pad=pad, truncate=truncate, hash_max=hash_max, no_hash=no_hash, verify=verify, verify_table=verify_table)
        if width is None:
            if truncate:
                raise ValueError("gather_records_batch_tensors: truncate needs a width")
            total = self.gather_records_batch(index, ptrs, lens, recs, 0, 0, layout="packed", **opts)[2].total
            layout, shape = "packed", (total,)
        else:
            total, layout, shape = m * int(width), "padded", (m, int(width))
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        lengths, offsets = torch.empty(max(m, 1), dtype=torch.int64, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev)
        self._torch_sync()   # (the caching allocator may hand out memory that is still in use on torch's stream)
        res, _, info, _ = self.gather_records_batch(index, ptrs, lens, recs, buf.data_ptr() if total else 0, total, layout=layout,
                                                    width=width or 0, lengths_ptr=lengths.data_ptr() if m else 0,
                                                    offsets_ptr=offsets.data_ptr(), **opts)
        if info.total != total:
            raise RuntimeError("gather_records_batch_tensors: the index changed between the size query and the gather")
        if width is None:
            return buf[:total], offsets, lengths[:m], res
        return buf[:total].view(shape), lengths[:m], res

    def gather_records_stats(self):
        """gather_ranges_stats of the last call plus the slots of the record lookup (out[19] ...): record_find_launches, record_find_us (HIP
        events), record_find_bytes_downloaded (24 per range); and of a record batch's finish (out[22] ...): batch_fill_launches,
        batch_fill_us (HIP events), batch_bytes_filled, batch_bytes_uploaded (into the lengths and offsets arrays)."""
        keys = _STATS["Context.ranges_stats"][2] + self.GATHER_STATS + self.RECORD_STATS + self.BATCH_STATS
        a = (C.c_uint64 * len(keys))()
        k = self.L.zgpu_debug_ranges_stats(self.h, a, len(keys))
        return dict(zip(keys[:k], a[:k]))

    def gather_tensor_records(self, tensors, recs, index, hash_max=0, no_hash=False, verify=False, verify_table=False, packed=False):
        """gather_records_indexed_device_src on torch tensors, the sibling of gather_tensor_ranges(index=...): tensors[i] is a contiguous
        torch.uint8 tensor on this context's device holding shard i, recs[j] = (entry, first, count[, flags]) the records wanted of shard
        `entry`, index a SeekIndex over these shards that holds their record offsets. record_ranges sizes the destinations — the lookup
        knows every range's length —, and the bytes go to ONE new torch.uint8 tensor. Returns (tensors, results, seeks) or, packed=True,
        (buffer, offsets, results, seeks), as gather_tensor_ranges does."""
        self._tensor_check(tensors, "gather_tensor_records")
        ptrs, lens = [t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors]
        ranges, _ = self.record_ranges(index, recs)
        caps = [r[2] for r in ranges]
        if packed:
            offs = [0]
            for cp in caps:
                offs.append(offs[-1] + cp)
            buf, _, base = self._slot_tensor([offs[-1]])
            dsts = [base[0] + o for o in offs[:-1]]
        else:
            buf, offs, dsts = self._slot_tensor(caps)
        res, seeks = self.gather_records_indexed_device_src(index, ptrs, lens, recs, dsts, caps, hash_max=hash_max, no_hash=no_hash, verify=verify,
                                                            verify_table=verify_table)
        if packed:
            return buf[:offs[-1]], offs, res, seeks
        return self._views(buf, offs, res), res, seeks

    def gather_tensor_ranges(self, tensors, ranges, hash_max=0, no_hash=False, verify=False, verify_table=False, packed=False, index=None):
        """gather_ranges_seek_table_device_src on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding
        seekable shard i, ranges[j] = (entry, begin, len) the record wanted of shard `entry`. A frames_seek_table_many_device call of its own
        sizes the destinations by min(len, seek.bound), so no byte of the input crosses to the host. The bytes go to ONE new torch.uint8
        tensor. Returns (tensors, results, seeks) — tensors[j] a view of range j's 256-byte aligned slot cut to `written` bytes (empty unless
        status == 0) — or, packed=True, (buffer, offsets, results, seeks): the slots back to back without padding, range j at
        buffer[offsets[j]:offsets[j + 1]] (a failed range's slot keeps its room and holds nothing of the range). Same single-runtime rule as
        decode_tensors. torch is imported here, not by `import zgpu`.
        index: a SeekIndex over these shards (seek_index_tensors) — the selection and the sizes come from it (frames_seek_indexed_device,
        gather_ranges_indexed_device_src): index a shard once, gather per step. Without it the call is what it always was."""
        self._tensor_check(tensors, "gather_tensor_ranges")
        ptrs, lens = [t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors]
        seeks = self.frames_seek_table_many_device(ptrs, lens, ranges) if index is None else self.frames_seek_indexed_device(index, ranges)
        caps = [min(int(r[2]), s.bound) for r, s in zip(ranges, seeks)]
        if packed:
            offs = [0]
            for cp in caps:
                offs.append(offs[-1] + cp)
            buf, _, base = self._slot_tensor([offs[-1]])
            dsts = [base[0] + o for o in offs[:-1]]
        else:
            buf, offs, dsts = self._slot_tensor(caps)
        if index is None:
            res, seeks = self.gather_ranges_seek_table_device_src(ptrs, lens, ranges, dsts, caps, hash_max=hash_max, no_hash=no_hash, verify=verify,
                                                                  verify_table=verify_table)
        else:
            res, seeks = self.gather_ranges_indexed_device_src(index, ptrs, lens, ranges, dsts, caps, hash_max=hash_max, no_hash=no_hash,
                                                               verify=verify, verify_table=verify_table)
        if packed:
            return buf[:offs[-1]], offs, res, seeks
        return self._views(buf, offs, res), res, seeks

    def ranges_stats(self, verify_table=False):
        """the last frames_seek_device / decode_ranges_device_src call or seek-table call (zgpu_debug_ranges_stats). verify_table=True: with the
        five fields of verify_table as well — compare_launches (out[8]), compare_us (zg_k_seeksums' time, HIP events), compare_bytes_downloaded
        (32 per entry), frames_compared and entries_failed_table (out[12])."""
        return self._stats("ranges_stats", 13 if verify_table else 8)

    def decode_tensor_ranges(self, tensors, ranges, anchors=None, hash_max=0, no_hash=False, verify=False, seek_table=False, verify_table=False):
        """decode_ranges_device_src on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding entry i's
        compressed bytes, ranges[i] = (begin, len) the plaintext bytes wanted of it. The bytes go to ONE new torch.uint8 tensor, every entry's
        slot 256-byte aligned and sized by min(len, seek.bound) — a frames_seek_device call of its own finds the bound, so no byte of the
        input crosses to the host. Returns (tensors, results, seeks): tensors[i] is a view of entry i's slot cut to `written` bytes (empty
        unless status == 0). Same single-runtime rule as decode_tensors. torch is imported here, not by `import zgpu`.
        seek_table=True: the selections come from the entries' seek tables (decode_ranges_seek_table_device_src; anchors must be None), and
        verify_table=True enforces the tables' checksums (only with seek_table=True: there is no table otherwise)."""
        if verify_table and not seek_table:
            raise ValueError("decode_tensor_ranges: verify_table needs seek_table=True")
        self._tensor_check(tensors, "decode_tensor_ranges")
        if seek_table and anchors is not None:
            raise ValueError("decode_tensor_ranges: a seek table is the index, there is nothing to anchor")
        ptrs, lens = [t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors]
        seeks = self.frames_seek_table_device(ptrs, lens, ranges) if seek_table else self.frames_seek_device(ptrs, lens, ranges, anchors)
        caps = [min(int(r[1]), s.bound) for r, s in zip(ranges, seeks)]
        buf, offs, dsts = self._slot_tensor(caps)
        if seek_table:
            res, seeks = self.decode_ranges_seek_table_device_src(ptrs, lens, ranges, dsts, caps, hash_max=hash_max, no_hash=no_hash, verify=verify,
                                                                  verify_table=verify_table)
        else:
            res, seeks = self.decode_ranges_device_src(ptrs, lens, ranges, dsts, caps, anchors=anchors, hash_max=hash_max, no_hash=no_hash,
                                                       verify=verify)
        return self._views(buf, offs, res), res, seeks

    def _torch_sync(self):
        import torch
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()

    def _tensor_check(self, tensors, what):
        import torch
        self._one_hip_runtime()
        dev = torch.device("cuda", self.device)
        for t in tensors:
            if t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
                raise ValueError("%s: contiguous torch.uint8 tensors on %s" % (what, dev))
        self._torch_sync()                       # the tensors may still be written on torch's stream

    def _slot_tensor(self, caps):
        """(tensor, offs, addresses): ONE new torch.uint8 tensor on this context's device with a slot of caps[i] bytes per entry (_slots), handed
        out once torch's current stream there has drained — the caching allocator may hand out memory that is still in use on it"""
        import torch
        offs, total = _slots(caps)
        buf = torch.empty(max(total, 256), dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._torch_sync()
        base = buf.data_ptr()
        return buf, offs, [base + o for o in offs]

    @staticmethod
    def _views(buf, offs, res):
        """entry i's slot of buf cut to `written` bytes (empty unless status == 0)"""
        return [buf[o:o + (r.written if r.status == 0 else 0)] for o, r in zip(offs, res)]

    def split_tensor_frames(self, tensor):
        """One view per zstd frame of a contiguous torch.uint8 tensor on this context's device that holds concatenated frames, cut at the frame
        boundaries frames_table_device finds (skippable frames are left out; no byte of the tensor crosses to the host). The views can go
        straight into decode_tensors, each as an entry of its own. A tensor whose header chain breaks yields the frames in front of the break
        and the broken one, up to where the chain left it."""
        self._tensor_check([tensor], "split_tensor_frames")
        _, _, frames = self.frames_table_device([tensor.data_ptr() if tensor.numel() else 0], [tensor.numel()])
        return [tensor[f.src_begin:f.src_end] for f in frames if f.header_status == 0]

    @staticmethod
    def _one_hip_runtime():
        hip = set(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln) if os.path.exists("/proc/self/maps") else ()
        if len(hip) > 1:
            raise RuntimeError("two HIP runtimes are loaded (%s): import torch before creating the first zgpu.Context" % ", ".join(sorted(hip)))

    def decode_tensors(self, tensors, caps=None, hash_max=0, no_hash=False, verify=False):
        """decode_frames_device_src on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on this context's device holding entry i's
        compressed bytes. The plaintext goes to ONE new torch.uint8 tensor, every entry's slot 256-byte aligned with caps[i] bytes of room.
        caps=None sizes the slots with frames_index_device — zgpu_plaintext_bound of every entry, taken on the device from its headers: no
        byte of the input crosses to the host. Returns (tensors, results) like decode_frames_to_tensors, under the same single-runtime rule
        (import torch before creating the first Context). verify: as decode_frames_device — an entry that fails its checksum comes back as an
        empty view with E_CHECKSUM_MISMATCH. torch is imported here, not by `import zgpu`."""
        self._tensor_check(tensors, "decode_tensors")
        ptrs, lens = [t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors]
        if caps is None:
            caps = [e.bound for e in self.frames_index_device(ptrs, lens)]
        buf, offs, dsts = self._slot_tensor(caps)
        res = self.decode_frames_device_src(ptrs, lens, dsts, caps, hash_max=hash_max, no_hash=no_hash, verify=verify)
        return self._views(buf, offs, res), res

    def decode_frames_to_tensors(self, entries, caps=None, hash_max=0, no_hash=False, verify=False):
        """decode_frames_device into ONE torch.uint8 tensor on this context's device, every entry's slot 256-byte aligned (caps: bytes of room per
        entry, default plaintext_bound of the entry). Returns (tensors, results): tensors[i] is a view of entry i's slot cut to `written` bytes
        (empty unless status == 0), results[i] its DeviceEntryResult. torch is imported here, not by `import zgpu`.
        torch wheels ship a HIP runtime of their own: the process must run on ONE runtime for torch's memory to be known to this library,
        which it does when torch is imported before the first Context is created (load_library); otherwise this raises."""
        import torch   # noqa: F401 (before the check: its runtime has to be among the loaded ones)
        self._one_hip_runtime()
        n = len(entries)
        srcs, lens, keep = self._entries(entries)
        if caps is None:
            caps = self._bounds(srcs, lens, n)
        buf, offs, dsts = self._slot_tensor(caps)
        res = self.decode_frames_device([(srcs[i] or 0, lens[i]) for i in range(n)], dsts, caps, hash_max=hash_max, no_hash=no_hash, verify=verify)
        del keep
        return self._views(buf, offs, res), res


class SeekIndex:
    """A seek index handle (zgpu_seek_index; Context.seek_index makes one): per entry the prefix sums of its rows in device memory, reused by
    any number of Context.frames_seek_indexed_device / gather_ranges_indexed_device_src calls. It belongs to its context, which closes the
    indexes it still holds when it is closed. infos[i]: entry i's SeekIndexInfo."""

    def __init__(self, ctx, h):
        self.ctx, self.L, self.h = ctx, ctx.L, h
        n = self.L.zgpu_seek_index_entries(h)
        rec = SeekIndexInfoC()
        self.infos = []
        for i in range(n):
            ctx._check(self.L.zgpu_seek_index_info_of(h, i, C.byref(rec)), "zgpu_seek_index_info_of")
            self.infos.append(SeekIndexInfo(rec))
        self.device_bytes = self.stats()["device_bytes"]
        ctx._indexes.append(self)

    def stats(self, sums=False):
        """the build (zgpu_seek_index_stats): launches, kernel_us (HIP events), bytes_downloaded, device_bytes held, rows, input_bytes_to_host
        (always 0); of a measured index also measure_submits, measure_us (their phase-1 time, HIP events) and frames_measured. Gather calls on
        the index do not change it: the index is never rebuilt. sums=True: what hash appends as well — hash_submits, hash_us (the hash
        kernels' time), frames_hashed, sums_bytes (held now), hash_runs."""
        return _read_stats(self.L, "SeekIndex.sums_stats" if sums else "SeekIndex.stats", self.h)

    def _open(self, what):
        if not self.h:
            raise ValueError("%s: an open SeekIndex" % what)

    def hash(self, src_ptrs, lens, which=None, run_bytes=0):
        """zgpu_seek_index_hash_device: every zstd frame of every chosen entry decoded once, its plaintext hashed on the device, the sums —
        the low 32 bits of XXH64 per row — kept in the index; nothing is delivered. src_ptrs / lens name the index's entries (all of them).
        which: one truth value per entry (None: all). run_bytes: plaintext per run of rows (0: 64 MiB). This sees what measuring does not:
        Huffman descriptions and streams, offsets, content checksums. An entry with a failing run keeps no sums; sums_infos says which and
        why, ctx.last_error names the first. Returns sums_infos."""
        self._open("hash")
        n = len(src_ptrs)
        _one_per("hash", n, lens, which)
        w = None if which is None else bytes(1 if x else 0 for x in which)
        self.ctx._check(self.L.zgpu_seek_index_hash_device(self.ctx.h, self.h, _ptr_array(src_ptrs), _size_array(lens), n, w, int(run_bytes)),
                        "zgpu_seek_index_hash_device")
        return self.sums_infos

    def hash_tensors(self, tensors, which=None, run_bytes=0):
        """hash on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on the index's device holding shard i."""
        self._open("hash_tensors")
        self.ctx._tensor_check(tensors, "hash_tensors")
        return self.hash([t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors], which, run_bytes)

    def sums(self, entry):
        """zgpu_seek_index_read_sums: entry `entry`'s sums, one int per row (0 for a skippable row); E_BAD_ARG for an entry without sums"""
        self._open("sums")
        n = C.c_uint32(0)
        rows = self.infos[entry].nrows if 0 <= entry < len(self.infos) else 0
        a = (C.c_uint32 * max(rows, 1))()
        self.ctx._check(self.L.zgpu_seek_index_read_sums(self.h, entry, a, rows, C.byref(n)), "zgpu_seek_index_read_sums")
        return list(a[:n.value])

    def set_sums(self, entry, sums):
        """zgpu_seek_index_set_sums: the caller's own sums for entry `entry`, one per row — a promise, as an anchor is"""
        self._open("set_sums")
        a = (C.c_uint32 * max(len(sums), 1))(*[int(x) & 0xFFFFFFFF for x in sums])
        self.ctx._check(self.L.zgpu_seek_index_set_sums(self.h, entry, a, len(sums)), "zgpu_seek_index_set_sums")

    @property
    def sums_infos(self):
        """one SeekIndexSums per entry (zgpu_seek_index_sums_of), as it stands now"""
        self._open("sums_infos")
        rec, out = SeekIndexSumsC(), []
        for i in range(len(self.infos)):
            self.ctx._check(self.L.zgpu_seek_index_sums_of(self.h, i, C.byref(rec)), "zgpu_seek_index_sums_of")
            out.append(SeekIndexSums(rec))
        return out

    def records_stats(self):
        """stats(sums=True) plus what records appends (zgpu_seek_index_stats [14] ...): records_submits, records_us (count + scan + emit, HIP
        events), records_chunks, records_held and records_offset_bytes (held now), records_bytes_downloaded"""
        self._open("records_stats")
        return _read_stats(self.L, "SeekIndex.records_stats", self.h)

    def records(self, src_ptrs, lens, delimiter=b"\n", which=None, run_bytes=0):
        """zgpu_seek_index_records_device: every zstd frame of every chosen entry decoded once, every byte equal to `delimiter` (one byte, or
        an int 0 .. 255) found on the device, and where each record begins kept in the index; nothing is delivered. src_ptrs / lens name the
        index's entries (all of them). which: one truth value per entry (None: all). run_bytes: plaintext per run of rows (0: 64 MiB). An
        entry with a failing run keeps no offsets; records_infos says which and why, ctx.last_error names the first. A record index is a
        promise about bytes, not a verdict: a stale one delivers the wrong bytes with status 0. Returns records_infos."""
        self._open("records")
        n = len(src_ptrs)
        _one_per("records", n, lens, which)
        d = delimiter[0] if isinstance(delimiter, (bytes, bytearray)) and len(delimiter) == 1 else delimiter
        if not isinstance(d, int) or d < 0:
            raise ValueError("records: a delimiter of one byte")
        w = None if which is None else bytes(1 if x else 0 for x in which)
        self.ctx._check(self.L.zgpu_seek_index_records_device(self.ctx.h, self.h, _ptr_array(src_ptrs), _size_array(lens), n, w, d, int(run_bytes)),
                        "zgpu_seek_index_records_device")
        return self.records_infos()

    def records_tensors(self, tensors, delimiter=b"\n", which=None, run_bytes=0):
        """records on torch tensors: tensors[i] is a contiguous torch.uint8 tensor on the index's device holding shard i."""
        self._open("records_tensors")
        self.ctx._tensor_check(tensors, "records_tensors")
        return self.records([t.data_ptr() if t.numel() else 0 for t in tensors], [t.numel() for t in tensors], delimiter, which, run_bytes)

    def record_offsets(self, entry, first=0, count=None):
        """zgpu_seek_index_read_records: O[first .. first + count) of entry `entry` (count None: to the end, O[R] = the entry's plaintext
        length included), as a list of ints; E_BAD_ARG for an entry without records. A size query, then the call."""
        self._open("record_offsets")
        n = C.c_uint64(0)
        self.ctx._check(self.L.zgpu_seek_index_read_records(self.h, entry, 0, None, 0, C.byref(n)), "zgpu_seek_index_read_records")
        cap = max(n.value - first, 0) if count is None else min(int(count), max(n.value - first, 0))
        a = (C.c_uint64 * max(cap, 1))()
        self.ctx._check(self.L.zgpu_seek_index_read_records(self.h, entry, int(first), a, cap, C.byref(n)), "zgpu_seek_index_read_records")
        return list(a[:n.value])

    def set_records(self, entry, offsets, delimiter=b"\n", open_tail=False):
        """zgpu_seek_index_set_records: the caller's own offsets for entry `entry` — O[0] = 0, strictly increasing, O[-1] = the entry's
        plaintext length, len(offsets) - 1 records; open_tail: the last record ends in no delimiter (the call cannot see the bytes) — a
        promise, as an anchor is"""
        self._open("set_records")
        d = delimiter[0] if isinstance(delimiter, (bytes, bytearray)) and len(delimiter) == 1 else delimiter
        if not isinstance(d, int) or d < 0 or not len(offsets):
            raise ValueError("set_records: a delimiter of one byte and at least O[0]")
        a = (C.c_uint64 * len(offsets))(*[int(x) for x in offsets])
        self.ctx._check(self.L.zgpu_seek_index_set_records(self.h, entry, a, len(offsets) - 1, d | (RECORDS_OPEN_TAIL if open_tail else 0)),
                        "zgpu_seek_index_set_records")

    def records_infos(self):
        """one SeekIndexRecords per entry (zgpu_seek_index_records_of), as it stands now"""
        self._open("records_infos")
        rec, out = SeekIndexRecordsC(), []
        for i in range(len(self.infos)):
            self.ctx._check(self.L.zgpu_seek_index_records_of(self.h, i, C.byref(rec)), "zgpu_seek_index_records_of")
            out.append(SeekIndexRecords(rec))
        return out

    def export_seek_table(self, entry, checksums=False):
        """zgpu_seek_index_export_seek_table_ex: entry `entry`'s rows as one seek table frame of zstd's seekable format, as bytes — what
        seek_table_frame(csizes, dsizes) builds for those rows, or, checksums=True, seek_table_frame(csizes, dsizes, self.sums(entry)) (the
        entry must have sums). Appended behind the entry's bytes it makes the entry seekable: a file written that way never needs measuring
        again, and with checksums it passes verify_table by its table. A size query, then the call."""
        self._open("export_seek_table")
        flags = EXPORT_CHECKSUMS if checksums else 0
        need = C.c_size_t(0)
        st = self.L.zgpu_seek_index_export_seek_table_ex(self.h, entry, flags, None, 0, C.byref(need))
        if st != E_TARGET_TOO_SMALL:
            self.ctx._check(st if st else E_BAD_ARG, "zgpu_seek_index_export_seek_table_ex")
        buf = C.create_string_buffer(need.value)
        self.ctx._check(self.L.zgpu_seek_index_export_seek_table_ex(self.h, entry, flags, buf, need.value, C.byref(need)),
                        "zgpu_seek_index_export_seek_table_ex")
        return buf.raw[:need.value]

    def close(self):
        if getattr(self, "h", None):
            self.L.zgpu_seek_index_destroy(self.h)
            self.h = None
            if self in self.ctx._indexes:
                self.ctx._indexes.remove(self)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __len__(self):
        return len(self.infos)


class Batch:
    """A run of whole frames resident on the device (zgpu_batch)."""

    def __init__(self, ctx, src):
        self.ctx, self.L = ctx, ctx.L
        h = C.c_void_p()
        self.parse_status = self.L.zgpu_batch_prepare(ctx.h, src, len(src), C.byref(h))
        if not h:
            raise ZgpuError(self.parse_status)
        self.h = h
        self.nframes = self.L.zgpu_batch_num_frames(h)
        self.nblocks = self.L.zgpu_batch_num_blocks(h)

    def close(self):
        if getattr(self, "h", None):
            self.L.zgpu_batch_destroy(self.h)
            self.h = None

    __del__ = close

    def run(self):
        self.ctx._check(self.L.zgpu_batch_run(self.h))

    def sync(self):
        tot, bf, bs = C.c_uint64(), C.c_uint32(), C.c_uint32()
        st = self.L.zgpu_batch_sync(self.h, C.byref(tot), C.byref(bf), C.byref(bs))
        if st != E_UNSUPPORTED:
            self.ctx._check(st)
        self.total_out, self.bad_frame, self.bad_status = tot.value, bf.value, bs.value or st
        return self.total_out

    def timings(self):
        a = (C.c_float * 10)()
        self.L.zgpu_batch_timings(self.h, a, 10)
        return dict(zip(_TIMING_KEYS, list(a)))

    def debug_timers(self):
        a = (C.c_uint64 * 1024)()
        self.L.zgpu_batch_debug_timers(self.h, a)
        return list(a)

    def sweep_mode(self):
        """after sync: 0 plain chain of sweep steps, 1 split into tails and heads, 2 split and then repeated as a plain chain"""
        return int(self.L.zgpu_batch_debug_sweep_mode(self.h))

    def lit_direct(self):
        """after run: did the last run decode its Huffman literals after the position scan (ZG_FLAG_LIT_DIRECT: zg_k_litfix finds their verdicts)"""
        return bool(self.L.zgpu_batch_debug_lit_direct(self.h))

    def units(self):
        """[(first_block, nblocks, scratch_base, size, noseq)] — the units zg_k_flatten worked on (size valid after sync); noseq: bit 0: no
        block of the unit has sequences, bit 1: direct unit (resolved to bytes by the flatten itself); either way it has no scratch
        words and no sweep step"""
        out = []
        for u in range(self.L.zgpu_batch_num_units(self.h)):
            fb, nb, base = C.c_uint32(), C.c_uint32(), C.c_uint64()
            assert self.L.zgpu_batch_unit(self.h, u, C.byref(fb), C.byref(nb), C.byref(base)) == 0
            info = (C.c_uint32 * 4)()
            assert self.L.zgpu_batch_debug_scratch(self.h, 1, 16 * u, info, 16) == 0
            out.append((fb.value, nb.value, base.value, info[0], int(info[1])))
        return out

    def scratch_words(self, base, n):
        """n effective offsets (u32) of the flatten scratch starting at word `base`, as a numpy array"""
        import numpy as np
        arr = np.empty(max(n, 1), dtype=np.uint32)
        st = self.L.zgpu_batch_debug_scratch(self.h, 0, 4 * base, arr.ctypes.data_as(C.c_void_p), 4 * n)
        if st:
            raise ZgpuError(st)
        return arr[:n]

    def frame_info(self, f):
        fi = FrameInfo()
        assert self.L.zgpu_batch_frame_info(self.h, f, C.byref(fi)) == 0
        return fi

    def read(self, off, n):
        buf = C.create_string_buffer(max(n, 1))
        st = self.L.zgpu_batch_read(self.h, off, buf, n)
        if st:
            raise ZgpuError(st)
        return buf.raw[:n]

    def checksums(self):
        """zgpu_batch_checksums (after sync): XXH64 (seed 0, 64 bits) of every frame's output bytes, computed on the device"""
        a = (C.c_uint64 * max(self.nframes, 1))()
        st = self.L.zgpu_batch_checksums(self.h, a, self.nframes)
        if st:
            raise ZgpuError(st)
        return [int(x) for x in a][:self.nframes]

    def frame_bytes(self, f):
        fi = self.frame_info(f)
        return self.read(fi.out_base, fi.out_size)

    def output_device_ptr(self):
        return self.L.zgpu_batch_output_device(self.h)

    def block_info(self, b):
        bi = BlockInfo()
        st = self.L.zgpu_batch_block_info(self.h, b, C.byref(bi))
        if st:
            raise ZgpuError(st)
        return bi

    def block_literals(self, b, n):
        buf = C.create_string_buffer(max(n, 1))
        got = C.c_size_t()
        st = self.L.zgpu_batch_block_literals(self.h, b, buf, n, C.byref(got))
        if st:
            raise ZgpuError(st)
        return buf.raw[:got.value]

    def block_sequences(self, b, n):
        arr = (Seq * max(n, 1))()
        got = C.c_size_t()
        st = self.L.zgpu_batch_block_sequences(self.h, b, arr, n, C.byref(got))
        if st:
            raise ZgpuError(st)
        return [(arr[i].of, arr[i].ml, arr[i].mdst, arr[i].lit_start) for i in range(got.value)]

    def fse_slot(self, slot):
        ent = (C.c_uint32 * 1280)()
        lg = (C.c_uint8 * 4)()
        st = self.L.zgpu_batch_fse_slot(self.h, slot, ent, lg)
        if st:
            raise ZgpuError(st)
        return ent, list(lg)

    def huf_slot(self, slot):
        ent = (C.c_uint16 * 2048)()
        mb = C.c_int()
        st = self.L.zgpu_batch_huf_slot(self.h, slot, ent, C.byref(mb))
        if st:
            raise ZgpuError(st)
        return ent, mb.value


class FrameDecoder:
    """Mirror of ruzstd::decoding::FrameDecoder (frame_decoder.rs:80-627) on the GPU engine."""

    def __init__(self, ctx=None):
        self.ctx = ctx or Context()
        self.L = self.ctx.L
        h = C.c_void_p()
        st = self.L.zgpu_decoder_create(self.ctx.h, C.byref(h))
        if st:
            raise ZgpuError(st)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.zgpu_decoder_destroy(self.h)
            self.h = None

    __del__ = close

    def set_max_window_size(self, n):
        self.ctx.set_max_window_size(n)

    def init(self, src):
        """reset(): returns (status, consumed, skip_magic, skip_len); SkipFrame is a status, as in the reference"""
        c, sm, sl = C.c_size_t(), C.c_uint32(), C.c_uint32()
        st = self.L.zgpu_decoder_init(self.h, src, len(src), C.byref(c), C.byref(sm), C.byref(sl))
        return st, c.value, sm.value, sl.value

    reset = init

    def decode_blocks(self, src, strat=STRAT_ALL, n=0):
        c, fin = C.c_size_t(), C.c_int()
        st = self.L.zgpu_decoder_decode_blocks(self.h, src, len(src), C.byref(c), strat, n, C.byref(fin))
        return st, c.value, bool(fin.value)

    def add_dict(self, raw):
        return self.ctx.add_dict(raw)

    def force_dict(self, dict_id):
        return self.L.zgpu_decoder_force_dict(self.h, dict_id)

    def decode_from_to(self, src, cap):
        """returns (status, bytes_read, output_bytes) — frame_decoder.rs:439-529"""
        buf = C.create_string_buffer(max(cap, 1))
        r, w = C.c_size_t(), C.c_size_t()
        st = self.L.zgpu_decoder_decode_from_to(self.h, src, len(src), buf, cap, C.byref(r), C.byref(w))
        return st, r.value, buf.raw[:w.value]

    def can_collect(self):
        return self.L.zgpu_decoder_can_collect(self.h)

    def collect(self):
        n = self.can_collect()
        buf = C.create_string_buffer(max(n, 1))
        got = self.L.zgpu_decoder_collect(self.h, buf, n)
        return buf.raw[:got]

    def read(self, cap):
        buf = C.create_string_buffer(max(cap, 1))
        got = self.L.zgpu_decoder_read(self.h, buf, cap)
        return buf.raw[:got]

    def is_finished(self):
        return bool(self.L.zgpu_decoder_is_finished(self.h))

    def set_hash(self, on):
        self.L.zgpu_decoder_set_hash(self.h, 1 if on else 0)

    def set_read_ahead(self, n):
        self.L.zgpu_decoder_set_read_ahead(self.h, n)

    def blocks_decoded(self):
        return self.L.zgpu_decoder_blocks_decoded(self.h)

    def bytes_read_from_source(self):
        return self.L.zgpu_decoder_bytes_read_from_source(self.h)

    def content_size(self):
        return self.L.zgpu_decoder_content_size(self.h)

    def get_checksum_from_data(self):
        v = C.c_uint32()
        return v.value if self.L.zgpu_decoder_checksum_from_data(self.h, C.byref(v)) else None

    def get_calculated_checksum(self):
        return self.L.zgpu_decoder_calculated_checksum(self.h)

    def decode_all(self, src, cap):
        return self.ctx.decode_all(src, cap)

    def collect_to_writer(self, writer):
        """collect_to_writer (frame_decoder.rs:395-407); writer.write(bytes) -> number of bytes taken"""
        def wr(_user, data, n):
            return writer.write(C.string_at(data, n))
        cb = WRITE_FN(wr)
        done = C.c_size_t()
        st = self.L.zgpu_decoder_collect_to_writer(self.h, cb, None, C.byref(done))
        if st:
            raise ZgpuError(st)
        return done.value


def plan(costs, n_workers):
    """the work queue's plan, host only: (LPT order, worker of every job, load per worker) — zgpu_pool_plan"""
    L = load_library()
    n = len(costs)
    c = (C.c_uint64 * max(n, 1))(*costs)
    order, worker, load = (C.c_uint32 * max(n, 1))(), (C.c_uint32 * max(n, 1))(), (C.c_uint64 * n_workers)()
    st = L.zgpu_pool_plan(c, n, n_workers, order, worker, load)
    if st:
        raise ZgpuError(st)
    return list(order)[:n], list(worker)[:n], list(load)


class Pool:
    """Frames over the GPUs of one node through the library's work queue (zgpu_pool): one worker thread + engine per GPU."""

    def __init__(self, n_gpus=0, devices=None, dev=False):
        self.L = load_library(dev)
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            st = self.L.zgpu_pool_create_on(arr, len(devices), C.byref(h))
        else:
            st = self.L.zgpu_pool_create(n_gpus, C.byref(h))
        if st:
            raise ZgpuError(st, "zgpu_pool_create: no usable MI355X/HIP device — the engine has no CPU path")
        self.h = h
        self.n_gpus = self.L.zgpu_pool_num_gpus(h)
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.zgpu_pool_destroy(self.h)
            self.h = None

    __del__ = close

    def decode_all(self, src, cap):
        import numpy as np
        w = C.c_size_t()
        arr = np.empty(max(cap, 1), dtype=np.uint8)
        st = self.L.zgpu_pool_decode_all(self.h, src, len(src), arr.ctypes.data_as(C.c_void_p), cap, C.byref(w))
        if st:
            raise ZgpuError(st)
        return arr[:w.value].tobytes()

    def stage(self, frames):
        n = len(frames)
        ptrs = (C.c_char_p * max(n, 1))(*frames)
        lens = (C.c_size_t * max(n, 1))(*[len(f) for f in frames])
        self._keep = frames
        st = self.L.zgpu_pool_stage(self.h, ptrs, lens, n)
        if st:
            raise ZgpuError(st)
        self.nstaged = n

    def run(self):
        """one pass over everything staged; returns (per-GPU kernel ms, wall ms)"""
        g, w = (C.c_float * self.n_gpus)(), C.c_float()
        st = self.L.zgpu_pool_run(self.h, g, C.byref(w))
        if st:
            raise ZgpuError(st)
        return list(g), w.value

    def timings(self, g=0):
        """per-kernel times (ms) of GPU g's last pass + (plaintext bytes, compressed bytes, blocks) of its resident submit"""
        a = (C.c_float * 10)()
        pb, cb, nb, nj = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        st = self.L.zgpu_pool_timings(self.h, g, a, 10, C.byref(pb), C.byref(cb), C.byref(nb), C.byref(nj))
        if st:
            raise ZgpuError(st)
        self.last_njobs = nj.value
        return dict(zip(_TIMING_KEYS, list(a))), pb.value, cb.value, nb.value

    def plan_stats(self, g=0):
        """the LZ77 plan of GPU g's resident jobs after a run (zgpu_pool_plan_stats)"""
        return _read_stats(self.L, "Pool.plan_stats", self.h, g, counted=False)

    def frame(self, i):
        gpu, size, st = C.c_int(), C.c_uint64(), C.c_uint32()
        r = self.L.zgpu_pool_frame(self.h, i, C.byref(gpu), C.byref(size), C.byref(st))
        if r:
            raise ZgpuError(r)
        return gpu.value, size.value, st.value

    def read(self, i, cap):
        import numpy as np
        arr = np.empty(max(cap, 1), dtype=np.uint8)
        w = C.c_size_t()
        st = self.L.zgpu_pool_read(self.h, i, arr.ctypes.data_as(C.c_void_p), cap, C.byref(w))
        if st:
            raise ZgpuError(st)
        return arr[:w.value].tobytes()


class CStreamingDecoder:
    """zgpu_streaming (the C-ABI mirror of StreamingDecoder, streaming_decoder.rs:40-156) over a Python file-like source, or over
    bytes / a numpy array (source=None, data=...: zgpu_streaming_create_slice, nothing is copied on the host).
    read_ahead: bytes decoded ahead of the reader at most (ring size); NO_READ_AHEAD: the reference's block-by-block schedule."""

    def __init__(self, ctx, source=None, data=None, read_ahead=0, checksum=True, pipe_after=0, first_run_blocks=0, copy_threads=0):
        self.L, self.source, self.ctx = ctx.L, source, ctx      # (the context must outlive the stream)
        o = StreamOpts(read_ahead, 0 if checksum else 1, copy_threads, pipe_after, first_run_blocks, 0)
        h = C.c_void_p()
        if source is not None:
            def rd(_user, dst, n):
                b = source.read(n)
                C.memmove(dst, b, len(b))
                return len(b)
            self._cb = READ_FN(rd)
            st = self.L.zgpu_streaming_create_ex(ctx.h, self._cb, None, C.byref(o), C.byref(h))
        else:
            self._keep = data
            if isinstance(data, (bytes, bytearray)):
                self._buf = (C.c_char * len(data)).from_buffer_copy(data) if isinstance(data, bytes) else (C.c_char * len(data)).from_buffer(data)
                ptr, n = C.addressof(self._buf), len(data)
            elif isinstance(data, tuple):                  # (address, length): e.g. pinned memory of a torch tensor
                ptr, n = data
            else:                                          # numpy array
                ptr, n = data.ctypes.data, data.nbytes
            st = self.L.zgpu_streaming_create_slice(ctx.h, ptr, n, C.byref(o), C.byref(h))
        if st:
            raise ZgpuError(st)
        self.h = h

    def read(self, n):
        buf = C.create_string_buffer(max(n, 1))
        got = C.c_size_t()
        st = self.L.zgpu_streaming_read(self.h, buf, n, C.byref(got))
        if st:
            raise ZgpuError(st)
        return buf.raw[:got.value]

    def read_into(self, addr, n):
        """read(&mut buf[..n]) into memory the caller owns; returns the byte count"""
        got = C.c_size_t()
        st = self.L.zgpu_streaming_read(self.h, addr, n, C.byref(got))
        if st:
            raise ZgpuError(st)
        return got.value

    def copy_to_sink(self, buf_size):
        """std::io::copy(&mut decoder, &mut io::sink()) with a buffer of buf_size bytes; returns the bytes copied"""
        total = C.c_uint64()
        st = self.L.zgpu_streaming_copy(self.h, buf_size, None, None, C.byref(total))
        if st:
            raise ZgpuError(st)
        return total.value

    def _dec(self):
        self.L.zgpu_streaming_decoder.restype = C.c_void_p
        self.L.zgpu_streaming_decoder.argtypes = [C.c_void_p]
        return self.L.zgpu_streaming_decoder(self.h)

    def device_bytes(self):
        """device memory the frame holds right now (zgpu_decoder_device_bytes of the decoder behind the stream)"""
        return self.L.zgpu_decoder_device_bytes(self._dec())

    def is_finished(self):
        return bool(self.L.zgpu_decoder_is_finished(self._dec()))

    def get_calculated_checksum(self):
        return self.L.zgpu_decoder_calculated_checksum(self._dec())

    def get_checksum_from_data(self):
        v = C.c_uint32()
        return v.value if self.L.zgpu_decoder_checksum_from_data(self._dec(), C.byref(v)) else None

    def blocks_decoded(self):
        return self.L.zgpu_decoder_blocks_decoded(self._dec())

    def bytes_read_from_source(self):
        return self.L.zgpu_decoder_bytes_read_from_source(self._dec())

    def error(self):
        """the engine error that ended the stream (every read() returns it from then on); 0: none"""
        return self.L.zgpu_decoder_stream_error(self._dec())

    def source_position(self):
        return self.L.zgpu_streaming_source_position(self.h)

    def stats(self):
        return _read_stats(self.L, "CStreamingDecoder.stats", self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.zgpu_streaming_destroy(self.h)
            self.h = None

    __del__ = close


class StreamingDecoder:
    """Mirror of ruzstd::decoding::StreamingDecoder (streaming_decoder.rs:40-156): an io-style reader over ONE frame.

    source: a binary file-like object positioned at the frame header. The decoder reads exactly the bytes the
    reference would: the frame header, then whole blocks as read() needs them."""

    def __init__(self, source, decoder=None, ctx=None, max_window_size=None):
        self.source = source
        self.decoder = decoder or FrameDecoder(ctx)
        if max_window_size is not None:
            self.decoder.set_max_window_size(max_window_size)
        # frame header: 4 magic + 1 descriptor tell how long the rest is (frame.rs:6-85)
        head = source.read(5)
        if len(head) == 5 and head[:4] == bytes([0x28, 0xB5, 0x2F, 0xFD]):
            desc = head[4]
            single = (desc >> 5) & 1
            extra = (0 if single else 1) + (0, 1, 2, 4)[desc & 3] + ((1 if single else 0), 2, 4, 8)[desc >> 6]
            head += source.read(extra)
        else:
            head += source.read(3)
        self._cs = len(head) >= 5 and bool((head[4] >> 2) & 1)
        st, used, _, _ = self.decoder.reset(head)
        if st:
            raise ZgpuError(st)
        assert used == len(head)

    def _read_blocks(self, n):
        """n whole blocks (or up to the last block) from the source, as one byte string"""
        out = []
        for _ in range(n):
            hdr = self.source.read(3)
            out.append(hdr)
            if len(hdr) < 3:
                break
            btype = (hdr[0] >> 1) & 3
            size = (hdr[0] >> 3) | (hdr[1] << 5) | (hdr[2] << 13)
            out.append(self.source.read(1 if btype == 1 else size))
            if hdr[0] & 1:
                if (self.decoder_checksum_flag):
                    out.append(self.source.read(4))
                break
        return b"".join(out)

    @property
    def decoder_checksum_flag(self):
        return self._cs

    def read(self, n=-1):
        """impl Read (streaming_decoder.rs:119-155)"""
        d = self.decoder
        if n is None or n < 0:
            chunks = []
            while True:
                c = self.read(1 << 20)
                if not c:
                    return b"".join(chunks)
                chunks.append(c)
        if d.is_finished() and d.can_collect() == 0:
            return b""
        while d.can_collect() < n and not d.is_finished():
            need = n - d.can_collect()
            m = max(1, (need + (128 << 10) - 1) // (128 << 10))      # UptoBytes(need) never stops before ceil(need / 128 KiB) blocks
            data = self._read_blocks(m)
            st, used, fin = d.decode_blocks(data, STRAT_UPTO_BLOCKS, m)
            if st:
                raise ZgpuError(st)
        return d.read(n)

    def into_frame_decoder(self):
        return self.decoder


class BlockFrame:
    """The thin boundary (include/zgpu.h: zgpu_frame_begin / zgpu_blocks_submit / zgpu_sync / zgpu_read): the caller parses the
    frame header and the 3-byte block headers itself (as ruzstd's FrameDecoder does before it calls decode_block_content,
    frame_decoder.rs:319-375) and submits block tables."""

    def __init__(self, ctx, window_size, content_size=0, dict_id=0):
        self.L = ctx.L
        self.h = C.c_void_p()
        st = self.L.zgpu_frame_begin(ctx.h, window_size, content_size, dict_id, C.byref(self.h))
        if st:
            self.h = None
            raise ZgpuError(st)

    def close(self):
        if self.h:
            self.L.zgpu_frame_end(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def submit(self, src, blocks):
        """blocks: [(src_off, src_len, type, last, raw_rle_size)] offsets into src"""
        arr = (Block * max(len(blocks), 1))()
        for i, (off, ln, ty, last, sz) in enumerate(blocks):
            arr[i].src_off, arr[i].src_len, arr[i].type, arr[i].last, arr[i].raw_rle_size = off, ln, ty, last, sz
        st = self.L.zgpu_blocks_submit(self.h, src, len(src), arr, len(blocks))
        if st:
            raise ZgpuError(st)

    def sync(self):
        """returns (first_bad_block or None, its status)"""
        bad, st = C.c_size_t(), C.c_int32()
        r = self.L.zgpu_sync(self.h, C.byref(bad), C.byref(st))
        if r:
            raise ZgpuError(r)
        return (None if bad.value == C.c_size_t(-1).value else bad.value), st.value

    def available(self, finished):
        return self.L.zgpu_available(self.h, 1 if finished else 0)

    def read(self, cap, finished):
        buf = C.create_string_buffer(max(cap, 1))
        n = C.c_size_t()
        st = self.L.zgpu_read(self.h, buf, cap, 1 if finished else 0, C.byref(n))
        if st:
            raise ZgpuError(st)
        return buf.raw[:n.value]

    def device_output(self):
        p, n = C.c_void_p(), C.c_size_t()
        st = self.L.zgpu_device_output(self.h, C.byref(p), C.byref(n))
        if st:
            raise ZgpuError(st)
        return p.value, n.value

    def checksum(self):
        return self.L.zgpu_frame_checksum(self.h)

    def blocks_decoded(self):
        return self.L.zgpu_frame_blocks_decoded(self.h)
