"""The C ABI of the record index (zgpu_seek_index_records_device, _records_of, _read_records, _set_records,
zgpu_seek_index_record_ranges_device, zgpu_gather_records_indexed_device_src, and the appended slots of zgpu_seek_index_stats and
zgpu_debug_ranges_stats) and its marshalling in zgpu.py, without a GPU: both libraries export the symbols and the header declares them, the
records' sizes and fields are the header's, the constants match, the appended statistics slots are the enumerators of zg_capi_int.h and the
header documents them, the argument rules that need no device answer ZGPU_E_BAD_ARG, and the methods of zgpu.SeekIndex and zgpu.Context hand
the C functions what they are given (checked on a fake handle over a recording library)."""
import ctypes as C
import inspect
import os
import re

import pytest

import zgpu
from test_seek_index_sums_binding_cpu import _Ctx, _Recorder, _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zgpu_seek_index_records_device", "zgpu_seek_index_records_of", "zgpu_seek_index_read_records", "zgpu_seek_index_set_records",
       "zgpu_seek_index_record_ranges_device", "zgpu_gather_records_indexed_device_src")


class _RecordsCtx(_Ctx):
    """the fake context with what the record calls of zgpu.Context use"""
    _index_handle = zgpu.Context._index_handle
    _record_ranges = staticmethod(zgpu.Context._record_ranges)
    _decode_call = zgpu.Context._decode_call
    record_ranges = zgpu.Context.record_ranges
    gather_records_indexed_device_src = zgpu.Context.gather_records_indexed_device_src


def _fields(header, name):
    body = header.split("} %s;" % name)[0].rsplit("typedef struct {", 1)[1]
    return [f for decl in re.findall(r"uint(?:32|64)_t ([\w, ]+);", body) for f in decl.split(", ")]


def _snake(text, prefix):
    names = re.findall(r"\b%s(\w+)" % prefix, [m for m in re.findall(r"enum\s*\{([^}]*)\}", text) if prefix in m][0])
    assert names[-1] == "Count"
    return [re.sub(r"(?<!^)([A-Z])", r"_\1", k).lower() for k in names[:-1]]


def test_symbols_structs_and_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in NEW:
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym) and re.search(r"^int %s\(" % sym, header, re.M), sym
    assert C.sizeof(zgpu.SeekIndexRecordsC) == 32 and C.sizeof(zgpu.RecordRangeC) == 24 and C.sizeof(zgpu.EntryRangeC) == 24
    assert (zgpu.SeekIndexRecordsC.nrecords.offset, zgpu.SeekIndexRecordsC.row_lo.offset, zgpu.RecordRangeC.entry.offset) == (16, 24, 16)
    assert _fields(header, "zgpu_seek_index_records") == [f for f, _ in zgpu.SeekIndexRecordsC._fields_] == list(zgpu.SeekIndexRecords.FIELDS)
    line = [ln for ln in header.splitlines() if "} zgpu_record_range;" in ln][0]
    assert re.findall(r"uint(?:32|64)_t ([\w, ]+);", line) == ["first, count", "entry, flags"]
    assert [f for f, _ in zgpu.RecordRangeC._fields_] == ["first", "count", "entry", "flags"]
    assert "#define ZGPU_RECORDS_STRIP %du" % zgpu.RECORDS_STRIP in header and zgpu.RECORDS_STRIP == 1
    assert "#define ZGPU_RECORDS_OPEN_TAIL 0x%08Xu" % zgpu.RECORDS_OPEN_TAIL in header and zgpu.RECORDS_OPEN_TAIL == 1 << 31
    assert (zgpu.RECORDS_NONE, zgpu.RECORDS_FOUND, zgpu.RECORDS_SET) == (0, 1, 2)
    # the appended statistics: the enumerators of zg_capi_int.h behind those the getters always had, and the header says where they lie
    text = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_capi_int.h")).read()
    keys = zgpu._STATS["SeekIndex.records_stats"][2]
    assert keys[:14] == zgpu._STATS["SeekIndex.sums_stats"][2]
    assert _snake(text, "kRecStat") == ["submits", "us", "chunks", "records_held", "offset_bytes", "bytes_downloaded"]
    assert list(keys[14:]) == ["records_submits", "records_us", "records_chunks", "records_held", "records_offset_bytes", "records_bytes_downloaded"]
    assert ["record_find_" + k for k in _snake(text, "kRecFindStat")] == list(zgpu.Context.RECORD_STATS)
    assert len(zgpu._STATS["Context.ranges_stats"][2]) + len(zgpu.Context.GATHER_STATS) == 19
    section = header.split("record index: gather delimited records", 1)[1].split("the same over several GPUs", 1)[0]
    for word in ("[14] decode submits of the record passes", "[15] the microseconds of count + scan + emit", "[16] chunks scanned", "[17] records held",
                 "[18] bytes of offsets held", "[19] bytes that came back from the side pass", "A caller that\n * asks for 14 gets what it always got",
                 "[19] record find launches, [20] their microseconds, [21] bytes back",
                 "A PROMISE ABOUT BYTES, NOT A VERDICT", "ALL OR NOTHING PER ENTRY", "PEAK EXTRA DEVICE MEMORY IS TWICE THE FINAL ARRAY",
                 "zg_k_recs_count", "zg_k_recs_scan", "zg_k_recs_emit", "zg_k_recs_find", "Out of scope: host sources, several GPUs, multi-byte delimiters"):
        assert word in section, word
    # the kernels' header has the house form: what each wave reads and writes, and the ISA facts
    rec = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_records.h")).read()
    for word in ("ZG_RECORDS_TYPES", "ZG_RECORDS_WAVE", "Reads:", "gfx950 ISA", "VGPRs", "no scratch", "global_load_dwordx4", "global_store_dwordx2",
                 "kChunk = 4096"):
        assert word in rec, word
    # the Python surface
    for meth in ("records", "records_tensors", "record_offsets", "set_records", "records_infos", "records_stats"):
        assert callable(getattr(zgpu.SeekIndex, meth)), meth
    for meth in ("record_ranges", "gather_records_indexed_device_src", "gather_tensor_records", "gather_records_stats"):
        assert callable(getattr(zgpu.Context, meth)), meth
    sig = inspect.signature(zgpu.SeekIndex.records).parameters
    assert sig["delimiter"].default == b"\n" and sig["which"].default is None and sig["run_bytes"].default == 0
    sig = inspect.signature(zgpu.SeekIndex.record_offsets).parameters
    assert sig["first"].default == 0 and sig["count"].default is None


def test_argument_rules_need_no_gpu():
    for dev in (False, True):
        L = zgpu.load_library(dev=dev)
        n = 1
        srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
        fake = C.create_string_buffer(4096)    # stands for a context where the call refuses before it looks at it
        mine = C.create_string_buffer(4096)    # a handle of that context that holds no entry: the first word of a zgpu_seek_index is its context
        C.memmove(mine, C.byref(C.c_void_p(C.addressof(fake))), 8)
        other = C.create_string_buffer(4096)   # a handle of another context
        C.memmove(other, C.byref(C.c_void_p(C.addressof(fake) + 64)), 8)
        # the pass: no context, no handle, a handle of another context, n that is not the entry count, a delimiter that is no byte
        assert L.zgpu_seek_index_records_device(None, mine, srcs, lens, 0, None, 10, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_device(fake, None, srcs, lens, 0, None, 10, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_device(fake, other, srcs, lens, 0, None, 10, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_device(fake, mine, srcs, lens, n, None, 10, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_device(fake, mine, srcs, lens, 0, None, 256, 0) == zgpu.E_BAD_ARG
        # offsets in and out: a null handle, an entry out of range, null pointers
        a, got = (C.c_uint64 * 3)(0, 2, 4), C.c_uint64(9)
        assert L.zgpu_seek_index_set_records(None, 0, a, 2, 10) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_set_records(mine, 0, a, 2, 10) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_read_records(None, 0, 0, a, 3, C.byref(got)) == zgpu.E_BAD_ARG and got.value == 0
        assert L.zgpu_seek_index_read_records(mine, 0, 0, a, 3, C.byref(got)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_read_records(mine, 0, 0, a, 3, None) == zgpu.E_BAD_ARG
        assert list(a) == [0, 2, 4]
        rec = zgpu.SeekIndexRecordsC()
        assert L.zgpu_seek_index_records_of(None, 0, C.byref(rec)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_of(mine, 0, C.byref(rec)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_records_of(mine, 0, None) == zgpu.E_BAD_ARG
        # the lookup and the gather: no context, no handle, another context's handle, null arrays with m > 0
        rr, out, st = (zgpu.RecordRangeC * 1)(), (zgpu.EntryRangeC * 1)(), (C.c_uint32 * 1)(7)
        assert L.zgpu_seek_index_record_ranges_device(None, mine, rr, 1, out, st) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_record_ranges_device(fake, None, rr, 1, out, st) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_record_ranges_device(fake, other, rr, 1, out, st) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_record_ranges_device(fake, mine, None, 1, out, st) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_record_ranges_device(fake, mine, rr, 1, out, None) == zgpu.E_BAD_ARG and st[0] == 7
        res, dsts, caps = (zgpu.RangeResultC * 1)(), (C.c_void_p * 1)(), (C.c_size_t * 1)()
        assert L.zgpu_gather_records_indexed_device_src(None, mine, srcs, lens, 0, rr, 1, dsts, caps, None, res) == zgpu.E_BAD_ARG
        assert L.zgpu_gather_records_indexed_device_src(fake, other, srcs, lens, 0, rr, 1, dsts, caps, None, res) == zgpu.E_BAD_ARG
        assert L.zgpu_gather_records_indexed_device_src(fake, mine, srcs, lens, n, rr, 1, dsts, caps, None, res) == zgpu.E_BAD_ARG
        assert L.zgpu_gather_records_indexed_device_src(fake, mine, srcs, lens, 0, rr, 1, dsts, caps, None, None) == zgpu.E_BAD_ARG
        # the getters on a null handle or context write nothing
        out20 = (C.c_uint64 * 22)(*([7] * 22))
        assert L.zgpu_seek_index_stats(None, out20, 20) == 0 and L.zgpu_debug_ranges_stats(None, out20, 22) == 0 and list(out20) == [7] * 22


def test_marshalling_on_a_fake_handle():
    L = _Recorder()
    x = _index(L, [3, 0])
    # records: the handle, one pointer and one length per entry, `which` as bytes, the delimiter as a byte's value, run_bytes
    x.records([4096, 0], [10, 0], which=[0, 5], run_bytes=1 << 20)
    name, a = L.calls[0]
    assert name == "zgpu_seek_index_records_device" and a[0] == 1234 and a[1] == 77 and list(a[2]) == [4096, None] and list(a[3]) == [10, 0]
    assert a[4:] == (2, b"\x00\x01", 10, 1 << 20)
    assert [c[0] for c in L.calls[1:]] == ["zgpu_seek_index_records_of"] * 2   # (records returns records_infos())
    L.calls.clear()
    x.records([4096, 0], [10, 0], delimiter=b"\x00")
    assert L.calls[0][1][4:] == (2, None, 0, 0)
    L.calls.clear()
    x.records([4096, 0], [10, 0], delimiter=255)
    assert L.calls[0][1][4:] == (2, None, 255, 0)
    for bad in (lambda: x.records([4096, 0], [10]), lambda: x.records([4096, 0], [10, 0], which=[1]), lambda: x.records([4096, 0], [10, 0], delimiter=b"ab"),
                lambda: x.set_records(0, [])):
        with pytest.raises(ValueError):
            bad()
    # set_records: nrecords + 1 words, the open-tail bit in the delimiter's word
    L.calls.clear()
    x.set_records(0, [0, 5, 9], delimiter=b"\x00", open_tail=True)
    x.set_records(1, [0])
    (name, a), (_, b) = L.calls
    assert name == "zgpu_seek_index_set_records" and a[:2] == (77, 0) and list(a[2]) == [0, 5, 9] and a[3:] == (2, zgpu.RECORDS_OPEN_TAIL)
    assert b[1] == 1 and list(b[2]) == [0] and b[3:] == (0, 10)

    # record_offsets: a size query, then a buffer of what is asked for, cut to what the call says it wrote
    def read(h, entry, first, dst, cap, n):
        if dst is None:
            n._obj.value = 6
            return 0
        for k in range(cap):
            dst[k] = 100 + first + k
        n._obj.value = cap
        return 0
    x = _index(_Recorder({"zgpu_seek_index_read_records": read}), [3, 0])
    assert x.record_offsets(0) == [100, 101, 102, 103, 104, 105] and x.record_offsets(0, 4) == [104, 105] and x.record_offsets(0, 1, 2) == [101, 102]
    assert x.record_offsets(0, 9) == [] and x.record_offsets(0, 2, 100) == [102, 103, 104, 105]
    assert [(c[1][2], c[1][4]) for c in x.L.calls if c[1][3] is not None] == [(0, 6), (4, 2), (1, 2), (9, 0), (2, 4)]
    # the lookup and the gather: (entry, first, count[, flags]) become zgpu_record_range records
    L = _Recorder()
    x = _index(L, [3, 0])
    x.ctx = _RecordsCtx(L)
    ranges, st = x.ctx.record_ranges(x, [(1, 2, 3), (0, 7, 1 << 63, zgpu.RECORDS_STRIP)])
    name, a = L.calls[0]
    assert name == "zgpu_seek_index_record_ranges_device" and a[:2] == (1234, 77) and a[3] == 2 and st == [0, 0] and ranges == [(0, 0, 0)] * 2
    assert [(r.entry, r.first, r.count, r.flags) for r in a[2][:2]] == [(1, 2, 3, 0), (0, 7, 1 << 63, 1)]
    L.calls.clear()
    x.ctx.gather_records_indexed_device_src(x, [4096, 0], [10, 0], [(0, 1, 1)], [8192], [64], verify_table=True)
    name, a = L.calls[0]
    assert name == "zgpu_gather_records_indexed_device_src" and a[:2] == (1234, 77) and list(a[2]) == [4096, None] and a[4] == 2 and a[6] == 1
    assert (a[5][0].entry, a[5][0].first, a[5][0].count) == (0, 1, 1) and list(a[7]) == [8192] and list(a[8]) == [64] and a[9]._obj.flags == 4
    with pytest.raises(ValueError):
        x.ctx.gather_records_indexed_device_src(x, [4096, 0], [10, 0], [(0, 1, 1)], [8192], [])
    # an error is raised with the call's name; a closed index refuses
    x = _index(_Recorder({"zgpu_seek_index_set_records": zgpu.E_BAD_ARG}), [3])
    with pytest.raises(zgpu.ZgpuError):
        x.set_records(0, [0, 2])
    x.h = None
    for call in (lambda: x.records([], []), lambda: x.record_offsets(0), lambda: x.set_records(0, [0]), lambda: x.records_infos(), lambda: x.records_stats()):
        with pytest.raises(ValueError):
            call()
