"""The C ABI of the record batch (zgpu_gather_records_batch_indexed_device_src and the slots it appends to zgpu_debug_ranges_stats) and its
marshalling in zgpu.py, without a GPU: both libraries export the symbol and the header declares it, the two structs have the header's sizes,
fields and order, the constants match, the appended statistics slots are the kBatchStat enumerators of zg_capi_int.h and the header says
where they lie, the argument rules that need no device answer ZGPU_E_BAD_ARG, and Context.gather_records_batch hands the C function what it
is given (checked on a fake context over a recording library)."""
import ctypes as C
import os
import re

import zgpu
from test_seek_index_records_binding_cpu import _RecordsCtx, _snake
from test_seek_index_sums_binding_cpu import _Recorder, _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "zgpu_gather_records_batch_indexed_device_src"


class _BatchCtx(_RecordsCtx):
    gather_records_batch = zgpu.Context.gather_records_batch


def _struct_fields(header, name):
    body = header.split("} %s;" % name)[0].rsplit("typedef struct {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [f.strip() for decl in re.findall(r"(?:void\*|uint(?:32|64)_t\*?)\s+([\w, ]+);", body) for f in decl.split(",")]


def test_symbol_structs_and_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    for dev in (False, True):
        assert SYM in zgpu.EXPORTS and hasattr(zgpu.load_library(dev=dev), SYM) and re.search(r"^int %s\(" % SYM, header, re.M)
    B, I = zgpu.RecordBatchC, zgpu.RecordBatchInfoC
    assert C.sizeof(B) == 64 and C.sizeof(I) == 32
    assert [f for f, _ in B._fields_] == _struct_fields(header, "zgpu_record_batch") == [
        "device_dst", "cap", "device_lengths", "device_offsets", "host_record_bytes", "width", "layout", "flags", "pad_byte", "reserved"]
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    line = [ln for ln in header.splitlines() if "} zgpu_record_batch_info;" in ln][0]
    assert re.findall(r"uint(?:32|64)_t ([\w, ]+);", line) == ["total, bytes_filled", "rows_ok, rows_failed, rows_truncated, pad"]
    assert [f for f, _ in I._fields_] == ["total", "bytes_filled", "rows_ok", "rows_failed", "rows_truncated", "pad"]
    assert [getattr(I, f).offset for f, _ in I._fields_] == [0, 8, 16, 20, 24, 28] and list(zgpu.RecordBatchInfo.FIELDS) == [f for f, _ in I._fields_][:5]
    for name, v in (("PADDED", zgpu.BATCH_PADDED), ("PACKED", zgpu.BATCH_PACKED), ("TRUNCATE", zgpu.BATCH_TRUNCATE)):
        assert re.search(r"#define ZGPU_BATCH_%s\s+%du" % (name, v), header), name
    assert (zgpu.BATCH_PADDED, zgpu.BATCH_PACKED, zgpu.BATCH_TRUNCATE) == (0, 1, 1)


def test_stats_keys_are_the_enumerators():
    text = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_capi_int.h")).read()
    assert ["batch_" + k for k in _snake(text, "kBatchStat")] == list(zgpu.Context.BATCH_STATS)
    assert _snake(text, "kBatchStat") == ["fill_launches", "fill_us", "bytes_filled", "bytes_uploaded"]
    assert len(zgpu._STATS["Context.ranges_stats"][2]) + len(zgpu.Context.GATHER_STATS) + len(zgpu.Context.RECORD_STATS) == 22
    header = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    section = header.split("record batches: gather records into one padded or packed tensor", 1)[1].split("the same over several GPUs", 1)[0]
    for word in ("[22] fill launches, [23] their microseconds (HIP events), [24]\n * bytes filled, [25] bytes uploaded into the two arrays",
                 "A caller that asks for 22 gets what it always got", "NOTHING IN DEVICE MEMORY IS WRITTEN", "cap == 0 with device_dst == NULL",
                 "IS EITHER A RECORD'S BYTE OR THE PAD BYTE", "zg_k_fill", "A wrong pointer is a status, never a GPU fault", "adds no status code",
                 "Out of scope: the fill fused into the scatter's chunks, record numbers that live in device memory, host sources, several GPUs"):
        assert word in section, word
    sc = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_scatter.h")).read()
    for word in ("fill_chunk", "kFillThreads = 64", "kFillMaxGroups = 2048", "kFillChunk = 4096", "ONE WAVE per chunk", "UNMEASURED", "gfx950 ISA of zg_k_fill",
                 "global_store_dwordx4", "global_store_byte"):
        assert word in sc, word


def test_argument_rules_need_no_gpu():
    for dev in (False, True):
        L = zgpu.load_library(dev=dev)
        srcs, lens = (C.c_void_p * 1)(), (C.c_size_t * 1)()
        fake = C.create_string_buffer(4096)    # stands for a context where the call refuses before it looks at it
        mine = C.create_string_buffer(4096)    # a handle of that context that holds no entry: the first word of a zgpu_seek_index is its context
        C.memmove(mine, C.byref(C.c_void_p(C.addressof(fake))), 8)
        other = C.create_string_buffer(4096)   # a handle of another context
        C.memmove(other, C.byref(C.c_void_p(C.addressof(fake) + 64)), 8)
        rr, res, info = (zgpu.RecordRangeC * 1)(), (zgpu.RangeResultC * 1)(), zgpu.RecordBatchInfoC(7, 7, 7, 7, 7, 7)
        good = dict(device_dst=None, cap=0, device_lengths=None, device_offsets=None, width=8, layout=0, flags=0, pad_byte=0, reserved=0)

        def call(c=fake, x=mine, n=0, m=1, recs=rr, results=res, inf=info, batch=True, **change):
            b = zgpu.RecordBatchC(**dict(good, **change))
            return L.zgpu_gather_records_batch_indexed_device_src(c, x, srcs, lens, n, recs, m, C.byref(b) if batch else None, None, results,
                                                                  C.byref(inf) if inf is not None else None)
        assert call(c=None) == zgpu.E_BAD_ARG and call(x=None) == zgpu.E_BAD_ARG and call(x=other) == zgpu.E_BAD_ARG
        assert call(n=1) == zgpu.E_BAD_ARG                                           # n is not the handle's entry count
        assert call(batch=False) == zgpu.E_BAD_ARG and call(results=None) == zgpu.E_BAD_ARG and call(inf=None) == zgpu.E_BAD_ARG
        assert call(recs=None) == zgpu.E_BAD_ARG
        assert call(results=None, m=0) == zgpu.E_BAD_ARG                             # results may not be null, whatever m is
        assert call(layout=2) == zgpu.E_BAD_ARG and call(flags=2) == zgpu.E_BAD_ARG and call(flags=3) == zgpu.E_BAD_ARG
        assert call(reserved=1) == zgpu.E_BAD_ARG and call(pad_byte=256) == zgpu.E_BAD_ARG
        assert call(width=0) == zgpu.E_BAD_ARG                                       # padded without a width
        assert call(layout=1, width=8) == zgpu.E_BAD_ARG                             # packed with a width and no TRUNCATE
        for k in range(1, 8):
            assert call(device_lengths=4096 + k) == zgpu.E_BAD_ARG and call(device_offsets=4096 + k) == zgpu.E_BAD_ARG, k
        assert [getattr(info, f) for f, _ in info._fields_] == [7] * 6               # nothing was written
        out = (C.c_uint64 * 26)(*([7] * 26))
        assert L.zgpu_debug_ranges_stats(None, out, 26) == 0 and list(out) == [7] * 26


def test_marshalling_on_a_fake_context():
    L = _Recorder()
    x = _index(L, [3, 0])
    x.ctx = _BatchCtx(L)
    res, seeks, info, rb = x.ctx.gather_records_batch(x, [4096, 0], [10, 0], [(0, 1, 1), (1, 0, 2, zgpu.RECORDS_STRIP)], 8192, 640, width=320, pad=0xEE,
                                                      truncate=True, lengths_ptr=1 << 20, offsets_ptr=2 << 20, verify_table=True)
    name, a = L.calls[0]
    assert name == "zgpu_" + "gather_records_batch_indexed_device_src" and a[:2] == (1234, 77) and list(a[2]) == [4096, None] and list(a[3]) == [10, 0]
    assert a[4] == 2 and a[6] == 2 and [(r.entry, r.first, r.count, r.flags) for r in a[5][:2]] == [(0, 1, 1, 0), (1, 0, 2, 1)]
    b = a[7]._obj
    assert (b.device_dst, b.cap, b.device_lengths, b.device_offsets, b.width, b.layout, b.flags, b.pad_byte, b.reserved) == (
        8192, 640, 1 << 20, 2 << 20, 320, zgpu.BATCH_PADDED, zgpu.BATCH_TRUNCATE, 0xEE, 0)
    assert a[8]._obj.flags == 4 and len(a) == 11 and isinstance(a[10]._obj, zgpu.RecordBatchInfoC)
    assert len(res) == len(seeks) == len(rb) == 2 and isinstance(info, zgpu.RecordBatchInfo) and info.total == 0
    # the size query of the packed layout: no destination, no arrays
    L.calls.clear()
    x.ctx.gather_records_batch(x, [4096, 0], [10, 0], [], 0, 0, layout="packed")
    b = L.calls[0][1][7]._obj
    assert (b.device_dst, b.cap, b.device_lengths, b.device_offsets, b.width, b.layout, b.flags) == (None, 0, None, None, 0, zgpu.BATCH_PACKED, 0)
    assert L.calls[0][1][6] == 0
    for meth in ("gather_records_batch", "gather_records_batch_tensors", "gather_records_stats"):
        assert callable(getattr(zgpu.Context, meth)), meth
