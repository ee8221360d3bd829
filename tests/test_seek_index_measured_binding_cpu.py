"""The measured seek index's C ABI (zgpu_seek_index_measure_device, zgpu_seek_index_export_seek_table) and its marshalling in zgpu.py,
without a GPU: both libraries export the two symbols and the header declares them, the kind enum of zgpu_seek_index_create_device is the
line it was, the new constants of the header are zgpu.py's, and the argument rules that need no device answer ZGPU_E_BAD_ARG."""
import ctypes as C
import inspect
import os
import re

import zgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zgpu_seek_index_measure_device", "zgpu_seek_index_export_seek_table")


def test_symbols_and_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in NEW:
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym) and re.search(r"^int %s\(" % sym, header, re.M), sym
    assert "enum { ZGPU_INDEX_SEEK_TABLE = 0, ZGPU_INDEX_DECLARED = 1, ZGPU_INDEX_AUTO = 2 };" in header
    assert zgpu._INDEX_KINDS == {"seek_table": 0, "declared": 1, "auto": 2}
    assert "enum { ZGPU_INDEX_MEASURED = %d };" % zgpu.INDEX_MEASURED in header and zgpu.INDEX_MEASURED == 3
    assert "#define ZGPU_INDEX_UNMEASURED %du" % zgpu.INDEX_UNMEASURED in header and zgpu.INDEX_UNMEASURED == 33
    assert "#define ZGPU_INDEX_DICT %du" % zgpu.INDEX_DICT in header and zgpu.INDEX_DICT == 34
    assert "enum { ZGPU_MEASURE_ALL = %d, ZGPU_MEASURE_UNSIZED = %d };" % (zgpu.MEASURE_ALL, zgpu.MEASURE_UNSIZED) in header
    assert (zgpu.MEASURE_ALL, zgpu.MEASURE_UNSIZED) == (0, 1)
    for meth in ("seek_index_measured", "seek_index_measured_tensors"):
        assert inspect.signature(getattr(zgpu.Context, meth)).parameters["only_unsized"].default is False, meth
    assert callable(zgpu.SeekIndex.export_seek_table)
    assert zgpu._STATS["SeekIndex.stats"][2][6:] == ("measure_submits", "measure_us", "frames_measured")
    # the header says what measuring does not see, and what stays out of scope
    section = header.split("seek index by measuring", 1)[1].split("the same over several GPUs", 1)[0]
    for word in ("WHAT MEASURING DOES NOT SEE", "Huffman", "checksums", "ZGPU_INDEX_AUTO falling through", "dictionary id"):
        assert word in section, word
    assert "entries with unsized frames (use a seek table)" not in header


def test_argument_rules_need_no_gpu():
    for dev in (False, True):
        L = zgpu.load_library(dev=dev)
        n = 1
        srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
        fake = C.create_string_buffer(4096)   # stands for a context where the call refuses before it looks at it
        h = C.c_void_p(7)
        assert L.zgpu_seek_index_measure_device(None, srcs, lens, n, zgpu.MEASURE_ALL, C.byref(h)) == zgpu.E_BAD_ARG and h.value is None
        assert L.zgpu_seek_index_measure_device(fake, srcs, lens, n, zgpu.MEASURE_ALL, None) == zgpu.E_BAD_ARG
        h = C.c_void_p(7)
        assert L.zgpu_seek_index_measure_device(fake, srcs, lens, n, 2, C.byref(h)) == zgpu.E_BAD_ARG and h.value is None
        assert L.zgpu_seek_index_measure_device(fake, None, lens, n, zgpu.MEASURE_UNSIZED, C.byref(h)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_measure_device(fake, srcs, None, n, zgpu.MEASURE_ALL, C.byref(h)) == zgpu.E_BAD_ARG
        # zgpu_seek_index_create_device is what it was: kind 3 is no kind
        assert L.zgpu_seek_index_create_device(fake, srcs, lens, n, zgpu.INDEX_MEASURED, C.byref(h)) == zgpu.E_BAD_ARG
        # export on a null handle
        buf, wrote = C.create_string_buffer(64), C.c_size_t(9)
        assert L.zgpu_seek_index_export_seek_table(None, 0, buf, 64, C.byref(wrote)) == zgpu.E_BAD_ARG and wrote.value == 0
        assert L.zgpu_seek_index_export_seek_table(None, 0, None, 0, C.byref(wrote)) == zgpu.E_BAD_ARG
        assert buf.raw == bytes(64)
