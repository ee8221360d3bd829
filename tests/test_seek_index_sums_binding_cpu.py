"""The C ABI of the seek index's sums (zgpu_seek_index_hash_device, _set_sums, _read_sums, _sums_of, _export_seek_table_ex, and
zgpu_seek_index_stats' appended slots) and their marshalling in zgpu.py, without a GPU: both libraries export the symbols and the header
declares them, the record's size and fields are the header's, the argument rules that need no device answer ZGPU_E_BAD_ARG, and the methods of
zgpu.SeekIndex hand the C functions what they are given (checked on a fake handle over a recording library)."""
import ctypes as C
import inspect
import os
import re

import pytest

import zgpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zgpu_seek_index_hash_device", "zgpu_seek_index_set_sums", "zgpu_seek_index_read_sums", "zgpu_seek_index_sums_of",
       "zgpu_seek_index_export_seek_table_ex")


def test_symbols_struct_and_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "zgpu.h")).read()
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in NEW + ("zgpu_seek_index_stats",):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym) and re.search(r"^int %s\(" % sym, header, re.M), sym
    assert C.sizeof(zgpu.SeekIndexSumsC) == 32 and C.sizeof(zgpu.SeekIndexInfoC) == 40
    body = header.split("} zgpu_seek_index_sums;")[0].rsplit("typedef struct {", 1)[1]
    fields = [f for decl in re.findall(r"uint(?:32|64)_t ([\w, ]+);", body) for f in decl.split(", ")]
    assert fields == [f for f, _ in zgpu.SeekIndexSumsC._fields_] == list(zgpu.SeekIndexSums.FIELDS)
    assert "#define ZGPU_EXPORT_CHECKSUMS %du" % zgpu.EXPORT_CHECKSUMS in header and zgpu.EXPORT_CHECKSUMS == 1
    assert (zgpu.SUMS_NONE, zgpu.SUMS_HASHED, zgpu.SUMS_SET) == (0, 1, 2)
    # the appended statistics: the enumerators of zg_capi_int.h behind the nine the getter always had
    text = open(os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_capi_int.h")).read()
    names = re.findall(r"\bkSumStat(\w+)", [m for m in re.findall(r"enum\s*\{([^}]*)\}", text) if "kSumStat" in m][0])
    snake = [re.sub(r"(?<!^)([A-Z])", r"_\1", k).lower() for k in names[:-1]]
    keys = zgpu._STATS["SeekIndex.sums_stats"][2]
    assert keys[:9] == zgpu._STATS["SeekIndex.stats"][2] and list(keys[9:]) == snake and names[-1] == "Count"
    assert snake == ["hash_submits", "hash_us", "frames_hashed", "sums_bytes", "hash_runs"]
    # the Python surface
    for meth in ("hash", "hash_tensors", "sums", "set_sums", "export_seek_table"):
        assert callable(getattr(zgpu.SeekIndex, meth)), meth
    assert isinstance(zgpu.SeekIndex.sums_infos, property)
    sig = inspect.signature(zgpu.SeekIndex.hash).parameters
    assert sig["which"].default is None and sig["run_bytes"].default == 0
    assert inspect.signature(zgpu.SeekIndex.export_seek_table).parameters["checksums"].default is False
    assert inspect.signature(zgpu.SeekIndex.stats).parameters["sums"].default is False
    # the header: the section, what the pass sees that measuring does not, what stays out of scope
    section = header.split("seek index checksums: hash a shard once", 1)[1].split("the same over several GPUs", 1)[0]
    for word in ("SEES WHAT MEASURING DOES NOT SEE", "Huffman", "offsets", "content checksums", "ALL OR NOTHING PER ENTRY", "zg_k_idxsums",
                 "VOUCHED FOR BY THE HANDLE", "Out of scope: sums for single rows of an entry, updating in place, host sources, several GPUs"):
        assert word in section, word
    assert "checksums in the exported table" not in header


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
        # the pass: no context, no handle, a handle of another context, n that is not the entry count, null arrays
        assert L.zgpu_seek_index_hash_device(None, mine, srcs, lens, 0, None, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_hash_device(fake, None, srcs, lens, 0, None, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_hash_device(fake, other, srcs, lens, 0, None, 0) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_hash_device(fake, mine, srcs, lens, n, None, 0) == zgpu.E_BAD_ARG
        # sums in and out: a null handle, an entry out of range, null pointers
        a, got = (C.c_uint32 * 4)(1, 2, 3, 4), C.c_uint32(9)
        assert L.zgpu_seek_index_set_sums(None, 0, a, 4) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_set_sums(mine, 0, a, 4) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_read_sums(None, 0, a, 4, C.byref(got)) == zgpu.E_BAD_ARG and got.value == 0
        assert L.zgpu_seek_index_read_sums(mine, 0, a, 4, C.byref(got)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_read_sums(mine, 0, a, 4, None) == zgpu.E_BAD_ARG
        assert list(a) == [1, 2, 3, 4]
        rec = zgpu.SeekIndexSumsC()
        assert L.zgpu_seek_index_sums_of(None, 0, C.byref(rec)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_sums_of(mine, 0, C.byref(rec)) == zgpu.E_BAD_ARG
        assert L.zgpu_seek_index_sums_of(mine, 0, None) == zgpu.E_BAD_ARG
        # export: a null handle, with and without the flag; the getter on a null handle writes nothing
        buf, wrote = C.create_string_buffer(64), C.c_size_t(9)
        for flags in (0, zgpu.EXPORT_CHECKSUMS, 2):
            assert L.zgpu_seek_index_export_seek_table_ex(None, 0, flags, buf, 64, C.byref(wrote)) == zgpu.E_BAD_ARG and wrote.value == 0
            assert L.zgpu_seek_index_export_seek_table_ex(mine, 0, flags, buf, 64, C.byref(wrote)) == zgpu.E_BAD_ARG
        assert buf.raw == bytes(64)
        out = (C.c_uint64 * 14)(*([7] * 14))
        assert L.zgpu_seek_index_stats(None, out, 14) == 0 and list(out) == [7] * 14


class _Recorder:
    """stands for the library under a SeekIndex: records every call, answers what `answers` says (default 0)"""

    def __init__(self, answers=None):
        self.calls, self.answers = [], answers or {}

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            ans = self.answers.get(name, 0)
            return ans(*args) if callable(ans) else ans
        return call


class _Ctx:
    h = 1234

    def __init__(self, L):
        self.L, self._indexes = L, []

    _check = zgpu.Context._check


def _index(L, nrows):
    x = zgpu.SeekIndex.__new__(zgpu.SeekIndex)
    x.ctx, x.L, x.h = _Ctx(L), L, 77
    x.infos = []
    for r in nrows:
        c = zgpu.SeekIndexInfoC()
        c.nrows = r
        x.infos.append(zgpu.SeekIndexInfo(c))
    return x


def test_marshalling_on_a_fake_handle():
    L = _Recorder()
    x = _index(L, [3, 0])
    # hash: the handle, one pointer and one length per entry, `which` as bytes, run_bytes
    x.hash([4096, 0], [10, 0], which=[0, 5], run_bytes=1 << 20)
    name, a = L.calls[0]
    assert name == "zgpu_seek_index_hash_device" and a[0] == 1234 and a[1] == 77 and list(a[2]) == [4096, None] and list(a[3]) == [10, 0]
    assert a[4:] == (2, b"\x00\x01", 1 << 20)
    assert [c[0] for c in L.calls[1:]] == ["zgpu_seek_index_sums_of"] * 2   # (hash returns sums_infos)
    L.calls.clear()
    x.hash([4096, 0], [10, 0])
    assert L.calls[0][1][4:] == (2, None, 0)
    with pytest.raises(ValueError):
        x.hash([4096, 0], [10])
    with pytest.raises(ValueError):
        x.hash([4096, 0], [10, 0], which=[1])
    # set_sums: nrows uint32 words
    L.calls.clear()
    x.set_sums(0, [1, 0xFFFFFFFF, 3])
    name, a = L.calls[0]
    assert name == "zgpu_seek_index_set_sums" and a[0] == 77 and a[1] == 0 and list(a[2]) == [1, 0xFFFFFFFF, 3] and a[3] == 3
    # sums: a buffer of the entry's rows, cut to what the call says it wrote

    def read(h, entry, dst, cap, n):
        for k in range(cap):
            dst[k] = 100 + k
        n._obj.value = cap
        return 0
    x = _index(_Recorder({"zgpu_seek_index_read_sums": read}), [3, 0])
    assert x.sums(0) == [100, 101, 102] and x.sums(1) == []
    assert [c[1][3] for c in x.L.calls] == [3, 0]
    # export: the flag travels; a size query, then the call
    L = _Recorder({"zgpu_seek_index_export_seek_table_ex": lambda h, e, fl, dst, cap, w: zgpu.E_TARGET_TOO_SMALL if dst is None else 0})
    x = _index(L, [3])
    x.export_seek_table(0, checksums=True)
    x.export_seek_table(0)
    assert [(c[0], c[1][2]) for c in L.calls] == [("zgpu_seek_index_export_seek_table_ex", 1)] * 2 + [("zgpu_seek_index_export_seek_table_ex", 0)] * 2
    # an error is raised with the call's name
    x = _index(_Recorder({"zgpu_seek_index_set_sums": zgpu.E_BAD_ARG}), [3])
    with pytest.raises(zgpu.ZgpuError):
        x.set_sums(0, [1, 2])
    # a closed index refuses
    x.h = None
    for call in (lambda: x.hash([], []), lambda: x.sums(0), lambda: x.set_sums(0, []), lambda: x.sums_infos, lambda: x.export_seek_table(0)):
        with pytest.raises(ValueError):
            call()
