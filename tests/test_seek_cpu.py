"""zg_k_seek's lane routine (zstd-rs_amd/csrc/zg_seek.h), compiled with g++ and run on the CPU. For every input and every range the routine
runs over a reader that counts every access outside [anchor_src, len) and every access to a byte of a block body (the bodies as
zgw::walk_entry's records give them), and every field of its record is compared with a model computed from zgi::index_entry<true>'s frame
records and frame_fields — existing code, not the routine under test. Demanded of every case:
  - reads outside [anchor_src, len) 0, reads of a block body 0;
  - the record equals the model's, field for field;
  - bound == plaintext_bound(bytes[src_lo:src_hi]);
  - [src_lo, src_hi) starts and ends on frame-record boundaries (src_hi == len where the chain broke);
  - a run anchored at a frame boundary in front of the selection gives the src_lo / src_hi / plain_lo / flags of the unanchored one, with
    nblocks no larger.
Ranges per input: begin at 0, at every frame's declared boundary - 1, + 0, + 1, at the declared total and at the total + 5; len 1, 2, to the
end, 2^63 (and 0, which must read nothing). Each range runs unanchored and anchored at every frame boundary at which an anchor is valid: in
front of begin with every frame in front of it skipped by the unanchored run (a boundary behind an unsized or a taken frame is no anchor:
anchor_plain would not be known, or would lie behind begin).
The corpus is tests/test_walk_cpu.py's and concatenations of 2-6 of its inputs with skippable frames between them. The same ranges run once
more in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which every entry lies in a heap block of exactly
its length. tests/emu/zg_lane_seek.cpp is the harness, built by tests/lanesuite.py."""
import ctypes as C
import random
import struct

import lanesuite
import zgpu
from test_walk_cpu import MAGIC, block, corpus, hand_built, skippable


class SeekC(C.Structure):
    _fields_ = [("src_lo", C.c_uint64), ("src_hi", C.c_uint64), ("plain_lo", C.c_uint64), ("bound", C.c_uint64), ("plain_seen", C.c_uint64),
                ("status", C.c_uint32), ("frames_skipped", C.c_uint32), ("frames_taken", C.c_uint32), ("nblocks", C.c_uint32),
                ("why", C.c_uint32), ("flags", C.c_uint32)]


def sized_frame(payload, checksum=False):
    """a single-segment frame with a 1-byte Frame_Content_Size and one raw block (payload up to 255 bytes)"""
    return MAGIC + bytes([0x20 | (0x04 if checksum else 0), len(payload)]) + block(payload, btype=0) + (b"\x00\x00\x00\x00" if checksum else b"")


def inputs():
    out = list(corpus())
    base = [z for _, z in out]
    hb = hand_built()
    rng = random.Random(0x5EEC)
    small = [z for z in base if 0 < len(z) <= 1 << 16]
    for k in range(60):
        parts = [rng.choice(small) for _ in range(rng.randint(2, 6))]
        out.append(("cat:%d" % k, b"".join(p + skippable(bytes([k & 255]) * rng.randint(0, 9)) for p in parts)))
    # sized frames, so that there are frames to skip: in front of an unsized frame, of a defect, of an empty frame
    a, b, e = sized_frame(b"a" * 100), sized_frame(b"b" * 255, checksum=True), sized_frame(b"")
    out.append(("sized:plain", a + b + a + skippable(b"xy") + b + a))
    out.append(("sized:empty_between", a + e + b + e + e + a))
    out.append(("sized:then_unsized", a + b + hb["raw_rle_blocks"] + a))
    out.append(("sized:broken_behind", a + b + a + hb["body_past_end"]))
    out.append(("sized:broken_in_skipped", a + b + a[:-40] ))
    out.append(("sized:garbage_behind", a + b + b"\x00\x01\x02\x03\x04\x05"))
    out.append(("sized:skip_past_end", a + b + skippable(b"abc", length=40) ))
    out.append(("sized:fcs8", hb["single_segment_fcs8"] + a + hb["fcs2_dict4"] + b))
    out.append(("sized:lie_small", MAGIC + bytes([0x20, 3]) + block(b"q" * 50, btype=0) + a + b))
    out.append(("sized:huge", MAGIC + bytes([0xE0]) + struct.pack("<Q", 2 ** 64 - 2) + block(b"abc", btype=0) + a + b))
    return out


def _declare(L):
    L.sk_check.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sk_check.restype = C.c_uint32
    L.sk_coverage.argtypes = [C.POINTER(C.c_uint64)]
    L.sk_one.argtypes = [C.c_void_p] + [C.c_uint64] * 5 + [C.c_void_p]


built = lanesuite.built_fixture("zg_lane_seek.cpp", "seek", "SEEK_MAIN", lanesuite.HOST_PARSE, _declare)


def test_seek_equals_the_model_on_every_range(built):
    L, _, _ = built
    where = C.c_uint64(0)
    cases = inputs()
    assert len(cases) > 370
    for name, z in cases:
        buf = lanesuite.exact_buffer(z)
        bad = L.sk_check(buf, len(z), C.byref(where))
        assert bad == 0, (name, "begin", where.value, "bits", bad)
    cov = (C.c_uint64 * 16)()
    L.sk_coverage(cov)
    assert cov[0] > 20000 and cov[6] > 2000, list(cov)
    assert cov[1] > 0, "an open-ended selection"
    assert cov[2] > 0, "a broken chain in front of the range"
    assert cov[3] > 0, "a broken chain inside the selection"
    assert cov[4] > 0, "an empty frame at a boundary"
    assert cov[5] > 0, "bit 2: nothing taken"
    assert cov[7] > 0 and cov[8] > 0


def test_seek_pinned_examples(built):
    L, _, _ = built
    a, b = sized_frame(b"a" * 100), sized_frame(b"b" * 255, checksum=True)
    z = a + b + skippable(b"xy") + a + b
    buf = lanesuite.exact_buffer(z)
    s = SeekC()

    def one(begin, n, asrc=0, aplain=0):
        L.sk_one(buf, len(z), begin, n, asrc, aplain, C.byref(s))
        return (s.src_lo, s.src_hi, s.plain_lo, s.bound, s.status, s.frames_skipped, s.frames_taken, s.flags)

    la, lb, ls = len(a), len(b), 10
    assert one(0, 1) == (0, la, 0, 100, 0, 0, 1, 0)
    assert one(99, 2) == (0, la + lb, 0, 355, 0, 0, 2, 0)
    assert one(100, 1) == (la, la + lb, 100, 255, 0, 1, 1, 0)
    assert one(355, 1) == (la + lb + ls, 2 * la + lb + ls, 355, 100, 0, 2, 1, 0)      # the skippable frame lies in front of the selection
    assert one(354, 2) == (la, 2 * la + lb + ls, 100, 355, 0, 1, 2, 0)                # ... and inside it
    assert one(355, 1, la + lb, 355) == one(355, 1)[:5] + (0, 1, 0)
    assert one(710, 1) == (len(z), len(z), 710, 0, 0, 4, 0, 4)
    assert one(0, 2 ** 64 - 1) == (0, len(z), 0, 710, 0, 0, 4, 0)
    assert one(5, 0) == (0,) * 8
    assert one(5, 1, len(z) + 1, 0)[4] == 93 and one(5, 1, 0, 6)[4] == 93


def test_seek_under_address_sanitizer_stand_alone(built):
    _, exe, d = built
    path = d / "entries.bin"
    with open(path, "wb") as f:
        for _, z in inputs():
            f.write(struct.pack("<Q", len(z)) + z)
    lanesuite.run_stand_alone(exe, [path], b"seek_asan ok", timeout=600)


def test_ranges_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = 1
    srcs, lens, dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    rg, sk, res = (zgpu.RangeC * n)(), (zgpu.SeekC * n)(), (zgpu.RangeResultC * n)()
    assert C.sizeof(zgpu.RangeC) == 32 and C.sizeof(zgpu.SeekC) == 64 and C.sizeof(zgpu.RangeResultC) == 40 + 64
    assert [f[0] for f in zgpu.SeekC._fields_] == [f[0] for f in SeekC._fields_]
    assert L.zgpu_frames_seek_device(None, srcs, lens, n, rg, sk) == 93          # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_decode_ranges_device_src(None, srcs, lens, n, rg, dsts, caps, None, res) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(4):
        a = [srcs, lens, rg, sk]
        a[k] = None
        assert L.zgpu_frames_seek_device(fake, *a[:2], n, *a[2:]) == 93, k
    for k in range(6):
        a = [srcs, lens, rg, dsts, caps, res]
        a[k] = None
        assert L.zgpu_decode_ranges_device_src(fake, a[0], a[1], n, a[2], a[3], a[4], None, a[5]) == 93, k
    out = (C.c_uint64 * 8)()
    assert L.zgpu_debug_ranges_stats(None, out, 8) == 0
    assert zgpu.E_CONTENT_SIZE_MISMATCH == 71
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        assert lib_.zgpu_status_name(71) == b"ContentSizeMismatch"
        for sym in ("zgpu_frames_seek_device", "zgpu_decode_ranges_device_src", "zgpu_debug_ranges_stats"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for m in ("frames_seek_device", "decode_ranges_device_src", "ranges_stats", "decode_tensor_ranges"):
        assert hasattr(zgpu.Context, m)
    assert callable(zgpu.anchor_before)
