"""zg_k_scatter's chunk plan and lane routine (zstd-rs_amd/csrc/zg_scatter.h), compiled with g++ and run lane by lane: every destination
against a Python slice copy, guard bytes on both sides intact, every read inside the chunk's own source range, every 16-byte store aligned and
inside the chunk's own destination range, every byte written exactly once; and zgpu_decode_frames_device's argument check, which needs no GPU.
tests/emu/zg_lane_scatter.cpp is the harness, built by tests/lanesuite.py."""
import ctypes as C
import random

import lanesuite

SENT = 0xA5
GUARD = 64


class Seg(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("dst", C.c_uint64), ("len", C.c_uint64)]


class Chunk(C.Structure):
    _fields_ = [("seg", C.c_uint32), ("len", C.c_uint32), ("at", C.c_uint64)]


def _declare(L):
    L.sc_chunk_bytes.argtypes = [C.c_uint32]
    L.sc_chunk_bytes.restype = C.c_uint32
    L.sc_default_chunk.restype = C.c_uint32
    L.sc_threads.restype = C.c_uint32
    L.sc_plan.argtypes = [C.POINTER(Seg), C.c_uint32, C.c_uint32, C.POINTER(Chunk), C.c_uint64]
    L.sc_plan.restype = C.c_uint64
    L.sc_run.argtypes = [C.c_void_p, C.POINTER(Seg), C.POINTER(Chunk), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]


lib = lanesuite.built_fixture("zg_lane_scatter.cpp", "scatter_lane", declare=_declare)


class Source:
    """random bytes the segments read from (a batch output stands in)"""

    def __init__(self, n, seed):
        self.bytes = random.Random(seed).randbytes(n)
        self.buf = C.create_string_buffer(self.bytes, n)


def _run(L, source, segs, chunk, threads=None):
    """segs: (src_off, dst_off, len) with dst_off counted inside an arena this builds, 256-byte aligned, sentinel-filled, with guard bytes around
    everything. Plans, checks the plan, runs the lanes, compares the arena with slice copies."""
    T = threads or L.sc_threads()
    C_ = L.sc_chunk_bytes(chunk)
    span = max([d + n for _, d, n in segs] + [0])
    arena = C.create_string_buffer(bytes([SENT]) * (span + 2 * GUARD + 512), span + 2 * GUARD + 512)
    base = (C.addressof(arena) + GUARD + 255) & ~255
    a0 = base - C.addressof(arena)
    cs = (Seg * max(len(segs), 1))()
    for i, (s, d, n) in enumerate(segs):
        cs[i].src_off, cs[i].dst, cs[i].len = s, base + d, n
    nch = L.sc_plan(cs, len(segs), chunk, None, 0)
    ch = (Chunk * max(nch, 1))()
    assert L.sc_plan(cs, len(segs), chunk, ch, nch) == nch
    # the plan: every byte of every segment in exactly one chunk, in order; inner boundaries on 16 bytes of the destination; bounded chunks
    at = {}
    for k in range(nch):
        c = ch[k]
        assert c.seg < len(segs) and 0 < c.len <= C_, (k, c.seg, c.len)
        assert c.at == at.get(c.seg, 0), (k, c.seg, c.at)
        if c.at:
            assert (cs[c.seg].dst + c.at) % 16 == 0, (k, c.seg, c.at)
        at[c.seg] = c.at + c.len
    for i, (_, _, n) in enumerate(segs):
        assert at.get(i, 0) == n, i
    counts = (C.c_uint64 * 4)()
    L.sc_run(C.addressof(source.buf), cs, ch, nch, T, counts)
    assert list(counts) == [0, 0, 0, 0], (list(counts), segs)
    want = bytearray([SENT]) * len(arena.raw)
    for s, d, n in segs:
        want[a0 + d:a0 + d + n] = source.bytes[s:s + n]
    assert arena.raw == bytes(want), segs


def _lengths(chunk):
    return [0, 1, 15, 16, 17, 31, 32, 33, 255, 4096 + 13, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]


def _offset_grid(L, chunk):
    C_ = L.sc_chunk_bytes(chunk)
    lens = _lengths(C_)
    source = Source(max(lens) + 64, 0x5CA7)
    for so in range(32):
        for do in range(32):
            segs, d = [], do
            for n in lens:
                segs.append((so, d, n))
                d += n + GUARD + ((do - (d + n + GUARD)) % 32)   # (guard bytes between, every destination at offset do mod 32)
            assert all(x[1] % 32 == do for x in segs)
            _run(L, source, segs, chunk)


def test_every_offset_pair_smallest_chunk(lib):
    _offset_grid(lib, 4096)


def test_every_offset_pair_default_chunk(lib):
    assert lib.sc_chunk_bytes(0) == lib.sc_default_chunk()
    _offset_grid(lib, 0)


def test_random_segment_lists(lib):
    rng = random.Random(0xD15C)
    source = Source(1 << 20, 0xBEEF)
    for case in range(300):
        chunk = rng.choice([4096, 4096 + 16, 8192, 0])
        C_ = lib.sc_chunk_bytes(chunk)
        segs, d = [], rng.randrange(0, 64)
        for _ in range(rng.randrange(1, 13)):
            n = rng.choice([0, rng.randrange(0, 64), rng.randrange(0, 5000), rng.randrange(0, 3 * C_ + 1)])
            n = min(n, 200000)
            segs.append((rng.randrange(0, len(source.bytes) - n + 1), d, n))
            d += n + rng.choice([0, 0, rng.randrange(1, 100)])   # (0: the next frame of the same entry, back to back)
        _run(lib, source, segs, chunk, threads=rng.choice([None, None, 64, 16]))


def test_chunk_size_is_clamped(lib):
    assert lib.sc_chunk_bytes(1) == 4096 and lib.sc_chunk_bytes(5000) == 4992 and lib.sc_chunk_bytes(1 << 20) == 1 << 20


def test_decode_frames_device_bad_args_need_no_gpu():
    import zgpu
    L = zgpu.load_library()
    n = 1
    srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)()
    res = (zgpu.DeviceEntryResultC * n)()
    opts = zgpu.DeviceOptsC(0, 0, 0)
    assert L.zgpu_decode_frames_device(None, srcs, lens, n, dsts, caps, C.byref(opts), res) == 93     # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_decode_frames_device(None, None, None, 0, None, None, None, None) == 93
    # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    fake = C.create_string_buffer(4096)
    for k in range(5):
        a = [srcs, lens, dsts, caps, res]
        a[k] = None
        assert L.zgpu_decode_frames_device(fake, a[0], a[1], n, a[2], a[3], None, a[4]) == 93, k
    out = (C.c_uint64 * 7)()
    assert L.zgpu_debug_frames_device_stats(None, out, 7) == 0
    assert C.sizeof(zgpu.DeviceEntryResultC) == 40 and C.sizeof(zgpu.DeviceOptsC) == 16
    assert "zgpu_decode_frames_device" in zgpu.EXPORTS and "zgpu_debug_frames_device_stats" in zgpu.EXPORTS
