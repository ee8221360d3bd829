"""zg_k_fill's chunk plan and lane routine (zstd-rs_amd/csrc/zg_scatter.h: plan_chunks with kFillChunk, fill_chunk), compiled with g++ and run
lane by lane: every region against a Python model — the pad byte in the region, the sentinel everywhere else —, every store inside the
chunk's own range, every 16-byte store aligned, every byte written exactly once. Destination alignments 0 .. 15; lengths 0 .. 48, then 255,
256, 257, 4095, 4096, 4097, the plan's chunk size and the chunk size +- 1; T = the kernel's thread count; pad bytes 0x00, 0xA5, 0xFF. The
stand-alone AddressSanitizer program runs the same cases with every region ending with its heap block. tests/emu/zg_lane_fill.cpp is the
harness, built by tests/lanesuite.py."""
import ctypes as C
import os
import struct

import lanesuite
from test_scatter_cpu import Chunk, Seg

SENT = 0x5A                     # (no pad byte of the cases)
GUARD = 64
PADS = (0x00, 0xA5, 0xFF)


def _declare(L):
    L.fl_chunk.restype = L.fl_threads.restype = L.fl_max_groups.restype = C.c_uint32
    L.fl_plan.argtypes = [C.POINTER(Seg), C.c_uint32, C.POINTER(Chunk), C.c_uint64]
    L.fl_plan.restype = C.c_uint64
    L.fl_run.argtypes = [C.POINTER(Seg), C.POINTER(Chunk), C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.fl_plan_rows.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint32)]


built = lanesuite.built_fixture("zg_lane_fill.cpp", "fill_lane", "FILL_MAIN", declare=_declare)


def lengths(chunk):
    return list(range(49)) + [255, 256, 257, 4095, 4096, 4097, chunk - 1, chunk, chunk + 1]


def _run(L, regions, byte):
    """regions: (offset, len) inside an arena this builds — 256-byte aligned, full of the sentinel, guard bytes around everything. Plans,
    checks the plan, runs the lanes with the kernel's thread count, compares the arena with the model."""
    span = max([d + n for d, n in regions] + [0])
    size = span + 2 * GUARD + 512
    arena = C.create_string_buffer(bytes([SENT]) * size, size)
    base = (C.addressof(arena) + GUARD + 255) & ~255
    a0 = base - C.addressof(arena)
    cs = (Seg * max(len(regions), 1))()
    for i, (d, n) in enumerate(regions):
        cs[i].src_off, cs[i].dst, cs[i].len = 0, base + d, n
    nch = L.fl_plan(cs, len(regions), None, 0)
    ch = (Chunk * max(nch, 1))()
    assert L.fl_plan(cs, len(regions), ch, nch) == nch
    # the plan: every byte of every region in exactly one chunk, in order; inner boundaries on 16 bytes of the destination; bounded chunks
    at = {}
    for k in range(nch):
        c = ch[k]
        assert c.seg < len(regions) and 0 < c.len <= L.fl_chunk(), (k, c.seg, c.len)
        assert c.at == at.get(c.seg, 0) and (not c.at or (cs[c.seg].dst + c.at) % 16 == 0), (k, c.seg, c.at)
        at[c.seg] = c.at + c.len
    assert all(at.get(i, 0) == n for i, (_, n) in enumerate(regions))
    counts = (C.c_uint64 * 3)()
    L.fl_run(cs, ch, nch, byte, L.fl_threads(), counts)
    assert list(counts) == [0, 0, 0], (list(counts), regions)      # stores outside, unaligned 16-byte stores, chunks not written exactly once
    want = bytearray([SENT]) * size
    for d, n in regions:
        want[a0 + d:a0 + d + n] = bytes([byte]) * n
    assert arena.raw == bytes(want), regions
    return nch


def test_constants_are_the_headers(built):
    L = built[0]
    assert (L.fl_threads(), L.fl_max_groups(), L.fl_chunk()) == (64, 2048, 4096) and L.fl_chunk() % 16 == 0


def test_every_alignment_and_length(built):
    L = built[0]
    for byte in PADS:
        for align in range(16):
            regions, d = [], align
            for n in lengths(L.fl_chunk()):
                regions.append((d, n))
                d += n + GUARD
                d += (align - d) % 16                                # (guard bytes between, every region at `align` mod 16)
            assert all(x[0] % 16 == align for x in regions)
            _run(L, regions, byte)


def test_regions_back_to_back_and_long_ones(built):
    """rows of a padded batch: pad regions of every length behind records of every length, nothing between a row's end and the next record;
    and regions of several chunks"""
    L = built[0]
    regions, at = [], 3
    for j in range(200):
        rec, pad = (7 * j) % 53, (11 * j) % 67
        regions.append((at + rec, pad))
        at += rec + pad
    assert _run(L, regions, 0xEE) == sum(1 for _, n in regions if n)
    C_ = L.fl_chunk()
    assert _run(L, [(5, 3 * C_ + 9), (5 + 3 * C_ + 9, 0), (5 + 3 * C_ + 9, C_ + 1)], 0x00) == 4 + 2


def test_stand_alone_asan_program_runs_the_same_cases(built):
    L, exe, d = built
    path = os.path.join(str(d), "cases.bin")
    cases = [(a, n, b) for b in PADS for a in range(16) for n in lengths(L.fl_chunk())]
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("<3I", *c))
    out = lanesuite.run_stand_alone(exe, [path], b"fill_asan ok: %d cases" % len(cases), timeout=120)
    assert out
