"""zg_k_dictfill's plan and lane routine (zstd-rs_amd/csrc/zg_dictfill.h) and the host walk with a dictionary lookup (zg_host_parse.cpp),
compiled with g++: every destination against a slice copy with guard bytes on both sides, every read inside the chunk's own source range,
every 16-byte store aligned and inside the chunk's own destination range, every byte written exactly once; the chunk table cut by the
<= 64 KiB and 16-byte rules and ordered by source and source window; a dictionary frame of the walk gets dict_len, history and carry mask, its first
unit is not direct, and without a lookup the walk is what it was. tests/emu/zg_lane_dictfill.cpp is the harness, built by tests/lanesuite.py."""
import ctypes as C
import random

import lanesuite
from golden_io import read_pack

SENT = 0xA5
GUARD = 64
CHUNK = 64 << 10


class Seg(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("len", C.c_uint64)]


class Chunk(C.Structure):
    _fields_ = [("seg", C.c_uint32), ("len", C.c_uint32), ("at", C.c_uint64)]


def _declare(L):
    L.df_plan.argtypes = [C.POINTER(Seg), C.c_uint32, C.c_uint32, C.POINTER(Chunk), C.c_uint64]
    L.df_plan.restype = C.c_uint64
    L.df_run.argtypes = [C.POINTER(Seg), C.POINTER(Chunk), C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
    L.df_image.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.df_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]


lib = lanesuite.built_fixture("zg_lane_dictfill.cpp", "dictfill_lane", extra_sources=lanesuite.HOST_PARSE, declare=_declare)


def _run(L, source, segs, threads=256):
    """segs: (src_off, dst_off, len), dst_off inside an arena this builds: 256-byte aligned, sentinel-filled, guard bytes around everything.
    Plans, checks the plan, runs the lanes, compares the arena with slice copies. Returns the chunk table."""
    sbuf = C.create_string_buffer(source, len(source))
    sbase = C.addressof(sbuf)
    span = max([d + n for _, d, n in segs] + [0])
    arena = C.create_string_buffer(bytes([SENT]) * (span + 2 * GUARD + 512), span + 2 * GUARD + 512)
    base = (C.addressof(arena) + GUARD + 255) & ~255
    a0 = base - C.addressof(arena)
    cs = (Seg * max(len(segs), 1))()
    for i, (s, d, n) in enumerate(segs):
        cs[i].src, cs[i].dst, cs[i].len = sbase + s, base + d, n
    nch = L.df_plan(cs, len(segs), 0, None, 0)
    ch = (Chunk * max(nch, 1))()
    assert L.df_plan(cs, len(segs), 0, ch, nch) == nch
    # the cut: every byte of every segment in exactly one chunk, a segment's chunks in order; inner boundaries on 16 bytes of the
    # destination; no chunk longer than 64 KiB. The order: by source, then by the 64 KiB window of it a chunk copies, never backwards
    at, last_window = {}, (-1, -1)
    for k in range(nch):
        c = ch[k]
        assert c.seg < len(segs) and 0 < c.len <= CHUNK, (k, c.seg, c.len)
        assert c.at == at.get(c.seg, 0), (k, c.seg, c.at)
        if c.at:
            assert (cs[c.seg].dst + c.at) % 16 == 0, (k, c.seg, c.at)
        at[c.seg] = c.at + c.len
        w = (cs[c.seg].src, (c.at + CHUNK // 2) // CHUNK)
        assert w >= last_window, k
        last_window = w
    for i, (_, _, n) in enumerate(segs):
        assert at.get(i, 0) == n, i
    counts = (C.c_uint64 * 4)()
    L.df_run(cs, ch, nch, threads, counts)
    assert list(counts) == [0, 0, 0, 0], (list(counts), segs)
    want = bytearray([SENT]) * len(arena.raw)
    for s, d, n in segs:
        want[a0 + d:a0 + d + n] = source[s:s + n]
    assert arena.raw == bytes(want), segs
    return [(ch[k].seg, ch[k].at, ch[k].len) for k in range(nch)]


LENGTHS = [0, 1, 15, 16, 17, 65535, 65536, 65537]


def test_lengths_at_every_destination_and_source_misalignment(lib):
    source = random.Random(0xD1C7).randbytes(65537 + 16)
    for so in range(4):
        for do in range(16):
            segs, d = [], do
            for n in LENGTHS:
                segs.append((so, d, n))
                d += n + GUARD
                d += (do - d) % 16                      # (guard bytes between, every destination at misalignment do)
            assert all(x[1] % 16 == do for x in segs)
            _run(lib, source, segs)


def test_replicated_segments_run_window_by_window(lib):
    """one 150,000-byte source to 24 destinations of different alignment, as a dictionary goes to the frames of a submit: the chunks
    that start in the same 64 KiB of the source lie together in the table, whatever their segment"""
    source = random.Random(5).randbytes(150000)
    segs, d = [], 0
    for j in range(24):
        segs.append((0, d + (7 * j) % 16, len(source)))
        d += len(source) + GUARD + 32
        d -= d % 16
    table = _run(lib, source, segs, threads=64)
    firsts = [k for k, (_, at, _) in enumerate(table) if at == 0]
    assert firsts == list(range(24))                    # every segment's first chunk before any second one
    # ... and small segments of another source (the tables) mix in without breaking the cut
    small = [(100, d + 5000 * j + 3, 5120) for j in range(6)] + [(9000, d + 40000 + j, 1) for j in range(3)]
    _run(lib, source, segs[:3] + small)


def test_image_layout(lib):
    out = (C.c_uint64 * 6)()
    lib.df_image(0x10000, 112640 + 5, out)
    content, fse, logs, huf, maxbits, total = list(out)
    assert content == 0x10000 and fse == 0x10000 + 112656 and fse % 16 == 0
    assert logs == fse + 5120 and huf == logs + 16 and maxbits == huf + 4096 and total == maxbits + 16 - content


# ---- the host walk with a lookup --------------------------------------------------------------------------------------------------------------
def _walk(L, z, did=0, content_len=0, hist=(1, 4, 8)):
    out = (C.c_uint64 * (3 + 64))()
    h = (C.c_uint32 * 3)(*hist)
    L.df_walk(z, len(z), did, content_len, h, out)
    frames = [tuple(out[3 + 8 * f:3 + 8 * f + 8]) for f in range(min(out[1], 8))]
    return int(out[0]), int(out[2]), frames


def _dict_id(z):
    assert z[:4] == (0xFD2FB528).to_bytes(4, "little") and z[4] & 3 == 3
    at = 5 + (0 if (z[4] >> 5) & 1 else 1)
    return int.from_bytes(z[at:at + 4], "little")


def test_walk_with_and_without_a_lookup(lib):
    pack = read_pack("dict_tests.pack")
    names = sorted(n for n in pack if n != "dictionary")
    plain = read_pack("decodecorpus.pack")["z000033.zst"]
    seen_carried = direct_without = 0
    for n in names[:60]:
        z = pack[n]
        did = _dict_id(z)
        # no lookup: the walk ends at the dictionary frame, as it always did — also behind a frame without one
        assert _walk(lib, z)[0] == 7 and _walk(lib, z)[2] == []
        st, bound0, frames = _walk(lib, plain + z)
        assert st == 7 and len(frames) == 1 and frames[0][0] == 0 and frames[0][7] == 0
        # a lookup that does not know the id: the same
        st, bound_other, frames_other = _walk(lib, plain + z, did + 1, 1000)
        assert (st, bound_other, frames_other) == (7, bound0, frames)
        # a lookup that does: the frame is in the submit, with the dictionary's content length, history and tables
        st, bound, frames = _walk(lib, plain + z + plain, did, 112640, (11, 22, 33))
        assert st == 0 and len(frames) == 3
        assert frames[0][:4] == (0, 1, 4, 8) and frames[2][:4] == (0, 1, 4, 8) and frames[0][7] == frames[2][7] == 0
        dlen, h0, h1, h2, carried, first_noseq, nunits, fid = frames[1]
        assert (dlen, h0, h1, h2, fid) == (112640, 11, 22, 33, did)
        assert nunits >= 1 and not first_noseq & 2, n        # its first unit is not a direct unit (ZG_UNIT_DIRECT) ...
        direct_without += (_walk(lib, z, did, 0)[2][0][5] & 2) != 0   # ... which the same blocks get when nothing lies in front of them
        seen_carried |= carried
        assert bound == _walk(lib, plain + plain)[1] + 112640 + (_walk(lib, z, did, 0)[1])
    assert direct_without > 30
    assert seen_carried == 0xF                                # Treeless literals and Repeat-mode LL / OF / ML tables resolve to the carry slots
    # without a lookup nothing changed for frames that name no dictionary
    assert _walk(lib, plain + plain, 5, 99)[:2] == _walk(lib, plain + plain)[:2]
    assert _walk(lib, plain + plain, 5, 99)[2] == _walk(lib, plain + plain)[2]
