"""The record index's kernels (zstd-rs_amd/csrc/zg_records.h: zg_k_recs_count, zg_k_recs_scan, zg_k_recs_emit, zg_k_recs_find) and their host
forms (zgr::records_host, zgr::cut_chunks, zgr::find_host), compiled with g++ over the SIMT emulator (tests/emu/zg_simt.h) and run on the CPU:
the fibers, ballots and shuffles of the source as it is compiled for gfx950. tests/emu/zg_emu_records.cpp is the harness, built by
tests/lanesuite.py. Every case runs over accessors that count every access outside what a wave may touch. Demanded of every case:
  - counts, prefixes, the total, the frames' totals and every staged offset equal the model's (tests/records.py: numpy.flatnonzero(plain == d)
    + 1 in the entry's coordinates), and the 64 lanes of a count wave hold the same count;
  - no byte read outside the wave's own chunk [out_off, out_off + len), no 16-byte load at an address that is no multiple of 16, no scan
    access outside its arrays, no staged offset outside the chunk's own slots, as many stores as there are delimiters, guard bands intact.
Cases, each a few KiB: frame lengths 0, 1, 15, 16, 17, kChunk - 1, kChunk, kChunk + 1, 2 * kChunk + 5 at each of the 16 alignments of out_base,
between bytes full of delimiters that must not be counted; one delimiter at the first and the last byte of the frame, of a chunk, of a
16-byte group, of a wave step, and all of those at once; no delimiter; every byte a delimiter (16 per lane); d in {0x00, 0x0A, 0x7F, 0x80,
0xFF} over random bytes of the alphabet {d - 1, d, d + 1}; a dictionary-style gap full of delimiters between two frames; two frames of
several chunks whose counts cross the prefix. Find lanes: first in {0, R - 1, R, R + 1, 2^64 - 1} x count in {0, 1, R, 2^64 - 1} x strip
on a closed and an open last record, a record that is the delimiter alone, lanes with a status (which read nothing); a lane reads at most
two offsets, both its own entry's. The same cases run once more in a stand-alone AddressSanitizer program (its own main, no Python in the
process) in which every array lies in a heap block of exactly its length."""
import ctypes as C
import random
import struct

import pytest

import lanesuite
import records
from records import CHUNK, STRIP, U64

LENGTHS = (0, 1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
DELIMS = (0x00, 0x0A, 0x7F, 0x80, 0xFF)
BAD_ARG = 93


def _declare(L):
    vp = C.c_void_p
    L.zgemu_records.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp]
    L.zgemu_records.restype = C.c_uint32
    L.zgemu_records_find.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp]
    L.zgemu_records_find.restype = None
    L.zgemu_records_scan.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp]   # (tests/test_recshapes_cpu.py: the scan alone)
    L.zgemu_records_scan.restype = None
    L.zgemu_records_host.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, vp, C.c_uint64]
    L.zgemu_records_host.restype = C.c_uint64
    L.zgemu_records_cut.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint64]
    L.zgemu_records_cut.restype = C.c_uint64


built = lanesuite.built_fixture("zg_emu_records.cpp", "records", "RECORDS_MAIN", declare=_declare)


def _alphabet(rng, d, n):
    return bytes(rng.choice(((d - 1) & 255, d, (d + 1) & 255)) for _ in range(n))


def _around(plains, d, first_off, gaps=None, base0=0):
    """(buf, frames): the plaintexts byte-tight from first_off (gaps[i] bytes in front of frame i), everything else full of delimiters"""
    buf, frames, base = bytearray([d]) * first_off, [], base0
    for i, p in enumerate(plains):
        buf += bytes([d]) * (gaps[i] if gaps else 0)
        frames.append((len(buf), len(p), base))
        buf += p
        base += len(p)
    return bytes(buf + bytes([d]) * 40), frames


def cases():
    """[(name, buf, frames, d)]"""
    rng = random.Random(0x2EC0)
    out = []
    for n in LENGTHS:
        for align in range(16):
            buf, frames = _around([_alphabet(rng, 0x0A, n)], 0x0A, 32 + align, base0=rng.randrange(1 << 40))
            out.append(("len%d:a%d" % (n, align), buf, frames, 0x0A))
    # one delimiter at an edge: of the frame, of a chunk, of a 16-byte group, of a wave step (1024 bytes of the interior)
    n, off = 2 * CHUNK + 5, 32 + 5
    head = (16 - off % 16) % 16
    edges = {0, n - 1, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, head - 1, head, head + 15, head + 16, head + 1023, head + 1024, head + 2047,
             head + 2048, CHUNK + ((16 - (off + CHUNK) % 16) % 16) + 1024, CHUNK + ((16 - (off + CHUNK) % 16) % 16) + 1023}
    for p in sorted(edges):
        plain = bytearray(b"x" * n)
        plain[p] = 0x0A
        out.append(("edge:%d" % p, *_around([bytes(plain)], 0x0A, off), 0x0A))
    plain = bytearray(b"x" * n)
    for p in edges:
        plain[p] = 0x0A
    out.append(("edges", *_around([bytes(plain)], 0x0A, off), 0x0A))
    for align in (0, 7, 15):
        out.append(("none:a%d" % align, *_around([b"y" * n], 0x0A, 16 + align), 0x0A))
        out.append(("all:a%d" % align, *_around([b"\n" * n], 0x0A, 16 + align), 0x0A))
    for d in DELIMS:
        for align in (0, 3, 9):
            out.append(("d%02x:a%d" % (d, align), *_around([_alphabet(rng, d, CHUNK + 1000)], d, 48 + align, base0=7), d))
    # a dictionary-style gap full of delimiters in front of the second frame; two frames of several chunks: counts that cross the prefix
    out.append(("gap", *_around([_alphabet(rng, 0x0A, 300), _alphabet(rng, 0x0A, CHUNK + 77)], 0x0A, 19, gaps=[0, 1234], base0=1000), 0x0A))
    out.append(("two", *_around([_alphabet(rng, 0x0A, 2 * CHUNK + 5), b"", _alphabet(rng, 0x0A, 3 * CHUNK - 1)], 0x0A, 33, base0=(1 << 33) + 5), 0x0A))
    return out


def _packed(table):
    return b"".join(struct.pack("<QQII", o, b, n, f) for o, b, n, f in table)


@pytest.fixture(scope="module")
def expected():
    """[(name, buf, frames, d, table, fstart, (counts, prefix, totals, staging))]: the model, computed once"""
    out = []
    for name, buf, frames, d in cases():
        table, fstart = records.chunks(frames)
        out.append((name, buf, frames, d, table, fstart, records.expected(buf, frames, d)))
    return out


def test_count_scan_emit_equal_the_model_and_stay_inside_their_windows(built, expected):
    L = built[0]
    seen = {"dense": 0, "none": 0, "multi": 0}
    for name, buf, frames, d, table, fstart, (counts, prefix, totals, staging) in expected:
        hold, at = lanesuite.aligned_copy(buf)
        nch, nf, cap = len(table), len(frames), len(staging)
        tb, fs = lanesuite.exact_buffer(_packed(table)), (C.c_uint32 * (nf + 1))(*fstart)
        got_c, got_p, got_t, got_s = (C.c_uint32 * max(nch, 1))(), (C.c_uint64 * max(nch, 1))(), (C.c_uint64 * (nf + 1))(), (C.c_uint64 * max(cap, 1))()
        counters = (C.c_uint64 * 6)()
        bad = L.zgemu_records(at, tb, nch, fs, nf, d, got_c, got_p, got_t, got_s, cap, counters)
        assert bad == 0, (name, "lanes of a count wave disagree")
        assert list(got_c[:nch]) == counts, (name, list(got_c[:nch]), counts)
        assert list(got_p[:nch]) == prefix and list(got_t) == totals, (name, list(got_t), totals)
        assert list(got_s[:cap]) == staging, (name, [(i, a, b) for i, (a, b) in enumerate(zip(got_s[:cap], staging)) if a != b][:5])
        assert tuple(counters) == (0, 0, 0, 0, cap, 0), (name, tuple(counters))
        seen["dense"] += any(c == n for c, (_, _, n, _) in zip(counts, table) if n >= 1024)
        seen["none"] += cap == 0
        seen["multi"] += nch > 2
    assert seen["dense"] >= 3 and seen["none"] >= 3 and seen["multi"] >= 30, seen


def _entries():
    """the handle's array: four entries' offsets back to back — closed, open tail, one whose records include a delimiter alone, empty"""
    plains = [b"ab\ncd\n\nefg\n", b"one\ntwo\nthree", b"\n\nx\n\n", b""]
    ents, words = [], []
    for p in plains:
        O, tail = records.offsets(p, 0x0A)
        ents.append((len(words), O, tail))
        words += O
    return ents, words


def find_lanes():
    """[(first, count, rpre, nrec, flags, status, entry, window, want)]"""
    ents, _ = _entries()
    lanes = []
    for e, (rpre, O, tail) in enumerate(ents):
        R = len(O) - 1
        for first in sorted({0, max(R - 1, 0), R, R + 1, U64}):
            for count in sorted({0, 1, R, U64}):
                for strip in (0, STRIP):
                    begin, n = records.find(O, tail, first, count, strip)
                    lanes.append((first, count, rpre, R, strip | (2 if tail else 0), 0, e, (rpre, rpre + R + 1), (begin, n, e, 0)))
    lanes.append((0, 5, 0, 0, 0, BAD_ARG, 9, (0, 0), (0, 0, 9, BAD_ARG)))    # lanes the host gave a status: nothing is read
    lanes.append((1, 1, 0, 0, STRIP, 74, 2, (0, 0), (0, 0, 2, 74)))
    return lanes


def _packed_lanes(lanes):
    return b"".join(struct.pack("<QQQQIIII", f, c, rp, R, fl, st, e, 0) for f, c, rp, R, fl, st, e, _, _ in lanes)


def test_find_lanes_equal_the_model_and_read_two_offsets_of_their_entry(built):
    L = built[0]
    ents, words = _entries()
    o = (C.c_uint64 * len(words))(*words)
    lanes = find_lanes()
    # the strips the issue names, pinned: a closed last record loses its delimiter, an open one nothing, a delimiter alone gives len 0
    assert records.find(ents[0][1], False, 3, 1, STRIP) == (7, 3) and records.find(ents[1][1], True, 2, 1, STRIP) == (8, 5)
    assert records.find(ents[2][1], False, 1, 1, STRIP) == (1, 0) and records.find(ents[1][1], True, 0, U64, STRIP) == (0, 13)
    for lo in range(0, len(lanes), 64):
        part = lanes[lo:lo + 64]
        m = len(part)
        lb, lat = lanesuite.aligned_copy(_packed_lanes(part))
        win = (C.c_uint64 * (2 * m))(*[x for ln in part for x in ln[7]])
        out, host, counters = C.create_string_buffer(24 * m), C.create_string_buffer(24 * m), (C.c_uint64 * 2)()
        L.zgemu_records_find(o, lat, m, win, out, host, counters)
        for j, ln in enumerate(part):
            got, h = struct.unpack_from("<QQII", out.raw, 24 * j), struct.unpack_from("<QQII", host.raw, 24 * j)
            assert got == ln[8] and h == ln[8], (ln[:7], got, h, ln[8])
        assert counters[1] == 0 and counters[0] <= 2 * sum(1 for ln in part if not ln[5]), tuple(counters)


def test_the_host_forms_equal_the_model(built):
    L = built[0]
    rng = random.Random(0xA10E)
    for d in DELIMS:
        for n in (0, 1, 2, 17, 5000):
            for p in (_alphabet(rng, d, n), bytes([d]) * n, bytes([(d + 1) & 255]) * n):
                want = [1000 + x for x in records.delimiters(p, d)]
                out = (C.c_uint64 * max(len(want), 1))()
                assert L.zgemu_records_host(p, n, d, 1000, out, len(want)) == len(want) and list(out[:len(want)]) == want, (d, n)
    for off, size, base in ((0, 0, 0), (5, 1, 9), (37, CHUNK, 1 << 40), (3, CHUNK + 1, 0), (16, 5 * CHUNK - 1, 77)):
        want, _ = records.chunks([(off, size, base)])
        out = C.create_string_buffer(24 * max(len(want), 1))
        assert L.zgemu_records_cut(off, size, base, 0, out, len(want)) == len(want)
        assert [struct.unpack_from("<QQII", out.raw, 24 * i) for i in range(len(want))] == want
    # the offsets of whole entries: the open-tail rule (pinned)
    assert records.offsets(b"", 10) == ([0], False) and records.offsets(b"\n", 10) == ([0, 1], False) and records.offsets(b"a", 10) == ([0, 1], True)
    assert records.offsets(b"a\nb", 10) == ([0, 2, 3], True) and records.offsets(b"a\nb\n", 10) == ([0, 2, 4], False)


def test_records_under_address_sanitizer_stand_alone(built, expected):
    _, exe, d_ = built
    src, dst = d_ / "cases.bin", d_ / "out.bin"
    lanes = find_lanes()
    _, words = _entries()
    with open(src, "wb") as f:
        for name, buf, frames, d, table, fstart, (counts, prefix, totals, staging) in expected:
            f.write(struct.pack("<IIIIQ", 0, len(table), len(frames), d, len(staging)) + _packed(table) + struct.pack("<%dI" % len(fstart), *fstart))
            for o, _, n, _ in table:
                f.write(buf[o:o + n])
        f.write(struct.pack("<IIIIQ", 1, len(lanes), 0, 0, len(words)) + _packed_lanes(lanes) + struct.pack("<%dQ" % len(words), *words))
    lanesuite.run_stand_alone(exe, [src, dst], b"records_asan ok", timeout=300)
    raw, at = open(dst, "rb").read(), 0
    for name, buf, frames, d, table, fstart, (counts, prefix, totals, staging) in expected:
        nch, nf, cap = len(table), len(frames), len(staging)
        got = struct.unpack_from("<%dI%dQ%dQ%dQ" % (nch, nch, nf + 1, cap), raw, at)
        at += 4 * nch + 8 * (nch + nf + 1 + cap)
        assert list(got) == counts + prefix + totals + staging, name
    for ln in lanes:
        assert struct.unpack_from("<QQII", raw, at) == ln[8], ln[:7]
        at += 24
    assert at == len(raw)
