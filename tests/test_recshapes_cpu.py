"""The record index's kernels past the shapes test_records_cpu stops at (zstd-rs_amd/csrc/zg_records.h: zgr::recs_scan with stretches longer than
one chunk, more than 256 frames and sums in every wave; the whole pass — count, scan, emit — over more than 256 chunks and frames; zgr::recs_find
in more than one workgroup), on the CPU through the SIMT emulator: the harness is tests/emu/zg_emu_records.cpp, the one test_records_cpu builds.
The shapes are tests/recshapes.py's; every expectation is tests/records.py's, in plain Python integers.

The scan alone (zgemu_records_scan: no plaintext, so a large nchunks costs nothing): nchunks of NCHUNKS x counts that are all 4096, all 0, one
single 1 at each stretch edge in turn (recshapes.edge_chunks: the last chunk of the stretches of threads 0, 1, 63, 64, 127, 128, 191, 192 and
the last working one, and the first chunk behind each), or seeded values <= 4096, over nframes of NFRAMES (every nframes for the seeded
counts, in turn for the others) whose fstart has equal neighbours at the front, in the middle and at the end (a trailing frame whose first
chunk is nchunks). Demanded of every case: every prefix, the total and every frame's total equal records.scan; exactly nchunks prefix stores,
one store of the total and nframes of a frame's total; no access outside an array, guard bands intact.

The whole pass: stretch-257, stretch-513, frames-257 and every dense shape through zgemu_records against records.expected, with the demands
of test_records_cpu (stretch-513 takes about a second here, so it stays). lanes(m) for every m go through zgemu_records_find in ONE call each:
ceil(m / 64) workgroups, the last one partial. In the stand-alone AddressSanitizer program every array is a heap block of exactly its length:
every scan case up to 513 chunks and, of the larger nchunks, the seeded, the all-4096 and the last edge case (the case file stays at a few MiB);
lanes(65) and lanes(1000).

The generator is pinned: chunk and frame counts per shape, non-zero sums in every wave that has chunks (all four but for stretch-257 and
stretch-513, whose stretches end in the third wave: recshapes' docstring), the alignments 0, 5 and 15 of the dense frames, silent's middle run
without a delimiter, the refused lanes and one lane of each clip case."""
import ctypes as C
import random
import struct

import pytest

import lanesuite
import records
import recshapes
from records import CHUNK, STRIP, U64
from test_records_cpu import BAD_ARG, _packed, _packed_lanes, built   # noqa: F401 (built: the fixture, one build per session)

NCHUNKS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 131072 + 300)
NFRAMES = (1, 255, 256, 257, 1000)
WHOLE = ("stretch-257", "stretch-513", "frames-257") + tuple("dense-a%d-d%02x" % (a, d) for a in recshapes.DENSE_ALIGNS for d in recshapes.DENSE_DELIMS)


def _fstart(rng, nchunks, nframes):
    """nframes + 1 frame starts over nchunks chunks; from three frames on: equal neighbours at the front, in the middle and at the end"""
    fs = [0] + sorted(rng.randrange(nchunks + 1) for _ in range(nframes - 1)) + [nchunks]
    if nframes >= 3:
        fs[1] = 0
        fs[nframes // 2 + 1] = fs[nframes // 2]
        fs[nframes - 1] = nchunks
    assert all(a <= b for a, b in zip(fs, fs[1:])) and len(fs) == nframes + 1
    return fs


def scan_cases():
    """[(name, counts, fstart)]"""
    rng = random.Random(0x5CA9)
    out, turn = [], 0
    for n in NCHUNKS:
        kinds = [("full", [CHUNK] * n), ("zero", [0] * n)]
        for chunk in sorted({c for c, _ in recshapes.edge_chunks(n)}):
            kinds.append(("edge%d" % chunk, [int(i == chunk) for i in range(n)]))
        for name, counts in kinds:
            nf = NFRAMES[turn % len(NFRAMES)]
            turn += 1
            out.append(("n%d:%s:f%d" % (n, name, nf), counts, _fstart(rng, n, nf)))
        for nf in NFRAMES:
            out.append(("n%d:seeded:f%d" % (n, nf), [rng.randrange(CHUNK + 1) for _ in range(n)], _fstart(rng, n, nf)))
    return out


@pytest.fixture(scope="module")
def scans():
    """[(name, counts, fstart, (prefix, total, frame totals))]: the model, computed once"""
    return [(name, counts, fs, records.scan(counts, fs)) for name, counts, fs in scan_cases()]


def test_the_scan_alone_equals_the_model_past_one_chunk_per_thread(built, scans):
    L = built[0]
    seen = {"per>1": 0, "four waves": 0, "frames>256": 0, "trailing": 0}
    for name, counts, fs, (prefix, total, ftot) in scans:
        n, nf = len(counts), len(fs) - 1
        c, f = (C.c_uint32 * n)(*counts), (C.c_uint32 * (nf + 1))(*fs)
        got_p, got_t, counters = (C.c_uint64 * n)(), (C.c_uint64 * (nf + 1))(), (C.c_uint64 * 5)()
        L.zgemu_records_scan(c, n, f, nf, got_p, got_t, counters)
        assert got_t[0] == total and list(got_t[1:]) == ftot, (name, got_t[0], total, [(i, a, b) for i, (a, b) in enumerate(zip(got_t[1:], ftot)) if a != b][:4])
        assert list(got_p) == prefix, (name, [(i, a, b) for i, (a, b) in enumerate(zip(got_p, prefix)) if a != b][:4])
        assert tuple(counters) == (0, n, 1, nf, 0), (name, tuple(counters))
        seen["per>1"] += n > 256
        seen["four waves"] += all(recshapes.wave_sums(counts))
        seen["frames>256"] += nf > 256
        seen["trailing"] += nf >= 3 and fs[nf - 1] == n and total > 0
    assert seen["per>1"] >= 50 and seen["four waves"] >= 40 and seen["frames>256"] >= 40 and seen["trailing"] >= 100, seen


@pytest.fixture(scope="module")
def whole():
    """[(shape, buf, frames, table, fstart, (counts, prefix, totals, staging))] of WHOLE"""
    out = []
    for name in WHOLE:
        s = recshapes.by_name(name)
        buf, frames = s.output(32), s.layout(32)
        table, fstart = records.chunks(frames)
        out.append((s, buf, frames, table, fstart, records.expected(buf, frames, s.d)))
    return out


def test_the_whole_pass_equals_the_model_past_256_chunks_and_frames(built, whole):
    L = built[0]
    for s, buf, frames, table, fstart, (counts, prefix, totals, staging) in whole:
        O, tail = s.offsets()[0]
        assert staging == O[1:len(O) - 1 if tail else len(O)], s.name      # (one entry: the staging is its offsets behind O[0], in front of an open tail's L)
        hold, at = lanesuite.aligned_copy(buf)
        nch, nf, cap = len(table), len(frames), len(staging)
        assert (nch, nf) == s.submits()[0]
        tb, fs = lanesuite.exact_buffer(_packed(table)), (C.c_uint32 * (nf + 1))(*fstart)
        got_c, got_p, got_t, got_s = (C.c_uint32 * nch)(), (C.c_uint64 * nch)(), (C.c_uint64 * (nf + 1))(), (C.c_uint64 * max(cap, 1))()
        counters = (C.c_uint64 * 6)()
        bad = L.zgemu_records(at, tb, nch, fs, nf, s.d, got_c, got_p, got_t, got_s, cap, counters)
        assert bad == 0, (s.name, "lanes of a count wave disagree")
        assert list(got_c) == counts, (s.name, [(i, a, b) for i, (a, b) in enumerate(zip(got_c, counts)) if a != b][:4])
        assert list(got_p) == prefix, (s.name, [(i, a, b) for i, (a, b) in enumerate(zip(got_p, prefix)) if a != b][:4])
        assert list(got_t) == totals, (s.name, [(i, a, b) for i, (a, b) in enumerate(zip(got_t, totals)) if a != b][:4])
        assert list(got_s[:cap]) == staging, (s.name, [(i, a, b) for i, (a, b) in enumerate(zip(got_s[:cap], staging)) if a != b][:5])
        assert tuple(counters) == (0, 0, 0, 0, cap, 0), (s.name, tuple(counters))


def _find_lanes(m):
    """(the handle's array, [(first, count, rpre, nrec, flags, status, entry, window, want)]) of recshapes.lanes(m), as lookup_records lays them out"""
    model = recshapes.lane_entries().offsets()
    words, rpre = [], []
    for O, _ in model:
        rpre.append(len(words))
        words += O
    lanes = []
    for ln, ((e, begin, n), refused) in zip(*recshapes.lanes(m)):
        flags = ln[3] if len(ln) > 3 else 0
        if refused:
            lanes.append((ln[1], ln[2], 0, 0, flags, BAD_ARG, e, (0, 0), (0, 0, e, BAD_ARG)))
            continue
        O, tail = model[e]
        R = len(O) - 1
        lanes.append((ln[1], ln[2], rpre[e], R, (flags & STRIP) | (2 if tail else 0), 0, e, (rpre[e], rpre[e] + R + 1), (begin, n, e, 0)))
    return words, lanes


@pytest.mark.parametrize("m", recshapes.LANES)
def test_find_lanes_in_one_call_of_several_workgroups(built, m):
    L = built[0]
    words, lanes = _find_lanes(m)
    o = (C.c_uint64 * len(words))(*words)
    lb, lat = lanesuite.aligned_copy(_packed_lanes(lanes))
    win = (C.c_uint64 * (2 * m))(*[x for ln in lanes for x in ln[7]])
    out, host, counters = C.create_string_buffer(24 * m), C.create_string_buffer(24 * m), (C.c_uint64 * 2)()
    L.zgemu_records_find(o, lat, m, win, out, host, counters)
    for j, ln in enumerate(lanes):
        got, h = struct.unpack_from("<QQII", out.raw, 24 * j), struct.unpack_from("<QQII", host.raw, 24 * j)
        assert got == ln[8] and h == ln[8], (j, ln[:7], got, h, ln[8])
    assert counters[1] == 0 and counters[0] <= 2 * sum(1 for ln in lanes if not ln[5]), tuple(counters)


def _asan_scans(scans):
    """the scan cases the stand-alone program runs: all up to 513 chunks; of a larger nchunks the seeded, the all-4096 and the last edge case"""
    out, last_edge = [], {}
    for case in scans:
        if len(case[1]) > 513 and ":edge" in case[0]:
            last_edge[len(case[1])] = case
    for case in scans:
        n, name = len(case[1]), case[0]
        if n <= 513 or name.endswith(":seeded:f257") or ":full:" in name or case is last_edge[n]:
            out.append(case)
    return out


def test_the_scan_and_the_lanes_under_address_sanitizer_stand_alone(built, scans):
    _, exe, d_ = built
    src, dst = d_ / "shapes_cases.bin", d_ / "shapes_out.bin"
    chosen = _asan_scans(scans)
    assert sum(len(c[1]) > 65000 for c in chosen) >= 12 and len(chosen) > 150
    finds = [_find_lanes(m) for m in (65, 1000)]
    with open(src, "wb") as f:
        for name, counts, fs, _ in chosen:
            f.write(struct.pack("<IIIIQ", 2, len(counts), len(fs) - 1, 0, 0) + struct.pack("<%dI" % len(counts), *counts) + struct.pack("<%dI" % len(fs), *fs))
        for words, lanes in finds:
            f.write(struct.pack("<IIIIQ", 1, len(lanes), 0, 0, len(words)) + _packed_lanes(lanes) + struct.pack("<%dQ" % len(words), *words))
    lanesuite.run_stand_alone(exe, [src, dst], b"records_asan ok", timeout=300)
    raw, at = open(dst, "rb").read(), 0
    for name, counts, fs, (prefix, total, ftot) in chosen:
        n, nf = len(counts), len(fs) - 1
        got = struct.unpack_from("<%dQ" % (n + 1 + nf), raw, at)
        at += 8 * (n + 1 + nf)
        assert list(got) == prefix + [total] + ftot, name
    for words, lanes in finds:
        for ln in lanes:
            assert struct.unpack_from("<QQII", raw, at) == ln[8], ln[:7]
            at += 24
    assert at == len(raw)


# ---- the generator, pinned -----------------------------------------------------------------------------------------------------------------------
def test_the_shapes_hold_what_they_are_built_for():
    for n in recshapes.STRETCH:
        s = recshapes.stretch(n)
        table, fstart = s.table()
        assert s.submits() == [(n, 3 if n % 2 else 2)] and len(s.entries) == 1 and s.run_bytes == len(s.plain(0))
        assert all(size % 16 for _, size, _ in s.layout()) and any(off % CHUNK for off, _, _ in s.layout()[1:])   # chunk and frame boundaries out of step
        counts = records.expected(s.output(0, 0), s.layout(), s.d)[0]
        have = recshapes.waves_with_chunks(n)
        assert have == [True, True, True, n not in (257, 513)], (n, have)
        assert [bool(x) for x in recshapes.wave_sums(counts)] == have, (n, recshapes.wave_sums(counts))
        plain = s.plain(0)
        for chunk, where in recshapes.edge_chunks(n):                          # the edges: a delimiter at the chunk's last / first byte
            off, _, ln, _ = table[chunk]
            assert plain[off + ln - 1 if where == "last" else off] == s.d, (n, chunk, where)
    per = {n: recshapes.stretches(n)[0] for n in recshapes.STRETCH}
    assert per == {255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 1025: 5}
    assert recshapes.stretches(1025)[1][205:] == [(1025, 1025)] * 51           # the last threads: lo == hi == nchunks
    for F in recshapes.FRAMES:
        s = recshapes.frames(F)
        table, fstart = s.table()
        assert s.submits() == [(F - 4, F)] and len(fstart) == F + 1
        assert fstart[0] == fstart[1] and fstart[F // 2] == fstart[F // 2 + 1] and fstart[F - 2] == fstart[F - 1] == fstart[F] == F - 4
        sizes = [len(p) for p in s.plains(0)]
        assert set(sizes) == set(range(48)) and sum(isinstance(p, recshapes.Skip) for p in s.entries[0]) == F // 50
        none = sum(1 for p in s.plains(0) if p and s.d not in p)
        assert F // 4 < none < F // 2, none                                    # some frames without a delimiter, most with
    aligns = set()
    for a in recshapes.DENSE_ALIGNS:
        for d in recshapes.DENSE_DELIMS:
            s = recshapes.dense(a, d)
            lay = s.layout()
            fillers = [lay[i][1] for i in (0, 2, 4)]
            assert fillers[0] == a and s.submits() == [(10 + sum(1 for x in fillers if x), 6)], (s.name, fillers, s.submits())
            assert [lay[i][0] % 16 for i in recshapes.dense_frames(s)] == [a] * 3
            aligns.add(a)
            p = s.plains(0)
            assert p[1] == bytes([d]) * (3 * CHUNK + 7) and p[3].count(bytes([d])) * 2 == len(p[3]) and p[5][:32] == bytes([d]) * 16 + bytes([(d + 1) & 255]) * 16
            counts = records.expected(s.output(0, 0), lay, d)[0]
            assert CHUNK in counts and CHUNK // 2 in counts                    # 16 hits in every lane of a chunk; 8 in every lane
    assert aligns == {0, 5, 15}
    s = recshapes.silent()
    (OA, tailA), (OB, tailB), (OC, tailC) = s.offsets()
    assert s.run_bytes == 1 and s.submits() == [(8 + 18 + 3 + 2 + 2, 5)]
    assert s.d not in s.plains(0)[1] and len(s.plains(0)[1]) == 70000 and s.plains(0)[0].count(b"\n") > 100 and s.plains(0)[2].count(b"\n") > 50
    assert tailA and (OB, tailB) == ([0, 5000], True) and (OC, tailC) == (list(range(5001)), False)
    b = recshapes.silent_alone()
    assert b.offsets() == [([0, 5000], True)] and b.submits() == [(2, 1)] and b.run_bytes == 1   # (a submit whose total is 0)
    assert len(recshapes.shapes()) == 7 + 2 + 9 + 2 and len({x.name for x in recshapes.shapes()}) == 20


@pytest.mark.parametrize("m", recshapes.LANES)
def test_the_lanes_hold_refused_lanes_and_every_clip_case(m):
    lanes, want = recshapes.lanes(m)
    model = recshapes.lane_entries().offsets()
    assert len(lanes) == len(want) == m and len(model) == 4
    refused = [j for j, (_, r) in enumerate(want) if r]
    assert refused == sorted({0, 63, 64, m - 1} & set(range(m)))
    assert lanes[0][0] >= 4 and lanes[m - 1][3] & ~STRIP                       # an entry out of range; an unknown flag bit
    assert m < 1000 or (lanes[63][3] & ~STRIP and lanes[64][0] >= 4)
    seen = {"a>=b": 0, "open": 0, "closed": 0, "zero": 0, "first=max": 0, "count=max": 0}
    for ln, ((e, begin, n), r) in zip(lanes, want):
        if r:
            continue
        O, tail = model[e]
        R = len(O) - 1
        a, b = min(ln[1], R), min(min(ln[1] + ln[2], U64), R)
        strip = len(ln) > 3 and ln[3] & STRIP
        seen["a>=b"] += a >= b
        seen["open"] += a < b == R and tail and strip and n == O[b] - O[a]
        seen["closed"] += a < b == R and not tail and strip and n == O[b] - O[a] - 1
        seen["zero"] += a < b and strip and n == 0
        seen["first=max"] += ln[1] == U64
        seen["count=max"] += ln[2] == U64
    assert all(seen.values()), seen
