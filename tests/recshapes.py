"""Shapes built at the scan, lane and launch edges of the record index (test helper, no tests): zg_k_recs_count / _scan / _emit / _find of
zstd-rs_amd/csrc/zg_records.h with their host glue (records_submit in zg_frames.cpp, records_entries / relay_records in zg_ranges.cpp). The
suites before this one (test_records_cpu, test_gpu_seek_index_records) never hand the scan more than 108 chunks or 14 frames, nor the find
kernel more than 38 lanes; these shapes are what aims past that. tests/test_recshapes_cpu.py runs them through the SIMT emulator and pins
what each one rests on, tests/test_gpu_recshapes.py through the public calls on the GPU.

A shape is a Shape: entries (each a list of frames: a plaintext, or Skip(payload) for a skippable frame), a delimiter, the run_bytes to pass,
and the model's expectation — offsets() per entry from records.offsets, submits() = [(chunks, frames)] from records.chunks. The plaintexts are
built, not sampled: filler bytes with delimiters at chosen places, so the compressed frames are small.

What the expectation rests on, read out of the source:
  * cut_runs (zg_ranges.cpp) closes a run in front of a zstd row when the run already holds one and would, with that row, exceed run_bytes; the
    runs of a call are the sub-entries of decode_entries (zg_frames.cpp), which gathers them into submits of at most kFramesSubmitBytes =
    512 MiB of plaintext bound. Everything here is a few MiB, so EVERY CALL IS ONE SUBMIT however its runs are cut, and the scan sees every
    chunk of the call at once: submits() is one pair per call. The shapes that must be one run pass their plaintext's length as run_bytes all
    the same; `silent` passes 1, so that every frame is a run of its own;
  * the frames of a submit lie byte-tight from a start at a multiple of 16 (zg_records.h: "frames follow each other byte-tight"): layout()
    is that rule, and the alignment of a frame is the sum of the sizes in front of it mod 16;
  * zg_k_recs_scan's thread t of 256 takes the chunks [t * per, (t + 1) * per), per = ceil(nchunks / 256): stretches() is that rule. With
    per >= 2 fewer than 256 threads have chunks — ceil(257 / 2) = 129, ceil(513 / 3) = 171, ceil(1025 / 5) = 205 —, so stretch-257 and
    stretch-513 CANNOT put a sum into the fourth wave (threads 192 .. 255): they hold a non-zero sum in every wave that has chunks, the other
    stretch shapes in all four.

Families:
  stretch-N   one entry, one run, N chunks, N of STRETCH: 257 is the smallest with per = 2, 513 gives 3, 1025 gives 5 (the last threads have
              lo == hi == nchunks). Filler 'x'; for every thread t of EDGE_THREADS and the last working one a delimiter at the last byte of chunk
              t * per + per - 1 and at the first byte of chunk (t + 1) * per where those exist; a seeded sprinkling into every wave that has
              chunks. Three frames whose sizes are no multiples of 16: chunk and frame boundaries are out of step.
  frames-F    one entry, one run, F zstd frames, F of FRAMES: sizes cycle through 1 .. 47; frames of size 0 at the front, in the middle and as
              the last two; a skippable frame behind every 50th; a seeded pattern of delimiters that leaves some frames without any. nframes
              > 256 and > 512, equal neighbours in fstart, trailing frames whose first chunk is nchunks.
  dense-aA-dD three dense frames — 3 * kChunk + 7 bytes that are all the delimiter; delimiter and another byte in turn (8 per lane); whole
              16-byte groups of delimiters, every second group skipped — each behind filler frames that put it at output alignment A of
              DENSE_ALIGNS; delimiter D of DENSE_DELIMS.
  silent      three entries in one call, run_bytes 1: A = text 30000, 70000 bytes without a delimiter, text 9000 (the middle run finds nothing);
              B = 5000 bytes without a delimiter (O == [0, L], an open tail and no device piece); C = 5000 delimiters and nothing else.
  silent-b    B in a call of its own: a submit whose total is 0 (records_submit allocates no staging and launches no emit).
  lanes(m)    m of LANES seeded (entry, first, count[, STRIP]) over the entries of stretch-257 and silent (lane_entries()): first of
              0 .. R + 2 and 2^64 - 1, count of 0 .. 5, R, 2^63 and 2^64 - 1; lanes the host must refuse (entry out of range, an unknown
              flag bit) at positions 0, 63, 64 and m - 1; one lane of each clip case at positions 1 .. 5."""
import functools
import random

import records
from records import CHUNK, STRIP, U64

SCAN_THREADS = 256                      # zgr::kScanThreads
STRETCH = (255, 256, 257, 511, 512, 513, 1025)
FRAMES = (257, 513)
DENSE_ALIGNS = (0, 5, 15)
DENSE_DELIMS = (0x0A, 0x00, 0xFF)
LANES = (63, 64, 65, 1000)
EDGE_THREADS = (0, 1, 63, 64, 127, 128, 191, 192)
NL = 0x0A
BAD_FLAG = 2                            # no bit of ZGPU_RECORDS_STRIP


class Skip:
    """a skippable frame of this payload"""

    def __init__(self, payload):
        self.payload = payload


class Shape:
    def __init__(self, name, entries, d, run_bytes):
        self.name, self.entries, self.d, self.run_bytes = name, entries, d, run_bytes

    def plains(self, e):
        """the plaintexts of entry e's zstd frames"""
        return [p for p in self.entries[e] if not isinstance(p, Skip)]

    def plain(self, e):
        return b"".join(self.plains(e))

    @functools.lru_cache(None)
    def offsets(self):
        """[(O, open_tail)] per entry"""
        return [records.offsets(self.plain(e), self.d) for e in range(len(self.entries))]

    @functools.lru_cache(None)
    def layout(self, first_off=0):
        """[(out_off, size, base)] of every zstd frame of the call, byte-tight from first_off (a multiple of 16); base in its entry's coordinates"""
        assert first_off % 16 == 0
        out, off = [], first_off
        for e in range(len(self.entries)):
            base = 0
            for p in self.plains(e):
                out.append((off, len(p), base))
                off += len(p)
                base += len(p)
        return out

    def table(self):
        """(chunk table, fstart) of the call's one submit"""
        return records.chunks(self.layout())

    def submits(self):
        """[(chunks, frames)] per expected submit"""
        table, fstart = self.table()
        return [(len(table), len(fstart) - 1)]

    def output(self, first_off=32, behind=40):
        """the submit's output as layout(first_off) has it, full of delimiters in front and behind"""
        body = b"".join(self.plain(e) for e in range(len(self.entries)))
        return bytes([self.d]) * first_off + body + bytes([self.d]) * behind

    def frames(self, e, content_size=True):
        """[(frame, plaintext or None)] of entry e, as test_gpu_seek_index_measured.Shard takes them"""
        import zgdata
        from test_walk_cpu import skippable
        return [(skippable(p.payload), None) if isinstance(p, Skip) else (zgdata.zstd_compress(p, checksum=False, content_size=content_size), p)
                for p in self.entries[e]]


def stretches(nchunks):
    """(per, [(lo, hi)] per thread): the chunks zg_k_recs_scan's thread t walks"""
    per = (nchunks + SCAN_THREADS - 1) // SCAN_THREADS
    return per, [(min(t * per, nchunks), min(min(t * per, nchunks) + per, nchunks)) for t in range(SCAN_THREADS)]


def wave_sums(counts):
    """the four waves' sums of the threads' sums"""
    _, st = stretches(len(counts))
    sums = [sum(counts[lo:hi]) for lo, hi in st]
    return [sum(sums[64 * w:64 * w + 64]) for w in range(SCAN_THREADS // 64)]


def waves_with_chunks(nchunks):
    _, st = stretches(nchunks)
    return [any(lo < hi for lo, hi in st[64 * w:64 * w + 64]) for w in range(SCAN_THREADS // 64)]


def edge_chunks(nchunks):
    """[(chunk, 'last' or 'first')]: the last byte of the last chunk of an edge thread's stretch, the first byte of the first chunk behind it"""
    per, st = stretches(nchunks)
    working = [t for t, (lo, hi) in enumerate(st) if lo < hi]
    out = []
    for t in sorted(set(EDGE_THREADS) | {working[-1]}):
        if t * per + per - 1 < nchunks:
            out.append((t * per + per - 1, "last"))
        if (t + 1) * per < nchunks:
            out.append(((t + 1) * per, "first"))
    return out


def _split(n, k):
    """n chunks over k frames, every frame at least one chunk, no two alike"""
    a = n // k
    parts = [a - 7, a + 12] + [a] * (k - 2) if k > 1 else [n]
    parts[-1] += n - sum(parts)
    assert sum(parts) == n and min(parts) >= 1
    return parts


@functools.lru_cache(None)
def stretch(n):
    assert n in STRETCH
    rng = random.Random(0x57E7 + n)
    nfr = 3 if n % 2 else 2
    rem = (1001, 2077, 3003)[:nfr]                       # the bytes of a frame's last chunk: no frame is a multiple of 16 long
    sizes = [(c - 1) * CHUNK + r for c, r in zip(_split(n, nfr), rem)]
    assert all(s % 16 for s in sizes)
    plains = [bytearray(b"x" * s) for s in sizes]
    table, _ = records.chunks([(0, s, 0) for s in sizes])   # (chunk -> (place in its frame, len, frame); out_off is not used here)
    assert len(table) == n

    def put(chunk, at):
        _, base, ln, f = table[chunk]
        plains[f][base + (at if at >= 0 else ln + at)] = NL

    for chunk, where in edge_chunks(n):
        put(chunk, -1 if where == "last" else 0)
    _, st = stretches(n)
    for w in range(SCAN_THREADS // 64):                     # the sprinkling: three chunks of every wave that has any
        mine = [i for lo, hi in st[64 * w:64 * w + 64] for i in range(lo, hi)]
        for chunk in rng.sample(mine, min(3, len(mine))):
            for _ in range(rng.randrange(1, 4)):
                put(chunk, rng.randrange(table[chunk][2]))
    total = sum(sizes)
    return Shape("stretch-%d" % n, [[bytes(p) for p in plains]], NL, total)


@functools.lru_cache(None)
def frames(F):
    assert F in FRAMES
    rng = random.Random(0xF7A3 + F)
    sizes = [1 + i % 47 for i in range(F)]
    for i in (0, F // 2, F - 2, F - 1):
        sizes[i] = 0
    entry = []
    for i, s in enumerate(sizes):
        p = bytearray(rng.choice(b"abcdefgh") for _ in range(s))
        if s and rng.random() < 0.6:                        # (four frames in ten keep no delimiter)
            for _ in range(rng.randrange(1, 4)):
                p[rng.randrange(s)] = NL
        entry.append(bytes(p))
        if i % 50 == 49:
            entry.append(Skip(b"skip%d" % i))
    return Shape("frames-%d" % F, [entry], NL, sum(sizes))


@functools.lru_cache(None)
def dense(align, d):
    assert align in DENSE_ALIGNS and d in DENSE_DELIMS
    o = (d + 1) & 255
    allofit = bytes([d]) * (3 * CHUNK + 7)
    turns = bytes([d, o]) * (CHUNK + 9)                                       # 8 of 16 bytes per lane
    groups = (bytes([d]) * 16 + bytes([o]) * 16) * (CHUNK // 16 + 3)           # whole groups, every second one skipped
    entry, at = [], 0
    for p in (allofit, turns, groups):
        pad = (align - at) % 16                                                # the filler frame in front: 0, 5 or 15 bytes for the first
        entry.append(bytes([o]) * pad)
        at += pad
        assert at % 16 == align
        entry.append(p)
        at += len(p)
    return Shape("dense-a%d-d%02x" % (align, d), [entry], d, at)


def dense_frames(shape):
    """the indices, among the zstd frames of a dense shape, of its three dense frames"""
    return (1, 3, 5)


def _text(rng, n):
    """n bytes of words in lines of 20 .. 90 bytes; the last byte is no newline"""
    out = bytearray()
    while len(out) < n:
        line = rng.randrange(20, 91)
        while line > 0:
            w = rng.randrange(1, 9)
            out += bytes(rng.choice(b"etaoinshr") for _ in range(w)) + b" "
            line -= w + 1
        out[-1] = NL
    out = out[:n]
    out[-1] = ord("z")
    return bytes(out)


@functools.lru_cache(None)
def silent():
    rng = random.Random(0x511E)
    a = [_text(rng, 30000), b"q" * 70000, _text(rng, 9000)]
    return Shape("silent", [a, [b"w" * 5000], [b"\n" * 5000]], NL, 1)


@functools.lru_cache(None)
def silent_alone():
    """silent's entry B in a call of its own: the submit's total is 0 — no staging is allocated, no emit launched, the run has no buffer"""
    return Shape("silent-b", [silent().entries[1]], NL, 1)


def shapes():
    """every shape of the four families"""
    return ([stretch(n) for n in STRETCH] + [frames(F) for F in FRAMES] + [dense(a, d) for a in DENSE_ALIGNS for d in DENSE_DELIMS] +
            [silent(), silent_alone()])


def by_name(name):
    return {s.name: s for s in shapes()}[name]


@functools.lru_cache(None)
def lane_entries():
    """the shape lanes(m) look records up in: the entry of stretch-257, then the three of silent"""
    return Shape("lanes", stretch(257).entries + silent().entries, NL, 1)


@functools.lru_cache(None)
def lanes(m):
    """[(entry, first, count[, flags])], and what the host and the kernel must answer: [((entry, begin, len), refused)]"""
    assert m in LANES
    rng = random.Random(0x1A9E + m)
    model = lane_entries().offsets()
    n = len(model)
    A, B, Cc = 1, 2, 3                                      # silent's entries: open tail, O == [0, L], delimiters alone
    RA, RC = len(model[A][0]) - 1, len(model[Cc][0]) - 1
    fixed = {1: (A, RA + 1, 3),                             # a >= b: first behind the last record
             2: (A, RA - 2, 9, STRIP),                      # b == R on an open tail: nothing is stripped
             3: (Cc, RC - 2, 9, STRIP),                     # b == R on a closed last record: its delimiter goes
             4: (Cc, 17, 1, STRIP),                         # a record that is the delimiter alone: stripped to length 0
             5: (B, 0, U64, STRIP)}                         # the entry without a delimiter: one open record
    refused = {0: (n, 0, 1), 63: (0, 1, 1, BAD_FLAG), 64: (n + 7, 2, 2, STRIP), m - 1: (1, 0, 1, STRIP | BAD_FLAG)}
    out = []
    for j in range(m):
        if j in refused:
            out.append(refused[j])
            continue
        if j in fixed:
            out.append(fixed[j])
            continue
        e = rng.randrange(n)
        R = len(model[e][0]) - 1
        first = rng.choice(list(range(R + 3)) + [U64] * max(1, R // 8))
        count = rng.choice([0, 1, 2, 3, 4, 5, R, 1 << 63, U64])
        out.append((e, first, count, STRIP) if rng.random() < 0.5 else (e, first, count))
    want = []
    for ln in out:
        e, flags = ln[0], ln[3] if len(ln) > 3 else 0
        if e >= n or flags & ~STRIP:
            want.append(((e, 0, 0), True))
        else:
            O, tail = model[e]
            want.append(((e,) + records.find(O, tail, ln[1], ln[2], flags), False))
    return out, want
