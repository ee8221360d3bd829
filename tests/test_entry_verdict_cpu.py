"""zstd-rs_amd/csrc/zg_entry.h on the CPU (tests/emu/zg_lane_entry.cpp): what is known about a decoded entry turned into its result, and the
pieces an entry's clips take of its frames.

1. The verdicts against a restatement, in Python, of what include/zgpu.h says of zgpu_decode_frames_device, zgpu_decode_ranges_device_src,
   ZGPU_DEVICE_VERIFY and ZGPU_DEVICE_VERIFY_SEEK_TABLE — written from that text, not from the C++ — over every combination of: 1 - 3 frames; a
   decode error (a block error, ZGPU_E_UNSUPPORTED) in none or in each frame; a walk error or none; a dictionary frame or none; no ranges (room
   or not), an empty span, one clip or two (each with room and without), a seek table's promise on and off; no frame, each frame, or the promise declaring a
   wrong size; ZGPU_DEVICE_VERIFY off, or on with a mismatch in a hashed frame, in an unhashed frame, in none; no table record, one that vouches,
   three that do not (a differing frame, a frame no row covers, a table without checksums) and one with a `why`. No case is left out.
   A second, small sweep covers what only an entry decoded alone can be: frames that are not known one by one, the buffer of the selection's
   bound, hashing switched off behind a host that hashed.
2. The pieces against Python slicing: 1 - 4 frames of 0, 1, 2 or 5 bytes, every combination, clips whose begin and end sit at 0, at every frame
   boundary - 1 / + 0 / + 1 and behind the end, lengths up to 2^64 - 1, in spans of 0 - 3 clips; applying the pieces gives exactly
   concat[skip:skip + len] per clip and touches no other byte of its destination.
The stand-alone AddressSanitizer program runs the same cases with every array in a heap block of exactly its length."""
import ctypes as C
import itertools
import os
import struct

import lanesuite

OK, BLOCK_ERR, UNSUPPORTED, WALK_ERR = 0, 20, 80, 7          # (a block error and a walk error stand for any: the ladder passes a status through)
TOO_SMALL, SIZE_MISMATCH, CHECKSUM, SEEK_CHECKSUM = 12, 71, 70, 73
TOP = 2 ** 64 - 1
NO_ROW = 0xFFFFFFFF
KOUT = 14
VERIFY, NO_HASH, RECORD, UNKNOWN, DICT, BOUND_BUFFER, RANGES, PROMISE = 1, 2, 4, 8, 16, 32, 64, 128
SIZES = (5, 3, 7)


def _declare(L):
    L.ze_settle.restype = C.c_uint64
    L.ze_settle.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.ze_pieces.restype = C.c_uint64
    L.ze_pieces.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]


built = lanesuite.built_fixture("zg_lane_entry.cpp", "entry", "ENTRY_MAIN", declare=_declare)


def test_status_values_are_the_headers():
    text = open(os.path.join(lanesuite.ROOT, "include", "zgpu.h")).read()
    for name, v in (("TARGET_TOO_SMALL", TOO_SMALL), ("CONTENT_SIZE_MISMATCH", SIZE_MISMATCH), ("CHECKSUM_MISMATCH", CHECKSUM),
                    ("SEEK_CHECKSUM_MISMATCH", SEEK_CHECKSUM), ("UNSUPPORTED", UNSUPPORTED)):
        assert "ZGPU_E_%s = %d," % (name, v) in text, name


# ---- a case: what the test knows of an entry, the bytes the harness takes, the result include/zgpu.h promises ------------------------------------
class Case:
    """frames: dicts with yielded, declared (None: declares nothing), stored (None: no Content_Checksum), digest, hashed; fail: None or (frame,
    status) — that frame and none in front of it fails to decode; walk; dict; clips: None (no ranges, cap) or [(skip, len, cap)]; promise: None
    or what the table says the frames yield together; verify, no_hash; rec: None or the compare's record (8 ints); known / counted / bound_buffer:
    an entry decoded alone (module docstring)."""

    def __init__(self, frames, fail=None, walk=0, dict=False, cap=0, clips=None, promise=None, verify=False, no_hash=False, rec=None, known=True,
                 counted=0, bound_buffer=False, decode=None):
        self.__dict__.update(locals())
        self.total = sum(f["yielded"] for f in frames)

    def pack(self):
        fl = ((VERIFY if self.verify else 0) | (NO_HASH if self.no_hash else 0) | (RECORD if self.rec else 0) | (0 if self.known else UNKNOWN) |
              (DICT if self.dict else 0) | (BOUND_BUFFER if self.bound_buffer else 0) | (RANGES if self.clips is not None else 0) |
              (PROMISE if self.promise is not None else 0))
        decode = self.decode if self.decode is not None else self.fail[1] if self.fail else 0
        # the facts a producer hands over: the bytes of the frames in front of the first failing one; what the frames declare together
        sound = sum(f["yielded"] for f in self.frames[:self.fail[0] if self.fail else None])
        decl = self.promise if self.promise is not None else TOP if any(f["declared"] is None for f in self.frames) else sum(f["declared"] for f in self.frames)
        clips = self.clips or []
        b = struct.pack("<3I2iI4Q", len(self.frames), len(clips), fl, decode, self.walk, self.counted, sound, self.total, self.cap, decl)
        at = 0
        for f in self.frames:
            word = (f["stored"] or 0) | (1 << 32 if f["hashed"] else 0) | (1 << 33 if f["stored"] is not None else 0) | (1 << 34 if f["declared"] is not None else 0)
            b += struct.pack("<6Q", at, 10, f["yielded"], f["declared"] or 0, f["digest"], word)
            at += 10
        for c in clips:
            b += struct.pack("<3Q", *c)
        if self.rec:
            b += struct.pack("<8I", *self.rec)
        return b

    def expect(self):
        """(the 12 leading output words or None where the call itself fails, [(written, small)] per clip or None where they mean nothing)"""
        fr, n = self.frames, len(self.frames)
        failed = lambda st, sums=0, bad=0, unv=0: [st, 0, 0, sums, bad, 0, 0, unv, 0, 0, 0, 0]   # noqa: E731
        clipped = None
        if self.clips is None:
            # zgpu_decode_frames_device: "what zgpu_decode_all of entry i ALONE returns". An entry with a dictionary frame is decoded frame by
            # frame, each read out before the next is looked at, so the first thing met in stream order ends it; any other in one submit: a
            # decode error, else the walk's, else TARGET_TOO_SMALL
            if self.dict:
                got = 0
                for k, f in enumerate(fr):
                    if self.fail and self.fail[0] == k:
                        return failed(self.fail[1]), None
                    got += f["yielded"]
                    if got > self.cap:
                        return failed(TOO_SMALL), None
                if self.walk:
                    return failed(self.walk), None
            else:
                st = self.fail[1] if self.fail else self.walk if self.walk else TOO_SMALL if self.total > self.cap else 0
                if self.decode is not None:
                    st = self.decode
                if st:
                    return failed(st), None
            written = self.total
        else:
            # zgpu_decode_ranges_device_src: "the order is one — decode and walk, size, TARGET_TOO_SMALL, checksum — for every entry: with or
            # without dictionary frames, in a shared submit or decoded alone"
            if self.decode == TOO_SMALL and self.bound_buffer:        # alone: only a frame that yields more than it declares overflows the bound
                return failed(SIZE_MISMATCH), None
            if self.fail or self.decode:
                return failed(self.decode or self.fail[1]), None
            if self.walk:
                return failed(self.walk), None
            # "A TAKEN frame that declares a size and decodes to another length fails its entry"; "an entry whose taken frames decode to another
            # total than the table promises"; frames that are not known are measured together
            if self.known and any(f["declared"] is not None and f["declared"] != f["yielded"] for f in fr):
                return failed(SIZE_MISMATCH), None
            if not self.known and all(f["declared"] is not None for f in fr) and sum(f["declared"] for f in fr) != self.total:
                return failed(SIZE_MISMATCH), None
            if self.promise is not None and self.promise != self.total:
                return failed(SIZE_MISMATCH), None
            # "written is the CLIPPED count ... and ZGPU_E_TARGET_TOO_SMALL is decided by that count against caps[i]"; of several ranges
            # "E_TARGET_TOO_SMALL is each range's own": the group stands as long as one of them has room
            clipped = []
            for skip, ln, cap in self.clips:
                w = len(range(self.total)[skip:skip + ln])
                clipped.append((0, 1) if w > cap else (w, 0))
            if self.clips and all(s for _, s in clipped):
                return failed(TOO_SMALL), clipped
            written = sum(w for w, _ in clipped)
        nframes = n if self.known else self.counted
        view = fr if self.known else []                             # "should the checksums of such an entry not be computable, it reports its frames with checksums = ... = 0"
        hashed = lambda f: f["hashed"] and not self.no_hash        # noqa: E731
        carried = [f for f in view if f["stored"] is not None]
        differ = lambda f: f["stored"] != f["digest"] & 0xFFFFFFFF  # noqa: E731
        # ZGPU_DEVICE_VERIFY: "An entry that would have had status 0 and holds a hashed frame whose low 32 digest bits differ from its stored
        # checksum gets ZGPU_E_CHECKSUM_MISMATCH instead: written = nframes = 0 ... r.checksums and r.checksum_mismatches of such an entry are still
        # filled (all its frames that carry a checksum / those that failed) ... every other field is 0"
        if self.verify:
            bad = [f for f in carried if f["hashed"] and differ(f)]
            if bad:
                return failed(CHECKSUM, len(carried), len(bad)), clipped
        # ZGPU_DEVICE_VERIFY_SEEK_TABLE: "The verdict ranks last ... the entry fails if any compared frame differs, if any decoded zstd frame
        # coincides with no row, or if the table carries no checksums"; "r.checksums is the frames compared, r.checksum_mismatches those that
        # differ, checksums_unverified the decoded frames not compared, every other field 0"; a table that changed fails the CALL
        if self.rec and nframes:
            rows, coinciding, compared, differing, first_bad, why, flags, _ = self.rec
            if why:
                return None, clipped
            if differing or coinciding != nframes or flags & 1:
                return failed(SEEK_CHECKSUM, compared, differing, nframes - compared), clipped
        first = view[0] if view else None
        return [0, written, nframes, len(carried), sum(1 for f in carried if hashed(f) and differ(f)),
                (first["stored"] or 0) if first else 0, first["digest"] & 0xFFFFFFFF if first and hashed(first) else 0,
                sum(1 for f in carried if not hashed(f)), 1 if first and hashed(first) else 0,
                sum(1 for f in view if hashed(f)), nframes - sum(1 for f in view if hashed(f)), 0], clipped


def frames_of(n, wrong=None, mismatch=None, unhashed=None):
    """n frames: even ones declare their size, odd ones nothing (frame `wrong` declares one byte too many); every frame but the second carries
    a Content_Checksum that holds (frame `mismatch`: one false bit); every frame is hashed but `unhashed`"""
    out = []
    for k in range(n):
        low = 0x1000 + 37 * k
        out.append({"yielded": SIZES[k], "declared": SIZES[k] + 1 if wrong == k else SIZES[k] if k % 2 == 0 else None,
                    "stored": None if k == 1 else low ^ (1 if mismatch == k else 0), "digest": 0xABCD00000000 | low, "hashed": unhashed != k})
    return out


def modes(total):
    """(cap, clips): no ranges with room and without; an empty span (zgpu_seek_index_hash_device: it wants no byte and is never too small); one
    clip, two clips, each with room and without"""
    yield total, None
    yield total - 1, None
    yield 0, []
    w = total - 2
    for room in (w, w - 1):
        yield 0, [(2, total, room)]
    for ra, rb in itertools.product((4, 3), (3, 2)):
        yield 0, [(0, 4, ra), (total - 3, 10, rb)]


def every_case():
    for n in (1, 2, 3):
        total = sum(SIZES[:n])
        fails = [None] + [(p, st) for p in range(n) for st in (BLOCK_ERR, UNSUPPORTED)]
        verifies = [(False, 0, None), (True, 0, None), (True, n - 1 if n != 2 else 0, n - 1 if n != 2 else 0), (True, None, None)]
        for fail, walk, dic, (cap, clips) in itertools.product(fails, (0, WALK_ERR), (False, True), modes(total)):
            promises = (None,) if clips is None else (None, total)
            for promise in promises:
                wrongs = [None] + list(range(n)) + (["promise"] if promise is not None else [])
                for wrong, (verify, mismatch, unhashed) in itertools.product(wrongs, verifies):
                    fr = frames_of(n, wrong if wrong != "promise" else None, mismatch, unhashed)
                    compared = sum(1 for f in fr if f["hashed"])
                    recs = [None] if clips is None else [None, (n, n, compared, 0, NO_ROW, 0, 0, 0), (n, n, compared, 1, 1, 0, 0, 0),
                                                         (n, n - 1, min(compared, n - 1), 0, NO_ROW, 0, 0, 0), (n, n, 0, 0, NO_ROW, 0, 1, 0),
                                                         (0, 0, 0, 0, 0, 21, 0, 0)]
                    for rec in recs:
                        yield Case(fr, fail, walk, dic, cap, clips, promise + 1 if wrong == "promise" else promise, verify, False, rec)


def alone_cases():
    for n in (1, 2, 3):
        total = sum(SIZES[:n])
        for (cap, clips), no_hash, known, verify in itertools.product(modes(total), (False, True), (True, False), (False, True)):
            if no_hash and verify:
                continue                                          # (the call refuses the two together)
            for wrong in (None, n - 1):
                fr = frames_of(n, wrong, mismatch=0)              # the host hashed every frame
                rec = None if clips is None else (n, n if known else 0, n if known else 0, 0, NO_ROW, 0, 0, 0)   # (nothing vouches for frames that are not known)
                yield Case(fr, cap=cap, clips=clips, verify=verify, no_hash=no_hash, rec=rec, known=known, counted=n + 1, bound_buffer=clips is not None)
            if clips is not None:                                 # the decoder itself ran out of a buffer that holds the selection's bound
                yield Case(frames_of(n), cap=cap, clips=clips, bound_buffer=True, decode=TOO_SMALL, known=known, counted=n)
                yield Case(frames_of(n), cap=cap, clips=clips, bound_buffer=True, decode=BLOCK_ERR, known=known, counted=n)


def run_cases(L, cases, hash_max=0):
    blob = b"".join(c.pack() for c in cases)
    words = sum(KOUT + 2 * len(c.clips or []) for c in cases)
    out = (C.c_uint64 * words)()
    assert L.ze_settle(blob, len(cases), hash_max, out) == len(blob)
    got, at = [], 0
    for c in cases:
        k = KOUT + 2 * len(c.clips or [])
        got.append(out[at:at + k])
        at += k
    return blob, got


def check(cases, got):
    seen = set()
    for c, g in zip(cases, got):
        want, clipped = c.expect()
        g = [x - 2 ** 64 if i == 0 and x >= 2 ** 63 else x for i, x in enumerate(g)]
        what = (c.frames, c.fail, c.walk, c.dict, c.cap, c.clips, c.promise, c.verify, c.no_hash, c.rec, c.known)
        if want is None:
            assert g[11] == 1, what
        else:
            assert g[:12] == want, (what, g, want)
        if clipped is not None:
            assert [tuple(g[KOUT + 2 * q:KOUT + 2 * q + 2]) for q in range(len(clipped))] == clipped, (what, g, clipped)
        seen.add(g[0] if want is not None else "call")
    return seen


def test_every_verdict_against_the_header(built):
    L = built[0]
    cases = list(every_case())
    _, got = run_cases(L, cases)
    assert check(cases, got) == {0, BLOCK_ERR, UNSUPPORTED, WALK_ERR, TOO_SMALL, SIZE_MISMATCH, CHECKSUM, SEEK_CHECKSUM, "call"}
    alone = list(alone_cases())
    _, got = run_cases(L, alone)
    assert check(alone, got) >= {0, BLOCK_ERR, TOO_SMALL, SIZE_MISMATCH, CHECKSUM, SEEK_CHECKSUM}
    # the compare list of an entry decoded alone: a frame longer than a nonzero hash_max_bytes is listed unhashed, one of 2^32 compressed bytes is left out
    c = Case(frames_of(3), cap=0, clips=[(0, 4, 4)], rec=(3, 3, 2, 0, NO_ROW, 0, 0, 0))
    _, got = run_cases(L, [c], hash_max=5)
    assert got[0][12:14] == [3, 2] and got[0][0] == 0
    blob = bytearray(c.pack())
    struct.pack_into("<Q", blob, 56 + 48 + 8, 1 << 32)            # frame 1's compressed length
    out = (C.c_uint64 * (KOUT + 2))()
    assert L.ze_settle(bytes(blob), 1, 0, out) == len(blob) and out[12:14] == [2, 2]


# ---- the pieces ------------------------------------------------------------------------------------------------------------------------------
def piece_cases():
    """(sizes, [spans of clips (skip, len, small)])"""
    for n in (1, 2, 3, 4):
        for sizes in itertools.product((0, 1, 2, 5), repeat=n):
            total = sum(sizes)
            pts = {0, total, total + 1, total + 3}
            for k in range(n + 1):
                b = sum(sizes[:k])
                pts |= {max(b - 1, 0), b, b + 1}
            pts = sorted(pts)
            clips = [(a, b - a, 0) for a in pts for b in pts if b >= a] + [(a, TOP, 0) for a in pts] + [(a, TOP - a, 0) for a in pts] + [(0, total, 1)]
            spans, at, k = [], 0, 0
            while at < len(clips):
                spans.append(clips[at:at + k % 4])
                at += k % 4
                k += 1
            yield sizes, spans


def test_pieces_against_slicing(built):
    L, exe, d = built
    fill, nclips = 0xEE, 0
    for sizes, spans in piece_cases():
        concat = bytes(range(1, sum(sizes) + 1))
        room = len(concat) + 2
        sz = (C.c_uint64 * len(sizes))(*sizes)
        for span in spans:
            flat = (C.c_uint64 * max(3 * len(span), 1))(*[x for cl in span for x in cl])
            dst = C.create_string_buffer(bytes([fill]) * (room * len(span) + 1), room * len(span) + 1)
            at = (C.c_uint64 * max(len(span), 1))()
            assert L.ze_pieces(sz, len(sizes), flat, len(span), dst, room, at) == 0, (sizes, span)
            for q, (skip, ln, small) in enumerate(span):
                want = b"" if small else concat[skip:skip + ln]
                assert at[q] == len(want) and dst.raw[q * room:(q + 1) * room] == want + bytes([fill]) * (room - len(want)), (sizes, span, q)
            assert dst.raw[-1] == fill
            nclips += len(span)
    assert nclips > 20000


def test_stand_alone_asan_program(built):
    L, exe, d = built
    cases = list(every_case())[::7] + list(alone_cases())
    _, got = run_cases(L, cases)
    blob = b"".join(struct.pack("<I", 1) + c.pack() for c in cases)
    want = b"".join(struct.pack("<%dQ" % len(g), *g) for g in got)
    for sizes, spans in itertools.islice(piece_cases(), 0, None, 5):
        concat = bytes(range(1, sum(sizes) + 1))
        for span in spans:
            blob += struct.pack("<3I", 2, len(sizes), len(span)) + struct.pack("<%dQ" % len(sizes), *sizes) + b"".join(struct.pack("<3Q", *cl) for cl in span)
            cut = [b"" if small else concat[skip:skip + ln] for skip, ln, small in span]
            want += struct.pack("<%dQ" % len(span), *[len(x) for x in cut]) + b"".join(cut)
    src, out = os.path.join(str(d), "cases.bin"), os.path.join(str(d), "records.bin")
    with open(src, "wb") as f:
        f.write(blob)
    lanesuite.run_stand_alone(exe, [src, out], b"entry_asan ok", 120)
    assert open(out, "rb").read() == want
