"""zg_k_seeksums' wave routine and the host form of its rule (zstd-rs_amd/csrc/zg_seeksums.h), compiled with g++ over the SIMT emulator
(tests/emu/zg_simt.h) and run on the CPU: 64 fibers, the ballots, shuffles and the prefix sum of the source as it is compiled for gfx950.
tests/emu/zg_emu_seeksums.cpp is the harness, built by tests/lanesuite.py. Every case runs over readers that count every access and every
access outside what the model (tests/seeksums.py) allows. Demanded of every case:
  - the wave's record equals the model's, field for field, and all 64 lanes hold the same record;
  - the host function's record equals it too (except where the model refuses the table frame's header: the host path does not fetch it);
  - no read of the entry outside the 9 footer bytes, the 8 bytes of the table frame's header and rows [first, first + taken); no access to
    the frame list outside the entry's slice; no digest read that the slice does not name; no access at all where nothing is taken.
Cases: taken in {0, 1, 2, 63, 64, 65, 128, 129} x first in {0, 1, 63, 64} (rows without a frame and unhashed frames among them, rows in front
and behind, decoy frames of other entries around the slice); the table at every alignment mod 16; a differing checksum at the first row, the
last row, lane 63 of a step and lane 0 of the next; a frame that coincides with no row because its length is off by one and because it spans
two rows; a table without checksums; a selection that leaves the table; a slot behind the digests; every single-byte edit of the 17 framing
bytes. The same cases run once more in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which every entry,
slice and digest array lies in a heap block of exactly its length."""
import ctypes as C
import random
import struct

import pytest

import lanesuite
import seeksums
import zgpu
from seeksums import FIELDS, NO_ROW, model

TAKEN, FIRST = (0, 1, 2, 63, 64, 65, 128, 129), (0, 1, 63, 64)
NOT_HASHED = 0xFFFFFFFF


class Case:
    """an entry (filler bytes in front of its table: the wave never reads them), the submit's frame list and digests, the entry's slice"""

    def __init__(self, name, rng, first, taken, extra=3, checksums=True, pad=0, plain=False):
        self.name, self.first, self.taken = name, first, taken
        nf = first + taken + extra
        self.cs = [rng.randint(5, 40) for _ in range(nf)]
        self.sums = [rng.getrandbits(32) for _ in range(nf)] if checksums else None
        self.digests = [rng.getrandbits(64) for _ in range(2)]            # two decoys in front: another entry's frames
        self.frames = [(0, self.cs[first] if taken else 7, 0), (self.cs[first] if taken else 9, 11, 1)]
        self.lo = 2
        at = 0
        for k in range(first, first + taken):
            if not plain and k % 14 == 3:
                self.cs[k] = 0                                            # an empty row
            if plain or k % 7 != 3:                                       # (every seventh row has no frame: a skippable one)
                if not plain and k % 11 == 5:
                    slot = None                                           # not hashed
                else:
                    slot = len(self.digests)
                    d = rng.getrandbits(64)
                    self.digests.append(d)
                    if checksums:
                        self.sums[k] = d & 0xFFFFFFFF
                self.frames.append((at, self.cs[k], slot))
            at += self.cs[k]
        self.n = len(self.frames) - self.lo
        self.frames += [(0, self.cs[first] if taken else 3, 0), (at, 5, 1)]   # and two behind
        self.front = bytes(rng.getrandbits(8) for _ in range(sum(self.cs) + pad))
        self.rebuild()

    def rebuild(self):
        self.table = zgpu.seek_table_frame(self.cs, [1] * len(self.cs), self.sums)
        self.entry = self.front + self.table
        return self

    def row(self, k):
        """selection row k as an index into the slice's frames, or None"""
        at = sum(self.cs[self.first:self.first + k])
        for i, f in enumerate(self.slice()):
            if f[0] == at:
                return i
        return None

    def slice(self):
        return self.frames[self.lo:self.lo + self.n]

    def want(self):
        return model(self.entry, self.first, self.taken, self.slice(), self.digests)


def cases():
    rng = random.Random(0x5EE5C5)
    out = []
    for taken in TAKEN:
        for first in FIRST:
            out.append(Case("t%d:f%d" % (taken, first), rng, first, taken))
    # the table at every alignment mod 16 (entries lie at 16-byte aligned addresses), two steps
    for a in range(16):
        c = Case("align%d" % a, random.Random(11), 1, 65)
        tab = len(c.entry) - len(c.table)
        out.append(Case("align%d" % a, random.Random(11), 1, 65, pad=(a - tab) % 16))
        assert (len(out[-1].entry) - len(out[-1].table)) % 16 == a
    # a differing checksum: the first row, the last row, lane 63 of a step and lane 0 of the next (every row has a hashed frame)
    for k in (0, 128, 63, 64):
        c = Case("differ:%d" % k, rng, 1, 129, plain=True)
        c.sums[1 + k] ^= 1 << rng.randrange(32)
        out.append(c.rebuild())
        assert c.want()[0][3:5] == (1, 1 + k)
    c = Case("differ:two", rng, 0, 70, plain=True)
    c.sums[69] ^= 4
    c.sums[5] ^= 8
    out.append(c.rebuild())
    assert c.want()[0][3:5] == (2, 5)
    # a decoded frame that coincides with no row: its length off by one; two rows merged into one frame
    c = Case("uncovered:off_by_one", rng, 2, 66, plain=True)
    i = c.lo + c.row(64)
    c.frames[i] = (c.frames[i][0], c.frames[i][1] + 1, c.frames[i][2])
    out.append(c)
    assert c.want()[0][:4] == (66, 65, 65, 0)
    c = Case("uncovered:merged", rng, 0, 10, plain=True)
    i = c.lo + c.row(4)
    c.frames[i] = (c.frames[i][0], c.frames[i][1] + c.frames[i + 1][1], c.frames[i][2])
    del c.frames[i + 1]
    c.n -= 1
    out.append(c)
    assert c.want()[0][:4] == (10, 8, 8, 0)
    # a table without checksums; one whose frames are all unhashed; a selection that leaves the table; a slot behind the digests; nothing there
    out.append(Case("no_checksums", rng, 1, 66, checksums=False))
    assert out[-1].want()[0][2] == 0 and out[-1].want()[0][6] == seeksums.NO_CHECKSUMS and out[-1].want()[0][1] > 50
    c = Case("all_unhashed", rng, 0, 5, plain=True)
    c.frames = [(b, n, None) for b, n, _ in c.frames]
    out.append(c)
    assert c.want()[0][:3] == (5, 5, 0)
    c = Case("leaves_table", rng, 3, 9, extra=0)
    c.taken += 1
    out.append(c)
    assert out[-1].want()[0][5] == seeksums.WHY_ROWS
    c = Case("bad_slot", rng, 0, 66, plain=True)
    i = c.lo + c.row(65)
    c.frames[i] = (c.frames[i][0], c.frames[i][1], len(c.digests))
    out.append(c)
    assert c.want()[0] == (0, 0, 0, 0, 0, seeksums.WHY_LIST, 0)
    c = Case("no_frames", rng, 0, 3, plain=True)
    c.n = 0
    out.append(c)
    assert c.want()[0][:3] == (3, 0, 0)
    c = Case("short_entry", rng, 0, 2, extra=0, plain=True)
    c.entry = c.entry[-16:]
    out.append(c)
    # every single-byte edit of the 17 framing bytes of one table: a why, or a record the model agrees with
    good = Case("edit", rng, 1, 3, extra=1, plain=True)
    n, tab = len(good.entry), len(good.entry) - len(good.table)
    for pos in list(range(tab, tab + 8)) + list(range(n - 9, n)):
        for v in range(256):
            if v != good.entry[pos]:
                c = Case.__new__(Case)
                c.__dict__.update(good.__dict__)
                c.name, c.entry = "edit:%d:%d" % (pos - tab, v), good.entry[:pos] + bytes([v]) + good.entry[pos + 1:]
                out.append(c)
    return out


def _declare(L):
    L.zgemu_seeksums.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                 C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.zgemu_seeksums.restype = C.c_uint32


built = lanesuite.built_fixture("zg_emu_seeksums.cpp", "seeksums", "SEEKSUMS_MAIN", declare=_declare)


@pytest.fixture(scope="module")
def expected():
    """[(case, record, windows)]: the model, computed once"""
    return [(c,) + c.want() for c in cases()]


def _packed_frames(frames):
    return b"".join(struct.pack("<QII", b, n, NOT_HASHED if s is None else s) for b, n, s in frames)


def _records(raw, at):
    return struct.unpack_from("<7I", raw, at), struct.unpack_from("<7I", raw, at + 32)


def _host_agrees(host, rec):
    """the host path reads the footer and the rows, not the table frame's header: what the header check refuses it answers from the footer"""
    return host == rec or rec[5] == zgpu.SEEKTAB_BAD_FRAME


def test_seeksums_equals_the_model_and_stays_inside_its_windows(built, expected):
    L, _, _ = built
    whys, seen = set(), {"differ": 0, "uncovered": 0, "unhashed": 0, "rowless": 0, "nothing": 0}
    for c, rec, win in expected:
        buf, at = lanesuite.aligned_copy(c.entry)
        fbuf, fat = lanesuite.aligned_copy(_packed_frames(c.frames))
        dig = (C.c_uint64 * max(len(c.digests), 1))(*c.digests)
        w = (C.c_uint64 * 6)(*[x for lo_hi in win for x in lo_hi] + [0] * (6 - 2 * len(win)))
        out, counts = C.create_string_buffer(64), (C.c_uint64 * 4)()
        bad = L.zgemu_seeksums(at, len(c.entry), c.first, c.taken, fat, len(c.frames), c.lo, c.n, dig,
                               len(c.digests), w, len(win), out, counts)
        assert bad == 0, (c.name, "lanes of a wave disagree")
        got, host = _records(out.raw, 0)
        assert got == rec, (c.name, dict(zip(FIELDS, got)), dict(zip(FIELDS, rec)))
        assert _host_agrees(host, rec), (c.name, dict(zip(FIELDS, host)), dict(zip(FIELDS, rec)))
        assert tuple(counts[1:]) == (0, 0, 0), (c.name, "reads outside the windows / the slice / the named digests", tuple(counts))
        if not win:
            assert counts[0] == 0, (c.name, "nothing taken, or an entry below 17 bytes, reads nothing")
        whys.add(rec[5])
        if not rec[5] and c.taken:
            seen["differ"] += rec[3] > 0
            seen["uncovered"] += rec[1] < c.n
            seen["unhashed"] += rec[2] < rec[1] and not rec[6]
            seen["rowless"] += rec[1] < rec[0]
        seen["nothing"] += not win
    assert whys >= {0, 16, 17, 18, 19, 21, 22}, whys
    assert seen["differ"] >= 5 and seen["uncovered"] >= 2 and seen["unhashed"] > 10 and seen["rowless"] > 10 and seen["nothing"] >= 5, seen
    assert len(expected) > 4000


def test_seeksums_pinned_example(built):
    """rows (c, checksum): a frame, a skippable frame, a frame, an unhashed frame; rows 1 .. 4 of a table of 6 are the selection"""
    cs, sums = [9, 10, 8, 30, 5, 7], [1, 0xAAAA0001, 3, 0xAAAA0003, 0xAAAA0004, 6]
    e = bytes(69) + zgpu.seek_table_frame(cs, [4] * 6, sums)
    frames = [(0, 10, 0), (18, 30, 1), (48, 5, None)]
    tab = 69
    assert model(e, 1, 4, frames, [0x55AAAA0001, 0x77AAAA0003]) == ((4, 3, 2, 0, NO_ROW, 0, 0), [(len(e) - 9, len(e)), (tab, tab + 8), (tab + 20, tab + 68)])
    assert model(e, 1, 4, frames, [0x55AAAA0001, 0x77AAAA0002])[0] == (4, 3, 2, 1, 3, 0, 0)
    assert seeksums.vouched((4, 3, 2, 0, NO_ROW, 0, 0), 3) and not seeksums.vouched((4, 3, 2, 0, NO_ROW, 0, 0), 4)
    assert not seeksums.vouched((4, 3, 2, 1, 3, 0, 0), 3) and not seeksums.vouched((4, 3, 0, 0, NO_ROW, 0, 1), 3)
    assert seeksums.failed_counts((4, 3, 2, 1, 3, 0, 0), 3) == (2, 1, 1)
    assert model(e, 0, 0, frames, [])[0] == seeksums.ZERO and model(e, 3, 4, frames, [])[0][5] == seeksums.WHY_ROWS


def test_seeksums_under_address_sanitizer_stand_alone(built, expected):
    _, exe, d = built
    src, dst = d / "cases.bin", d / "records.bin"
    with open(src, "wb") as f:
        for c, _, _ in expected:
            f.write(struct.pack("<QIIII", len(c.entry), c.first, c.taken, c.n, len(c.digests)) + _packed_frames(c.slice()) +
                    b"".join(struct.pack("<Q", x) for x in c.digests) + c.entry)
    lanesuite.run_stand_alone(exe, [src, dst], b"seeksums_asan ok", timeout=900)
    recs = open(dst, "rb").read()
    assert len(recs) == 64 * len(expected)
    for i, (c, rec, _) in enumerate(expected):
        got, host = _records(recs, 64 * i)
        assert got == rec and _host_agrees(host, rec), (c.name, got, host, rec)


def test_verify_table_argument_rules_need_no_gpu():
    n = 1
    srcs, lens, dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    rg, res, dres = (zgpu.RangeC * n)(), (zgpu.RangeResultC * n)(), (zgpu.DeviceEntryResultC * n)()
    fake = C.create_string_buffer(4096)   # (not a context: the calls below are refused before the context is looked at)
    assert (zgpu.DEVICE_NO_HASH, zgpu.DEVICE_VERIFY, zgpu.DEVICE_VERIFY_SEEK_TABLE, zgpu.E_SEEK_CHECKSUM_MISMATCH) == (1, 2, 4, 73)
    for dev in (False, True):
        L = zgpu.load_library(dev=dev)
        assert L.zgpu_status_name(73) == b"SeekChecksumMismatch"
        for flags in (4, 6):
            opts = zgpu.DeviceOptsC(0, flags, 0)
            # bit 2 on the calls that have no seek table
            assert L.zgpu_decode_frames_device(fake, srcs, lens, n, dsts, caps, C.byref(opts), dres) == zgpu.E_BAD_ARG
            assert L.zgpu_decode_frames_device_src(fake, srcs, lens, n, dsts, caps, C.byref(opts), dres) == zgpu.E_BAD_ARG
            assert L.zgpu_decode_ranges_device_src(fake, srcs, lens, n, rg, dsts, caps, C.byref(opts), res) == zgpu.E_BAD_ARG
        # bit 2 with bit 0 (hash nothing, verify everything)
        for flags in (5, 7):
            opts = zgpu.DeviceOptsC(0, flags, 0)
            assert L.zgpu_decode_ranges_seek_table_device_src(fake, srcs, lens, n, rg, dsts, caps, C.byref(opts), res) == zgpu.E_BAD_ARG
        out = (C.c_uint64 * 16)(*([7] * 16))
        assert L.zgpu_debug_ranges_stats(None, out, 13) == 0
    import inspect
    assert inspect.signature(zgpu.Context.decode_tensor_ranges).parameters["verify_table"].default is False
    assert inspect.signature(zgpu.Context.decode_ranges_seek_table_device_src).parameters["verify_table"].default is False
    assert inspect.signature(zgpu.Context.ranges_stats).parameters["verify_table"].default is False
    assert zgpu._opts(0, False, True, True).flags == 6 and zgpu._opts(5, True, False).flags == 1
    keys = zgpu._STATS["Context.ranges_stats"][2]
    assert keys[8:] == ("compare_launches", "compare_us", "compare_bytes_downloaded", "frames_compared", "entries_failed_table") and len(keys) == 13
