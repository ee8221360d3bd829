"""zg_k_idxsums' wave routine and the host form of its rule (zstd-rs_amd/csrc/zg_idxsums.h), compiled with g++ over the SIMT emulator
(tests/emu/zg_simt.h) and run on the CPU: 64 fibers and the ballots of the source as it is compiled for gfx950. tests/emu/zg_emu_idxsums.cpp
is the harness, built by tests/lanesuite.py. Every case runs over readers that count every access and every access outside what the model
(tests/idxsums.py) allows. Demanded of every case:
  - the wave's record equals the model's, field for field, and all 64 lanes hold the same record;
  - the host function's record (zgh::sums_pairs, the rule of the groups decoded alone) equals it too;
  - no read of the handle's pairs outside rows [first, first + taken] of the entry, none of its sums outside rows [first, first + taken); no
    access to the frame list outside the group's slice; no digest read that the slice does not name; no access at all where nothing is taken
    or the group leaves the entry.
The entry lies between two other entries' rows in the handle's arrays, and the rows in front of and behind the group hold poison sums.
Cases: taken in {1, 63, 64, 65, 128, 129} x first in {0, 1, 63, 64} (skippable rows at the front, between frames and at the end of a step,
unhashed frames, decoy frames of other groups around the slice); a differing sum in lane 0, in lane 63 and in the second step; a frame
whose begin matches and whose length does not; a frame between two rows; a frame left out of the list; a slot at the digest count; a group
that leaves the entry; nothing taken. The same cases run once more in a stand-alone AddressSanitizer program (its own main, no Python in
the process) in which the pairs and sums the wave may read, the slice and the digests each lie in a heap block of exactly their length.
One rule behind both routes: every case of test_seeksums_cpu's list whose table is accepted and carries checksums runs through this routine
as well, its rows turned into pairs and sums, and both records must equal the table route's."""
import ctypes as C
import random
import struct

import pytest

import idxsums
import lanesuite
import test_seeksums_cpu as table_suite
from idxsums import FIELDS, NO_ROW, model

TAKEN, FIRST = (1, 63, 64, 65, 128, 129), (0, 1, 63, 64)
NOT_HASHED = 0xFFFFFFFF
POISON = 0xDEADBEEF


class Case:
    """an entry's pairs and sums (between two neighbours' in the handle's arrays), the submit's frame list and digests, the group's slice"""

    def __init__(self, name, rng, first, taken, extra=3, plain=False):
        self.name, self.first, self.taken = name, first, taken
        n = self.nrows = first + taken + extra
        cs = [rng.randint(12, 40) for _ in range(n)]
        ds = [rng.randint(1, 90) for _ in range(n)]
        self.sums = [POISON ^ k for k in range(n)]                        # (rows outside the group keep these)
        self.digests = [rng.getrandbits(64) for _ in range(2)]            # two decoys in front: another group's frames
        self.frames = [(0, cs[first] if taken else 7, 0), (cs[first] if taken else 9, 11, 1)]
        self.lo = 2
        at = 0
        for k in range(first, first + taken):
            skippable = not plain and (k - first) % 64 in (0, 7, 63)      # the front, between frames, the end of a step
            if skippable:
                ds[k], self.sums[k] = 0, 0
            else:
                if not plain and k % 11 == 5:
                    slot = None                                           # not hashed
                else:
                    slot = len(self.digests)
                    d = rng.getrandbits(64)
                    self.digests.append(d)
                    self.sums[k] = d & 0xFFFFFFFF
                self.frames.append((at, cs[k], slot))
            at += cs[k]
        self.n = len(self.frames) - self.lo
        self.frames += [(0, cs[first] if taken else 3, 0), (at, 5, 1)]    # and two behind
        self.C, self.D = [1000], [77]                                     # (prefix sums need not begin at 0 for the rule: only differences count)
        for c, d in zip(cs, ds):
            self.C.append(self.C[-1] + c)
            self.D.append(self.D[-1] + d)
        self.front, self.back = rng.randint(1, 5), rng.randint(1, 5)      # rows of the neighbours in the arrays

    def row(self, k):
        """group row k (0-based in the group) as an index into the slice's frames, or None"""
        at = self.C[self.first + k] - self.C[self.first]
        for i, f in enumerate(self.slice()):
            if f[0] == at:
                return i
        return None

    def slice(self):
        return self.frames[self.lo:self.lo + self.n]

    def want(self):
        return model(self.C, self.sums, self.first, self.taken, self.slice(), self.digests)

    def arrays(self):
        """(pairs bytes, sums bytes, pair0, sum0): the handle's arrays with a neighbour on each side"""
        pairs = [(5, 5)] * (self.front + 1) + list(zip(self.C, self.D)) + [(9, 9)] * (self.back + 1)
        sums = [POISON] * self.front + self.sums + [POISON] * self.back
        return (b"".join(struct.pack("<QQ", c, d) for c, d in pairs), struct.pack("<%dI" % len(sums), *sums), self.front + 1, self.front)


def cases():
    rng = random.Random(0x1D5C5)
    out = []
    for taken in TAKEN:
        for first in FIRST:
            out.append(Case("t%d:f%d" % (taken, first), rng, first, taken))
            out.append(Case("plain:t%d:f%d" % (taken, first), rng, first, taken, plain=True))
            assert out[-1].want()[0][:4] == (taken, taken, taken, 0)
    # a differing sum: lane 0, lane 63, the second step (every row has a hashed frame)
    for k in (0, 63, 64, 128):
        c = Case("differ:%d" % k, rng, 1, 129, plain=True)
        c.sums[1 + k] ^= 1 << rng.randrange(32)
        out.append(c)
        assert c.want()[0][3:5] == (1, 1 + k)
    c = Case("differ:two", rng, 0, 70, plain=True)
    c.sums[69] ^= 4
    c.sums[5] ^= 8
    out.append(c)
    assert c.want()[0][3:5] == (2, 5)
    # a frame whose begin matches and whose length does not; a frame between two rows; a frame left out of the list
    c = Case("uncovered:length", rng, 2, 66, plain=True)
    i = c.lo + c.row(64)
    c.frames[i] = (c.frames[i][0], c.frames[i][1] + 1, c.frames[i][2])
    out.append(c)
    assert c.want()[0][:4] == (66, 65, 65, 0)
    c = Case("uncovered:between", rng, 0, 10, plain=True)
    i = c.lo + c.row(4)
    c.frames[i] = (c.frames[i][0] + 3, c.frames[i][1] - 3, c.frames[i][2])
    out.append(c)
    assert c.want()[0][:4] == (10, 9, 9, 0)
    c = Case("left_out", rng, 63, 65, plain=True)
    del c.frames[c.lo + c.row(1)]
    c.n -= 1
    out.append(c)
    assert c.want()[0][:4] == (65, 64, 64, 0)
    # all unhashed; a slot at the digest count; a group that leaves the entry; nothing taken; no frames
    c = Case("all_unhashed", rng, 0, 5, plain=True)
    c.frames = [(b, n, None) for b, n, _ in c.frames]
    out.append(c)
    assert c.want()[0][:3] == (5, 5, 0)
    c = Case("bad_slot", rng, 0, 66, plain=True)
    i = c.lo + c.row(65)
    c.frames[i] = (c.frames[i][0], c.frames[i][1], len(c.digests))
    out.append(c)
    assert c.want()[0] == (0, 0, 0, 0, 0, idxsums.WHY_LIST, 0)
    for first, taken in ((3, 9), (0, 1), (64, 64)):
        c = Case("leaves_entry:%d:%d" % (first, taken), rng, first, taken, extra=0)
        c.taken += 1
        out.append(c)
        assert c.want() == ((0, 0, 0, 0, 0, idxsums.WHY_ROWS, 0), None, None)
    for first in FIRST:
        c = Case("nothing:f%d" % first, rng, first, 0)
        out.append(c)
        assert c.want() == (idxsums.ZERO, None, None)
    c = Case("no_frames", rng, 0, 3, plain=True)
    c.n = 0
    out.append(c)
    assert c.want()[0][:3] == (3, 0, 0)
    return out


def _declare(L):
    L.zgemu_idxsums.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.zgemu_idxsums.restype = C.c_uint32


built = lanesuite.built_fixture("zg_emu_idxsums.cpp", "idxsums", "IDXSUMS_MAIN", declare=_declare)


table_built = table_suite.built   # the table route's harness (lanesuite builds a harness once per session)


@pytest.fixture(scope="module")
def expected():
    """[(case, record, pair window, sum window)]: the model, computed once"""
    return [(c,) + c.want() for c in cases()]


def _packed_frames(frames):
    return b"".join(struct.pack("<QII", b, n, NOT_HASHED if s is None else s) for b, n, s in frames)


def _records(raw, at):
    return struct.unpack_from("<7I", raw, at), struct.unpack_from("<7I", raw, at + 32)


def test_idxsums_equals_the_model_and_stays_inside_its_windows(built, expected):
    L, _, _ = built
    whys, seen = set(), {"differ": 0, "uncovered": 0, "unhashed": 0, "rowless": 0, "nothing": 0}
    for c, rec, pw, sw in expected:
        pairs, sums, pair0, sum0 = c.arrays()
        pbuf, pat = lanesuite.aligned_copy(pairs)
        sbuf, sat = lanesuite.aligned_copy(sums)
        fbuf, fat = lanesuite.aligned_copy(_packed_frames(c.frames))
        dig = (C.c_uint64 * max(len(c.digests), 1))(*c.digests)
        win = (C.c_uint64 * 4)(*([pair0 + pw[0], pair0 + pw[1], sum0 + sw[0], sum0 + sw[1]] if pw else [0, 0, 0, 0]))
        out, counts = C.create_string_buffer(64), (C.c_uint64 * 5)()
        bad = L.zgemu_idxsums(pat, sat, pair0, sum0, c.nrows, c.first, c.taken, fat, c.lo, c.n, dig, len(c.digests), win, out, counts)
        assert bad == 0, (c.name, "lanes of a wave disagree")
        got, host = _records(out.raw, 0)
        assert got == rec, (c.name, dict(zip(FIELDS, got)), dict(zip(FIELDS, rec)))
        assert host == rec, (c.name, dict(zip(FIELDS, host)), dict(zip(FIELDS, rec)))
        assert tuple(counts[1:]) == (0, 0, 0, 0), (c.name, "reads outside the rows / the slice / the named digests", tuple(counts))
        if pw is None:
            assert counts[0] == 0, (c.name, "nothing taken, or a group that leaves its entry, reads nothing of the handle")
        else:
            assert counts[0] > 0
        whys.add(rec[5])
        if not rec[5] and c.taken:
            seen["differ"] += rec[3] > 0
            seen["uncovered"] += rec[1] < c.n
            seen["unhashed"] += rec[2] < rec[1]
            seen["rowless"] += rec[1] < rec[0]
        seen["nothing"] += pw is None
    assert whys == {0, idxsums.WHY_ROWS, idxsums.WHY_LIST}, whys
    assert seen["differ"] >= 5 and seen["uncovered"] >= 2 and seen["unhashed"] > 10 and seen["rowless"] > 10 and seen["nothing"] >= 7, seen


def test_both_routes_apply_one_rule(built, table_built):
    """The rule is written once (zgv::sums_step / zgv::Tally for the waves, zgv::sums_host for the hosts). Every case of the table suite whose
    table the wave accepts (no why of zg_seektab.h's) and that carries checksums: the rows become a handle's pairs (C[k] = the running sum of
    c) and sums, and the handle route's wave and host function give the table route's record for the same frames and digests, all eight
    fields — a selection that leaves the rows (kRows) and a slot behind the digests (kList) included."""
    L, T = built[0], table_built[0]
    ran, whys = 0, set()
    for c in table_suite.cases():
        e, n = c.entry, len(c.entry)
        buf, at = lanesuite.aligned_copy(e)
        fbuf, fat = lanesuite.aligned_copy(_packed_frames(c.frames))
        dig = (C.c_uint64 * max(len(c.digests), 1))(*c.digests)
        out, counts = C.create_string_buffer(64), (C.c_uint64 * 5)()
        open_win = (C.c_uint64 * 6)(0, n, 0, 0, 0, 0)
        assert T.zgemu_seeksums(at, n, c.first, c.taken, fat, len(c.frames), c.lo, c.n, dig, len(c.digests), open_win, 1, out, counts) == 0
        table = struct.unpack_from("<8I", out.raw, 0)
        if table[5] in (16, 17, 18, 19) or table[6]:   # a table the wave refuses; one without checksums
            continue
        nf, es = struct.unpack_from("<I", e, n - 9)[0], 12
        assert e[n - 5] & 0x80 and n >= nf * es + 17
        rows = [struct.unpack_from("<III", e, n - 9 - (nf - k) * es) for k in range(nf)]
        cs = [0]
        for r in rows:
            cs.append(cs[-1] + r[0])
        pbuf, pat = lanesuite.aligned_copy(b"".join(struct.pack("<QQ", x, 0) for x in cs))
        sbuf, sat = lanesuite.aligned_copy(struct.pack("<%dI" % max(nf, 1), *([r[2] for r in rows] or [0])))
        win = (C.c_uint64 * 4)(0, nf + 1, 0, nf)
        assert L.zgemu_idxsums(pat, sat, 0, 0, nf, c.first, c.taken, fat, c.lo, c.n, dig, len(c.digests), win, out, counts) == 0
        wave, host = struct.unpack_from("<8I", out.raw, 0), struct.unpack_from("<8I", out.raw, 32)
        assert wave == table and host == table, (c.name, dict(zip(FIELDS, wave)), dict(zip(FIELDS, host)), dict(zip(FIELDS, table)))
        ran += 1
        whys.add(table[5])
    # (the 32 taken x first cases, 16 alignments, 5 + 2 + 1 differing / uncovered / unhashed, the selection that leaves the table, the bad slot
    # and the empty slice: 59; the edits of the 17 framing bytes that leave the table acceptable come on top)
    assert ran >= 59 and whys == {0, idxsums.WHY_ROWS, idxsums.WHY_LIST}, (ran, whys)


def test_idxsums_pinned_example():
    """rows (c, sum): a frame, a skippable row, a frame, an unhashed frame; rows 1 .. 4 of an entry of 6 are the group"""
    C_, sums = [0, 9, 19, 27, 57, 62, 69], [1, 0xAAAA0001, 0, 0xAAAA0003, 0xAAAA0004, 6]
    frames = [(0, 10, 0), (18, 30, 1), (48, 5, None)]
    assert model(C_, sums, 1, 4, frames, [0x55AAAA0001, 0x77AAAA0003]) == ((4, 3, 2, 0, NO_ROW, 0, 0), (1, 6), (1, 5))
    assert model(C_, sums, 1, 4, frames, [0x55AAAA0001, 0x77AAAA0002])[0] == (4, 3, 2, 1, 3, 0, 0)
    assert idxsums.vouched((4, 3, 2, 0, NO_ROW, 0, 0), 3) and not idxsums.vouched((4, 3, 2, 0, NO_ROW, 0, 0), 4)
    assert idxsums.failed_counts((4, 3, 2, 1, 3, 0, 0), 3) == (2, 1, 1)
    assert model(C_, sums, 0, 0, frames, [])[0] == idxsums.ZERO and model(C_, sums, 3, 4, frames, [])[0][5] == idxsums.WHY_ROWS


def test_idxsums_under_address_sanitizer_stand_alone(built, expected):
    _, exe, d = built
    src, dst = d / "cases.bin", d / "records.bin"
    with open(src, "wb") as f:
        for c, _, pw, _ in expected:
            held = pw is not None
            f.write(struct.pack("<6I", c.nrows, c.first, c.taken, c.n, len(c.digests), int(held)) + _packed_frames(c.slice()) +
                    b"".join(struct.pack("<Q", x) for x in c.digests))
            if held:
                f.write(b"".join(struct.pack("<QQ", c.C[k], c.D[k]) for k in range(c.first, c.first + c.taken + 1)) +
                        struct.pack("<%dI" % c.taken, *c.sums[c.first:c.first + c.taken]))
    lanesuite.run_stand_alone(exe, [src, dst], b"idxsums_asan ok", timeout=300)
    recs = open(dst, "rb").read()
    assert len(recs) == 64 * len(expected)
    for i, (c, rec, _, _) in enumerate(expected):
        got, host = _records(recs, 64 * i)
        assert got == rec and host == rec, (c.name, got, host, rec)
