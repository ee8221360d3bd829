"""tests/framesuite.py's own test. Six suites rest on one lockstep(), so each of its assertions is shown to fire: it runs with the
oracle's FrameDecoder on both sides, through an adapter with zgpu.FrameDecoder's method names, and then with adapters that each
falsify one thing. The pure helpers run on tiny cases each."""
import pytest

import framesuite
import oracle

MAGIC = bytes.fromhex("28b52ffd")
PLAIN = b"abcdefghijkl"
# descriptor 0x04 (a content checksum), window byte 0; three raw blocks of 5, 3 and 4 bytes, the third the last; XXH64(PLAIN) & 0xFFFFFFFF
GOOD = MAGIC + b"\x04\x00" + b"\x28\x00\x00abcde" + b"\x18\x00\x00fgh" + b"\x21\x00\x00ijkl" + bytes.fromhex("b3d433a2")
# the same first block, then a block of the reserved type 3: the oracle's status 20
RESERVED = MAGIC + b"\x04\x00" + b"\x28\x00\x00abcde" + b"\x06\x00\x00" + b"\x21\x00\x00ijkl"


class Adapter:
    """oracle.FrameDecoder under zgpu.FrameDecoder's method names; `wrong` names the one thing it reports falsely"""
    wrong = None

    def __init__(self, _ctx):
        self.o, self.calls = oracle.FrameDecoder(), 0

    def reset(self, z):
        return self.o.init(z)

    def decode_blocks(self, src, strat, n):
        st, used, fin = self.o.decode_blocks(src, strat, n)
        self.calls += 1
        if self.calls == 2:
            st, used, fin = st + (self.wrong == "status"), used + (self.wrong == "used"), fin != (self.wrong == "fin")
        return st, used, fin

    def blocks_decoded(self):
        return self.o.blocks_decoded() + (self.wrong == "blocks_decoded")

    def bytes_read_from_source(self):
        return self.o.bytes_read_from_source() + (self.wrong == "bytes_read_from_source")

    def can_collect(self):
        return self.o.can_collect() + (self.wrong == "can_collect")

    def collect(self):
        got = self.o.collect()
        return got[:-1] + bytes([got[-1] ^ 1]) if got and self.wrong == "collect" else got

    def is_finished(self):
        return self.o.is_finished()

    def get_calculated_checksum(self):
        return self.o.calculated_checksum() ^ (self.wrong == "checksum")

    def close(self):
        pass


def test_lockstep_passes_on_equal_decoders():
    assert framesuite.lockstep(None, "good", GOOD, header=(0, 6), decoder=Adapter) == (0, PLAIN, 3)
    assert framesuite.lockstep(None, "good", GOOD, k=2, decoder=Adapter) == (0, PLAIN, 2)
    assert framesuite.lockstep(None, "reserved", RESERVED, decoder=Adapter) == (20, b"", 2)
    with pytest.raises(AssertionError):
        framesuite.lockstep(None, "good", GOOD, header=(0, 5), decoder=Adapter)


@pytest.mark.parametrize("wrong", ["status", "used", "fin", "blocks_decoded", "bytes_read_from_source", "can_collect", "collect", "checksum"])
def test_lockstep_catches(wrong):
    """an adapter that differs from the oracle in one thing (the status, used and fin of the second call; a counter, can_collect,
    the last byte collected, the checksum) fails the comparison"""
    broken = type("Broken", (Adapter,), {"wrong": wrong})
    with pytest.raises(AssertionError):
        framesuite.lockstep(None, "good", GOOD, decoder=broken)


def test_interleave():
    v, four, one = ["v%d" % i for i in range(7)], ["i0", "i1", "i2", "i3"], ["i0"]
    assert framesuite.interleave(v, four, 2) == ["v0", "v1", "i0", "v2", "v3", "i1", "v4", "v5", "i2", "v6", "i3"]
    assert framesuite.interleave(v, four, 3) == ["v0", "v1", "v2", "i0", "v3", "v4", "v5", "i1", "v6", "i2", "i3"]
    assert framesuite.interleave(v, four, 5) == ["v0", "v1", "v2", "v3", "v4", "i0", "v5", "v6", "i1", "i2", "i3"]
    assert framesuite.interleave(v, one, 2) == ["v0", "v1", "i0", "v2", "v3", "v4", "v5", "v6"]
    assert framesuite.interleave(v, one, 3) == ["v0", "v1", "v2", "i0", "v3", "v4", "v5", "v6"]
    assert framesuite.interleave(v, one, 5) == ["v0", "v1", "v2", "v3", "v4", "i0", "v5", "v6"]
    assert framesuite.interleave(v, [], 2) == v and framesuite.interleave([], four, 2) == four


def test_raw_block_in_front():
    z = framesuite.raw_block_in_front(RESERVED)
    assert z == RESERVED[:6] + b"\x40\x06\x00" + bytes(range(200)) + RESERVED[6:]
    assert framesuite.lockstep(None, "reserved", z, header=(0, 6), decoder=Adapter) == (20, b"", 3)
    with pytest.raises(AssertionError):
        framesuite.raw_block_in_front(MAGIC + b"\x24\x00" + RESERVED[6:])


def test_defines(tmp_path):
    src = tmp_path / "k.h"
    src.write_text("#define ZG_A 12\n#define  ZG_B\t7   // seven\n#define ZG_C (3 * ZG_A)\n")
    assert framesuite.defines(src, ("ZG_A", "ZG_B")) == {"ZG_A": 12, "ZG_B": 7}
    for missing in ("ZG_C", "ZG_D"):                     # not a plain number; not there
        with pytest.raises(AssertionError):
            framesuite.defines(src, ("ZG_A", missing))


def test_families():
    built, seen = [], []

    def fam(name, frames):
        return lambda: built.append(name) or frames

    f = framesuite.Families({"a": fam("a", [("a0", b"z0", b"p0"), ("a1", b"z1", None)]), "b": fam("b", [("b0", b"z2", b"")])}, seen.append)
    assert f.family("b") == [("b0", b"z2", b"")] and built == ["b"]
    frames = f.all_frames()
    assert frames == [("a", "a0", b"z0", b"p0"), ("a", "a1", b"z1", None), ("b", "b0", b"z2", b"")]
    assert f.valid_frames() == [frames[0], frames[2]] and f.invalid_frames() == [frames[1]]
    assert built == ["b", "a"] and seen == [frames] * 3            # built once; the check ran on every whole set
    twice = framesuite.Families({"a": fam("a", [("x", b"", b"")]), "b": fam("b", [("x", b"", b"")])})
    assert twice.family("a") and twice.family("b")
    with pytest.raises(AssertionError, match="frame names repeat"):
        twice.all_frames()


class _Info:
    def __init__(self, status, bad_block, out_size):
        self.status, self.bad_block, self.out_size = status, bad_block, out_size


class FakeContext:
    """prepare() gives a batch that reports `table`: per frame (status, bad_block, bytes); lit_direct() reports `late`"""

    def __init__(self, table, late=True, parse_status=0):
        self.table, self.late, self.parse_status = table, late, parse_status

    def prepare(self, src):
        return FakeBatch(self)


class FakeBatch:
    def __init__(self, c):
        self.c, self.parse_status, self.nframes = c, c.parse_status, len(c.table)

    def run(self):
        pass

    sync = close = run

    def lit_direct(self):
        return self.c.late

    def frame_info(self, f):
        st, at, data = self.c.table[f]
        return _Info(st, at, len(data))

    def frame_bytes(self, f):
        return self.c.table[f][2]


def test_submit_verdicts():
    """the one-submit check of invalid among valid frames passes on what the oracle says and fails on one wrong status, failing
    block, size or byte, on a valid frame with a status or other bytes, on a walk that stopped, and on the other literals path"""
    frames = [("f", "v0", b"z", b"plain"), ("f", "i0", b"z", None), ("v1", b"z", b"")]
    status, good, at = {"i0": 33}, {"i0": b"good"}, {"i0": 2}
    right = [(0, 0, b"plain"), (33, 2, b"good"), (0, 0, b"")]
    framesuite.submit_verdicts(FakeContext(right), frames, status, good, at.get)
    framesuite.submit_verdicts(FakeContext(right), frames, status, good, at.get, lit_direct=True)
    framesuite.submit_verdicts(FakeContext(right, late=False), frames, status, good, at.get, lit_direct=False)
    for f, entry in ((1, (34, 2, b"good")), (1, (33, 1, b"good")), (1, (33, 2, b"goo")), (1, (33, 2, b"gooD")), (1, (0, 0, b"good")),
                     (0, (0, 0, b"plaiN")), (0, (33, 0, b"plain")), (2, (0, 0, b"x"))):
        table = list(right)
        table[f] = entry
        with pytest.raises(AssertionError):
            framesuite.submit_verdicts(FakeContext(table), frames, status, good, at.get)
    with pytest.raises(AssertionError):
        framesuite.submit_verdicts(FakeContext(right, parse_status=20), frames, status, good, at.get)
    framesuite.submit_verdicts(FakeContext(right, parse_status=20), frames, status, good, at.get, parse_status=20)
    for late in (False, True):
        with pytest.raises(AssertionError):
            framesuite.submit_verdicts(FakeContext(right, late=late), frames, status, good, at.get, lit_direct=not late)
