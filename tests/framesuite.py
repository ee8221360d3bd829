"""What the suites of hand-built frames share (test helper, no tests): tabframes, hufstreams, seqstreams, repframes, blockframes and
seqframes with their GPU and CPU test files. For the generators the family cache and the reader of kernel constants; for the GPU tests
the fixtures, the one-submit check, the development-build context, the mixed decode_frames call and the call-by-call comparison with
the oracle; for the CPU tests the per-frame check on the harness. The generators import this module and the CPU tests import the
generators, so torch, zgpu and emu are imported inside the functions that need them. A frame is (family, name, zst, plaintext or None),
or the last three of these."""
import contextlib
import re

import pytest

import blockcheck
import oracle

# ---- for the generators -----------------------------------------------------------------------------------------------------------


class Families:
    """the families of a generator: name -> builder of [(name, zst, plaintext or None)], each built once. check(all frames) holds the
    generator's own asserts on the whole set"""

    def __init__(self, builders, check=None):
        self.builders, self.check, self.cache = builders, check, {}

    def family(self, name):
        if name not in self.cache:
            self.cache[name] = self.builders[name]()
        return self.cache[name]

    def all_frames(self):
        """[(family, name, zst, plaintext or None)]"""
        out = [(fam, *f) for fam in self.builders for f in self.family(fam)]
        assert len(set(n for _, n, _, _ in out)) == len(out), "frame names repeat"
        if self.check:
            self.check(out)
        return out

    def valid_frames(self):
        return [f for f in self.all_frames() if f[3] is not None]

    def invalid_frames(self):
        return [f for f in self.all_frames() if f[3] is None]


def defines(path, names):
    """{name: value} of the `#define NAME <digits>` lines of a source file; every name must be there"""
    text = open(path).read()
    out = {}
    for k in names:
        m = re.search(r"^#define\s+%s\s+(\d+)\b" % k, text, re.M)
        assert m, k
        out[k] = int(m.group(1))
    return out


# ---- for the GPU tests: every helper takes the context first and closes what it opens ---------------------------------------------

DEV_PATHS = [
    {"ZGPU_FLAT_T": "512"},
    {"ZGPU_UNIT_BLOCKS": "1"},
    {"ZGPU_UNIT_BLOCKS": "3", "ZGPU_FLAT_T": "512"},
    {"ZGPU_FORCE_INORDER": "1"},
    {"ZGPU_SPARSE_MAX": "0"},
    {"ZGPU_SPARSE_MAX": "100000000"},
    {"ZGPU_DIRECT": "0"},
    {"ZGPU_SEQ_PACKED": "1"},
    {"ZGPU_SWEEP_SPLIT": "0"},
]


def env_id(env):
    return ",".join("%s=%s" % kv for kv in env.items())


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


def frame_fixtures(gen):
    """the module-scoped fixtures (valid, invalid, oblocks) of a generator module: its valid and its invalid frames, and the oracle's
    per-block records of every valid frame by name, each made once"""
    @pytest.fixture(scope="module")
    def valid():
        return gen.valid_frames()

    @pytest.fixture(scope="module")
    def invalid():
        return gen.invalid_frames()

    @pytest.fixture(scope="module")
    def oblocks():
        return {name: blockcheck.oracle_blocks(z) for _, name, z, _ in gen.valid_frames()}

    return valid, invalid, oblocks


@contextlib.contextmanager
def dev_context(monkeypatch, env):
    """a context of the development build under the switches of env (the engine reads them when it is created)"""
    import zgpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = zgpu.Context(0, dev=True)
    try:
        yield c
    finally:
        c.close()


POISONS = (0x00, 0xA5, 0xFF)


@contextlib.contextmanager
def poisoned_context(monkeypatch, poison, env=None):
    """a fresh context of the development build under ZGPU_POISON=poison (and the switches of env): every byte of device memory the
    design does not define when a submit starts holds that value (zstd-rs_amd/csrc/zg_engine.h: Poison). A context of its own per
    poison: the fill covers a buffer's whole capacity, which an earlier submit of the same context may have grown"""
    with dev_context(monkeypatch, dict(env or {}, ZGPU_POISON=str(poison))) as c:
        assert c.tuning()["poison"] == poison
        yield c


def oracle_verdict(z):
    """(status, failing block, bytes of the good blocks) of the frame at the start of z, from the oracle block by block: nothing is
    drained, so what its decode buffer holds after the last call that succeeded is the good blocks' bytes. A valid frame: (0, its
    number of blocks, its plaintext)"""
    d = oracle.FrameDecoder()
    d.set_max_window_size(1 << 31)
    st, pos, _, _ = d.init(z)
    assert st == 0
    good = 0
    while True:
        st, used, fin = d.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
        if st:
            return st, d.blocks_decoded(), d.held()[:good]
        pos += used
        good = len(d.held())
        if fin:
            return 0, d.blocks_decoded(), d.held()


def frame_alone(c, z):
    """the frame at the start of z as a submit of its own: (status, failing block, out_size, bytes) as sync() leaves them, and behind
    them the status of the host's walk (not 0: the host found the error, and a submit ends with such a frame)"""
    b = c.prepare(z)
    try:
        b.run()
        b.sync()
        fi = b.frame_info(0)
        return fi.status, fi.bad_block, fi.out_size, (b.read(fi.out_base, fi.out_size) if fi.out_size else b""), b.parse_status
    finally:
        b.close()


def submit(c, frames, oblocks=None, extra=(), lit_direct=None):
    """frames in one submit, `extra` (more valid frames) behind them: parse_status, nframes, bad_status, total_out, every frame's
    out_size and bytes (from one read of the whole output and from b.frame_bytes); with oblocks (name -> the oracle's records, or a
    callable (name, zst)) nblocks and the per-block intermediates of every frame of `frames`, and without `extra` that these are all
    the submit's blocks; with lit_direct (True / False) that the run decoded its literals after the scan, or did not
    (b.lit_direct()). Returns the out_base of every frame"""
    every = [f[-3:] for f in list(frames) + list(extra)]
    b = c.prepare(b"".join(z for _, z, _ in every))
    try:
        assert b.parse_status == 0 and b.nframes == len(every)
        b.run()
        b.sync()
        assert lit_direct is None or b.lit_direct() == lit_direct, ("literals after the scan", b.lit_direct())
        assert b.bad_status == 0, (b.bad_frame, b.bad_status)
        assert b.total_out == sum(len(p) for _, _, p in every)
        out = b.read(0, b.total_out) if b.total_out else b""
        info = [b.frame_info(f) for f in range(len(every))]
        bad = [(f, name) for f, (fi, (name, _, plain)) in enumerate(zip(info, every))
               if fi.out_size != len(plain) or out[fi.out_base:fi.out_base + fi.out_size] != plain or b.frame_bytes(f) != plain]
        assert not bad, bad[:20]
        if oblocks is not None:
            first = 0
            for fi, (name, z, _) in zip(info, every[:len(frames)]):
                ob = oblocks(name, z) if callable(oblocks) else oblocks[name]
                assert fi.nblocks == len(ob), name
                first += blockcheck.check_frame(b, first, ob, name)
            assert extra or first == b.nblocks
        return [fi.out_base for fi in info]
    finally:
        b.close()


def submit_verdicts(c, frames, status, good, bad_block, lit_direct=None, parse_status=0):
    """frames, invalid among valid, in one submit: an invalid frame (plaintext None) has the oracle's status[name], failing block
    bad_block(name) and out_size, and holds good[name], the bytes of its good blocks; a valid one has status 0 and its plaintext;
    with lit_direct (True / False) the run decoded its literals after the scan, or did not. parse_status: what the host's walk
    finds in the last frame, where that frame is one that ends the walk"""
    frames = [f[-3:] for f in frames]
    b = c.prepare(b"".join(z for _, z, _ in frames))
    try:
        assert b.parse_status == parse_status and b.nframes == len(frames), (b.parse_status, b.nframes, len(frames))
        b.run()
        b.sync()
        assert lit_direct is None or b.lit_direct() == lit_direct, ("literals after the scan", b.lit_direct())
        wrong = []
        for f, (name, _, plain) in enumerate(frames):
            fi = b.frame_info(f)
            if plain is None:
                ok = (fi.status, fi.bad_block, fi.out_size) == (status[name], bad_block(name), len(good[name])) and b.frame_bytes(f) == good[name]
            else:
                ok = fi.status == 0 and b.frame_bytes(f) == plain
            if not ok:
                wrong.append((name, fi.status, fi.bad_block, fi.out_size))
        assert not wrong, (len(wrong), wrong[:20])
    finally:
        b.close()


def interleave(valid, invalid, every):
    """the valid frames in their order with an invalid one behind every `every`-th, the invalid ones left over at the end"""
    out = []
    for i, f in enumerate(valid):
        out.append(f)
        if i % every == every - 1 and i // every < len(invalid):
            out.append(invalid[i // every])
    out += invalid[len(valid) // every:]
    assert len(out) == len(valid) + len(invalid)
    return out


def _oracle_first_frame(z, dict_raw=None):
    """(checksum_from_data or 0, calculated_checksum) of the entry's first frame, as the reference's FrameDecoder reports them"""
    _, d = oracle.decode_frame_all(z, dict_raw=dict_raw)
    v = d.checksum_from_data()
    return (v or 0), d.calculated_checksum()


def _zgpu_alone(c, z, cap):
    import zgpu
    try:
        return 0, c.decode_all(z, cap)
    except zgpu.ZgpuError as e:
        return e.status, None


def check_entries(c, entries, caps, res, dict_raw=None):
    """every result of a decode_frames call against what the oracle and decode_all give for that entry alone"""
    from devmem import MAGIC, oracle_alone
    assert len(res) == len(entries)
    for i, (z, cap, r) in enumerate(zip(entries, caps, res)):
        st, out = oracle_alone(z, cap, dict_raw)
        assert r.status == st, (i, r, st)
        zs, zout = _zgpu_alone(c, z, cap)
        assert r.status == zs, (i, r, zs)
        if st:
            assert r.written == 0 and r.data is None, i
            continue
        assert r.data == out == zout, i
        assert r.written == len(out)
        if r.nframes and z[:4] == MAGIC:
            assert (r.checksum_from_data, r.calculated_checksum) == _oracle_first_frame(z, dict_raw), i


def check_decode_frames(c, frames, status):
    """the frames as entries of one decode_frames call: check_entries; an invalid entry carries status[name] and no data, a valid one
    its plaintext, one frame and one matching content checksum"""
    entries = [z for _, _, z, _ in frames]
    caps = [len(p) if p is not None else 1 << 20 for _, _, _, p in frames]
    res = c.decode_frames(entries, caps)
    check_entries(c, entries, caps, res)
    for (_, name, _, plain), r in zip(frames, res):
        if plain is None:
            assert r.status == status[name] and r.data is None, (name, r.status)
        else:
            assert r.status == 0 and r.data == plain, name
            assert r.nframes == 1 and r.checksums == 1 and r.checksum_mismatches == 0, (name, r)


def invalid_alone(c, invalid, status):
    """decode_all of each invalid frame alone raises with status[name]"""
    import zgpu
    got = []
    for _, name, z, _ in invalid:
        try:
            c.decode_all(z, 1 << 20)
            got.append((name, 0, status[name]))
        except zgpu.ZgpuError as e:
            got.append((name, e.status, status[name]))
    assert [g for g in got if g[1] != g[2]] == []


def raw_block_in_front(z):
    """the frame with a valid raw block of 200 bytes in front of its blocks (tabframes' frame header: descriptor, window byte)"""
    assert z[4] == 0x04
    payload = bytes(range(200))
    return z[:6] + (0 | (0 << 1) | (len(payload) << 3)).to_bytes(3, "little") + payload + z[6:]


def _block_count(z, pos):
    """the blocks whose headers chain from pos on: up to the last one, a reserved type or the end of z"""
    n = 0
    while pos + 3 <= len(z):
        h = int.from_bytes(z[pos:pos + 3], "little")
        n += 1
        if h & 1 or (h >> 1) & 3 == 3:
            break
        pos += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
    return n


def lockstep(c, name, z, k=1, header=None, decoder=None, oracle_decoder=oracle.FrameDecoder):
    """FrameDecoder.decode_blocks(UptoBlocks, k) on frame z against the oracle, call by call: the header step's status and consumed
    bytes (and == header where given); after every call the status, the bytes used and `finished` of a call that succeeds (an error
    carries neither: include/zgpu.h), the counters, can_collect and what collect() returns, the failing call included; after a clean
    finish is_finished() and the calculated checksum. Returns (last status, the bytes collected, calls made). decoder(c) and
    oracle_decoder() make the two decoders: zgpu.FrameDecoder and oracle.FrameDecoder unless the helpers' own test puts others in"""
    import zgpu
    d, o = (decoder or zgpu.FrameDecoder)(c), oracle_decoder()
    try:
        st, pos, _, _ = d.reset(z)
        ost, opos, _, _ = o.init(z)
        assert (st, pos) == (ost, opos), (name, st, pos, ost, opos)
        assert header is None or (st, pos) == header, (name, st, pos)
        out, calls, fin, most = bytearray(), 0, False, _block_count(z, pos) // k + 2
        while not (st or fin):
            assert calls < most, (name, "more calls than the frame has blocks for")
            st, used, fin = d.decode_blocks(z[pos:], zgpu.STRAT_UPTO_BLOCKS, k)
            ost, oused, ofin = o.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, k)
            calls += 1
            assert st == ost, (name, k, st, ost)
            if not st:
                assert (used, fin) == (oused, ofin), (name, k, used, fin, oused, ofin)
            pos += used
            assert d.blocks_decoded() == o.blocks_decoded() and d.bytes_read_from_source() == o.bytes_read_from_source(), name
            assert d.can_collect() == o.can_collect(), name
            got = d.collect()
            assert got == o.collect(), (name, k, d.blocks_decoded())
            out += got
        if not st:
            assert d.is_finished() and d.get_calculated_checksum() == o.calculated_checksum(), name
        return st, bytes(out), calls
    finally:
        d.close()


# ---- for the CPU tests ------------------------------------------------------------------------------------------------------------

def check_on_harness(name, z, plain, status, oblocks=blockcheck.oracle_blocks):
    """one frame through the CPU harness: an invalid one (plain None) gets status[name] from decode_all_verdict; a valid one decodes to
    its plaintext, agrees block by block with the oracle's records oblocks(z), and zg_k_exact's source (drain rule 1) accepts it.
    Returns the emu.EmuBatch it decoded (tests/test_poison_cpu.py compares what it left under another fill)"""
    import emu
    if plain is None:
        e = emu.EmuBatch(z, max_window=1 << 31)
        assert emu.decode_all_verdict(z, batch=e) == status[name], name
        return e
    e = emu.EmuBatch(z, max_window=1 << 31)
    assert e.parse_status == 0 and e.nframes == 1, name
    out, st = e.frame_bytes(0)
    assert st == 0 and out == plain, name
    ob = oblocks(z)
    assert e.nblocks == len(ob), name
    blockcheck.check_frame(e, 0, ob, name)
    ex = e.exact(drain_rule=1)
    assert ex[0][0] == 0, (name, ex)
    return e
