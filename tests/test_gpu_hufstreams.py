"""Frames built from chosen Huffman streams (tests/hufstreams.py) on the GPU: zg_k_huf on streams no encoder emits. Codes that never
re-synchronise (63 redo rounds of the 64 the loop gives: zx_shfl_up, zx_alignbit and the wave's unbarriered LDS traffic in the
gfx950 build), chunks of exactly ZG_HP_ROWS symbols and of one more (the switch to dense chunks, in the first window and behind
it), stream lengths at the chunk and window edges, all 16 start alignments under a byte of 0xBA / 0xFF, last codes that reach
below the stream's start at each of those alignments (the zeroing of the staged piece that straddles the start), four streams of 1 .. 12 literals (zg_k_huf_uneven for the splits that differ from the format's),
workgroups of one and two waves on a shared table. Every valid frame is checked against its plaintext (serial_decode of the
streams it was given, executed by a plain LZ77) and the oracle, block by block; every invalid one must get the oracle's status.
The frames are built on the CPU side, once; tests/test_hufstreams_cpu.py asserts what they reach."""
import pytest

import blockcheck
import oracle
import hufstreams

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def valid():
    return hufstreams.valid_frames()        # [(family, name, zst, plaintext)]


@pytest.fixture(scope="module")
def invalid():
    return hufstreams.invalid_frames()      # [(family, name, zst, None)]


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def _one_submit(c, valid):
    b = c.prepare(b"".join(z for _, _, z, _ in valid))
    assert b.parse_status == 0 and b.nframes == len(valid)
    b.run()
    b.sync()
    assert b.bad_status == 0, (b.bad_frame, b.bad_status)
    assert b.total_out == sum(len(p) for _, _, _, p in valid)
    first = 0
    for f, (_, name, z, plain) in enumerate(valid):
        assert b.frame_bytes(f) == plain, name
        ob = blockcheck.oracle_blocks(z)
        assert b.frame_info(f).nblocks == len(ob), name
        first += blockcheck.check_frame(b, first, ob, name)
    assert first == b.nblocks
    b.close()


def test_one_batch_with_intermediates(ctx, valid):
    """all valid frames in one submit (the streams start wherever the frames in front leave them): every frame's bytes, and block by
    block the Huffman table, the literals, the sequences and the offset history against the oracle's"""
    _one_submit(ctx, valid)


@pytest.mark.parametrize("env", [{"ZGPU_LIT_DIRECT": "0"}, {"ZGPU_UNIT_BLOCKS": "1"}, {"ZGPU_DIRECT": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_development_paths(valid, env, monkeypatch):
    """the same submit in the development build: the literals never after the scan, a unit per block, no direct units"""
    import zgpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = zgpu.Context(0, dev=True)
    try:
        _one_submit(c, valid)
    finally:
        c.close()


def test_direct_literals(ctx, valid):
    """a submit of the frames without sequences only, so that the host's own rule runs the literals after the scan and zg_k_huf
    writes them straight to the output (ZG_FLAG_LIT_DIRECT). The rule relied on is BatchBuilder::finish's (zg_host_parse.cpp,
    "literals after the scan?"; zg_engine.cpp sets the flag from it): lit_direct = gain_us > b * loss_us + c with gain_us = the
    Huffman literals of blocks without sequences / a, and loss_us = 0 in a submit without sequences. hufstreams.direct_rule reads
    a, b and c out of that source (2.5e6, 1.5 and 20: 50 MB) and fails if the rule has another form; the set is repeated until
    it holds a tenth more literals than the rule asks for. The submit's flags are not exported, so that the path was taken is not
    asserted here"""
    noseq = [f for f in valid if f[1].endswith("_n")]
    assert len(noseq) * 2 == len(valid)
    for _, name, _, _ in noseq:
        assert all(r["nseq"] == 0 for r in hufstreams.META[name]["hs"]), name
    per_us, factor, floor_us = hufstreams.direct_rule()
    lits = sum(r["regen"] for _, name, _, _ in noseq for r in hufstreams.META[name]["hs"])
    reps = int(1.1 * floor_us * per_us) // lits + 1
    assert reps * lits / per_us > factor * 0.0 + floor_us and reps * sum(len(z) for _, _, z, _ in noseq) < 1 << 28
    b = ctx.prepare(b"".join(z for _, _, z, _ in noseq) * reps)
    try:
        assert b.parse_status == 0 and b.nframes == len(noseq) * reps
        b.run()
        b.sync()
        assert b.bad_status == 0, (b.bad_frame, b.bad_status)
        assert b.total_out == sum(len(p) for _, _, _, p in noseq) * reps
        out = b.read(0, b.total_out)
        bad = []
        for f in range(b.nframes):
            fi = b.frame_info(f)
            _, name, _, plain = noseq[f % len(noseq)]
            if out[fi.out_base:fi.out_base + fi.out_size] != plain:
                bad.append((f, name))
        assert not bad, bad[:20]
        first = 0
        for _, name, z, _ in noseq:                          # the first copy of the set block by block as well
            first += blockcheck.check_frame(b, first, blockcheck.oracle_blocks(z), name)
    finally:
        b.close()


def test_decode_frames(ctx, valid, invalid):
    """all frames, valid and invalid mixed, as entries of one decode_frames call: every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    from test_gpu_decode_frames import _check
    frames = []
    for i, f in enumerate(valid):                        # an invalid frame after every fifth valid one
        frames.append(f)
        if i % 5 == 4 and i // 5 < len(invalid):
            frames.append(invalid[i // 5])
    frames += invalid[len(valid) // 5:]
    assert len(frames) == len(valid) + len(invalid)
    entries = [z for _, _, z, _ in frames]
    caps = [len(p) if p is not None else 1 << 20 for _, _, _, p in frames]
    res = ctx.decode_frames(entries, caps)
    _check(ctx, entries, caps, res)
    for (_, name, _, plain), r in zip(frames, res):
        if plain is None:
            assert r.status == hufstreams.STATUS[name] and r.data is None, (name, r.status)
        else:
            assert r.status == 0 and r.data == plain, name
            assert r.nframes == 1 and r.checksums == 1 and r.checksum_mismatches == 0, (name, r)


def test_invalid_frames_alone(ctx, invalid):
    import zgpu
    got = []
    for _, name, z, _ in invalid:
        try:
            ctx.decode_all(z, 1 << 20)
            got.append((name, 0, hufstreams.STATUS[name]))
        except zgpu.ZgpuError as e:
            got.append((name, e.status, hufstreams.STATUS[name]))
    assert [g for g in got if g[1] != g[2]] == []


def test_invalid_behind_a_valid_block(ctx, invalid):
    """a valid raw block in front of each invalid frame's blocks, in one frame: FrameDecoder.decode_blocks(UptoBlocks, 1) agrees
    with the oracle call by call (status, the bytes used by a call that succeeds, the counters and what may be collected after every call,
    the failing one included)"""
    import zgpu
    for _, name, z, _ in invalid:
        assert z[4] == 0x04                              # tabframes' frame header: descriptor, window byte
        payload = bytes(range(200))
        zz = z[:6] + (0 | (0 << 1) | (len(payload) << 3)).to_bytes(3, "little") + payload + z[6:]
        d, o = zgpu.FrameDecoder(ctx), oracle.FrameDecoder()
        try:
            st, c, _, _ = d.reset(zz)
            ost, oc, _, _ = o.init(zz)
            assert (st, c) == (ost, oc) == (0, 6), name
            pos = c
            for _ in range(8):
                st, used, fin = d.decode_blocks(zz[pos:], zgpu.STRAT_UPTO_BLOCKS, 1)
                ost, oused, ofin = o.decode_blocks(zz[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
                assert st == ost, (name, st, ost)
                if not st:                                   # (an error carries neither a count nor "finished": include/zgpu.h)
                    assert (used, fin) == (oused, ofin), name
                pos += used
                assert d.blocks_decoded() == o.blocks_decoded() and d.bytes_read_from_source() == o.bytes_read_from_source(), name
                assert d.can_collect() == o.can_collect(), name
                assert d.collect() == o.collect(), name
                if st or fin:
                    break
            assert st == hufstreams.STATUS[name], (name, st)
        finally:
            d.close()
