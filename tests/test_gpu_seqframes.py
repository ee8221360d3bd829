"""Frames built from chosen sequences (tests/seqframes.py) on the GPU: offsets 1..65 under matches up to 131000 bytes, match
lengths at the 15-bit split of the packed sequence words, literal runs near the 17-bit literal field, blocks of exactly 131072
bytes, nbSeq at its 1/2/3-byte forms, offsets of exactly the window size, every literal and FSE mode. Every frame is checked
against its plaintext (a plain LZ77 execution of its sequences) and the oracle, through decode_all, one submit with the per-block
intermediates of every kernel, the development build's other paths, decode_frames and the FrameDecoder surface."""
import pytest

import blockcheck
import oracle
import seqframes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames():
    return seqframes.all_frames()          # [(family, name, zst, plaintext)]


def test_decode_all_each_frame(ctx, frames):
    bad = [name for _, name, z, plain in frames if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def test_one_batch_with_intermediates(ctx, frames):
    """all frames in one submit: every frame's bytes, and block by block the Huffman tables and literals (zg_k_tables, zg_k_huf), FSE
    tables and sequences (zg_k_tables, zg_k_seq) and the offset history at every block start (zg_k_scan) against the oracle's"""
    b = ctx.prepare(b"".join(z for _, _, z, _ in frames))
    assert b.parse_status == 0 and b.nframes == len(frames)
    b.run()
    b.sync()
    assert b.bad_status == 0, (b.bad_frame, b.bad_status)
    assert b.total_out == sum(len(p) for _, _, _, p in frames)
    first = 0
    for f, (_, name, z, plain) in enumerate(frames):
        assert b.frame_bytes(f) == plain, name
        ob = blockcheck.oracle_blocks(z)
        assert b.frame_info(f).nblocks == len(ob), name
        first += blockcheck.check_frame(b, first, ob, name)
    assert first == b.nblocks
    b.close()


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


@pytest.mark.parametrize("env", DEV_PATHS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_development_paths(frames, env, monkeypatch):
    """the whole set in one submit of the development build under each switch (the engine reads them when it is created): other
    tile shapes, a unit (and a sweep step) per block, zg_k_lz in order, no zg_k_sparse / zg_k_sparse for every frame, no direct
    units, zg_k_seq's packed tables, the plain sweep chain"""
    import zgpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = zgpu.Context(0, dev=True)
    b = c.prepare(b"".join(z for _, _, z, _ in frames))
    b.run()
    b.sync()
    assert b.bad_status == 0, (b.bad_frame, b.bad_status)
    bad = [name for f, (_, name, _, plain) in enumerate(frames) if b.frame_bytes(f) != plain]
    assert not bad, bad
    b.close()
    c.close()


def test_decode_frames(ctx, frames):
    """every frame an entry of one decode_frames call: each gets what decode_all of it alone gives and the oracle's verdict and bytes,
    and its content checksum, computed on the device or the host, matches the frame's"""
    from test_gpu_decode_frames import _check
    entries = [z for _, _, z, _ in frames]
    caps = [len(p) for _, _, _, p in frames]
    res = ctx.decode_frames(entries, caps)
    _check(ctx, entries, caps, res)
    for (_, name, _, plain), r in zip(frames, res):
        assert r.status == 0 and r.data == plain, name
        assert r.nframes == 1 and r.checksums == 1 and r.checksum_mismatches == 0, (name, r)


def test_far_offsets_block_by_block(ctx):
    """FrameDecoder.decode_blocks(UptoBlocks, 1) on the far-offset frames: after every call the counters and the bytes that may be
    collected (the window-retention rule) equal the oracle's, with offsets of exactly window_size reaching across the kept window"""
    import zgpu
    for name, z, plain in seqframes.family("far_offsets"):
        d, o = zgpu.FrameDecoder(ctx), oracle.FrameDecoder()
        st, c, _, _ = d.reset(z)
        ost, oc, _, _ = o.init(z)
        assert (st, c) == (ost, oc) == (0, c), name
        pos, out, oout = c, bytearray(), bytearray()
        for _ in range(10000):
            st, used, fin = d.decode_blocks(z[pos:], zgpu.STRAT_UPTO_BLOCKS, 1)
            ost, oused, ofin = o.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
            assert (st, used, fin) == (ost, oused, ofin), name
            pos += used
            assert d.blocks_decoded() == o.blocks_decoded() and d.bytes_read_from_source() == o.bytes_read_from_source(), name
            assert d.can_collect() == o.can_collect(), name
            out += d.collect()
            oout += o.collect()
            if fin:
                break
        assert bytes(out) == bytes(oout) == plain and d.is_finished(), name
        assert d.get_calculated_checksum() == o.calculated_checksum(), name
        d.close()
