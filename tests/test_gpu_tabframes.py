"""Frames built from chosen table descriptions (tests/tabframes.py) on the GPU: Huffman weight counts at the slot edges of
zg_k_tables' wave builder, tables of 2 to 2048 entries, whole-wave runs, 256 weights, FSE tables with 0-bit states, low-probability
cells only and the highest symbols (zg_fse_build_wave), descriptions at every alignment and past the staged row (zg_k_fparse), and
descriptions that must be refused with the oracle's status. Every valid frame is checked against its plaintext (a plain LZ77
execution of what the writer was given) and the oracle, table entry for table entry; the frames are built on the CPU side, once."""
import pytest

import blockcheck
import oracle
import tabframes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def valid():
    return tabframes.valid_frames()        # [(family, name, zst, plaintext)]


@pytest.fixture(scope="module")
def invalid():
    return tabframes.invalid_frames()      # [(family, name, zst, None)]


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
    """all valid frames in one submit: every frame's bytes, and block by block the Huffman tables (zg_k_tables' wave builder) and
    literals, the FSE tables (zg_fse_build_wave) and sequences and the offset history against the oracle's, entry for entry"""
    _one_submit(ctx, valid)


@pytest.mark.parametrize("env", [{"ZGPU_SEQ_PACKED": "1"}, {"ZGPU_FORCE_INORDER": "1"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_development_paths(valid, env, monkeypatch):
    """the same submit in the development build with zg_k_seq's packed tables and with zg_k_lz in order"""
    import zgpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = zgpu.Context(0, dev=True)
    try:
        _one_submit(c, valid)
    finally:
        c.close()


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
            assert r.status == tabframes.STATUS[name] and r.data is None, (name, r.status)
        else:
            assert r.status == 0 and r.data == plain, name
            assert r.nframes == 1 and r.checksums == 1 and r.checksum_mismatches == 0, (name, r)


def test_invalid_frames_alone(ctx, invalid):
    import zgpu
    got = []
    for _, name, z, _ in invalid:
        try:
            ctx.decode_all(z, 1 << 20)
            got.append((name, 0, tabframes.STATUS[name]))
        except zgpu.ZgpuError as e:
            got.append((name, e.status, tabframes.STATUS[name]))
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
            assert st == tabframes.STATUS[name], (name, st)
        finally:
            d.close()
