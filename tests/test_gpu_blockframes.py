"""Frames of chosen non-sequence blocks (tests/blockframes.py) on the GPU: zg_k_lit with zg_wg_copy and zg_wg_fill on Raw blocks, RLE
blocks and compressed blocks without sequences (raw, RLE, Huffman and treeless literals) of 0 .. 131072 bytes, at every alignment
of destination and source, next to 1-byte neighbours of other kinds and among thousands of empty blocks; and the same blocks as
the sources of matches in the blocks behind them (zg_k_lit and the direct literals of zg_k_huf in front of the LZ stage, the skip
of such blocks in zg_flat1.h / zg_flat4.h, zg_k_sparse, zg_k_lz, zg_k_exact). The CPU harness replaces zg_k_lit with a serial model,
so these tests are the ones that run the kernel itself. Every valid frame is checked against its plaintext (a plain LZ77 execution
of what the writer was given) and the oracle, block by block; every invalid one must get the oracle's status. The frames are built
on the CPU side, once; tests/test_blockframes_cpu.py asserts what they reach."""
import pytest
import torch   # noqa: F401  (before the library is loaded: the process must run on one HIP runtime, Context.decode_frames_to_tensors)

import blockcheck
import blockframes
import hufstreams
import oracle
from test_gpu_seqframes import DEV_PATHS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def valid():
    return blockframes.valid_frames()       # [(family, name, zst, plaintext)]


@pytest.fixture(scope="module")
def invalid():
    return blockframes.invalid_frames()     # [(family, name, zst, None)]


@pytest.fixture(scope="module")
def obs(valid):
    """the oracle's per-block records of every valid frame, made once"""
    return {name: blockcheck.oracle_blocks(z) for _, name, z, _ in valid}


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def _one_submit(c, frames, obs=None, extra=(), per_frame=False):
    """frames [(name, zst, plaintext)] in one submit, `extra` behind them: bytes of every frame (from one read of the whole output;
    per_frame: from b.frame_bytes as well), total_out, bad_status and, with obs, the per-block intermediates. Returns the bad names
    (bytes) and the out_base of every frame"""
    b = c.prepare(b"".join(z for _, z, _ in list(frames) + list(extra)))
    try:
        assert b.parse_status == 0 and b.nframes == len(frames) + len(extra)
        b.run()
        b.sync()
        assert b.bad_status == 0, (b.bad_frame, b.bad_status)
        assert b.total_out == sum(len(p) for _, _, p in list(frames) + list(extra))
        out = b.read(0, b.total_out) if b.total_out else b""
        bad, bases, first = [], [], 0
        for f, (name, z, plain) in enumerate(list(frames) + list(extra)):
            fi = b.frame_info(f)
            bases.append(fi.out_base)
            if fi.out_size != len(plain) or out[fi.out_base:fi.out_base + fi.out_size] != plain or (per_frame and b.frame_bytes(f) != plain):
                bad.append((f, name))
            if obs is not None and f < len(frames):
                assert fi.nblocks == len(obs[name]), name
                first += blockcheck.check_frame(b, first, obs[name], name)
        assert obs is None or extra or first == b.nblocks
        return bad, bases
    finally:
        b.close()


def _check_batch_order(bases):
    order, where = blockframes.batch_alignment()
    for name, idx in where.items():
        assert sorted(bases[f] % 16 for f in idx) == list(range(16)), name


def test_one_batch_with_intermediates(ctx, valid, obs):
    """all valid frames in one submit: every frame's bytes (b.frame_bytes, and one read of the whole output), total_out, and block by
    block the types, literals, Huffman tables, sequences and offset history against the oracle's"""
    bad, _ = _one_submit(ctx, [f[1:] for f in valid], obs, per_frame=True)
    assert not bad, bad


def test_batch_alignment_order(ctx):
    """the representative frames behind pad frames of 0 .. 15 bytes in one submit: each lies at every residue mod 16 of the output
    (frame_out.out_base, from frame_info), and every frame's bytes are its plaintext"""
    order, _ = blockframes.batch_alignment()
    bad, bases = _one_submit(ctx, order)
    assert not bad, bad
    _check_batch_order(bases)


def _both_submits(c, valid):
    bad, _ = _one_submit(c, [f[1:] for f in valid])
    assert not bad, bad
    bad, bases = _one_submit(c, blockframes.batch_alignment()[0])
    assert not bad, bad
    _check_batch_order(bases)


@pytest.mark.parametrize("env", DEV_PATHS + [{"ZGPU_LIT_DIRECT": "0"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_development_paths(valid, env, monkeypatch):
    """the two submits in the development build under each switch of test_gpu_seqframes.DEV_PATHS (other tile shapes, a unit and a
    sweep step per block, zg_k_lz in order, zg_k_sparse never and for every frame, no direct units, zg_k_seq's packed tables, the
    plain sweep chain), and with the literals never after the scan (zg_k_huf writes the arena, zg_k_lit copies from it)"""
    import zgpu
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = zgpu.Context(0, dev=True)
    try:
        _both_submits(c, valid)
    finally:
        c.close()


def test_direct_literals(ctx, valid, obs):
    """the literals after the scan (ZG_FLAG_LIT_DIRECT): zg_k_huf writes the Huffman and treeless blocks without sequences straight
    to the output, zg_k_lit leaves them alone, and the matches of the sources family read what zg_k_huf wrote. The host takes that
    path by its own rule (BatchBuilder::finish, "literals after the scan?"): gain_us = the Huffman literals of blocks without
    sequences / a must exceed b * loss_us + c, with loss_us = per_seq * the most sequences a block has (one round of chains: the
    submit has far fewer blocks with sequences than the 32 chains per CU). hufstreams.direct_rule and blockframes.loss_per_sequence
    read a, b, c and per_seq out of that source and fail if the rule has another form. All valid frames go in front; copies of the
    131072-byte four-stream frame behind them bring the literals a tenth above what the rule asks for. The submit's flags are not
    exported, so that the path was taken is not asserted here"""
    import emu
    frames = [f[1:] for f in valid]
    per_us, factor, floor_us = hufstreams.direct_rule()
    per_seq = blockframes.loss_per_sequence()
    max_nseq = nsb = have = 0
    for name, z, _ in frames:
        for rec in obs[name]:
            if rec["type"] == 2 and rec["sequences"]:
                max_nseq, nsb = max(max_nseq, len(rec["sequences"])), nsb + 1
    assert 0 < nsb < 1024
    for name, z, _ in frames:
        e = emu.EmuBatch(z, max_window=1 << 31)
        for blk in (e.block(b) for b in range(e.nblocks)):
            if blk["btype"] == 2 and not blk["nseq"] and blk["lit_type"] >= 2:
                have += blk["regen_size"]
    filler = next(f for f in frames if f[0] == "lit_sizes_lit_huf4_131072")
    need = 1.1 * per_us * (factor * per_seq * max_nseq + floor_us)
    reps = int((need - have) // len(filler[2])) + 1
    assert (have + reps * len(filler[2])) / per_us > factor * per_seq * max_nseq + floor_us and reps * len(filler[1]) < 1 << 27
    bad, _ = _one_submit(ctx, frames, obs, extra=[filler] * reps)
    assert not bad, bad[:20]


def test_decode_frames(ctx, valid, invalid):
    """all frames, valid and invalid mixed, as entries of one decode_frames call: every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    from test_gpu_decode_frames import _check
    frames = []
    for i, f in enumerate(valid):                        # an invalid frame after every second valid one
        frames.append(f)
        if i % 2 == 1 and i // 2 < len(invalid):
            frames.append(invalid[i // 2])
    frames += invalid[len(valid) // 2:]
    assert len(frames) == len(valid) + len(invalid)
    entries = [z for _, _, z, _ in frames]
    caps = [len(p) if p is not None else 1 << 20 for _, _, _, p in frames]
    res = ctx.decode_frames(entries, caps)
    _check(ctx, entries, caps, res)
    for (_, name, _, plain), r in zip(frames, res):
        if plain is None:
            assert r.status == blockframes.STATUS[name] and r.data is None, (name, r.status)
        else:
            assert r.status == 0 and r.data == plain, name
            assert r.nframes == 1 and r.checksums == 1 and r.checksum_mismatches == 0, (name, r)


def test_decode_frames_device_and_device_src(ctx, valid):
    """decode_frames_device and decode_frames_device_src on the neighbours, sources and alignment frames: destinations are slots of
    a sentinel-filled device tensor at the shifts of test_gpu_decode_frames_device, the sources lie in device memory at the shifts
    of test_gpu_decode_frames_device_src; both calls agree, the bytes are the plaintext and every guard byte is untouched"""
    from test_gpu_decode_frames_device_src import _both
    frames = [f for f in valid if f[0] in ("neighbours", "sources", "lit_alignment")]
    entries = [z for _, _, z, _ in frames]
    plains = [p for _, _, _, p in frames]
    caps = [len(p) + (j % 2) * 5 for j, p in enumerate(plains)]
    arena, res, _ = _both(ctx, entries, caps, shifts=[(7 * j) % 32 for j in range(len(entries))],
                          src_shifts=[(3 * j) % 18 for j in range(len(entries))])
    for (_, name, _, plain), r in zip(frames, res):
        assert (r.status, r.written, r.nframes, r.checksum_mismatches) == (0, len(plain), 1, 0), (name, r)
    arena.check(plains)


def _block_by_block(ctx, name, z):
    """FrameDecoder.decode_blocks(UptoBlocks, 1) against the oracle call by call. Returns (last status, the bytes collected)"""
    import zgpu
    d, o = zgpu.FrameDecoder(ctx), oracle.FrameDecoder()
    try:
        st, c, _, _ = d.reset(z)
        ost, oc, _, _ = o.init(z)
        assert (st, c) == (ost, oc) == (0, blockframes.HDR), name
        pos, out = c, bytearray()
        for _ in range(10000):
            st, used, fin = d.decode_blocks(z[pos:], zgpu.STRAT_UPTO_BLOCKS, 1)
            ost, oused, ofin = o.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
            assert st == ost, (name, st, ost)
            if not st:                                   # (an error carries neither a count nor "finished": include/zgpu.h)
                assert (used, fin) == (oused, ofin), name
            pos += used
            assert d.blocks_decoded() == o.blocks_decoded() and d.bytes_read_from_source() == o.bytes_read_from_source(), name
            assert d.can_collect() == o.can_collect(), name
            got, want = d.collect(), o.collect()
            assert got == want, name
            out += got
            if st or fin:
                break
        if not st:
            assert d.is_finished() and d.get_calculated_checksum() == o.calculated_checksum(), name
        return st, bytes(out)
    finally:
        d.close()


def test_sources_block_by_block(ctx):
    """every block of the sources frames in a submit of its own, so the block a match reads from was written by an earlier submit:
    status, used bytes, counters, can_collect and the bytes collected equal the oracle's after every call"""
    for name, z, plain in blockframes.family("sources"):
        st, out = _block_by_block(ctx, name, z)
        assert st == 0 and out == plain, name


def test_invalid_block_by_block(ctx, invalid):
    """the invalid frames call by call: the good blocks in front decode as the oracle's, the failing call has the oracle's status,
    and what is held after it is what the oracle holds"""
    for _, name, z, _ in invalid:
        st, _ = _block_by_block(ctx, name, z)
        assert st == blockframes.STATUS[name], (name, st)


def test_invalid_frames_alone(ctx, invalid):
    import zgpu
    got = []
    for _, name, z, _ in invalid:
        try:
            ctx.decode_all(z, 1 << 20)
            got.append((name, 0, blockframes.STATUS[name]))
        except zgpu.ZgpuError as e:
            got.append((name, e.status, blockframes.STATUS[name]))
    assert [g for g in got if g[1] != g[2]] == []
