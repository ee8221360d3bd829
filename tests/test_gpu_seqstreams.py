"""Frames built from chosen sequence bitstreams (tests/seqstreams.py) on the GPU: zg_k_seq at the bit rates and stream positions no
encoder reaches. In valid frames: phases of ZG_SEQ_CH sequences of 79 and 80 bits (the mover's request -> land -> read pipeline), the
last sequence and the FAST -> CAREFUL switch at every phase position, bursts between 20 and 80 bits, 0-bit states, the highest-rate
stream at every 16-byte piece offset, and zg_k_seqpost's extra-bit read with so == 31 and 32 and fields of up to 58 bits. One
stream at every residue of the 512-byte ring in one submit (ZG_SEQ_RING, the mirror store of zg_ring_put). In rejected frames:
phases of 12 x 89 bits (ZG_SEQ_CMAX, ZG_SEQ_MARGIN), streams that end at every position relative to the switch, and a workgroup of
ZG_SEQ_G mixed blocks of which four fail. Every valid frame is checked against its plaintext (a plain LZ77 execution of what the
writer was given) and, in the shared submits, block by block against the oracle's sequences, tables and offset history; every
invalid one must get the oracle's status, alone, among valid neighbours and call by call. The frames are built on the CPU side,
once; tests/test_seqstreams_cpu.py asserts what they reach."""
import pytest

import blockcheck
import framesuite
import seqstreams
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, invalid, _ = framesuite.frame_fixtures(seqstreams)


def _split(valid):
    """(the frames over 16 and 64 MiB of history, the others): two submits"""
    large = [f for f in valid if f[1] in seqstreams.LARGE]
    assert len(large) == len(seqstreams.LARGE)
    return large, [f for f in valid if f[1] not in seqstreams.LARGE]


def test_decode_all_each_frame(ctx, valid):
    """each frame alone: its stream lies at the front of the source buffer (the floorA clamp of the ring's fill)"""
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def _ring_submit(c):
    z, plain, n = seqstreams.ring_submit()
    b = c.prepare(z)
    try:
        assert b.parse_status == 0 and b.nframes == n == seqstreams.RING
        b.run()
        b.sync()
        assert b.bad_status == 0, (b.bad_frame, b.bad_status)
        assert b.total_out == n * len(plain)
        out = b.read(0, b.total_out)
        info = [b.frame_info(f) for f in range(n)]
        assert [f for f, fi in enumerate(info) if out[fi.out_base:fi.out_base + fi.out_size] != plain] == []
        ob = seqstreams.oracle_blocks("ring_mod", z[:len(z) // n])
        first = 0
        for f in range(n):
            first += blockcheck.check_frame(b, first, ob, "ring_mod copy %d" % f)
        assert first == b.nblocks
    finally:
        b.close()


def test_one_batch_with_intermediates(ctx, valid):
    """all valid frames but the large-history ones in one submit (the streams start wherever the frames in front leave them): every
    frame's bytes, and block by block the sequences (zg_k_seq's states through zg_k_seqpost), the FSE tables and the offset history
    against the oracle's, entry for entry"""
    framesuite.submit(ctx, _split(valid)[1], seqstreams.oracle_blocks)


def test_large_history_batch_with_intermediates(ctx, valid):
    """the frames over 16 and 64 MiB of RLE blocks in a submit of their own: offset codes 24 and 26, blocks that regenerate up to
    10 MB (their ZgSeq positions are compared mod 2^17, blockcheck.check_frame), so == 31 and 32"""
    framesuite.submit(ctx, _split(valid)[0], seqstreams.oracle_blocks)


def test_ring_submit(ctx):
    """ZG_SEQ_RING copies of a frame of odd length in one submit: the one stream of more than ZG_SEQ_RING bytes at every residue
    of the ring, every copy's bytes and sequences against the oracle's"""
    _ring_submit(ctx)


@pytest.mark.parametrize("env", [{"ZGPU_SEQ_PACKED": "1"}, {"ZGPU_FORCE_INORDER": "1"}], ids=framesuite.env_id)
def test_development_paths(valid, env, monkeypatch):
    """the same three submits in the development build with zg_k_seq's packed tables and with zg_k_lz in order"""
    with framesuite.dev_context(monkeypatch, env) as c:
        large, small = _split(valid)
        framesuite.submit(c, small, seqstreams.oracle_blocks)
        framesuite.submit(c, large, seqstreams.oracle_blocks)
        _ring_submit(c)


def test_decode_frames(ctx, valid, invalid):
    """valid and invalid frames mixed as entries of one decode_frames call. The ZG_SEQ_G frames of workgroup_mixes come first and in
    their order, so that their blocks with sequences are the first workgroup of zg_k_seq: four of its quads fail (in a FAST phase,
    in the CAREFUL one, with bits left over, in the execution) while their wave neighbours run on. Behind them every other frame
    but the large-history ones, an invalid one after every second valid one. Every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    mix = [("workgroup_mixes", *f) for f in seqstreams.mix_submit()]
    assert len(mix) == seqstreams.G and sum(f[3] is None for f in mix) == 4
    names = {f[1] for f in mix}
    v = [f for f in _split(valid)[1] if f[1] not in names]
    inv = [f for f in invalid if f[1] not in names]
    frames = mix + framesuite.interleave(v, inv, 2)
    assert len(frames) == len(valid) - len(seqstreams.LARGE) + len(invalid)
    framesuite.check_decode_frames(ctx, frames, seqstreams.STATUS)


def test_invalid_frames_alone(ctx, invalid):
    framesuite.invalid_alone(ctx, invalid, seqstreams.STATUS)


def test_rejected_frames_call_by_call(ctx):
    """the max_rate_rejected frames as they are (a raw block or RLE blocks in front of the failing one): FrameDecoder.decode_blocks(
    UptoBlocks, 1) agrees with the oracle call by call (status, the bytes used by a call that succeeds, the counters and what may be
    collected after every call, the failing one included: the bytes the reference keeps in front of the failure)"""
    frames = seqstreams.family("max_rate_rejected")
    assert len(frames) == 4
    for name, z, plain in frames:
        assert plain is None
        st, _, calls = framesuite.lockstep(ctx, name, z, header=(0, 6))
        assert st == seqstreams.STATUS[name] and calls >= 2, (name, st, calls)
