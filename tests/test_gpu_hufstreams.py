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
import framesuite
import hufstreams
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, invalid, oblocks = framesuite.frame_fixtures(hufstreams)


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def test_one_batch_with_intermediates(ctx, valid, oblocks):
    """all valid frames in one submit (the streams start wherever the frames in front leave them): every frame's bytes, and block by
    block the Huffman table, the literals, the sequences and the offset history against the oracle's"""
    framesuite.submit(ctx, valid, oblocks)


@pytest.mark.parametrize("env", [{"ZGPU_LIT_DIRECT": "0"}, {"ZGPU_UNIT_BLOCKS": "1"}, {"ZGPU_DIRECT": "0"}], ids=framesuite.env_id)
def test_development_paths(valid, oblocks, env, monkeypatch):
    """the same submit in the development build: the literals never after the scan, a unit per block, no direct units"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid, oblocks)


def test_direct_literals(ctx, valid, oblocks):
    """a submit of the frames without sequences only, so that the host's own rule runs the literals after the scan and zg_k_huf
    writes them straight to the output (ZG_FLAG_LIT_DIRECT). The rule relied on is BatchBuilder::finish's (zg_host_parse.cpp,
    "literals after the scan?"; zg_engine.cpp sets the flag from it): lit_direct = gain_us > b * loss_us + c with gain_us = the
    Huffman literals of blocks without sequences / a, and loss_us = 0 in a submit without sequences. hufstreams.direct_rule reads
    a, b and c out of that source (2.5e6, 1.5 and 20: 50 MB) and fails if the rule has another form; the set is repeated until
    it holds a tenth more literals than the rule asks for; b.lit_direct() says that the path was taken"""
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
        assert b.lit_direct()
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
            first += blockcheck.check_frame(b, first, oblocks[name], name)
    finally:
        b.close()


def test_decode_frames(ctx, valid, invalid):
    """all frames, valid and invalid mixed, as entries of one decode_frames call: every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    framesuite.check_decode_frames(ctx, framesuite.interleave(valid, invalid, 5), hufstreams.STATUS)


def test_invalid_frames_alone(ctx, invalid):
    framesuite.invalid_alone(ctx, invalid, hufstreams.STATUS)


def test_invalid_behind_a_valid_block(ctx, invalid):
    """a valid raw block in front of each invalid frame's blocks, in one frame: FrameDecoder.decode_blocks(UptoBlocks, 1) agrees
    with the oracle call by call (status, the bytes used by a call that succeeds, the counters and what may be collected after every call,
    the failing one included)"""
    for _, name, z, _ in invalid:
        st, _, _ = framesuite.lockstep(ctx, name, framesuite.raw_block_in_front(z), header=(0, 6))
        assert st == hufstreams.STATUS[name], (name, st)
