"""Frames built from chosen sequences (tests/seqframes.py) on the GPU: offsets 1..65 under matches up to 131000 bytes, match
lengths at the 15-bit split of the packed sequence words, literal runs near the 17-bit literal field, blocks of exactly 131072
bytes, nbSeq at its 1/2/3-byte forms, offsets of exactly the window size, every literal and FSE mode. Every frame is checked
against its plaintext (a plain LZ77 execution of its sequences) and the oracle, through decode_all, one submit with the per-block
intermediates of every kernel, the development build's other paths, decode_frames and the FrameDecoder surface."""
import pytest

import framesuite
import seqframes
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, _, oblocks = framesuite.frame_fixtures(seqframes)     # (every frame is valid)


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def test_one_batch_with_intermediates(ctx, valid, oblocks):
    """all frames in one submit: every frame's bytes, and block by block the Huffman tables and literals (zg_k_tables, zg_k_huf), FSE
    tables and sequences (zg_k_tables, zg_k_seq) and the offset history at every block start (zg_k_scan) against the oracle's"""
    framesuite.submit(ctx, valid, oblocks)


@pytest.mark.parametrize("env", framesuite.DEV_PATHS, ids=framesuite.env_id)
def test_development_paths(valid, env, monkeypatch):
    """the whole set in one submit of the development build under each switch (the engine reads them when it is created): other
    tile shapes, a unit (and a sweep step) per block, zg_k_lz in order, no zg_k_sparse / zg_k_sparse for every frame, no direct
    units, zg_k_seq's packed tables, the plain sweep chain"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid)


def test_decode_frames(ctx, valid):
    """every frame an entry of one decode_frames call: each gets what decode_all of it alone gives and the oracle's verdict and bytes,
    and its content checksum, computed on the device or the host, matches the frame's"""
    framesuite.check_decode_frames(ctx, valid, {})


def test_far_offsets_block_by_block(ctx):
    """FrameDecoder.decode_blocks(UptoBlocks, 1) on the far-offset frames: after every call the counters and the bytes that may be
    collected (the window-retention rule) equal the oracle's, with offsets of exactly window_size reaching across the kept window"""
    for name, z, plain in seqframes.family("far_offsets"):
        st, out, _ = framesuite.lockstep(ctx, name, z)
        assert st == 0 and out == plain, name
