"""Frames built from chosen table descriptions (tests/tabframes.py) on the GPU: Huffman weight counts at the slot edges of
zg_k_tables' wave builder, tables of 2 to 2048 entries, whole-wave runs, 256 weights, FSE tables with 0-bit states, low-probability
cells only and the highest symbols (zg_fse_build_wave), descriptions at every alignment and past the staged row (zg_k_fparse), and
descriptions that must be refused with the oracle's status. Every valid frame is checked against its plaintext (a plain LZ77
execution of what the writer was given) and the oracle, table entry for table entry; the frames are built on the CPU side, once."""
import pytest

import framesuite
import tabframes
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, invalid, oblocks = framesuite.frame_fixtures(tabframes)


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def test_one_batch_with_intermediates(ctx, valid, oblocks):
    """all valid frames in one submit: every frame's bytes, and block by block the Huffman tables (zg_k_tables' wave builder) and
    literals, the FSE tables (zg_fse_build_wave) and sequences and the offset history against the oracle's, entry for entry"""
    framesuite.submit(ctx, valid, oblocks)


@pytest.mark.parametrize("env", [{"ZGPU_SEQ_PACKED": "1"}, {"ZGPU_FORCE_INORDER": "1"}], ids=framesuite.env_id)
def test_development_paths(valid, oblocks, env, monkeypatch):
    """the same submit in the development build with zg_k_seq's packed tables and with zg_k_lz in order"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid, oblocks)


def test_decode_frames(ctx, valid, invalid):
    """all frames, valid and invalid mixed, as entries of one decode_frames call: every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    framesuite.check_decode_frames(ctx, framesuite.interleave(valid, invalid, 5), tabframes.STATUS)


def test_invalid_frames_alone(ctx, invalid):
    framesuite.invalid_alone(ctx, invalid, tabframes.STATUS)


def test_invalid_behind_a_valid_block(ctx, invalid):
    """a valid raw block in front of each invalid frame's blocks, in one frame: FrameDecoder.decode_blocks(UptoBlocks, 1) agrees
    with the oracle call by call (status, the bytes used by a call that succeeds, the counters and what may be collected after every call,
    the failing one included)"""
    for _, name, z, _ in invalid:
        st, _, _ = framesuite.lockstep(ctx, name, framesuite.raw_block_in_front(z), header=(0, 6))
        assert st == tabframes.STATUS[name], (name, st)
