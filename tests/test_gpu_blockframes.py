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

import blockframes
import framesuite
import hufstreams
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, invalid, oblocks = framesuite.frame_fixtures(blockframes)


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def _check_batch_order(bases):
    order, where = blockframes.batch_alignment()
    for name, idx in where.items():
        assert sorted(bases[f] % 16 for f in idx) == list(range(16)), name


def test_one_batch_with_intermediates(ctx, valid, oblocks):
    """all valid frames in one submit: every frame's bytes (b.frame_bytes, and one read of the whole output), total_out, and block by
    block the types, literals, Huffman tables, sequences and offset history against the oracle's"""
    framesuite.submit(ctx, valid, oblocks)


def test_batch_alignment_order(ctx):
    """the representative frames behind pad frames of 0 .. 15 bytes in one submit: each lies at every residue mod 16 of the output
    (frame_out.out_base, from frame_info), and every frame's bytes are its plaintext"""
    _check_batch_order(framesuite.submit(ctx, blockframes.batch_alignment()[0]))


@pytest.mark.parametrize("env", framesuite.DEV_PATHS + [{"ZGPU_LIT_DIRECT": "0"}], ids=framesuite.env_id)
def test_development_paths(valid, env, monkeypatch):
    """the two submits in the development build under each switch of framesuite.DEV_PATHS (other tile shapes, a unit and a
    sweep step per block, zg_k_lz in order, zg_k_sparse never and for every frame, no direct units, zg_k_seq's packed tables, the
    plain sweep chain), and with the literals never after the scan (zg_k_huf writes the arena, zg_k_lit copies from it)"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid)
        _check_batch_order(framesuite.submit(c, blockframes.batch_alignment()[0]))


def test_direct_literals(ctx, valid, oblocks):
    """the literals after the scan (ZG_FLAG_LIT_DIRECT): zg_k_huf writes the Huffman and treeless blocks without sequences straight
    to the output, zg_k_lit leaves them alone, and the matches of the sources family read what zg_k_huf wrote. The host takes that
    path by its own rule (BatchBuilder::finish, "literals after the scan?"): gain_us = the Huffman literals of blocks without
    sequences / a must exceed b * loss_us + c, with loss_us = per_seq * the most sequences a block has (one round of chains: the
    submit has far fewer blocks with sequences than the 32 chains per CU). hufstreams.direct_rule and blockframes.loss_per_sequence
    read a, b, c and per_seq out of that source and fail if the rule has another form. All valid frames go in front; copies of the
    131072-byte four-stream frame behind them bring the literals a tenth above what the rule asks for; b.lit_direct() says that the
    path was taken"""
    import emu
    frames = [f[1:] for f in valid]
    per_us, factor, floor_us = hufstreams.direct_rule()
    per_seq = blockframes.loss_per_sequence()
    max_nseq = nsb = have = 0
    for name, z, _ in frames:
        for rec in oblocks[name]:
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
    framesuite.submit(ctx, frames, oblocks, extra=[filler] * reps, lit_direct=True)


def test_decode_frames(ctx, valid, invalid):
    """all frames, valid and invalid mixed, as entries of one decode_frames call: every entry gets what decode_all of it alone gives
    and the oracle's verdict and bytes; every invalid entry carries the oracle's status and every valid neighbour is untouched"""
    framesuite.check_decode_frames(ctx, framesuite.interleave(valid, invalid, 2), blockframes.STATUS)


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


def test_sources_block_by_block(ctx):
    """every block of the sources frames in a submit of its own, so the block a match reads from was written by an earlier submit:
    status, used bytes, counters, can_collect and the bytes collected equal the oracle's after every call"""
    for name, z, plain in blockframes.family("sources"):
        st, out, _ = framesuite.lockstep(ctx, name, z, header=(0, blockframes.HDR))
        assert st == 0 and out == plain, name


def test_invalid_block_by_block(ctx, invalid):
    """the invalid frames call by call: the good blocks in front decode as the oracle's, the failing call has the oracle's status,
    and what is held after it is what the oracle holds"""
    for _, name, z, _ in invalid:
        st, _, _ = framesuite.lockstep(ctx, name, z, header=(0, blockframes.HDR))
        assert st == blockframes.STATUS[name], (name, st)


def test_invalid_frames_alone(ctx, invalid):
    framesuite.invalid_alone(ctx, invalid, blockframes.STATUS)
