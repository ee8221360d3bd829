"""Frames built from chosen repeat codes (tests/repframes.py) on the GPU: the symbolic offset history. zg_k_seqpost's scan (8
sequences per thread, wave shuffles, the wave maps through LDS, the carry from pass to pass) on blocks of repeat codes only and
runs of "repeat offset 1 minus one" around 8, 512 and 2048 sequences; zg_k_scan in its three forms on frames of 1 to 16385 blocks
(the second and third chunk of the chunked form, its carry_map) with a history-dependent sequence at every edge; zg_sym_resolve
in every executor (the development build's switches); offsets that become 0 only across a block boundary, where the verdict is
the executor's. Every valid frame is checked against its plaintext (the RFC's history rule and a plain LZ77 in Python) and
the oracle, block by block; every invalid one must get the oracle's status and keep the good blocks' bytes. The frames are built
on the CPU side, once per module (about 20 s, most of it the five frames of 8191 and more blocks); tests/test_repframes_cpu.py
asserts what they reach."""
import pytest

import framesuite
import oracle
import repframes
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, invalid, oblocks = framesuite.frame_fixtures(repframes)


def test_decode_all_each_frame(ctx, valid):
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


def test_one_batch_with_intermediates(ctx, valid, oblocks):
    """all valid frames in one submit: every frame's bytes, the history at every block start (zg_k_scan<1024, 8>: the largest frame
    picks the form for all) and every sequence (zg_k_seqpost) against the oracle's"""
    framesuite.submit(ctx, valid, oblocks)


def test_small_frames_in_the_one_wave_scan(ctx, valid, oblocks):
    """the frames of at most 64 blocks in a submit of their own (zg_k_scan<64, 1>), then with those of up to 1024 (zg_k_scan<1024, 1>)"""
    lo, mid = repframes.SCAN_LIMITS[:2]
    small = [f for f in valid if repframes.META[f[1]]["nblocks"] <= lo]
    medium = [f for f in valid if repframes.META[f[1]]["nblocks"] <= mid]
    assert len(small) >= 100 and len(medium) >= len(small) + 3
    framesuite.submit(ctx, small, oblocks)
    framesuite.submit(ctx, medium, oblocks)


def test_scan_frames_alone(ctx, valid, oblocks):
    """every scan_edges frame in a submit of its own: the form zg_launch_scan picks for its size, and zg_k_scan's one-frame branch
    (d.nframes == 1: no zg_k_scanf); for the frames of 8192 and more blocks the carry from chunk to chunk"""
    seen = set()
    for fr in valid:
        if fr[0] == "scan_edges":
            framesuite.submit(ctx, [fr], oblocks)
            seen.add(repframes.META[fr[1]]["nblocks"])
    assert seen == set(repframes.NBLOCKS)


@pytest.mark.parametrize("env", framesuite.DEV_PATHS, ids=framesuite.env_id)
def test_development_paths(valid, env, monkeypatch):
    """the valid frames in one submit of the development build under each switch, so that every consumer of a symbolic offset
    resolves them: zg_flat1.h and zg_flat4.h in other unit and tile shapes, zg_k_lz in order, zg_k_sparse for every frame and for
    none, zg_k_seq's packed tables in front of the post-pass, the plain sweep chain"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid)


def _mixed(valid, invalid):
    """the invalid frames among the valid ones of fewer than 1000 blocks, one after every third"""
    small = [f for f in valid if repframes.META[f[1]]["nblocks"] < 1000]
    assert len(small) >= 3 * len(invalid)
    return framesuite.interleave(small, invalid, 3)


def test_decode_frames(ctx, valid, invalid):
    """every frame an entry of one decode_frames call, the invalid ones among the valid: each gets what decode_all of it alone gives
    and the oracle's verdict and bytes; a valid entry's content checksum matches"""
    big = [f for f in valid if repframes.META[f[1]]["nblocks"] >= 1000]
    frames = _mixed(valid, invalid) + big
    assert len(frames) == len(valid) + len(invalid)
    framesuite.check_decode_frames(ctx, frames, repframes.STATUS)


STEP_FRAMES = ["scan_%d" % (repframes.SCAN_LIMITS[1] + 1), "scan_%d" % (repframes.CHUNK + 8), "dec_n%d_slot1" % (repframes.WAVE + 1),
               "dec_rows_%d_%d_%d_slot1" % (repframes.PASS + 1, 1, repframes.WAVE)]


@pytest.mark.parametrize("k", [1, 7, 64, 1025])
@pytest.mark.parametrize("name", STEP_FRAMES)
def test_decode_blocks_upto(ctx, valid, name, k):
    """FrameDecoder.decode_blocks(UptoBlocks, k): every call starts from the history the call in front left (hist_init other than
    1, 4, 8, runs of decrements continued across calls); after every call the counters and the collectable bytes, at the end the
    checksum, equal the oracle's"""
    fr = [f for f in valid if f[1] == name]
    assert len(fr) == 1, name
    st, out, _ = framesuite.lockstep(ctx, name, fr[0][2], k)
    assert st == 0 and out == fr[0][3], (name, k, st)


def test_invalid_frames_alone(ctx, invalid):
    """each invalid frame alone: decode_all's status; a one-frame submit's status, failing block and the good blocks' bytes;
    FrameDecoder.decode_blocks(All): the status, the counters and the bytes held after the Err (zg_k_partial) against the oracle's"""
    import zgpu
    framesuite.invalid_alone(ctx, invalid, repframes.STATUS)
    for _, name, z, _ in invalid:
        want, good, at = repframes.STATUS[name], repframes.GOOD[name], repframes.META[name]["bad_block"]
        b = ctx.prepare(z)
        try:
            b.run()
            b.sync()
            fi = b.frame_info(0)
            assert (fi.status, fi.bad_block, fi.out_size) == (want, at, len(good)), (name, fi.status, fi.bad_block, fi.out_size)
            assert b.read(fi.out_base, fi.out_size) == good, name
        finally:
            b.close()
        d, o = zgpu.FrameDecoder(ctx), oracle.FrameDecoder()
        try:
            st, c, _, _ = d.init(z)
            ost, oc, _, _ = o.init(z)
            assert (st, c) == (ost, oc) and st == 0, name
            st, _, _ = d.decode_blocks(z[c:])
            ost, _, _ = o.decode_blocks(z[c:])
            assert st == ost == want, (name, st, ost)
            assert d.blocks_decoded() == o.blocks_decoded() == at and d.bytes_read_from_source() == o.bytes_read_from_source(), name
            assert d.can_collect() == o.can_collect(), name
            assert d.collect() == o.collect(), name
        finally:
            d.close()


def test_invalid_among_valid_in_one_submit(ctx, valid, invalid):
    """all invalid frames among valid ones in one submit: the oracle's status per frame, the failing block, the good blocks' bytes;
    every valid neighbour untouched"""
    framesuite.submit_verdicts(ctx, _mixed(valid, invalid), repframes.STATUS, repframes.GOOD, lambda name: repframes.META[name]["bad_block"])
