"""Frames built at the edges of zg_k_sweep and the split sweep (tests/sweepframes.py) on the GPU: the value selection of a 4-byte
group under every pattern of equal and unequal effective offsets and every output alignment, the byte tail and the last batch of
a unit, sd.head on both sides of each step, the tail and head grids of zg_launch_sweep, the grouping of head launches, submits of
mixed windows and unit counts, and the repeat as a plain chain behind an offset beyond the window. The CPU harness has no sweep,
so these tests are the ones that run it; tests/test_sweepframes_cpu.py proves from the harness's plan that the frames hit what
they aim at, and every submit here first checks that the GPU's plan is that plan. The scratch words of every pointer-mode unit
are compared with tests/lz_model.py, so a wrong byte with right scratch words is the sweep's."""
import numpy as np
import pytest
import torch   # noqa: F401  (before the library is loaded: the process must run on one HIP runtime)

import framesuite
import lz_model
import sweepframes as S
from framesuite import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
valid, _invalid, oblocks = framesuite.frame_fixtures(S)


def check_submit(c, sname, frames, mode, planned=True):
    """the frames in one submit: every frame's bytes; planned: b.units() is the harness's plan of the same submit (else the aim is
    void), b.sweep_mode() is `mode`, and the scratch words of every pointer-mode unit are lz_model.expected_scratch"""
    b = c.prepare(b"".join(z for _, z, _ in frames))
    try:
        assert b.parse_status == 0 and b.nframes == len(frames), sname
        b.run()
        b.sync()
        assert b.bad_status == 0, (sname, b.bad_frame, b.bad_status)
        got_mode, units = b.sweep_mode(), b.units()
        per_frame, plan = S.plan_of(frames)
        if planned:
            assert [(fb, nb, noseq) for fb, nb, _, _, noseq in units] == [u[1:] for u in plan.units], (sname, "the GPU's plan is not the harness's")
        bad_scratch = []
        for (f, base, funits), (name, z, plain) in zip(per_frame, frames) if planned else ():
            if plan.frames[f][6]:
                continue                                 # (zg_k_sparse finishes it: no scratch words)
            e, bounds = lz_model.expected_scratch(z, [u[0] for u in funits])
            for i, (_, _, noseq) in enumerate(funits):
                _, _, sbase, size, _ = units[plan.frames[f][2] + i]
                assert size == bounds[i + 1] - bounds[i], (sname, name, i)
                if noseq:
                    continue
                got = b.scratch_words(sbase, size)
                wrong = np.flatnonzero(got != e[bounds[i]:bounds[i + 1]])
                if len(wrong):
                    bad_scratch.append((name, i, int(wrong[0])))
        assert not bad_scratch, (sname, "the flatten's scratch words differ from the model", bad_scratch[:10])
        out = b.read(0, b.total_out) if b.total_out else b""
        bad, at = [], 0
        for f, (name, _, plain) in enumerate(frames):
            got = out[at:at + len(plain)]
            if got != plain or b.frame_bytes(f) != plain:
                x = next((i for i, (p, q) in enumerate(zip(got, plain)) if p != q), -1)
                bad.append((name, x, [i for i, (s, n, _) in enumerate(S.LAYOUT.get(name, {"units": []})["units"]) if s <= x < s + n]))
            at += len(plain)
        assert b.total_out == at and not bad, (sname, "bytes differ: (frame, first wrong byte, its unit)", bad[:10])
        if planned:
            assert got_mode == mode, (sname, got_mode, mode)
        return got_mode
    finally:
        b.close()


def test_decode_all_each_frame(ctx, valid):
    """every frame alone: a unit_ends frame ends with the unit it is about, so that unit is the last of the submit's last frame"""
    bad = [name for _, name, z, plain in valid if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad


@pytest.mark.parametrize("sname", S.SUBMITS)
def test_submit(ctx, oblocks, sname):
    """each submit of sweepframes.submits() with no switch set: block by block the oracle's records, then the plan, the bytes, the
    scratch words and the expected sweep_mode()"""
    mode, frames = S.submits()[sname]
    framesuite.submit(ctx, frames, oblocks)
    check_submit(ctx, sname, frames, mode)


def test_big_frame(ctx):
    """hg_big, the frame with more than 78 * 16 steps (gs = 17 in zg_launch_sweep), in a submit of its own and through decode_all"""
    name, z, plain = S.head_groups_big()
    check_submit(ctx, name, [(name, z, plain)], 1)
    assert ctx.decode_all(z, len(plain)) == plain


@pytest.mark.parametrize("env", [{}] + framesuite.DEV_PATHS, ids=lambda e: framesuite.env_id(e) or "no_switch")
def test_development_build(valid, env, monkeypatch):
    """the development build: with no switch set everything test_submit checks; under each switch of framesuite.DEV_PATHS every submit's
    bytes and the whole set in one submit (a unit and a step per block, units of three blocks, other tiles, zg_k_lz in order,
    zg_k_sparse never and for every frame, no direct units, packed tables). The plain chain (ZGPU_SWEEP_SPLIT=0) reports mode 0"""
    with framesuite.dev_context(monkeypatch, env) as c:
        for sname, (mode, frames) in S.submits().items():
            got = check_submit(c, sname, frames, mode, planned=not env)
            if env == {"ZGPU_SWEEP_SPLIT": "0"}:
                assert got == 0, sname
        framesuite.submit(c, valid)


def test_big_frame_plain_chain_and_one_block_units(monkeypatch):
    for env in ({"ZGPU_SWEEP_SPLIT": "0"}, {"ZGPU_UNIT_BLOCKS": "1"}):
        with framesuite.dev_context(monkeypatch, env) as c:
            check_submit(c, "hg_big", [S.head_groups_big()], None, planned=False)
        for k in env:
            monkeypatch.delenv(k)


def test_decode_frames(ctx, valid):
    """all frames as entries of one decode_frames call: every entry gets what decode_all of it alone and the oracle give"""
    framesuite.check_decode_frames(ctx, valid, {})


@pytest.mark.parametrize("k", [1, 4])
def test_block_by_block(ctx, k):
    """tails_heads and beyond_window k blocks to a call: behind the first call every unit is a pointer-mode unit that reads the
    retained window in front of the output, and the split is off. Every call agrees with the oracle's (framesuite.lockstep); bw_w1
    ends where the oracle's block-by-block decoder, which has drained the bytes by then, refuses the offset of W + 1"""
    for fam in ("tails_heads", "beyond_window"):
        for name, z, plain in S.family(fam):
            st, out, _ = framesuite.lockstep(ctx, name, z, k=k, header=(0, 6))
            if name == "bw_w1":
                assert st != 0 and 0 < len(out) < len(plain) and out == plain[:len(out)], (name, st)
            else:
                assert st == 0 and out == plain, name
