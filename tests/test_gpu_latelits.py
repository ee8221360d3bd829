"""Frames whose literals verdict arrives after the scan (tests/latelits.py) on the GPU: submits that run their Huffman streams behind
zg_k_scan (ZG_FLAG_LIT_DIRECT), where zg_k_merge and zg_k_litfix rank a literal-stream verdict (30 .. 35) against what every other
stage found, cut the frame at the first failing block and rewrite its status, bad_block and good_blocks; zg_huf_group's branch
for a block the scan has already stopped; and the stages behind them (zg_k_lit, the flatten, zg_k_sparse, zg_k_lz, zg_k_fin,
zg_k_exact, zg_k_partial, Batch::sync's trim, the scatter of the device-resident calls) on frames cut that late. The development
build takes the path on these tiny submits with ZGPU_LIT_DIRECT=1, the product build by the host's own rule behind 50 MB of
literals; Batch.lit_direct() says in every test that the path was taken. The control ZGPU_LIT_DIRECT=0 must give the same verdicts.
Every verdict, failing block and held byte is the oracle's (tests/latelits.py asserts them when it builds the frames);
tests/test_latelits_cpu.py asserts what the frames reach.

What the host's walk finds itself (a block-header defect, a treeless section with no table in force, a defect of the sequences
section header: latelits.HOST_FINDS) ends the walk of a whole submit, so such a frame can only be a submit's last one: one of them,
a literal defect in a block the host stops at its sequences header, closes every one-submit test; all of them are checked alone
and as entries of the decode_frames calls, which walk every entry on its own into one shared submit."""
import pytest
import torch   # noqa: F401  (before the library is loaded: the process must run on one HIP runtime)

import blockframes
import framesuite
import hufstreams
import latelits
import oracle
from framesuite import ctx  # noqa: F401
from latelits import GOOD, META, STATUS

pytestmark = pytest.mark.gpu
valid, invalid, _ = framesuite.frame_fixtures(latelits)
ON = {"ZGPU_LIT_DIRECT": "1"}


def _bad(name):
    return META[name]["bad_block"]


def _mixed(valid, invalid):
    """every frame but those in which the host's walk finds an error, an invalid one behind every valid one; then one of those: a
    literal defect in a block whose sequences header stops the host (zg_huf_group's branch for a block that is not active, in a frame
    that is not the submit's first). Returns (frames, the parse_status of the submit)"""
    inv = [f for f in invalid if not META[f[1]]["host"]]
    last = next(f for f in invalid if META[f[1]].get("cell", (0,))[0] in (33, 34, 35) and META[f[1]]["cell"][2:] == ("seqhdr", "same"))
    assert len(inv) >= 300 and STATUS[last[1]] in (33, 34, 35)
    return framesuite.interleave(valid, inv, 1) + [last], 47 if META[last[1]]["code"] == "47h" else META[last[1]]["code"]


@pytest.mark.parametrize("env,want", [(ON, True), ({"ZGPU_LIT_DIRECT": "0"}, False), ({}, False)], ids=["1", "0", "unset"])
def test_switch_and_getter(valid, env, want, monkeypatch):
    """the development build on a submit of the valid family: ZGPU_LIT_DIRECT=1 takes the path, 0 does not, and without the switch
    the host's rule decides (these few kilobytes of literals: no)"""
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit(c, valid, lit_direct=want)


def test_product_build_small_submit(ctx, valid):
    """the product build on the same submit: the host's rule, no"""
    framesuite.submit(ctx, valid, lit_direct=False)


@pytest.mark.parametrize("env", [ON, {"ZGPU_LIT_DIRECT": "0"}, dict(ON, ZGPU_UNIT_BLOCKS="1"), dict(ON, ZGPU_FORCE_INORDER="1"),
                                 dict(ON, ZGPU_SPARSE_MAX="100000000"), dict(ON, ZGPU_DIRECT="0")], ids=framesuite.env_id)
def test_all_frames_in_one_submit(valid, invalid, env, monkeypatch):
    """invalid among valid in one submit: status, failing block, out_size and the good blocks' bytes of every invalid frame, the
    plaintext of every valid one; with the literals after the scan, with them in front of it (the control), and with the late cut
    in front of a unit per block, zg_k_lz in order, zg_k_sparse for every frame and the flatten without direct units"""
    with framesuite.dev_context(monkeypatch, env) as c:
        frames, ps = _mixed(valid, invalid)
        framesuite.submit_verdicts(c, frames, STATUS, GOOD, _bad, lit_direct=env["ZGPU_LIT_DIRECT"] == "1", parse_status=ps)


@pytest.mark.parametrize("env", [ON, dict(ON, ZGPU_PRESIZE="0")], ids=framesuite.env_id)
def test_presized_submit(valid, invalid, env, monkeypatch):
    """the same submit with an 8-byte Frame_Content_Size in every header: the output is sized in advance and launch_phase2 goes
    right behind the scan; and the same frames sized after it. A valid frame declares its plaintext's size; an invalid one 4096
    bytes and one per block, more than the scan lays out for it while its literals are still unknown (the largest block here has
    1100 bytes, every other one less than 100, a geometry frame one byte per block around them), so that no frame breaks its
    promise and sends the whole submit the slow way"""
    frames, ps = _mixed(valid, invalid)
    frames = [(fam, name, latelits.with_content_size(z, len(plain) if plain is not None else 4096 + META[name]["nblocks"]), plain)
              for fam, name, z, plain in frames]
    with framesuite.dev_context(monkeypatch, env) as c:
        framesuite.submit_verdicts(c, frames, STATUS, GOOD, _bad, lit_direct=True, parse_status=ps)


def test_invalid_frames_alone(invalid, monkeypatch):
    """each invalid frame alone with the literals after the scan: decode_all's status; a one-frame submit's status, failing block,
    out_size and bytes; FrameDecoder.decode_blocks(All): status, counters, can_collect and the bytes collected after the Err
    against the oracle's (what zg_k_partial leaves where an execution error in front of the literal defect decides)"""
    import zgpu
    with framesuite.dev_context(monkeypatch, ON) as c:
        framesuite.invalid_alone(c, invalid, STATUS)
        wrong = []
        for _, name, z, _ in invalid:
            want, good, at = STATUS[name], GOOD[name], _bad(name)
            b = c.prepare(z)
            try:
                assert b.parse_status == 0 or META[name]["host"], (name, b.parse_status)      # (the walk stops only where the host can find something)
                b.run()
                b.sync()
                assert b.lit_direct(), name
                fi = b.frame_info(0)
                if (fi.status, fi.bad_block, fi.out_size) != (want, at, len(good)) or b.read(fi.out_base, fi.out_size) != good:
                    wrong.append((name, "submit", fi.status, fi.bad_block, fi.out_size, want, at, len(good)))
            finally:
                b.close()
            d, o = zgpu.FrameDecoder(c), oracle.FrameDecoder()
            try:
                st, used, _, _ = d.init(z)
                ost, oused, _, _ = o.init(z)
                assert (st, used) == (ost, oused) and st == 0, name
                st, _, _ = d.decode_blocks(z[used:])
                ost, _, _ = o.decode_blocks(z[used:])
                got = (st, d.blocks_decoded(), d.bytes_read_from_source(), d.can_collect(), d.collect())
                ref = (ost, o.blocks_decoded(), o.bytes_read_from_source(), o.can_collect(), o.collect())
                assert ost == want and o.blocks_decoded() == at, name
                if got != ref:
                    wrong.append((name, "decoder") + got[:4] + ref[:4])
            finally:
                d.close()
        assert not wrong, (len(wrong), wrong[:20])


def test_pairs_block_by_block(monkeypatch):
    """the pairs frames (at most five blocks) call by call, FrameDecoder.decode_blocks(UptoBlocks, 1): every call's status, bytes
    used, counters and collectable bytes equal the oracle's, the failing call included"""
    with framesuite.dev_context(monkeypatch, ON) as c:
        for name, z, _ in latelits.family("pairs"):
            st, _, _ = framesuite.lockstep(c, name, z, header=(0, 6))
            assert st == STATUS[name], (name, st)


def test_decode_frames(valid, invalid, monkeypatch):
    """all frames as entries of one decode_frames call, the invalid among the valid: every entry gets what decode_all of it alone
    gives and the oracle's verdict and bytes"""
    with framesuite.dev_context(monkeypatch, ON) as c:
        framesuite.check_decode_frames(c, framesuite.interleave(valid, invalid, 1), STATUS)


def test_decode_frames_device_writes_nothing_of_a_failing_entry(valid, monkeypatch):
    """decode_frames_device on the pairs family, every second entry one of the valid twins, the destinations slots of a
    sentinel-filled device arena at the shifts of tests/test_gpu_blockframes.py: a failing entry has its status, written == 0 and
    not one byte of its slot or of the guards changed; a valid one is its plaintext"""
    from devmem import Arena
    pairs = [("pairs",) + f for f in latelits.family("pairs")]
    frames = framesuite.interleave(valid[:len(pairs)], pairs, 1)
    entries = [z for _, _, z, _ in frames]
    caps = [(len(p) if p is not None else len(GOOD[name]) + 64) + (j % 2) * 5 for j, (_, name, _, p) in enumerate(frames)]
    with framesuite.dev_context(monkeypatch, ON) as c:
        arena = Arena(caps, shifts=[(7 * j) % 32 for j in range(len(entries))])
        res = c.decode_frames_device(entries, arena.ptrs, caps)
        wrong = [(name, r.status, r.written) for (_, name, _, p), r in zip(frames, res)
                 if (r.status, r.written) != ((0, len(p)) if p is not None else (STATUS[name], 0))]
        assert not wrong, (len(wrong), wrong[:20])
        arena.check([p for _, _, _, p in frames])


def test_product_build_by_the_hosts_rule(ctx, invalid):
    """the product build takes the path by its own rule (BatchBuilder::finish, "literals after the scan?"): the pairs and geometry
    frames in front, copies of blockframes' 131072-byte four-stream frame behind them until gain_us = the Huffman literals of
    blocks without sequences / a exceeds b * loss_us + c by a tenth (hufstreams.direct_rule and blockframes.loss_per_sequence read
    a, b, c and per_seq out of the source, as tests/test_gpu_blockframes.py::test_direct_literals does). The front frames' own
    literals are not counted, and loss_us is taken for 16 sequences, more than any block here has or claims (12, the bitstream
    defect of a count too high): both only raise the number of copies"""
    front = [f for f in invalid if f[0] in ("pairs", "geometry") and not META[f[1]]["host"]]
    assert len(front) >= 250
    filler = next(f for f in blockframes.family("lit_sizes") if f[0] == "lit_sizes_lit_huf4_131072")
    per_us, factor, floor_us = hufstreams.direct_rule()
    per_seq = blockframes.loss_per_sequence()
    need = 1.1 * per_us * (factor * per_seq * 16 + floor_us)
    reps = int(need // len(filler[2])) + 1
    assert reps * len(filler[2]) / per_us > factor * per_seq * 16 + floor_us and reps * len(filler[1]) < 1 << 27
    framesuite.submit_verdicts(ctx, front + [("filler",) + filler] * reps, STATUS, GOOD, _bad, lit_direct=True)
