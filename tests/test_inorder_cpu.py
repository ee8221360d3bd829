"""The SOURCE of the in-order kernels (zstd-rs_amd/csrc/zg_inorder.h: zg_k_lz, zg_k_sparse, zg_k_partial and the retire routine they
share) on the CPU: tests/emu/zg_emu_inorder.cpp runs the three bodies through the SIMT emulator on the intermediates of the CPU
harness. Checked here, without a GPU: zg_lz_frame<256> turns every valid frame of the hand-built suites into its plaintext and leaves
the oracle's verdict and failing block on the invalid ones; zg_sparse_frame copies the matches of the sparse frames behind the real
zg_flat1_unit; zg_partial_block leaves what the oracle's decode buffer holds behind the good blocks of a frame whose execution fails.
The serial k_exec of tests/emu/zg_emu.cpp is the model the harness itself decodes with; the oracle and the generators' plaintext are
what the bodies are held to."""
import os
import random

import pytest

import blockframes
import emu
import oracle
import repframes
import seqframes
import sweepframes
import tabframes
import test_flat1_cpu
from tabframes import Block

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_BLOCKS = 900          # the emulator costs milliseconds per block: hg_big (5000 blocks), the scan-edge frames of repframes from 1023 blocks
                          # on and blockframes' two frames of 1012 and 2002 empty blocks stay out (LONG: how many per family)
# ... and about 2 ms per round of zg_retire<256> (256 fibers): the frames within MAX_BLOCKS that take more than about 2 s through
# zg_lz_frame<256> on the emulator, by family, with the seconds measured. They are blocks of thousands of sequences that copy from each
# other; their kind is covered by the frames of 2049 sequences and fewer that run. Everything else within MAX_BLOCKS runs.
SLOW = {
    ("seqframes", "short_offsets"): {"short_mix0": 30, "short_mix1": 12, "short_mix2": 2.3},
    ("seqframes", "seq_counts"): {"nseq2047": 4, "nseq2048": 4, "nseq2049": 4, "nseq32511": 64, "nseq32512": 57, "nseq32513": 53, "nseq43669": 72},
    ("seqframes", "far_offsets"): {"far_w17": 15, "far_w20": 19, "far_w24": 5},
    ("seqframes", "literal_modes"): {"lit_%s_multi_l%d" % (k, lv): 5 for k in ("raw", "rle", "huf") for lv in (1, 3, 19)},
    ("repframes", "perm_blocks"): {"perm_n2049_identity": 5, "perm_n2049_identity_of_rle": 5},
}
LONG = {("repframes", "scan_edges"): 8, ("blockframes", "neighbours"): 2}
PARTS = {("sweepframes", "unit_ends"): 4, ("repframes", "perm_blocks"): 3, ("repframes", "dec_chains"): 2}     # families of more than about 5 s: frame i in part i % n
NOT_ENOUGH_LITERALS, ZERO_OFFSET, OFFSET_TOO_BIG, DICT_TOO_SMALL = 50, 51, 52, 53


def batches(e, width):
    """per block with sequences of submit e: (sequences, batches of `width` that need more than one round of zg_retire: a match behind the
    first of its batch needs source bytes at or above that first match's destination)"""
    out = []
    for b in range(e.nblocks):
        blk = e.block(b)
        if blk["btype"] != 2 or not blk["nseq"] or blk["status"]:
            continue
        hist = e.block_hist(b)
        sq = e.block_sequences(b, blk["nseq"])
        multi = 0
        for s0 in range(0, len(sq), width):
            pend = [(mdst, emu.sym_resolve(of, hist), ml) for of, ml, mdst, _ in sq[s0:s0 + width] if ml]
            if not pend:
                continue
            hwm = pend[0][0]
            multi += any((max(mdst - off + ml, 0) if ml < off else mdst) > hwm for mdst, off, ml in pend[1:])
        out.append((blk["nseq"], multi))
    return out


# ---- zg_lz_frame, valid frames --------------------------------------------------------------------------------------------------

SUITES = {g.__name__: g for g in (seqframes, repframes, blockframes, sweepframes)}
VALID_FAMILIES = [(g, fam, part) for g in SUITES for fam in SUITES[g].FAMILIES if fam != "invalid" for part in range(PARTS.get((g, fam), 1))]
# among the frames that run (in every part of a family run in parts): the families in which no batch of 256 needs more than one round
# (no match copies from a match of its batch), and the families with a block of more than 256 sequences (the carry from batch to batch)
NO_MULTI_ROUND = {("blockframes", f) for f in ("lit_sizes", "lit_alignment", "neighbours")}      # (a sequence or none per block); every other family has some
CARRY = {("seqframes", "match_lengths"), ("seqframes", "block_sizes"), ("seqframes", "literal_modes"), ("repframes", "perm_blocks"),
         ("repframes", "dec_chains"), ("sweepframes", "groups"), ("sweepframes", "head_groups")}
assert not set(LONG) & set(PARTS)


@pytest.mark.parametrize("suite,fam,part", VALID_FAMILIES, ids=["%s-%s-%d" % gf for gf in VALID_FAMILIES])
def test_lz_valid_frames_decode_to_their_plaintext(suite, fam, part):
    """every valid frame of the family within MAX_BLOCKS, but the ones SLOW names, alone through zg_lz_frame<256>, taken off the flatten
    path as under ZGPU_FORCE_INORDER: the bytes are the generator's plaintext, the status stays 0"""
    ran, multi, carried, slow, long = [], 0, 0, set(), 0
    nparts = PARTS.get((suite, fam), 1)
    for name, z, plain in SUITES[suite].family(fam)[part::nparts]:
        if name in SLOW.get((suite, fam), {}):
            slow.add(name)
            continue
        e = emu.EmuBatch(z, max_window=1 << 31)
        assert e.parse_status == 0 and e.nframes == 1, name
        if e.nblocks > MAX_BLOCKS:
            long += 1
            continue
        out, verdicts = e.inorder_lz()
        assert verdicts == [(0, e.nblocks)] and out == plain, (name, verdicts)
        facts = batches(e, 256)
        multi += sum(m for _, m in facts)
        carried += sum(1 for n, _ in facts if n > 256)
        ran.append(name)
    print("\n%s %s: %d frames, %d slow, %d long, %d batches of more than one round, %d blocks of more than 256 sequences" % (suite, fam, len(ran), len(slow), long, multi, carried))
    # nothing is left out but what SLOW (every name of it a frame of the family) and LONG (no family of LONG is run in parts) account for
    assert set(SLOW.get((suite, fam), {})) <= {f[0] for f in SUITES[suite].family(fam)} and long == LONG.get((suite, fam), 0), (slow, long)
    assert ran and (multi > 0) == ((suite, fam) not in NO_MULTI_ROUND) and (carried > 0) == ((suite, fam) in CARRY), (multi, carried)


# ---- zg_lz_frame, invalid frames ------------------------------------------------------------------------------------------------

# Frames whose final verdict is not zg_k_lz's: zg_k_seqpost rejects a LATER sequence of the block (offset 0), so the block never reaches
# zg_k_lz; the reference executes in order and meets the unreachable offset in front of it first, which zg_k_exact finds
# (tests/test_exact_cpu.py, tests/test_repframes_cpu.py). zg_lz_frame must leave such a frame at zg_k_seqpost's verdict and block.
DECIDED_BY_EXACT = {"bad_zero_behind_out_of_reach": (ZERO_OFFSET, DICT_TOO_SMALL)}


def oracle_verdict(z):
    d = oracle.FrameDecoder()
    st, c, _, _ = d.init(z)
    assert st == 0
    st, _, _ = d.decode_blocks(z[c:], oracle.STRAT_ALL)
    return st, d.blocks_decoded(), d.held()


def exec_invalid():
    """the invalid frames of the suites that fail in sequence execution, within MAX_BLOCKS (seqframes has no invalid frame; repframes'
    bad_zero_across_block_8192 .. 8199 are too long)"""
    out = [(n, z) for g in (repframes, blockframes) for n, z, _ in g.family("invalid") if g.STATUS[n] in (ZERO_OFFSET, OFFSET_TOO_BIG, DICT_TOO_SMALL)]
    assert "invalid" not in seqframes.FAMILIES and len(out) >= 20
    return [(n, z) for n, z in out if len(blockframes.walk(z)) <= MAX_BLOCKS]


def test_lz_invalid_frames_get_the_oracles_verdict_and_block():
    """the frames that fail in execution: an offset beyond the frame start (zg_lz_frame's own check) and an offset of 0 (found by
    zg_k_seqpost's model in front of it: zg_lz_frame executes the good blocks and leaves the verdict alone) end with the oracle's
    status and failing block, and the good blocks' bytes are the oracle's. DECIDED_BY_EXACT lists the frames zg_k_exact decides"""
    own = left = 0
    for name, z in exec_invalid():
        e = emu.EmuBatch(z, max_window=1 << 31)
        ost, oblk, held = oracle_verdict(z)
        out, [(st, bad)] = e.inorder_lz()
        good = e.inorder_partial(0, bad, 0, False, 0, 0)[1]                  # where block `bad` starts
        if name in DECIDED_BY_EXACT:
            assert (st, ost) == DECIDED_BY_EXACT[name] and bad == oblk, (name, st, bad)
            assert e.exact(drain_rule=0)[0][:2] == (ost, oblk), name
        else:
            assert (st, bad) == (ost, oblk), (name, st, bad, ost, oblk)
        assert out[:good] == held[:good], name
        own += st in (OFFSET_TOO_BIG, DICT_TOO_SMALL)
        left += st == ZERO_OFFSET
    print("\nverdicts of zg_lz_frame's own check: %d, of zg_k_seqpost's left alone: %d" % (own, left))
    assert own >= 5 and left >= 5


# ---- zg_sparse_frame ------------------------------------------------------------------------------------------------------------

def sparse_chain_frame():
    """a sparse frame (few sequences for its blocks) one of whose blocks has 150 sequences, each copying from the match in front of it
    (and some overlapping themselves): batches of 64 that take many rounds, and a block that takes three batches"""
    rng = random.Random(6401)
    seqs, nlit = [], 0
    for i in range(150):
        ll, ml = rng.randint(0, 2), rng.randint(4, 12)
        dist = rng.randint(1, 4) + ll if i else 40        # into the match of the sequence in front (ml >= 4), sometimes shorter than ml
        seqs.append((ll, dist + 3, ml))
        nlit += ll
    blocks = [("raw", rng.randbytes(500)), Block(rng.randbytes(nlit + 7), seqs)] + [("raw", rng.randbytes(20 + i)) for i in range(40)]
    return tabframes.build("sparse_chain_150", blocks, window_log=12)


def test_sparse_body_on_a_block_of_more_than_64_chained_sequences():
    name, z, plain = sparse_chain_frame()
    e = emu.EmuBatch(z, max_window=1 << 31)
    facts = batches(e, 64)
    assert facts == [(150, 3)], facts                                       # every batch of 64 needs more than one round
    out, nsparse = e.inorder_sparse()
    assert nsparse == 1 and out == plain
    for shape in (0, 2):                                                     # ... and behind the real zg_flat1_unit
        st, got, _, _ = test_flat1_cpu.run_flatten(z, 4, shape)
        assert test_flat1_cpu.run_flatten.sparse == [1] and st == 0 and got == plain


def test_sparse_frames_of_the_suites_go_through_the_body():
    """zgemu_flatten runs zg_sparse_frame itself (no model of it is left): the sparse frame of sweepframes' mixed_counts submit in its
    submit, and the sparse frames of blockframes' sources family, decode to their plaintext through it"""
    _, frames = sweepframes.submits()["mixed_counts"]
    z = b"".join(f[1] for f in frames)
    st, got, _, _ = test_flat1_cpu.run_flatten(z, 0, 0)
    nsparse = sum(test_flat1_cpu.run_flatten.sparse)
    assert st == 0 and got == b"".join(f[2] for f in frames) and nsparse >= 1
    e = emu.EmuBatch(z, max_window=1 << 31)
    out, n = e.inorder_sparse()
    assert n == nsparse
    at = 0
    for f, (fname, _, plain) in enumerate(frames):
        if test_flat1_cpu.run_flatten.sparse[f]:
            assert out[at:at + len(plain)] == plain, fname
        at += len(plain)
    nblk = 0
    for name, z, plain in blockframes.family("sources"):
        if emu.Plan(z, unit_blocks=1).frames[0][6]:
            st, got, _, _ = test_flat1_cpu.run_flatten(z, 1, 0)
            assert st == 0 and got == plain, name
            nblk += 1
    assert nblk >= 13, nblk


# ---- zg_partial_block -----------------------------------------------------------------------------------------------------------

def partial_case(z):
    """(e, failing block, nexec, literal length of sequence nexec, the oracle's status, what the oracle holds, bytes of the good blocks):
    nexec as Batch::sync reads it, from the record zg_k_seqpost's model or zg_k_exact's source left for the failing block"""
    ost, oblk, held = oracle_verdict(z)
    e = emu.EmuBatch(z, max_window=1 << 31)
    assert e.parse_status == 0 and e.nframes == 1
    ex = e.exact(drain_rule=0)[0]
    st, bad = (ex[0], ex[1]) if ex[0] else e.frame(0)[2:]
    assert (st, bad) == (ost, oblk), (st, bad, ost, oblk)
    pad = e.block_pad(bad)
    assert 1 <= pad <= e.block(bad)["nseq"]
    sq = e.block_sequences(bad, pad)
    ll = sq[-1][2] - (sq[-2][2] + sq[-2][1] if pad > 1 else 0)
    good = e.inorder_partial(0, bad, 0, False, 0, 0)[1]
    return e, bad, pad - 1, ll, ost, held, good


def check_partial(name, z, total=None, next_lits=None):
    e, bad, nexec, ll, ost, held, good = partial_case(z)
    assert total is None or len(held) == total, (name, len(held))
    lits = ost != NOT_ENOUGH_LITERALS
    want = held[good:]
    room = len(want) + 64
    behind, at, left = e.inorder_partial(0, bad, nexec, lits, room, room)
    assert at == good and left == len(want), (name, at, good, left, len(want))
    assert behind == want + b"\xAA" * 64, name
    # the other setting of lits_of_next: the same without / with the literals of sequence nexec (what NotEnoughLiterals leaves / would not)
    behind, _, left = e.inorder_partial(0, bad, nexec, not lits, room, room)
    if lits:
        assert left == len(want) - ll and behind == want[:left] + b"\xAA" * (room - left), name
    else:                                                                    # (the run is taken at its recorded length; next_lits: the ones the block has)
        assert left == len(want) + ll and behind[:len(want) + len(next_lits)] == want + next_lits and behind[left:] == b"\xAA" * (room - left), name
    # one byte less room than the block leaves: nothing is written at all
    if want:
        behind, _, left = e.inorder_partial(0, bad, nexec, lits, len(want) - 1, room)
        assert left == 0xFFFFFFFF and behind == b"\xAA" * room, name
    return nexec, ll, len(want)


@pytest.mark.parametrize("name,total", [("exec_error_behind_good_blocks.zst", 315891), ("seqbits_240.zst", 2326)])
def test_partial_regression_frames_hold_what_the_oracle_holds(name, total):
    """the two frames of tests/test_gpu_api_soak.py: the good blocks' bytes plus zg_partial_block's output are the oracle's held();
    seqbits_240 has a block beyond 128 KiB in front (the records' position fields wrap, the frame is zg_k_lz's)"""
    z = open(os.path.join(HERE, "golden", "regress", name), "rb").read()
    nexec, ll, n = check_partial(name, z, total)
    print("\n%s: %d sequences executed, %d literals of the next, %d bytes behind the good blocks" % (name, nexec, ll, n))
    assert n > 0


def not_enough_literals_frame():
    """a block whose third sequence asks for more literals than are left behind a chain of matches (NotEnoughLiterals: its literals are
    not pushed, sequence_execution.rs:14-19)"""
    rng = random.Random(6402)
    seqs = [(3, 50 + 3, 9), (2, 4 + 3, 20)] + [(1, rng.randint(2, 6) + 3, rng.randint(3, 9)) for _ in range(70)] + [(9, 5 + 3, 4), (1, 6, 3)]
    nlit = sum(s[0] for s in seqs[:-2]) + 4                                 # the last but one sequence finds 4 of its 9 literals
    lits = rng.randbytes(nlit)
    return tabframes.build("partial_not_enough_literals", [("raw", rng.randbytes(300)), Block(lits, seqs)], valid=False) + (lits[-4:],)


def test_partial_invalid_frames_with_and_without_the_literals_of_the_failing_sequence():
    """the invalid frames of repframes and blockframes that fail in execution (lits_of_next set: the reference has pushed the failing
    sequence's literals, sequence_execution.rs:20-38) and a frame that runs out of literals (clear), each also with the other setting
    and with a limit one byte short"""
    cases = exec_invalid()
    nel, z, _, found = not_enough_literals_frame()
    assert oracle_verdict(z)[0] == NOT_ENOUGH_LITERALS
    cases.append((nel, z))
    some = lits_seen = chained = 0
    for name, z in cases:
        nexec, ll, n = check_partial(name, z, next_lits=found if name == nel else None)
        some += n > 0
        lits_seen += ll > 0
        chained += nexec > 64
    print("\n%d frames, %d leave bytes behind the good blocks, %d with literals of the failing sequence, %d of more than 64 sequences" % (len(cases), some, lits_seen, chained))
    assert some >= 5 and lits_seen >= 3 and chained >= 2
