"""zg_k_seqsize's source (zstd-rs_amd/csrc/zg_seqsize.h) on the CPU, under the SIMT emulator (tests/emu/zg_emu_seqsize.cpp): per block with
sequences the kernel's sum of literal lengths, sum of match lengths and status against the oracle's sequences of that block. The inputs are
the seam frames of tests/test_gpu_prefix_edges.py (the kernel takes 8 sequences per thread, 512 per wave and 2048 per pass, as zg_k_seqpost
does: the same seams), the extra-bit frames of tests/seqstreams.py — so == 31 and 32, the LL codes 30 .. 35 and ML codes 43 .. 52 a valid
frame can hold, every (pa & 3, q_ll & 7) pair of the three-dword read, each frame at four alignments of the input — and two blocks at
the one verdict the sums decide here: literal lengths that add up to exactly the block's literals, and to one more. The harness counts
every dword the kernel is served from outside the dwords that hold a block's bitstream — none may be — and every dword the buffer
resource refuses: never the first of a load, the one that holds the field's lowest bit."""
import ctypes as C

import pytest

import blockcheck
import lanesuite
import seqstreams
import tabframes
from test_gpu_prefix_edges import NSEQ, _seam_frame

NOT_ENOUGH_LITERALS = 50
IDENTITY = [1 << 30, 2 << 30, 3 << 30]


class SzBlock(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("frame", "block", "nseq", "regen", "front_status", "status", "sum_ll", "sum_ml")] + [
        ("hist", C.c_uint32 * 3), ("pad", C.c_uint32), ("nbytes", C.c_uint32), ("lead", C.c_uint32)]


def _declare(L):
    L.sz_run.restype = C.c_int32
    L.sz_run.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(SzBlock), C.POINTER(C.c_uint64 * 4)]
    L.sz_per_thread.restype = C.c_uint32


built = lanesuite.built_fixture("zg_emu_seqsize.cpp", "seqsize", extra_sources=lanesuite.HOST_PARSE, declare=_declare)


def run(L, z, shift=0):
    """[SzBlock] of the blocks with sequences of z, and the reader's counts (loads, dwords from outside, dwords refused, first dwords refused)"""
    cap = 4096
    out, counts = (SzBlock * cap)(), (C.c_uint64 * 4)()
    n = L.sz_run(z, len(z), shift, cap, out, C.byref(counts))
    assert 0 <= n <= cap, n
    return list(out[:n]), list(counts)


def oracle_sums(ob):
    """[(sum of literal lengths, sum of match lengths, number of sequences)] of the oracle's blocks that have sequences"""
    return [(sum(s[0] for s in r["sequences"]), sum(s[1] for s in r["sequences"]), len(r["sequences"]))
            for r in ob if r["type"] == 2 and r["sequences"]]


def check_valid(L, name, z, ob, shifts):
    want = oracle_sums(ob)
    seen = set()
    for shift in shifts:
        got, counts = run(L, z, shift)
        assert len(got) == len(want), (name, len(got), len(want))
        for g, (ll, ml, n) in zip(got, want):
            assert (g.front_status, g.status, g.nseq, g.sum_ll, g.sum_ml) == (0, 0, n, ll, ml), (name, shift, g.block, g.status, g.sum_ll, ll, g.sum_ml, ml)
            assert list(g.hist) == IDENTITY and g.pad == 0, (name, g.block)
            seen.add(g.lead)
        assert counts[1] == 0 and counts[3] == 0 and (counts[0] > 0) == bool(want), (name, shift, counts)
        assert counts[2] <= 2 * counts[0]                 # (only a load's second and third dword may lie behind the stream)
    return seen


def test_sequences_per_thread_is_what_the_seams_are_built_for(built):
    assert built.sz_per_thread() == 8     # (another count: add blocks with nseq at its own thread, wave and pass seams +- 1)


@pytest.mark.parametrize("n", NSEQ)
def test_seam_frames(built, n):
    """1 .. 4097 sequences: the thread, row, wave and pass seams of the scans and of the cross-wave step, the partial last thread"""
    for shift in (0, 3, 4):
        name, z, plain = _seam_frame(n, shift)
        assert plain is not None
        ob = blockcheck.oracle_blocks(z)
        assert n in [k for _, _, k in oracle_sums(ob)]
        check_valid(built, name, z, ob, (shift % 4,))


def test_extra_bit_frames(built):
    """every valid frame of tests/seqstreams.py at the four alignments of its input: the bit rates, the codes with the most extra bits and
    every phase of the three-dword read (tests/test_seqstreams_cpu.py asserts what they reach)"""
    leads, blocks = set(), 0
    for _, name, z, plain in seqstreams.valid_frames():
        ob = seqstreams.oracle_blocks(name, z)
        leads |= check_valid(built, name, z, ob, range(4))
        blocks += len(oracle_sums(ob))
    assert leads == {0, 1, 2, 3} and blocks >= 45
    cov = seqstreams.coverage(seqstreams.all_frames())
    assert {31, 32} <= cov["so"]["valid"] and len(cov["pairs"]["valid"]) == 32


def test_literal_lengths_at_the_blocks_literals(built):
    """the literal lengths add up to exactly Regenerated_Size: accepted; to one more: NotEnoughLiterals — in one pass and in the third"""
    import random
    rng = random.Random(0x512E)
    for nseq in (5, 4100):
        seqs = [(rng.randint(0, 3), 4 + rng.randint(0, 40), rng.randint(3, 9)) for _ in range(nseq)]   # (new offsets of 1 .. 41: inside the raw block)
        total = sum(s[0] for s in seqs)
        front = ("raw", rng.randbytes(64))
        name, z, plain = tabframes.build("sz_exact_%d" % nseq, [front, tabframes.Block(rng.randbytes(total), seqs)], differs={})
        assert plain is not None
        (g,), counts = run(built, z)
        assert (g.status, g.regen, g.sum_ll, g.sum_ml, g.nseq) == (0, total, total, sum(s[2] for s in seqs), nseq) and counts[1] == 0 and counts[3] == 0
        name, z, plain = tabframes.build("sz_short_%d" % nseq, [front, tabframes.Block(rng.randbytes(total - 1), seqs)], valid=False)
        assert plain is None and tabframes.STATUS[name] == NOT_ENOUGH_LITERALS
        (g,), counts = run(built, z)
        assert (g.front_status, g.status, g.regen, g.sum_ll, g.nseq) == (0, NOT_ENOUGH_LITERALS, total - 1, total, nseq), (g.status, g.sum_ll, total)
        assert counts[1] == 0 and counts[3] == 0
