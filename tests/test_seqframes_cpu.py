"""Frames built from chosen sequences (tests/seqframes.py) through the CPU harness: the kernel bodies of zg_huf.h, zg_flat1.h,
zg_flat4.h and zg_exact.h and the lane routines, on inputs whose sequences sit at the constants where the kernels go wrong. Each
frame is checked against its plaintext (a plain LZ77 execution of the sequences) and block by block against the oracle's
intermediates; the coverage test asserts that the families really reach those constants."""
import pytest

import blockcheck
import emu
import framesuite
import seqframes
import test_flat1_cpu
import test_flat4_cpu


@pytest.mark.parametrize("fam", sorted(seqframes.FAMILIES))
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per-block literals, sequences, offset history, Huffman and FSE tables == the oracle's;
    zg_k_exact's source (drain rule 1) accepts"""
    for name, z, plain in seqframes.family(fam):
        framesuite.check_on_harness(name, z, plain, None)


def test_single_block_frames_hold_their_sequences():
    """libzstd encodes exactly the sequences asked for: nseqN frames hold one compressed block of N sequences, the exact-block frames
    one of 131072 bytes"""
    for name, z, plain in seqframes.family("seq_counts") + seqframes.family("block_sizes") + seqframes.family("match_lengths"):
        e = emu.EmuBatch(z)
        if name.startswith("nseq"):
            assert e.nblocks == 1 and e.block(0)["btype"] == 2 and e.block(0)["nseq"] == int(name[4:]), name
        if "exact" in name:
            assert e.nblocks == 1 and len(plain) == seqframes.BLOCK, name


@pytest.mark.parametrize("fam", sorted(seqframes.FAMILIES))
def test_flatten_bodies(fam):
    """zg_flat4.h (direct units) and zg_flat1.h (pointer-mode units, one and two blocks per unit, on frames of more than one block):
    the scratch words == tests/lz_model.py's effective offsets, the bytes after the sweep model == the plaintext. A frame that is
    sparse (zg_k_sparse copies its matches) writes no scratch: bytes only. The short- and far-offset families run three tile
    shapes of zg_flat4.h and two of zg_flat1.h; the others, and frames of more than 2 MiB, run the GPU's (3 for zg_flat4.h, 2
    for zg_flat1.h). far_w24 (17 MB, about 90 s in the emulator) is left to the GPU tests."""
    nsparse = npointer = 0
    for name, z, plain in seqframes.family(fam):
        if name == "far_w24":
            continue
        big = len(plain) > 2 << 20 or fam not in ("short_offsets", "far_offsets")
        for shape in ((3,) if big else (0, 2, 3)):
            st, got, _ = test_flat4_cpu.run_flat4(z, 256, shape)
            assert st == 0 and got == plain, (name, shape)
        if len(blockcheck.oracle_blocks(z)) < 2:
            continue
        for ub, shape in (((2, 2),) if big else ((1, 0), (2, 2))):
            st, got, og, units = test_flat1_cpu.run_flatten(z, ub, shape)
            assert st == 0 and got == plain, (name, ub, shape)
            if test_flat1_cpu.run_flatten.sparse == [1]:
                nsparse += 1
                continue
            npointer += test_flat1_cpu.check_scratch(z, ub, shape)
    if fam in ("short_offsets", "far_offsets"):
        assert npointer >= (6 if fam == "short_offsets" else 40), npointer
    assert nsparse >= (1 if fam == "short_offsets" else 0), nsparse


def test_coverage():
    """what the families reach, walked with the CPU harness. Every literal type and stream count (raw, RLE, Huffman and treeless
    with 1 and 4 streams), every FSE mode (predefined, RLE, compressed, repeat) for LL, OF and ML, every repeat-offset form with
    LL == 0 and LL > 0, nseq from 0 to >= 0x7F00, ML up to 131072 (not 131074: ML code 52 can say it, but no block holds more than
    131072 bytes), LL 0 .. >= 131060, an offset equal to its frame's window size, a 131072-byte block."""
    cov = seqframes.coverage([z for _, _, z, _ in seqframes.all_frames()])
    print("\ncoverage:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    assert cov["lit"] >= {(0, 0), (1, 0), (2, 1), (2, 4), (3, 1), (3, 4)}, cov["lit"]
    for k in ("LL", "OF", "ML"):
        assert cov["fse"][k] == {0, 1, 2, 3}, (k, cov["fse"][k])
    assert cov["rep"] == {(z, of) for z in (False, True) for of in (1, 2, 3)}, cov["rep"]
    assert cov["nseq"][0] == 0 and cov["nseq"][1] >= 0x7F01 and cov["nseq"][1] == (seqframes.BLOCK - 64) // 3
    assert cov["ml"] == [3, 131072]
    assert cov["ll"][0] == 0 and cov["ll"][1] >= 131060
    assert cov["offset"][0] == 1 and cov["offset"][1] == 1 << 24
    assert cov["offset_eq_window"] >= 4
    assert cov["block_out_max"] == seqframes.BLOCK
