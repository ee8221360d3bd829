"""Frames of chosen non-sequence blocks (tests/blockframes.py) through the CPU harness: Raw, RLE and literal-only compressed blocks
at the edges of zg_k_lit, zg_wg_copy and zg_wg_fill, and as the sources of matches in the blocks behind them (the skip of such
blocks in zg_flat1.h and zg_flat4.h, the gathers of the sweep model). The harness writes these blocks with a serial model, so the
kernel itself is proven by tests/test_gpu_blockframes.py on the same frames; here every frame is checked against its plaintext (a
plain LZ77 execution of what the writer was given) and block by block against the oracle's intermediates, every invalid one must
get the oracle's status, and the coverage test asserts that the families reach what they aim at."""
import pytest

import blockframes
import emu
import framesuite
import test_flat1_cpu
import test_flat4_cpu

VALID = [f for f in blockframes.FAMILIES if f != "invalid"]


@pytest.mark.parametrize("fam", VALID)
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per-block literals, sequences, offset history, Huffman and FSE tables == the oracle's;
    zg_k_exact's source (drain rule 1) accepts"""
    for name, z, plain in blockframes.family(fam):
        framesuite.check_on_harness(name, z, plain, blockframes.STATUS)


def test_batch_alignment_order():
    """the submit order of blockframes.batch_alignment in one harness run: every frame's bytes, and each representative frame at
    every residue mod 16 of the output"""
    order, where = blockframes.batch_alignment()
    e = emu.EmuBatch(b"".join(z for _, z, _ in order), max_window=1 << 31)
    assert e.parse_status == 0 and e.nframes == len(order)
    for f, (name, _, plain) in enumerate(order):
        out, st = e.frame_bytes(f)
        assert st == 0 and out == plain, (f, name)
    for name, idx in where.items():
        assert sorted(e.frame(f)[0] % 16 for f in idx) == list(range(16)), name


def test_invalid_frames_get_the_oracles_status():
    bad = [(name, emu.decode_all_verdict(z), blockframes.STATUS[name]) for name, z, _ in blockframes.family("invalid")]
    assert [b for b in bad if b[1] != b[2]] == []


@pytest.mark.parametrize("fam", ["sources", "neighbours", "lit_alignment"])
def test_flatten_bodies(fam):
    """zg_flat4.h (direct units, three tile shapes) and zg_flat1.h (pointer-mode units of one, two and three blocks): the bytes after
    the sweep model == the plaintext, and where the frame is not sparse the scratch words == tests/lz_model.py's effective offsets.
    Blocks without sequences are skipped by both bodies (unit_size = bu0 + blk.regen_size) and read by the matches behind them.
    The sources family runs three tile shapes of zg_flat1.h; the other two have no sequences, so every unit of theirs leaves the
    body at once (u.noseq), which the smallest shape shows as well as the largest (the emulator's cost is a fiber per thread)"""
    nsparse = npointer = 0
    for name, z, plain in blockframes.family(fam):
        for shape in (0, 2, 3):
            st, got, _ = test_flat4_cpu.run_flat4(z, 256, shape)
            assert st == 0 and got == plain, (name, shape)
        if len(blockframes.walk(z)) < 2:
            continue
        for ub, shape in ((1, 0), (2, 2), (3, 3)) if fam == "sources" else ((1, 0), (2, 0), (3, 0)):
            if emu.Plan(z, unit_blocks=ub).frames[0][6]:
                st, got, og, units = test_flat1_cpu.run_flatten(z, ub, shape)
                assert test_flat1_cpu.run_flatten.sparse == [1]
                nsparse += 1
            else:
                npointer += test_flat1_cpu.check_scratch(z, ub, shape)           # (asserts the status and the oracle's bytes itself)
                st, got = 0, test_flat4_cpu.oracle_plain(z)
            assert st == 0 and got == plain, (name, ub, shape)
    if fam == "sources":
        assert nsparse >= 3 * 13 and npointer >= 3 * 26 * 3, (nsparse, npointer)


def test_libzstd_differs_is_short_and_true():
    """at most a tenth of the valid frames, only frames the oracle accepts (all_frames() asserts both), each with its reason, and
    each really not returned by libzstd"""
    import zgdata
    valid = {n: (z, p) for _, n, z, p in blockframes.valid_frames()}
    assert len(blockframes.BLOCK_LIBZSTD_DIFFERS) * 10 <= len(valid)
    for name, reason in blockframes.BLOCK_LIBZSTD_DIFFERS.items():
        assert reason
        z, plain = valid[name]
        try:
            got = zgdata.zstd_decompress(z, len(plain))
        except RuntimeError:
            got = None
        assert got != plain, name


def test_coverage():
    """what the families reach, walked with the CPU harness: every kind of block at every size of blockframes.SIZES it can hold
    (blockframes.can_hold has the format's reasons), 131072 bytes in every kind that can have them; in the alignment family every
    destination residue mod 8 with every source residue, for every kind and size; every ordered pair of kinds straddled by a
    match source; sources that begin in the last 1 .. 8 bytes of a block without sequences; self-overlapping matches at offsets
    1 .. 16, 31 .. 33 and 63 .. 65 with the period in a Raw and in an RLE block; the frame's first byte in an RLE block; every form
    in a first unit, in a later unit and across a unit without sequences; blocks without sequences between blocks with sequences
    inside one unit and last in the frame; sparse frames and others"""
    frames = blockframes.valid_frames()
    cov = blockframes.coverage([(n, z) for _, n, z, _ in frames])
    fams = {}
    for fam, n, z, _ in frames:
        fams.setdefault(fam, [0, 0])
        fams[fam][0] += 1
        fams[fam][1] += len(blockframes.walk(z))
    print("\nframes and blocks per family:", fams, "invalid:", len(blockframes.invalid_frames()))
    show = lambda v: sorted(v) if isinstance(v, set) else {k: show(x) for k, x in v.items()} if isinstance(v, dict) else v   # noqa: E731
    print("coverage:", {k: show(v) for k, v in cov.items() if k != "residues"})
    print("residue pairs per (kind, size):", sorted(set(len(v) for v in cov["residues"].values())), "in", len(cov["residues"]), "cells")
    six = sorted(set(blockframes.KIND6.values()))
    for kind in blockframes.KINDS:
        assert cov["sizes"][kind] >= blockframes.sizes_for(kind), (kind, sorted(blockframes.sizes_for(kind) - cov["sizes"][kind]))
    # what can_hold leaves: all of SIZES for Raw and RLE blocks, all but 0 for RLE literals, 131067 / 131068 at the top for raw literals,
    # the sizes below 1024 for one Huffman stream, and for four streams the sizes whose last stream is not empty
    everything = set(blockframes.SIZES)
    assert blockframes.sizes_for("raw") == blockframes.sizes_for("rle") == everything
    assert blockframes.sizes_for("lit_rle") == everything - {0}
    assert blockframes.sizes_for("lit_raw") == everything - {131071, 131072} | {131067, 131068}
    for k in ("lit_huf1", "lit_treeless1"):
        assert blockframes.sizes_for(k) == {n for n in everything if 1 <= n <= 25}
    for k in ("lit_huf4", "lit_treeless4"):
        assert blockframes.sizes_for(k) == everything - {0, 1, 2, 3, 5, 6, 9}
    for k in blockframes.KINDS:                          # (one stream: the sources family has blocks of up to 40 bytes)
        assert cov["largest"][k] == max(blockframes.sizes_for(k)) or k.endswith("1") and 25 <= cov["largest"][k] < 1024, (k, cov["largest"])
    both = {(d, s) for d in range(8) for s in range(8)}
    for kind in blockframes.KINDS:
        for n in blockframes.ALIGN_SIZES:
            if blockframes.can_hold(kind, n):
                assert cov["residues"][(kind, n)] == both, (kind, n)
    assert {k for k, n in cov["residues"]} == set(blockframes.KINDS)
    assert cov["pairs"] >= {(a, b) for a in six for b in six}, cov["pairs"]
    assert cov["tails"] == set(range(1, 9)), cov["tails"]
    assert cov["overlap"] >= {(k, o) for k in ("raw", "rle") for o in blockframes.OVERLAP_OFFS}, cov["overlap"]
    assert cov["first_byte_rle"] >= 3
    for form in ("inside", "straddle", "tail", "overlap", "first_byte"):
        assert cov["forms"][form] == {"first", "later", "across"}, (form, cov["forms"][form])
    assert cov["noseq_units_between"] >= 36 and cov["ns_between_seq_in_unit"] >= 36 and cov["ns_last_in_frame"] >= 36
    assert cov["sparse"] >= 13 and cov["dense"] >= 26
