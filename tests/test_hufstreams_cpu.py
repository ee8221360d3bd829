"""Frames built from chosen Huffman streams (tests/hufstreams.py) through the CPU harness: streams no encoder emits, at the edges
of zg_k_huf's windows. Every valid frame is checked against its plaintext and block by block against the oracle's intermediates,
every invalid one must get the oracle's status, and the SOURCE of zg_k_huf (zstd-rs_amd/csrc/zg_huf.h on the SIMT emulator of
tests/emu, as in tests/test_huf_cpu.py) must give serial_decode's literals and counts for every stream, in the arena and, for the
blocks without sequences, straight in the output. The coverage test asserts that the families reach what they aim at. The GPU
build of the same source is checked on the same frames by tests/test_gpu_hufstreams.py."""
import pytest

import framesuite
import hufstreams
from hufstreams import META, STATUS
from test_huf_cpu import _lib, check_against_model, run_huf

FAMS = sorted(hufstreams.FAMILIES)


@pytest.mark.parametrize("fam", FAMS)
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per-block literals, sequences, offset history and Huffman tables == the oracle's; an invalid
    frame gets the oracle's status"""
    for name, z, plain in hufstreams.family(fam):
        framesuite.check_on_harness(name, z, plain, STATUS)


def _kernel_source(name, z, plain, direct):
    """zg_huf.h on the frame: every block's literals (where the kernel put them) and per-stream counts against serial_decode, the
    status against the oracle's. Four streams that are not split the way the format says end with a count mismatch here and the
    true counts, which is what zg_k_huf_uneven starts from"""
    L = _lib()
    e, lit, dst, st, cnt = run_huf(z, direct)
    recs = iter(META[name]["hs"])
    for b in range(e.nblocks):
        k = e.block(b)
        if k["btype"] != 2:
            continue
        rec = next(recs)
        lens = [len(x) for x in rec["decoded"]]
        want = b"".join(rec["decoded"])
        even = len(lens) == 1 or lens == hufstreams.split4(rec["regen"])
        if plain is None and direct and k["nseq"] == 0 and not k["active"]:
            continue                                        # (the harness lays the output out from its serial decode, which has refused the block: the kernel leaves it alone)
        if len(lens) == 4:
            assert list(cnt[4 * b:4 * b + 4]) == lens, (name, b, list(cnt[4 * b:4 * b + 4]), lens)
        if plain is None:
            assert int(st[b]) & 0xFF == STATUS[name], (name, b, hex(int(st[b])))
            continue
        if not even:
            assert int(st[b]) & 0xFF == 35 and sum(lens) == k["regen_size"], (name, b, hex(int(st[b])))
            continue
        assert st[b] == 0 and k["regen_size"] == len(want), (name, b, hex(int(st[b])))
        if direct and k["nseq"] == 0:
            at = L.zgemu_block_out_base(e.h, b)
            got = dst[at:at + len(want)].tobytes()
        else:
            at = L.zgemu_block_lit_base(e.h, b)
            got = lit[at:at + len(want)].tobytes()
        assert got == want, (name, b, "direct" if direct else "arena")
    assert next(recs, None) is None, name


@pytest.mark.parametrize("fam", FAMS)
def test_kernel_source_against_serial_decode(fam):
    """every frame whose blocks parse, in the arena; the frames without sequences once more with ZG_FLAG_LIT_DIRECT"""
    for name, z, plain in hufstreams.family(fam):
        _kernel_source(name, z, plain, False)
        if name.endswith("_n"):
            _kernel_source(name, z, plain, True)


def test_kernel_source_against_the_serial_model():
    """tests/test_huf_cpu.py's own check (the harness's serial model of the literals) on the small frames of every family"""
    seen = 0
    for fam, name, z, plain in hufstreams.valid_frames():
        if len(z) > 6000 or "uneven" in name:
            continue
        seen += check_against_model(z)
        check_against_model(z, direct=True)
    assert seen >= 100


def test_libzstd_differs_is_short():
    frames = hufstreams.all_frames()
    valid = [f for f in frames if f[3] is not None]
    assert len(hufstreams.LIBZSTD_DIFFERS) * 10 <= len(valid)
    assert all(reason for reason in hufstreams.LIBZSTD_DIFFERS.values())


def test_coverage():
    """hufstreams.coverage asserts, with a model of the kernel's chunking that reads the chunk sizes out of zg_huf.h: a window of 60
    to 63 redo rounds in every four-stream frame of a code that never re-synchronises and none for the control; a chunk of exactly
    ZG_HP_ROWS symbols without a switch and one of ZG_HP_ROWS + 1 with it, in lane 0, in a later lane and in the second window, at
    least two dense windows behind the switch; the stream lengths at the chunk and window edges, the eight payload widths of the
    last byte and a lone marker byte; the 16 start alignments for a single stream and for a later one of four, under 0xBA and
    0xFF; a last code 1, 5 and 10 bits below the start in a single stream (valid, at each of the 16 start alignments under 0xBA: the
    zeroing of the staged piece that straddles the start; invalid with a count one short) and in each of four streams (status 34); four streams of 4 .. 12 literals, streams without a symbol, an uneven split; 1, 2, 3 and 5 streams
    on one table slot and a long stream grouped with a short one in both orders; every family with and without sequences"""
    cov = hufstreams.coverage(hufstreams.all_frames())
    print("\ncoverage:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    assert cov["valid"] >= 200 and cov["invalid"] >= 30
    assert cov["statuses"] >= {34, 35}
    assert cov["two_defects"] == 34                         # the stream's end is checked before the count (literals_section_decoder.rs:116-155)
    assert all(v == 0 for v in cov["tiny"].values())       # the reference accepts 1 .. 12 literals in four streams
