"""Frames built from chosen table descriptions (tests/tabframes.py) through the CPU harness: Huffman weights and FSE normalised
counts no encoder emits. Every valid frame is checked against its plaintext (a plain LZ77 execution of what the writer was given)
and block by block against the oracle's intermediates; every invalid one must get the oracle's status; the coverage test asserts
that the families really reach what they aim at. The harness builds its tables with the serial builders of zg_dev.h: the wave
builders of zg_k_tables and zg_k_ftab are proven by tests/test_gpu_tabframes.py on the same frames."""
import pytest

import emu
import framesuite
import tabframes

VALID = [f for f in sorted(tabframes.FAMILIES) if f != "invalid_tables"]


@pytest.mark.parametrize("fam", VALID)
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per-block literals, sequences, offset history, Huffman and FSE tables == the oracle's;
    zg_k_exact's source (drain rule 1) accepts"""
    for name, z, plain in tabframes.family(fam):
        framesuite.check_on_harness(name, z, plain, tabframes.STATUS)


def test_invalid_frames_get_the_oracles_status():
    bad = [(name, emu.decode_all_verdict(z), tabframes.STATUS[name]) for name, z, _ in tabframes.family("invalid_tables")]
    assert [b for b in bad if b[1] != b[2]] == []


def test_libzstd_differs_is_short():
    """the cap of the issue: at most a tenth of the valid frames, and only frames the oracle accepts (all_frames() asserts it)"""
    frames = tabframes.all_frames()
    valid = [f for f in frames if f[3] is not None]
    assert len(tabframes.LIBZSTD_DIFFERS) * 10 <= len(valid)
    assert all(reason for reason in tabframes.LIBZSTD_DIFFERS.values())


def test_coverage():
    """what the families reach, from the writer's own records: the weight counts at the slot edges of zg_k_tables (symbol = lane +
    64 * k) and at the direct form's limit, 256 weights, every max_bits from 1 to 11 asked for, a 1024-entry run and several
    whole-wave runs in one table, weight streams of both parities at accuracy logs 5 and 6, descriptions of 127 and 128 bytes;
    per field accuracy log 5 and the maximum and the highest symbol; a 0-bit state, a table of low-probability cells only, a
    single-symbol table, a final count in each form; every state and symbol a walk can reach visited where the block has 3 x the table's size in
    sequences; both sections at each byte alignment; a literals section under 136 bytes; three long descriptions (139 bytes) in front
    of a bitstream past the staged row; the statuses the invalid frames reach, OF's RLE byte 31 accepted and 32 refused"""
    cov = tabframes.coverage(tabframes.all_frames())
    print("\ncoverage:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items() if k != "status_of"})
    assert cov["nw"] >= set(tabframes.NW_LIST) | {256}, cov["nw"]
    assert cov["max_bits"] >= {1, 2, 3, 8, 11}, cov["max_bits"]
    assert cov["largest_run"] == 1024 and cov["whole_wave_runs"] >= 6
    assert cov["huf_fse_al"] == {5, 6} and cov["weight_parity"] == {0, 1}
    assert cov["desc_bytes"] >= {127, 128}
    assert cov["al"]["LL"] >= {5, 9} and cov["al"]["OF"] >= {5, 8} and cov["al"]["ML"] >= {5, 9}, cov["al"]
    assert cov["high"] == {"LL": 35, "OF": 31, "ML": 52}, cov["high"]
    assert cov["zero_bit"] and cov["all_low"] and cov["single"]
    assert cov["last_forms"] == {"short", "long"}
    assert cov["states"][1] > 3000 and cov["walks_short"] == [], cov["walks_short"]   # a block of 3 x the table's size visits every state
    assert cov["lit_align"] == {0, 1, 2, 3} and cov["seq_align"] == {0, 1, 2, 3}, (cov["lit_align"], cov["seq_align"])
    assert cov["min_comp"] < 136, cov["min_comp"]
    assert cov["long_desc"][0] == 43 + 34 + 62 and cov["long_desc"][1] > 336, cov["long_desc"]
    assert cov["status_of"]["bad_rle_of31_executes"] >= 50 and cov["status_of"]["bad_rle_OF_byte32"] == 43
    assert cov["statuses"] >= {30, 36, 40, 41, 43}, cov["statuses"]
    assert cov["valid"] >= 190 and cov["invalid"] >= 40
