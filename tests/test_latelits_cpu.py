"""Frames whose literals verdict arrives after the scan (tests/latelits.py) through the CPU harness and the generator's own checks.
The harness decodes literals in front of its scan (k_huf, k_seq, k_scan: the early order), so what it proves here is that the early
order gives the oracle's verdict on every one of these frames, the baseline the late order on the GPU (zg_k_merge and zg_k_litfix
behind zg_k_scan, tests/test_gpu_latelits.py) is compared with. compose() has asserted for every frame, when it was built, that
the verdict and the failing block predicted from the reference's order are the oracle's; test_prediction_is_the_oracles repeats
that from the records, and test_coverage asserts the matrix of (literal defect, with or without sequences, stage of the other
defect, relation) with its list of cells the format does not allow."""
import pytest

import framesuite
import latelits
import oracle
from latelits import GOOD, META, STATUS

FAMS = sorted(latelits.FAMILIES)


@pytest.mark.parametrize("fam", FAMS)
def test_family_on_the_harness(fam):
    """an invalid frame gets the oracle's status; a valid one decodes to its plaintext and agrees block by block with the oracle"""
    for name, z, plain in latelits.family(fam):
        framesuite.check_on_harness(name, z, plain, STATUS)


def test_prediction_is_the_oracles():
    """every invalid frame: the oracle's status, failing block and held bytes are STATUS, META's bad_block and GOOD, and the frame
    re-headered with a content size gets the same verdict (the reference never checks the value)"""
    n = 0
    for _, name, z, plain in latelits.invalid_frames():
        for zz in (z, latelits.with_content_size(z, 4096 + META[name]["nblocks"])):
            d = oracle.FrameDecoder()
            st, c, _, _ = d.init(zz)
            assert st == 0 and c == (6 if zz is z else 14), name
            st, _, _ = d.decode_blocks(zz[c:], oracle.STRAT_ALL)
            assert (st, d.blocks_decoded()) == (STATUS[name], META[name]["bad_block"]), name
            assert d.held()[:len(GOOD[name])] == GOOD[name], name
        n += 1
    assert n >= 400


def test_with_content_size_on_valid_frames():
    for _, name, z, plain in latelits.valid_frames()[::7]:
        zz = latelits.with_content_size(z, len(plain))
        out, d = oracle.decode_frame_all(zz)
        assert out == plain and d.content_size() == len(plain), name


def test_coverage():
    """latelits.coverage asserts: every (kind 30 .. 35, without / with sequences, stage, relation) cell but the skipped ones, each of
    those with its reason; every defect code of every stage; every variant (single stream and each of four) without and with
    sequences; every geometry index for every N, the pairs one stride apart, the three sides of lim and the two of an offset too
    far; the oracle's verdicts 30 .. 35 and every other stage's; frames in which the literal defect wins, in which the other wins by
    block order and in which it wins in the same block"""
    cov = latelits.coverage(latelits.all_frames())
    print("\ncoverage:", {k: (sorted(v, key=repr) if isinstance(v, set) else v) for k, v in cov.items() if k != "skipped"})
    print("skipped cells:", len(cov["skipped"]), sorted(set(cov["skipped"].values())))
    assert all(cov["skipped"].values()) and all(cov["skipped_variants"].values())
    assert not [c for c in cov["skipped"] if c[3] != "same"]          # only "in the same block" is ever impossible
    assert cov["valid"] >= 400 and cov["invalid"] >= 400
    # nothing of the geometry family is skipped: every index of every N is there (coverage asserts the set)
    assert len(cov["geo_at"]) == sum(1 for n in latelits.GEO_N for a in set(latelits.GEO_AT + (n - 1,)) if a < n)
