"""Frames built from chosen sequence bitstreams (tests/seqstreams.py) through the CPU harness and the oracle. zg_k_seq itself runs
on the GPU only (tests/test_gpu_seqstreams.py); here the frames are proven to be what they claim: every valid frame decodes to its
plaintext in the harness and agrees block by block with the oracle's intermediates, every invalid one gets the oracle's status,
serial_sequences (the plain reference of the bitstream) returns the oracle's sequences, and the coverage test asserts that the
families reach the kernel's limits: ZG_SEQ_CH x 89 bits in a phase, all 512 ring residues, and in the valid frames so == 31 and 32
and every (pa & 3, q_ll & 7) pair of zg_k_seqpost's read.

The frames are built once per module: 3.7 s here for all six families (94 frames, 240 MB of plaintext, of which three frames over
64 MiB of RLE blocks are 210 MB), measured alone on an idle machine."""
import pytest

import emu
import framesuite
import seqstreams
from seqstreams import CH, META, RING, STATUS

FAMS = sorted(seqstreams.FAMILIES)


@pytest.mark.parametrize("fam", FAMS)
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per-block literals, sequences, offset history and FSE tables == the oracle's; an invalid frame gets
    the oracle's status. The harness takes blocks that regenerate more than 128 KiB and the 64 MiB histories as they are"""
    for name, z, plain in seqstreams.family(fam):
        framesuite.check_on_harness(name, z, plain, STATUS, lambda z: seqstreams.oracle_blocks(name, z))


def test_ring_submit_in_the_harness():
    """the ZG_SEQ_RING copies of ring_mod as one input: every copy decodes to the plaintext"""
    z, plain, n = seqstreams.ring_submit()
    e = emu.EmuBatch(z)
    assert e.parse_status == 0 and e.nframes == n
    assert all(e.frame_bytes(f) == (plain, 0) for f in range(n))


def test_serial_sequences_against_the_oracle():
    """serial_sequences of every bitstream of every valid frame returns the oracle's last_sequences() of that block"""
    seen = 0
    for _, name, z, _ in seqstreams.valid_frames():
        comp = [r for r in seqstreams.oracle_blocks(name, z) if r["type"] == 2 and r["sequences"]]
        recs = META[name]["ss"]
        assert len(comp) == len(recs), name
        for rec, o in zip(recs, comp):
            assert rec["status"] == 0 and rec["remaining"] == 0, name
            assert rec["seqs"] == [(ll, ml, of) for ll, ml, of, _ in o["sequences"]], (name, rec["block"])
            assert sum(rec["bits"]) == rec["first"], name
            seen += len(rec["seqs"])
    assert seen >= 4000


def test_libzstd_differs():
    frames = seqstreams.all_frames()                     # (asserts: only valid frames, at most a fifth, one reason)
    assert len(seqstreams.LIBZSTD_DIFFERS) * 5 <= len([f for f in frames if f[3] is not None])
    assert set(seqstreams.LIBZSTD_DIFFERS.values()) == {seqstreams.BIG_BLOCK}


def test_coverage():
    """what the families are there for, from serial_sequences' bit counts (a phase: ZG_SEQ_CH consecutive sequences from a multiple
    of ZG_SEQ_CH on, as the kernel cuts them; a window: from any start): rejected frames reach exactly ZG_SEQ_CH x 89 bits in a
    phase and four times that in four consecutive ones; valid frames at least ZG_SEQ_CH x 79 and 4 x ZG_SEQ_CH x 79. What
    zg_k_seqpost reads is asserted on the VALID frames, the only ones it runs on: so takes 31 and 32, (pa & 3, q_ll & 7) all 32 pairs
    (for every frame decoded alone, and again for the shared submit of the GPU module), sh every value up to 31, and the widest
    field a valid frame can hold, 16 + 16 + 26 = 58 bits. The 63-bit field at sh == 31 that the read is built for exists in
    rejected frames only: serial_sequences reaches it, no kernel does. The streams of the ring submit start at all ZG_SEQ_RING
    residues, the highest-rate block at all 16 piece offsets; ExtraPadding, NotEnoughBytes and ExtraBits occur, a stream runs out
    in a FAST phase and in the CAREFUL one; the last sequence falls at every position of a phase"""
    frames = seqstreams.all_frames()
    cov = seqstreams.coverage(frames)
    show = lambda v: len(v) if isinstance(v, set) and len(v) > 40 else sorted(v) if isinstance(v, set) else v
    print("\ncoverage:", {k: ({a: show(b) for a, b in v.items()} if isinstance(v, dict) else show(v)) for k, v in cov.items()})
    assert seqstreams.HI_BITS == 79 and seqstreams.MAX_SEQ_BITS == 89
    assert cov["phase_bits"]["rejected"] == CH * seqstreams.MAX_SEQ_BITS <= seqstreams.K["ZG_SEQ_CMAX"] * 8
    assert cov["four_phase_bits"]["rejected"] == 4 * CH * seqstreams.MAX_SEQ_BITS
    assert cov["phase_bits"]["valid"] >= CH * seqstreams.HI_BITS and cov["four_phase_bits"]["valid"] >= 4 * CH * seqstreams.HI_BITS
    for k in ("", "four_"):
        assert all(cov[k + "window_bits"][kind] >= cov[k + "phase_bits"][kind] for kind in ("valid", "rejected"))
    assert cov["window_bits"]["rejected"] == CH * seqstreams.MAX_SEQ_BITS
    assert {31, 32} <= cov["so"]["valid"] and len(cov["pairs"]["valid"]) == 32 and cov["sh"]["valid"] == set(range(32))
    assert cov["field_bits"]["valid"] == 16 + 16 + 26
    assert cov["field_bits_at_sh31"]["rejected"] == 63                      # (in the model only)
    small = [f for f in frames if f[3] is not None and f[1] not in seqstreams.LARGE]
    large = [f for f in frames if f[1] in seqstreams.LARGE]
    for sub in (small, large):                                              # the two shared submits of tests/test_gpu_seqstreams.py
        c = seqstreams.coverage(sub, seqstreams.submit_offsets(sub))
        assert len(c["pairs"]["valid"]) == 32, len(c["pairs"]["valid"])
    assert {31, 32} <= c["so"]["valid"]
    assert cov["residues"] == set(range(RING)) and cov["hi_residues16"] == set(range(16))
    assert cov["statuses"] >= {seqstreams.EXTRA_PADDING, seqstreams.NOT_ENOUGH_BYTES, seqstreams.EXTRA_BITS, 51, 53}
    assert cov["runs_out"] == {"fast", "careful"}
    assert cov["nseq_mod"]["valid"] >= {n % CH for n in seqstreams.NSEQ_LIST}
    assert cov["max_nseq"] >= 600 and cov["max_lit_regen"] > 131072 and cov["max_regen"] > 6 << 20
    assert cov["valid"] >= 45 and cov["invalid"] >= 40
