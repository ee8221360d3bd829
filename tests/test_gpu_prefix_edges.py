"""The entropy prefix at the seams of its scans and of its reset (zg_kernels.hip): small frames built with the generators of
tests/repframes.py, tests/seqstreams.py and tests/tabframes.py, compared with the oracle byte for byte, sequence for sequence and,
where a frame is refused, status for status.

zg_k_seqpost scans the thread totals of a wave on DPP: rows of 16 lanes, then two broadcasts (tests/test_prefix_scans_cpu.py holds the
model). A thread takes 8 sequences, so the seams are 8 (thread), 128 (row), 512 (wave: the full against the record-by-record store
path) and 2048 sequences (pass: the carries). The seam frames put a repeat code 1, 2 or 3, with and without literals, on the last
sequence in front of every seam and on the first one behind it, so that a history map has to cross each of them, and literal lengths
that leave lit_pos at 0 on one side of the first seam and large on the other.

zg_seq_step picks a lane's state bits out of a window of four dwords at window-relative bit rel = 96 + position % 32 - bits of the
sequence + state bits of the lanes below: the selects turn at 32, 64 and 96. _steps() follows a stream the way the step does and says
where every field starts; the window frames are checked to reach the turning points in FAST steps before they are decoded.

zg_k_scan scans blocks: 8 per thread in its chunked form, rows of 16 lanes. zg_k_reset clears what the submit in front left behind:
statuses, the slots' table logs and max_bits, the totals."""
import random

import pytest

import blockcheck
import framesuite
import oracle
import repframes
import seqstreams
import tabframes
from framesuite import ctx  # noqa: F401
from golden_io import read_manifest, read_pack
from repframes import PASS, S, WAVE
from seqstreams import CH, FIELDS, HI, LL_BITS, META, MIX, ML_BITS, MOD, NR

pytestmark = pytest.mark.gpu

ROW = 16 * S                                             # 128: the sequences of a row of 16 lanes
NSEQ = (1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 2047, 2048, 2049, 4097)
VARIANTS = [(ov, zero) for zero in (False, True) for ov in (1, 2, 3)]      # offset_value 1 .. 3, literal length 0 or not
assert (S, ROW, WAVE, PASS) == (8, 128, 512, 2048)


# ---- zg_k_seqpost: the seams of its scans -----------------------------------------------------------------------------------------

def _seam_seqs(n, shift):
    """n sequences of repeat codes: the fill permutes the three slots with literals; around every seam p (8, 16 and the multiples of
    128) sequence p - 1 and sequence p carry the variant the seam's place and `shift` pick; the ten sequences in front of a row seam
    have no literals and the ten behind it 57 each, or (odd shifts) the other way round; with an even shift everything in front of
    the first row seam (or of 8, in a block without one) has no literals: lit_pos is 0 up to there"""
    seqs = [(1, 1 + i % 3, 3 + i % 3) for i in range(n)]
    seams = [p for p in (S, 2 * S) if p <= n] + list(range(ROW, n + 1, ROW))
    first = ROW if n > ROW else S
    if shift % 2 == 0:
        for i in range(min(first - 1, n)):
            seqs[i] = (0, 1 + i % 2, seqs[i][2])         # (offset_value 1 and 2 without literals: swaps only, nothing is decremented)
    for p in seams:
        if p % ROW == 0:
            lo, hi = (0, 57) if shift % 2 == 0 else (57, 0)
            for i in range(max(p - 11, 0), p - 1):
                seqs[i] = (lo, 1 + i % 2, seqs[i][2])
            for i in range(p + 1, min(p + 11, n)):
                seqs[i] = (hi, 1 + i % 2, seqs[i][2])
        ov, zero = VARIANTS[(p // S + shift) % 6]
        seqs[p - 1] = (0 if zero else 2, ov, 4)
        if p < n:
            ov, zero = VARIANTS[(p // S + shift + 4) % 6]
            seqs[p] = (0 if zero else 1, ov, 5)
    return seqs


def _seam_frame(n, shift):
    g = repframes._Gen("seam_n%d_v%d" % (n, shift), 100 * n + shift)
    g.raw(900)
    g.new_offsets([700, 500, 600])                       # far from 0: the frame decrements slot 0 a few hundred times at most
    g.comp(_seam_seqs(n, shift))
    g.use_all()
    return g.finish()


@pytest.fixture(scope="module")
def seam_frames():
    frames = [_seam_frame(n, shift) for n in NSEQ for shift in range(6)]
    seen = set()
    for name, z, plain in frames:
        assert plain is not None and len(z) < 64 << 10, name
    for n in NSEQ:                                       # every variant on both sides of a pass seam, a wave seam and a row seam
        for shift in range(6):
            s = _seam_seqs(n, shift)
            for p, kind in ((PASS, "pass"), (WAVE, "wave"), (ROW, "row"), (S, "thread")):
                if p < n:
                    seen.add((kind, "last", s[p - 1][1], s[p - 1][0] == 0))
                    seen.add((kind, "first", s[p][1], s[p][0] == 0))
    assert seen == {(k, w, ov, z) for k in ("pass", "wave", "row", "thread") for w in ("last", "first") for ov, z in VARIANTS}
    return frames


def _oracle_blocks(name, z):
    return blockcheck.oracle_blocks(z)


def test_seqpost_seams(ctx, seam_frames):
    """every seam frame's bytes and, block by block, every sequence record (offset, match position, literal position) and the history
    against the oracle's, in one submit; then the frames of one, two and three passes alone"""
    framesuite.submit(ctx, seam_frames, _oracle_blocks)
    for fr in seam_frames:
        if fr[0] in ("seam_n2047_v1", "seam_n2049_v2", "seam_n4097_v3", "seam_n513_v4", "seam_n129_v5"):
            framesuite.submit(ctx, [fr], _oracle_blocks)


def test_seqpost_seams_behind_packed_tables(seam_frames, monkeypatch):
    """the same submit behind zg_k_seq's packed form (development build)"""
    with framesuite.dev_context(monkeypatch, {"ZGPU_SEQ_PACKED": "1"}) as c:
        framesuite.submit(c, seam_frames, _oracle_blocks)


# ---- zg_seq_step: the seams of the window ------------------------------------------------------------------------------------------

TURNS = (31, 32, 33, 63, 64, 65, 95, 96)
# These frames stay at offset code 20 (a MiB of history) and LL code 30 (a literals section of at most 128 KiB, which libzstd decodes
# too): a sequence takes at most 26 state bits and 11 + 16 + 20 extra bits. The OF field (the lowest) starts at rel >= 96 - 73, the ML
# field 8 bits above it, the LL field at rel >= 96 - (47 + 9).
REACH = {"OF": set(TURNS), "ML": set(TURNS) - {31}, "LL": {63, 64, 65, 95, 96}}
TOP = {f: seqstreams.full_counts(f, [c]) for f, c in (("LL", 30), ("OF", 20), ("ML", 52))}       # every sequence: all the bits its tables allow
ZERO = {"LL": ("rle", 1), "OF": ("rle", 0), "ML": ("rle", 0)}                                 # no state bits, no extra bits: a sequence of 0 bits


def _steps(rec, stream, at):
    """one block's stream as zg_seq_step meets it when the stream starts at byte `at` of the source buffer: per sequence (left, tot,
    {field: (rel, state bits)}) — left: sequences not yet decoded (the FAST form runs while left > ZG_SEQ_CH), tot: the bits the
    sequence takes. Written from sequence_section_decoder.rs:154-221 like seqstreams.serial_sequences, which it must agree with"""
    tables, nseq = rec["tables"], rec["nseq"]
    v = int.from_bytes(stream, "little")
    pos = v.bit_length() - 1

    def get(n):
        nonlocal pos
        pos -= n
        return ((v >> pos) if pos >= 0 else (v << -pos)) & ((1 << n) - 1)

    st = {f: get(tables[f][1]) for f in ("LL", "OF", "ML") if tables[f][0] == "tab"}
    assert pos == rec["first"]
    out = []
    for i in range(nseq):
        p0 = pos
        code = {f: tables[f][1] if tables[f][0] == "rle" else tables[f][2][st[f]][2] for f in FIELDS}
        get(code["OF"]), get(ML_BITS[code["ML"]]), get(LL_BITS[code["LL"]])
        nb = dict.fromkeys(FIELDS, 0)
        if i + 1 < nseq:
            for f in ("LL", "ML", "OF"):
                if tables[f][0] == "tab":
                    base, nb[f], _ = tables[f][2][st[f]]
                    st[f] = base + get(nb[f])
        tot = p0 - pos
        assert tot == rec["bits"][i]
        rel = 96 + (p0 + 8 * (at % 4)) % 32 - tot        # the ring keeps the source's alignment: position + ring phase, mod 32
        out.append((nseq - i, tot, {"OF": (rel, nb["OF"]), "ML": (rel + nb["OF"], nb["ML"]), "LL": (rel + nb["OF"] + nb["ML"], nb["LL"])}))
    return out


def _window_frame(name, kind, n, pad, rng):
    hist = (1 << 20) + 131072 if kind in ("hi", "all") else 70000      # (offset code 20 needs a MiB in front)
    pre = seqstreams.rle_history(hist, rng) + [("raw", rng.randbytes(pad))]
    pos = hist + pad
    if kind == "mod":
        seqs, _ = seqstreams.table_seqs(n, pos, rng, MOD, lo_of=2)
        return seqstreams.frame(name, pre + [seqstreams.sblock(seqs, MOD, rng, lit="raw")])
    if kind == "nr":
        seqs, _ = seqstreams.table_seqs(n, pos, rng, NR, lo_of=14)
        return seqstreams.frame(name, pre + [seqstreams.sblock(seqs, NR, rng, lit="raw")])
    if kind == "mix":                                    # cheap symbols and full-rate ones in one block: the bits per sequence jump
        seqs = []
        for k in range(n):
            s, pos = seqstreams.cheap_seqs(1, pos, rng) if rng.random() < 0.7 else seqstreams.hi_seqs(1, pos, rng, of_code=11, ll_codes=(30,), ml_mask=0xFF)
            seqs += s
        T = dict(MIX, OF=seqstreams._shared_counts("OF", [8, 9, 10], [11]))
        return seqstreams.frame(name, pre + [seqstreams.sblock(seqs, T, rng)])
    if kind == "hi":
        seqs, _ = seqstreams.hi_seqs(n, pos, rng, of_code=20, ll_codes=(30,), ml_mask=0xFFF)
        T = dict(HI, OF=seqstreams.full_counts("OF", [1, 2, 20], low=[20]))
        return seqstreams.frame(name, pre + [seqstreams.sblock(seqs, T, rng)], window_log=23)
    if kind == "all":
        seqs, _ = seqstreams.hi_seqs(n, pos, rng, of_code=20, ll_codes=(30,), ml_mask=0xFFF)
        return seqstreams.frame(name, pre + [seqstreams.sblock(seqs, TOP, rng)], window_log=23)
    assert kind == "zero"
    return seqstreams.frame(name, pre + [seqstreams.sblock([(1, 1, 3)] * n, ZERO, rng, lit="raw")])


@pytest.fixture(scope="module")
def window_frames():
    """per kind of table set, sequence count (the phase boundary and the hand-over to the CAREFUL form) and alignment of the stream one
    frame; what their FAST steps reach is asserted here, from _steps on each frame decoded alone"""
    rng = random.Random(2607)
    frames = []
    for kind in ("mod", "nr", "mix", "hi", "all", "zero"):
        for n in (CH, CH + 1, 2 * CH, 2 * CH + 1):
            for pad in range(4 if kind != "zero" else 1):
                for rep in range(2 if kind in ("mod", "nr", "mix", "hi") else 1):
                    frames.append(_window_frame("win_%s_n%d_p%d_%d" % (kind, n, pad, rep), kind, n, pad, rng))
    starts = {f: set() for f in FIELDS}
    straddle = {f: set() for f in FIELDS}
    tots, nbs, careful = set(), set(), 0
    for name, z, plain in frames:
        assert plain is not None
        rec = META[name]["ss"][-1]
        for left, tot, fields in _steps(rec, z[rec["at"]:rec["end"]], rec["at"]):
            careful += left <= CH
            if left <= CH:
                continue
            tots.add(tot)
            for f, (rel, nb) in fields.items():
                assert 0 <= rel and rel + nb <= 128, (name, f, rel, nb)
                nbs.add(nb)
                if nb:
                    starts[f].add(rel)
                    straddle[f] |= {t for t in (32, 64, 96) if rel < t < rel + nb}
    for f in FIELDS:
        assert starts[f] >= REACH[f], (f, sorted(REACH[f] - starts[f]))
    assert straddle["OF"] == straddle["ML"] == {32, 64, 96} and straddle["LL"] >= {64, 96}, straddle
    assert {0, 9} <= nbs and 0 in tots and max(tots) == 26 + 11 + 16 + 20 and careful > 0, (sorted(nbs), sorted(tots))
    return [("window", *f) for f in frames]


def test_window_seams(ctx, window_frames):
    """each frame alone (its stream where _steps placed it), then all in one submit with every recorded sequence against the oracle's"""
    bad = [name for _, name, z, plain in window_frames if ctx.decode_all(z, len(plain)) != plain]
    assert not bad, bad
    framesuite.submit(ctx, window_frames, seqstreams.oracle_blocks)


def test_window_seams_packed_tables(window_frames, monkeypatch):
    with framesuite.dev_context(monkeypatch, {"ZGPU_SEQ_PACKED": "1"}) as c:
        framesuite.submit(c, window_frames, seqstreams.oracle_blocks)


# ---- zg_k_scan: blocks per thread, rows of lanes ----------------------------------------------------------------------------------

SCAN_BLOCKS = (9, 64, 65, 1024, 1025)


def _scan_frame(n):
    """n blocks of one to three sequences, nearly all of repeat codes only: every block's first sequence reads what older blocks left,
    so the history crosses every thread seam (8 blocks of a thread of the chunked form) and every row seam (16 lanes); every seventh
    block sets a new offset, so constants and symbols both travel"""
    g = repframes._Gen("pscan_%d" % n, 9000 + n)
    g.raw(300)
    g.new_offsets([210, 120, 33])
    for i in range(2, n):
        if i % 7 == 3:
            repframes._kind(g, "one")
        else:
            g.rand_rep(g.rng.randint(1, 3), allow4=i % 5 == 0)
    return g.finish()


@pytest.fixture(scope="module")
def scan_frames():
    frames = [_scan_frame(n) for n in SCAN_BLOCKS]
    assert [repframes.META[name]["nblocks"] for name, _, _ in frames] == list(SCAN_BLOCKS)
    return frames


def test_scan_seams(ctx, scan_frames):
    """each frame in a submit of its own (the form of zg_k_scan its size picks: one wave, 1024 threads, 8 blocks per thread), then
    all in one (the chunked form for every frame): the history at every block start and every sequence against the oracle's"""
    for fr in scan_frames:
        framesuite.submit(ctx, [fr], _oracle_blocks)
    framesuite.submit(ctx, scan_frames, _oracle_blocks)


# ---- zg_k_reset -------------------------------------------------------------------------------------------------------------------

def _statuses(c, frames):
    """frames [(name, zst, plaintext or None)] as the entries of one decode_frames call (one shared submit): per frame (status, bytes)"""
    res = c.decode_frames([z for _, z, _ in frames], [len(p) if p is not None else 1 << 20 for _, _, p in frames])
    return [(r.status, r.data) for r in res]


def test_second_submit_sees_nothing_of_the_first(ctx):
    """two decode_frames calls, each one shared submit, on one engine. The first: frames that describe FSE and Huffman tables in their
    first blocks (slot logs and max_bits are set for the lowest slots) and frames whose blocks fail in a table description, a literals
    stream and the execution (status, tab_status and lit_status are set). The second is smaller: frames whose FIRST block names tables
    that were never described (repeat mode; the treeless one is refused by the host's walk already and rides along) — with a stale
    log they would decode with the first submit's tables instead of getting the oracle's status — among valid frames, which a stale
    status word would fail. Both ways round, twice"""
    modes = [f for f in tabframes.family("fse_modes") if f[2] is not None][:6]
    hufs = [f for f in tabframes.family("huf_weight_streams") if f[2] is not None][:4]
    inv = {f[0]: f for f in tabframes.family("invalid_tables")}
    failing = [inv[n] for n in ("bad_huf_weight12", "bad_huf_stream_ends_in_0", "bad_fse_OF_log", "bad_rle_of31_executes")]
    first = modes + failing[:2] + hufs + failing[2:] + [f for f in repframes.family("invalid") if f[0] == "bad_zero_in_block"]
    untabled = [inv[n] for n in ("bad_repeat_in_first_block_ll", "bad_repeat_in_first_block_of_ml", "bad_treeless_in_first_block")]
    plain = [f for f in repframes.family("initial_history")][:3]
    second = [untabled[0], plain[0], untabled[1], plain[1], untabled[2], plain[2]]
    assert sum(len(f[1]) for f in second) < sum(len(f[1]) for f in first)
    status = dict(tabframes.STATUS)
    status.update(repframes.STATUS)
    for _ in range(2):
        for frames in (first, second):
            got = _statuses(ctx, frames)
            for (name, _, want), (st, out) in zip(frames, got):
                if want is None:
                    assert st == status[name] != 0, (name, st, status[name])
                else:
                    assert st == 0 and out == want, (name, st)


def test_continued_frame_with_carried_tables(ctx):
    """FrameDecoder.decode_blocks(UptoBlocks, 1): every block is a run of its own, and a block in repeat mode or with treeless literals
    gets its tables from the carry slots, which the run fills BEHIND the reset; call by call against the oracle"""
    names = ("modes_333", "modes_repeat_after_rle", "modes_repeat_across_raw_and_rle", "hws_al5_nw41_1s", "hws_align3_4s")      # (every hws_* frame has treeless blocks)
    picked = [f for fam in ("fse_modes", "huf_weight_streams") for f in tabframes.family(fam) if f[0] in names]
    assert len(picked) == len(names)
    for name, z, plain in picked:
        st, out, calls = framesuite.lockstep(ctx, name, z, 1)
        assert st == 0 and out == plain and calls >= 2, (name, st, calls)


def test_frames_with_a_registered_dictionary():
    """dictionary frames in a shared submit (zg_k_dictfill writes the dictionary's tables into the carry slots behind the reset) and
    alone, twice on one engine with a refused frame between: the oracle's bytes"""
    import zgpu
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    names = sorted(n for n in man if n != "dictionary")[:8]
    raw = pack["dictionary"]
    frames, sizes = [pack[n] for n in names], [man[n]["size"] for n in names]
    want = []
    for z in frames:
        d = oracle.FrameDecoder()
        d.add_dict(raw)
        st, out = d.decode_all(z, 1 << 24)
        assert st == 0
        want.append(out)
    bad = [f for f in tabframes.family("invalid_tables") if f[0] == "bad_fse_LL_log"][0]
    c = zgpu.Context(0)
    try:
        c.add_dict(raw)
        c.set_frames_shared_dicts(True)
        for _ in range(2):
            res = c.decode_frames(frames + [bad[1]], sizes + [1 << 16])
            assert [r.status for r in res[:-1]] == [0] * len(frames) and res[-1].status == tabframes.STATUS[bad[0]]
            assert [r.data for r in res[:-1]] == want
            assert c.decode_all(frames[0], sizes[0]) == want[0]
    finally:
        c.close()
