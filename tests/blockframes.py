"""Frames of chosen non-sequence blocks (test helper, no tests): Raw blocks, RLE blocks and compressed blocks without sequences
(raw, RLE, Huffman and treeless literals), which zg_k_lit and its helpers zg_wg_copy and zg_wg_fill write, at that kernel's own
edges, and as the sources of matches in the blocks behind them (zg_flat1.h and zg_flat4.h skip such blocks as "final already";
zg_k_sparse, zg_k_lz and the sweep gather from their bytes). The frames come from tabframes.build: the plaintext is seqframes.lz77
of what was asked for, checked there against the oracle and libzstd (except the names of BLOCK_LIBZSTD_DIFFERS).

Every valid frame is (name, zst, plaintext); invalid ones have plaintext None and STATUS[name] holds the oracle's answer."""
import functools
import random

import framesuite
import oracle
import tabframes
from tabframes import Block

MAX = 131072                                             # Block_Maximum_Size
HDR = 6                                                  # magic, descriptor, window byte: tabframes' frame header
WEIGHTS = [4, 3, 2, 1, 1]                                # 8 + 4 + 2 + 1 + 1 = 16: the implied symbol 5 takes the other 16; max_bits 5

# valid frames libzstd 1.4.9 does not return the plaintext for, each with its reason (only frames the oracle accepts, at most a
# tenth of the valid ones: all_frames() checks both)
BLOCK_LIBZSTD_DIFFERS = {
    "lit_sizes_zero_compressed": "a compressed block of 2 bytes (an empty literals section, no sequences): libzstd asks for 3 bytes at least",
    "lit_sizes_lit_raw_131068": "a compressed block whose content is exactly 131072 bytes: libzstd asks for less than the block size limit",
    "nb_empty_compressed": "runs of compressed blocks of 2 bytes, as lit_sizes_zero_compressed",
}

STATUS = {}

# the kinds of block zg_k_lit writes. The Huffman and treeless kinds come with one and with four streams
KINDS = ("raw", "rle", "lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "lit_treeless1", "lit_treeless4")
KIND6 = {"raw": "raw", "rle": "rle", "lit_raw": "lit_raw", "lit_rle": "lit_rle", "lit_huf1": "lit_huf", "lit_huf4": "lit_huf",
         "lit_treeless1": "lit_treeless", "lit_treeless4": "lit_treeless"}
SIZES = tuple(range(18)) + (23, 24, 25, 2040, 2047, 2048, 2049, 2056, 4095, 4096, 131071, 131072)
ALIGN_SIZES = (1, 7, 8, 9, 16, 17)
NEIGHBOUR_SIZES = (1, 2, 3, 9)
OVERLAP_OFFS = tuple(range(1, 17)) + (31, 32, 33, 63, 64, 65)


def can_hold(kind, n):
    """may a block of this kind regenerate n bytes? Raw literals share the block with a 3-byte header and the sequences byte
    (131068 at most); RLE literals of size 0 are not written; one Huffman stream goes with the 10-bit size format only (RFC 8878
    3.1.1.3.1.1: sizes below 1024); four streams hold (n + 3) / 4 bytes each in the first three and the rest in the last, which
    must not be empty (n - 3 * ceil(n / 4) >= 1: not 0 .. 3, 5, 6 and 9)"""
    if kind in ("raw", "rle"):
        return n <= MAX
    if kind == "lit_raw":
        return n <= MAX - 4
    if kind == "lit_rle":
        return 1 <= n <= MAX
    if kind.endswith("1"):
        return 1 <= n < 1024
    return n - 3 * ((n + 3) // 4) >= 1 and n <= MAX


def sizes_for(kind):
    """the sizes of SIZES a kind can hold; raw literals take 131067 and 131068 in place of 131071 and 131072"""
    out = {n for n in SIZES if can_hold(kind, n)}
    if kind == "lit_raw":
        out |= {MAX - 5, MAX - 4}
    return out


def mk(kind, n, rng):
    """one block of the kind that regenerates n bytes, as tabframes.build takes it"""
    assert can_hold(kind, n), (kind, n)
    if kind == "raw":
        return ("raw", rng.randbytes(n))
    if kind == "rle":
        return ("rle", rng.randrange(1, 256), n)
    if kind == "lit_raw":
        return Block(rng.randbytes(n), [])
    if kind == "lit_rle":
        return Block(bytes([rng.randrange(1, 256)]) * n, [], lit=("rle", None))
    data = bytes(rng.choices(range(6), k=n))
    if kind.startswith("lit_huf"):
        return Block(data, [], lit=("huf", WEIGHTS, "direct", int(kind[-1]), None))
    return Block(data, [], lit=("treeless", int(kind[-1]), None))


def table_block(rng):
    """a literal-only block that carries the Huffman table the treeless blocks behind it go on with"""
    return mk("lit_huf1", 40, rng)


def _build(name, blocks, **kw):
    r = tabframes.build(name, blocks, differs=BLOCK_LIBZSTD_DIFFERS, **kw)
    if r[2] is None:
        STATUS[name] = tabframes.STATUS[name]
    return r


# ---- the families: each returns [(name, zst, plaintext or None)] ------------------------------------------------------------

def lit_sizes():
    """zg_k_lit / zg_wg_copy / zg_wg_fill: every kind of block at regenerated sizes 0 .. 17 and 23 .. 25 (the n / 8 body against the
    n % 8 tail), 2040 .. 2056 (the 256 lanes of 8 bytes: one whole round at 2048, a second one begun at 2049 and 2056), 4095 / 4096
    and the largest a block holds (131071 / 131072; 131067 / 131068 raw literals). The small sizes share a frame per kind, so their
    stores start at every alignment; the sizes above 4096 go one to a frame"""
    rng = random.Random(601)
    out = []
    for kind in KINDS:
        want = sorted(sizes_for(kind))
        pre = [table_block(rng)] if "treeless" in kind else []
        for part, pick in (("small", [n for n in want if 1 <= n <= 25]), ("mid", [n for n in want if 2040 <= n <= 4096])):
            if pick:
                out.append(_build("lit_sizes_%s_%s" % (kind, part), pre + [mk(kind, n, rng) for n in pick]))
        for n in (n for n in want if n > 4096):
            out.append(_build("lit_sizes_%s_%d" % (kind, n), pre + [mk(kind, n, rng)]))
    # size 0: Raw and RLE blocks between others and last in the frame; the compressed block of 0 + 0 in a frame of its own
    out.append(_build("lit_sizes_zero", [("raw", b""), mk("raw", 5, rng), ("rle", 0x33, 0), mk("rle", 3, rng), ("raw", b""), ("rle", 0x44, 0)]))
    out.append(_build("lit_sizes_zero_compressed", [mk("raw", 5, rng), Block(b"", []), mk("rle", 3, rng), Block(b"", [])]))
    return out


def _enc(b, fr):
    """(encoded length of a block, header included; offset of its payload inside it: the raw bytes, the RLE byte, the Huffman section)"""
    if isinstance(b, tuple):
        return (3 + len(b[1]), 3) if b[0] == "raw" else (4, 3)
    lit, _ = tabframes._literals(fr, b)
    n = len(b.lits)
    if b.lit[0] == "raw":
        hdr = len(lit) - n
    elif b.lit[0] == "rle":
        hdr = len(lit) - 1
    else:
        assert len(lit) < 1024
        hdr = 3
    return 3 + len(lit) + 1, 3 + hdr


def lit_alignment():
    """zg_wg_copy's unaligned 8-byte stores and loads (zg_u64u, zg_ld64) and zg_wg_fill's stores: sizes 1, 7, 8, 9, 16 and 17 of every
    kind with the destination at each residue mod 8 and, independently, the payload in the source at each residue mod 8. In front of
    each block an RLE block of k bytes, k in 0 .. 7, moves the output by k and the source by 4, and j empty Raw blocks, j in 0 .. 7,
    move the source by 3 j and the output by nothing; k and j are solved for the residues wanted, pair by pair in the order that
    needs the fewest empty blocks. One frame per kind"""
    rng = random.Random(602)
    out = []
    for kind in KINDS:
        blocks, fr = [], tabframes._Frame()
        src, dst = HDR, 0
        if "treeless" in kind:
            blocks.append(table_block(rng))
            src, dst = src + _enc(blocks[0], fr)[0], 40
        for n in ALIGN_SIZES:
            if not can_hold(kind, n):
                continue
            todo = {(d, s) for d in range(8) for s in range(8)}
            while todo:                                  # the pairs in the order that needs the fewest empty blocks
                blk = mk(kind, n, rng)
                size, pay = _enc(blk, fr)
                # 3 j = s - (src + 4 + pay) mod 8, and 3 * 3 = 1 mod 8
                j, k, d, s = min(((3 * (s - (src + 4 + pay))) % 8, (d - dst) % 8, d, s) for d, s in todo)
                todo.remove((d, s))
                blocks += [("rle", rng.randrange(1, 256), k)] + [("raw", b"")] * j + [blk]
                src += 4 + 3 * j
                dst += k
                assert dst % 8 == d and (src + pay) % 8 == s
                src, dst = src + size, dst + n
        out.append(_build("lit_align_%s" % kind, blocks))
    return out


def neighbours():
    """zg_k_lit's stores against the blocks next to them, which other workgroups write: runs of 1-, 2-, 3- and 9-byte blocks of
    alternating kinds back to back (a store that leaves its block lands in a neighbour), 1000 empty blocks of each kind between
    non-empty ones and at the frame's end (workgroups with nothing to write, many blocks at one output position), a frame that is
    one empty last Raw block and a frame of empty blocks only"""
    rng = random.Random(603)
    out = []
    for n in NEIGHBOUR_SIZES:
        kinds = [k for k in KINDS if can_hold(k, n)]
        blocks = [mk("lit_huf1", n, rng)]                # (the table for the treeless blocks)
        while len(blocks) < 208:
            rng.shuffle(kinds)
            blocks += [mk(k, n, rng) for k in kinds]
        out.append(_build("nb_run_%db" % n, blocks))
    kinds = [k for k in KINDS if can_hold(k, 9)]
    blocks = [table_block(rng)]
    for i in range(240):                                 # the four sizes mixed
        n = NEIGHBOUR_SIZES[rng.randrange(4)]
        blocks.append(mk(rng.choice([k for k in kinds if can_hold(k, n)]), n, rng))
    out.append(_build("nb_run_mixed", blocks))
    out.append(_build("nb_empty_raw_rle", [mk("raw", 9, rng)] + [("raw", b"")] * 1000 + [mk("rle", 5, rng)] + [("rle", 0x21, 0)] * 1000))
    out.append(_build("nb_empty_compressed", [mk("raw", 9, rng)] + [Block(b"", [])] * 1000 + [mk("lit_rle", 7, rng)] + [Block(b"", [])] * 10))
    out.append(_build("nb_one_empty_raw", [("raw", b"")]))
    out.append(_build("nb_only_empty", [("raw", b""), ("rle", 0x23, 0)] * 20 + [("raw", b"")]))
    return out


class _Lay:
    """blocks laid out with their output positions known, so that a match can name its source by position"""

    def __init__(self, rng):
        self.rng, self.blocks, self.spans, self.pos = rng, [], [], 0     # spans: (kind or "seq", start, end)

    def ns(self, kind, n):
        self.blocks.append(mk(kind, n, self.rng))
        self.spans.append((kind, self.pos, self.pos + n))
        self.pos += n

    def seq(self, matches, fill, tail=3):
        """a block with sequences: matches [(ll, source position, ml or "reach": up to the match's own start)], then `fill` short
        matches with sources anywhere in front, then `tail` literals"""
        rng, p, seqs, nl = self.rng, self.pos, [], 0
        for ll, src, ml in matches:
            p += ll
            d = p - src
            assert 1 <= d <= p, (d, p)
            ml = max(d, 3) if ml == "reach" else ml
            seqs.append((ll, d + 3, ml))
            p, nl = p + ml, nl + ll
        for _ in range(fill):
            ll = rng.randint(0, 3)
            p += ll
            seqs.append((ll, rng.randint(1, p) + 3, rng.randint(3, 10)))
            p, nl = p + seqs[-1][2], nl + ll
        self.blocks.append(Block(rng.randbytes(nl + tail), seqs))
        self.spans.append(("seq", self.pos, p + tail))
        self.pos = p + tail

    def forms(self, recent, tails):
        """the matches of a block with sequences that comes next: one from the frame's first byte, two that start in the last
        t bytes (t of tails) of the block in front, if that has no sequences, and run up to their own start through this block's
        literals and matches, then one inside each of the last `recent` blocks without sequences and one across each boundary
        between two of them"""
        rng, m = self.rng, [(2, 0, 4)]
        k, s, e = self.spans[-1]
        if k != "seq":
            m += [(1 + i, e - t, "reach") for i, t in enumerate(tails) if t <= e - s]
        first = max(0, len(self.spans) - recent)
        for i in range(first, len(self.spans)):
            k, s, e = self.spans[i]
            if k == "seq":
                continue
            if e - s >= 3:
                ml = rng.randint(3, min(e - s, 12))
                m.append((rng.randint(0, 2), rng.randint(s, e - ml), ml))
            if i + 1 < len(self.spans) and self.spans[i + 1][0] != "seq":
                a, b = rng.randint(1, min(4, e - s)), rng.randint(2, min(5, self.spans[i + 1][2] - e))
                m.append((rng.randint(0, 2), e - a, a + b))
        return m


def _pair_frame(name, a, b, rng, fill, t0):
    """[P A B S] [S A B S] [B A A B] [S A B]: units of four blocks, which is the smallest the plan makes. P is an RLE block, or the
    block with the Huffman table where A or B needs one. The first S has sources and matches in the frame's first unit; the second
    reads the unit in front, the third its own (a later) unit with blocks without sequences between two that have them; the
    third unit has no sequences at all and the S behind it reads from it, its two tail matches from that unit's last block"""
    lay = _Lay(rng)
    n = lambda: rng.randint(13, 40)                      # noqa: E731  (13: the least that four streams hold besides 4, 7, 8, 10 .. 12)
    if "treeless" in a + b:
        lay.blocks.append(table_block(rng))
        lay.spans.append(("lit_huf1", 0, 40))
        lay.pos = 40
    else:
        lay.ns("rle", n())
    tails = lambda i: ((t0 + i) % 8 + 1, (t0 + i + 4) % 8 + 1)           # noqa: E731
    lay.ns(a, n()), lay.ns(b, n())
    lay.seq(lay.forms(3, tails(0)), fill)
    lay.seq(lay.forms(4, ()), fill)
    lay.ns(a, n()), lay.ns(b, n())
    lay.seq(lay.forms(3, tails(1)), fill)
    lay.ns(b, n()), lay.ns(a, n()), lay.ns(a, n()), lay.ns(b, n())
    lay.seq(lay.forms(4, tails(2)), fill)
    lay.ns(a, n()), lay.ns(b, n())
    return _build(name, lay.blocks)


def _overlap_frame(name, kind, rng, fill):
    """[R S R S] [R R R R] [S R S R], six times: every S starts with a match of no literals whose offset, one of OVERLAP_OFFS, is
    shorter than the match, so the period that repeats lies in the last bytes of the block R in front of it"""
    lay = _Lay(rng)
    offs = list(OVERLAP_OFFS) + [1, 8]

    def s():
        o = offs.pop(0)
        lay.seq([(0, lay.pos - o, 2 * o + 3 + rng.randint(0, 70))] + lay.forms(2, ()), fill)

    r = lambda: lay.ns(kind, rng.randint(66, 90))        # noqa: E731
    for _ in range(6):
        r(), s(), r(), s()
        r(), r(), r(), r()
        s(), r(), s(), r()
    assert not offs
    return _build(name, lay.blocks)


def sources():
    """zg_k_lit in front of the LZ stage, zg_k_huf's direct literals (ZG_FLAG_LIT_DIRECT) in front of it, and the skip of blocks
    without sequences in zg_flat1.h / zg_flat4.h (unit_size = bu0 + blk.regen_size): matches whose sources lie wholly inside a block
    without sequences, across the boundary between two of them (every ordered pair of kinds), in the last 1 .. 8 bytes of one and
    on into the matching block's own literals and matches, in an RLE or Raw block as the period of a self-overlapping match
    (offsets 1 .. 16, 31 .. 33, 63 .. 65), and at the frame's first byte in an RLE block; each in the frame's first unit, in a later
    unit, and behind a unit that has no sequences. Every third pair frame has few sequences (zg_k_sparse takes it), the others
    more than four a block (the flatten and the sweep)"""
    rng = random.Random(604)
    out = []
    six = ("raw", "rle", "lit_raw", "lit_rle", "lit_huf", "lit_treeless")
    i = 0
    for a in six:
        for b in six:
            st = lambda k: k + "14"[(i + (k == b)) % 2] if k in ("lit_huf", "lit_treeless") else k   # noqa: E731  (one and four streams in turn)
            out.append(_pair_frame("src_%s_%s" % (a, b), st(a), st(b), rng, 0 if i % 3 == 0 else 16, i))
            i += 1
    for kind in ("raw", "rle"):
        out.append(_overlap_frame("src_overlap_%s" % kind, kind, rng, 14))
    out.append(_overlap_frame("src_overlap_raw_sparse", "raw", rng, 0))
    return out


def _hand(name, body):
    """a frame whose blocks are written here byte by byte: header, body, nothing behind it"""
    z = tabframes.MAGIC + bytes([0x04, (17 - 10) << 3]) + body
    st, _ = oracle.FrameDecoder().decode_all(z, 1 << 20)
    assert st != 0, (name, "the oracle accepts a frame meant to be invalid")
    STATUS[name] = st
    return name, z, None


def _prefix(blocks):
    """the bytes of good blocks, none of them the last: a valid frame without its empty last block and its checksum"""
    z = tabframes.build("_prefix", blocks + [("raw", b"")], differs=BLOCK_LIBZSTD_DIFFERS)[1]
    del tabframes.META["_prefix"]
    return z[HDR:-7]


def invalid():
    """what must fail, with the oracle's status: a Raw and an RLE block header of 131073 bytes, a Raw block whose body ends 1 .. 8
    bytes early, an RLE block without its byte, a reserved block type behind a good block of each kind, compressed blocks of 0, 1 and
    2 bytes that lack a literals or a sequences header, a treeless block without sequences behind Raw and RLE blocks only, and
    matches behind blocks without sequences whose offset is one more than the bytes that exist"""
    rng = random.Random(605)
    bh = tabframes._bh
    out = []
    out.append(_hand("bad_raw_131073", bh(1, 0, MAX + 1) + rng.randbytes(MAX + 1) + bytes(4)))
    out.append(_hand("bad_rle_131073", bh(1, 1, MAX + 1) + b"\x5a" + bytes(4)))
    for cut in range(1, 9):
        out.append(_hand("bad_raw_cut%d" % cut, _prefix([mk("rle", 11, rng)]) + bh(1, 0, 20) + rng.randbytes(20 - cut)))
    out.append(_hand("bad_rle_no_byte", _prefix([mk("raw", 11, rng)]) + bh(1, 1, 20)))
    for kind in KINDS:
        pre = [table_block(rng)] if "treeless" in kind else []
        out.append(_hand("bad_reserved_behind_%s" % kind, _prefix(pre + [mk(kind, 17, rng)]) + bh(1, 3, 0) + bytes(4)))
    good = [mk("raw", 9, rng), mk("rle", 9, rng)]
    for nm, content in (("0", b""), ("1_no_sequences", b"\x00"), ("2_no_sequences", tabframes.lit_header(0, 1) + b"x"),
                        ("2_long_header_no_sequences", tabframes.lit_header(0, 0, sf=1)), ("1_half_a_header", b"\x04"),
                        ("2_half_a_header", b"\x0c\x00")):
        out.append(_build("bad_compressed_%s" % nm, good + [("bytes", content)], valid=False))
    out.append(_build("bad_treeless_behind_raw_rle", good + [("bytes", tabframes.lit_header(3, 8, 2, 1) + b"\x55\x01" + b"\x00")], valid=False))
    for kind in ("raw", "rle", "lit_raw", "lit_rle", "lit_huf4"):
        front = [mk("raw", 20, rng), mk(kind, 13, rng)]
        out.append(_build("bad_offset_behind_%s" % kind, front + [Block(rng.randbytes(6), [(4, 20 + 13 + 4 + 1 + 3, 3)])], valid=False))
        front = [mk(kind, 13, rng), Block(rng.randbytes(9), [(4, 5, 3)]), mk(kind, 16, rng)]
        out.append(_build("bad_offset_behind_%s_later" % kind, front + [Block(rng.randbytes(6), [(0, 13 + 12 + 16 + 1 + 3, 3)])], valid=False))
    return out


FAMILIES = {
    "lit_sizes": lit_sizes,
    "lit_alignment": lit_alignment,
    "neighbours": neighbours,
    "sources": sources,
    "invalid": invalid,
}


def _check_differs(frames):
    """the BLOCK_LIBZSTD_DIFFERS cap, once every family is built"""
    names = [n for _, n, _, p in frames if p is not None]
    assert set(BLOCK_LIBZSTD_DIFFERS) <= set(names), "BLOCK_LIBZSTD_DIFFERS may hold only frames the oracle accepts"
    assert len(BLOCK_LIBZSTD_DIFFERS) * 10 <= len(names), "BLOCK_LIBZSTD_DIFFERS holds more than a tenth of the valid frames"


_F = framesuite.Families(FAMILIES, _check_differs)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


BATCH_REPS = ("lit_sizes_raw_small", "lit_sizes_rle_mid", "lit_sizes_lit_raw_small", "lit_sizes_lit_rle_small", "lit_sizes_lit_huf4_mid",
              "lit_sizes_lit_treeless1_small", "lit_align_raw", "nb_run_1b", "nb_run_mixed", "src_raw_rle", "src_lit_huf_lit_treeless",
              "src_overlap_rle")


@functools.lru_cache(None)
def batch_alignment():
    """a submit order, not new frames: each of BATCH_REPS sixteen times, behind a pad frame (one Raw block) of 0 .. 15 bytes sized so
    that the frame's place in the output (frame_out.out_base: ualign in zg_flat4.h, lead in both flatten bodies, zg_k_lit's
    stores) takes each residue mod 16 once. Returns ([(name, zst, plaintext)], {name: [indices in the list]})"""
    rng = random.Random(606)
    by_name = {n: (n, z, p) for _, n, z, p in valid_frames()}
    pads = [_build("pad%d" % p, [("raw", rng.randbytes(p))]) for p in range(16)]
    order, where, at = [], {n: [] for n in BATCH_REPS}, 0
    for r in range(16):
        for n in BATCH_REPS:
            pad = pads[(r - at) % 16]
            order += [pad, by_name[n]]
            at += len(pad[2])
            assert at % 16 == r
            where[n].append(len(order) - 1)
            at += len(by_name[n][2])
    return order, where


def loss_per_sequence():
    """the microseconds per sequence of the longest block in the host's rule for literals after the scan (BatchBuilder::finish:
    loss_us = per_seq * max_nseq * rounds), read out of the source next to hufstreams.direct_rule's constants"""
    import os
    import re
    import hufstreams
    text = open(os.path.join(os.path.dirname(hufstreams._SRC), "zg_host_parse.cpp")).read()
    m = re.search(r"loss_us = ([0-9.]+) \* \(double\)max_nseq \* \(double\)\(rounds \? rounds : 1\);", text)
    assert m, "the rule that picks the direct path has changed: test_gpu_blockframes.test_direct_literals relies on it"
    return float(m.group(1))


# ---- what the frames reach --------------------------------------------------------------------------------------------------

def walk(z):
    """the blocks of a frame, read from its bytes: [(block type, position of the payload in the frame: the raw bytes, the RLE byte,
    a compressed block's literals behind their header)]"""
    pos, out = HDR, []
    while True:
        h = int.from_bytes(z[pos:pos + 3], "little")
        last, bt, size = h & 1, (h >> 1) & 3, h >> 3
        pay = pos + 3
        if bt == 2 and size:
            lt, sf = z[pay] & 3, (z[pay] >> 2) & 3
            pay += ((1, 2, 1, 3) if lt < 2 else (3, 3, 4, 5))[sf]
        out.append((bt, pay))
        pos += 3 + (1 if bt == 1 else size)
        if last:
            return out


def _kind(info):
    if info["btype"] < 2:
        return ("raw", "rle")[info["btype"]]
    if info["nseq"]:
        return "seq"
    return ("lit_raw", "lit_rle", "lit_huf%d", "lit_treeless%d")[info["lit_type"]] % (() if info["lit_type"] < 2 else (info["nstreams"],))


def coverage(frames):
    """walk each valid frame [(name, zst)] with the CPU harness (emu.EmuBatch; the units from emu.Plan, the host's plan). Returns, per
    kind, the sizes n, the largest, and the (destination, source) residues mod 8 (the source is the payload's place in the frame);
    per form of match source ("inside", "straddle", "tail", "overlap", "first_byte") the placements reached ("first": the match
    lies in the frame's first unit, "later": in a later one, "across": a unit without sequences lies between units with them and
    the match reads from it or from in front of it); the ordered kind pairs a source straddles; the t of sources that begin in the
    last t bytes, 1 .. 8, of a block without sequences and run on into the matching block; the (kind, offset) of self-overlapping
    matches whose period lies in one Raw or RLE block"""
    import emu
    cov = {"sizes": {k: set() for k in KINDS}, "largest": {k: 0 for k in KINDS}, "residues": {}, "forms": {}, "pairs": set(),
           "tails": set(), "overlap": set(), "first_byte_rle": 0, "blocks": 0, "seq_blocks": 0, "noseq_units_between": 0,
           "sparse": 0, "dense": 0, "ns_between_seq_in_unit": 0, "ns_last_in_frame": 0}
    for name, z in frames:
        e = emu.EmuBatch(z, max_window=1 << 31)
        assert e.parse_status == 0 and e.nframes == 1, name
        raw = walk(z)
        assert len(raw) == e.nblocks, name
        plan = emu.Plan(z)
        unit_of, seq_units = {}, []
        for u, (_, fb, nb, noseq) in enumerate(plan.units):
            unit_of.update({b: u for b in range(fb, fb + nb)})
            seq_units.append(not noseq & 1)
        between = [u for u in range(len(seq_units)) if not seq_units[u] and any(seq_units[:u]) and any(seq_units[u + 1:])]
        cov["noseq_units_between"] += len(between)
        cov["sparse" if plan.frames[0][6] else "dense"] += 1
        spans, at = [], 0
        for b in range(e.nblocks):
            info = e.block(b)
            kind = _kind(info)
            assert raw[b][0] == info["btype"], name
            size = info["regen_size"] + (sum(s[1] for s in e.block_sequences(b, info["nseq"])) if kind == "seq" else 0)
            spans.append((kind, at, at + size))
            cov["blocks"] += 1
            if kind != "seq":
                cov["sizes"][kind].add(size)
                cov["largest"][kind] = max(cov["largest"][kind], size)
                if name.startswith("lit_align") and size in ALIGN_SIZES:
                    cov["residues"].setdefault((kind, size), set()).add((at % 8, raw[b][1] % 8))
            at += size
        kinds = [s[0] for s in spans]
        cov["ns_last_in_frame"] += kinds[-1] != "seq" and "seq" in kinds
        for b in range(1, e.nblocks - 1 if "seq" in kinds else 0):
            if kinds[b] != "seq" and "seq" in [kinds[x] for x in range(b) if unit_of[x] == unit_of[b]] and \
                    "seq" in [kinds[x] for x in range(b + 1, e.nblocks) if unit_of[x] == unit_of[b]]:
                cov["ns_between_seq_in_unit"] += 1

        def block_at(p):
            return next(i for i, (_, s, t) in enumerate(spans) if s <= p < t)

        for b in range(e.nblocks):
            if kinds[b] != "seq":
                continue
            cov["seq_blocks"] += 1
            for of, ml, mdst, _ in e.block_sequences(b, e.block(b)["nseq"]):
                assert of >> 30 == 0, name               # (the frames use plain offsets only)
                dst = spans[b][1] + mdst
                lo, hi = dst - of, dst - of + min(of, ml)
                i, j = block_at(lo), block_at(hi - 1)
                um, us = unit_of[b], unit_of[i]
                place = {"first"} if um == 0 else {"later"}
                if any(us <= u < um for u in between):
                    place.add("across")
                found = []
                if lo == 0:
                    found.append("first_byte")
                    cov["first_byte_rle"] += kinds[0] == "rle"
                if i == j and kinds[i] != "seq":
                    found.append("inside")
                    if ml > of and kinds[i] in ("raw", "rle"):
                        found.append("overlap")
                        cov["overlap"].add((kinds[i], of))
                if j == i + 1 and "seq" not in (kinds[i], kinds[j]):
                    found.append("straddle")
                    cov["pairs"].add((KIND6[kinds[i]], KIND6[kinds[j]]))
                if kinds[i] != "seq" and j == b and spans[i][2] - lo <= 8 and spans[i][2] == spans[b][1]:
                    found.append("tail")
                    cov["tails"].add(spans[i][2] - lo)
                for f in found:
                    cov["forms"].setdefault(f, set()).update(place)
    return cov
