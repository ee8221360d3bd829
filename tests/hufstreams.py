"""Frames built from chosen Huffman streams (test helper, no tests): the streams of a literals section written bit by bit, so that
zg_k_huf (zstd-rs_amd/csrc/zg_huf.h) sees what no encoder emits: codes that never re-synchronise, chunks of exactly as many
symbols as a lane has rows and one more, stream lengths at the window edges, every start alignment, last codes that reach below
the stream's start, four streams of a handful of literals, and waves that share a table with a stream of another length. Built on
tests/tabframes.py, whose Block takes the streams as they are (the "hufstreams" literals kind).

serial_decode is the plain reference of the operation, written from RFC 8878 4.2.2 and the reference's loop. chunk_model follows
the kernel's chunking (it reads the chunk sizes, the warm-up and the row count out of zg_huf.h) and says how many redo rounds a
window needs and how many symbols a chunk holds: coverage() asserts with it that the frames reach what they aim at.

Every valid frame is checked when it is built: the oracle decodes it to the plaintext, the oracle's literals of every block equal
serial_decode of its streams, and libzstd returns the same bytes (except the frames of LIBZSTD_DIFFERS). Invalid frames come
back with plaintext None and the oracle's status in STATUS.

Two limits of the format shape the families. A single stream exists only with size format 0, whose compressed size has 10 bits:
description and stream together have at most 1023 bytes, so a single stream has at most 8183 bits, less than one window of
64 x 128 bits. Every stream length from 8191 bits up, and with it the carry from one window to the next, is built in four
streams. And a stream's share of the literals is fixed by the format, so a long stream beside a short one needs two blocks."""
import os
import random
import re

import blockcheck
import framesuite
import tabframes
from tabframes import META, STATUS, Block, RevBits, build, huf_codes, huf_table, lit_header, weights_direct, _lits_covering, _simple_seqs

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zstd-rs_amd", "csrc", "zg_huf.h")

# valid frames libzstd's decompressor does not return the plaintext for, each with its reason; all_frames() checks that these
# are frames the oracle accepts and at most a tenth of the valid ones
LIBZSTD_DIFFERS = {}
for _d in (1, 5, 10):
    for _q in ("n", "q"):
        LIBZSTD_DIFFERS["ov_1s_d%d_%s" % (_d, _q)] = "the last code reaches %d bits below the stream's start: libzstd wants a stream to end on its last bit" % _d
for _n in ("tiny_uneven_r8", "tiny_uneven_r6_empty"):
    for _q in ("n", "q"):
        LIBZSTD_DIFFERS["%s_%s" % (_n, _q)] = "the four streams do not hold the format's share of the literals each: libzstd decodes by that share"
for _r in (1, 2, 5):
    for _q in ("n", "q"):
        LIBZSTD_DIFFERS["tiny_r%d_%s" % (_r, _q)] = "three shares of (%d + 3) / 4 literals are more than the section holds: libzstd rejects it" % _r


def kernel_constants():
    """the chunking of zg_k_huf, read out of its source"""
    return framesuite.defines(_SRC, ("ZG_HP_CB", "ZG_HP_CB_DENSE", "ZG_HP_ROWS", "ZG_HP_WARM"))


def direct_rule():
    """the host's rule for literals after the scan (ZG_FLAG_LIT_DIRECT), read out of BatchBuilder::finish: (a, b, c) of
    gain_us = literals of blocks without sequences / a and lit_direct = gain_us > b * loss_us + c. A rule of another form fails here"""
    text = open(os.path.join(os.path.dirname(_SRC), "zg_host_parse.cpp")).read()
    g = re.search(r"gain_us = \(double\)huf_noseq / ([0-9.e+]+),", text)
    r = re.search(r"lit_direct = lit_direct_allowed && gain_us > ([0-9.]+) \* loss_us \+ ([0-9.]+);", text)
    assert g and r, "the rule that picks the direct path has changed: test_gpu_hufstreams.test_direct_literals relies on it"
    return float(g.group(1)), float(r.group(1)), float(r.group(2))


# ---- the reference and the model of the chunking ----------------------------------------------------------------------------

def serial_decode(weights, stream, max_bits):
    """one stream, symbol by symbol (RFC 8878 4.2.2; literals_section_decoder.rs:96-115): skip to the closing 1-bit, then peek
    max_bits bits, emit the entry's symbol and consume the entry's bits while bits_remaining > -max_bits; bits below the
    stream's start read as zeros. Returns (symbols, bits_remaining at the end): -max_bits when the last code ends on bit 0"""
    mb, ents, _ = huf_table(weights)
    assert mb == max_bits and stream and stream[-1]
    v = int.from_bytes(stream, "little")
    pos = v.bit_length() - 1                             # bits not yet consumed: the marker is skipped
    mask, out = (1 << mb) - 1, bytearray()
    while pos > 0:                                       # bits_remaining = pos - max_bits
        idx = (v >> (pos - mb) if pos >= mb else v << (mb - pos)) & mask
        sym, nb = ents[idx]
        out.append(sym)
        pos -= nb
    return bytes(out), pos - mb


_MODEL = {}


def chunk_model(weights, stream, K=None):
    """what zg_k_huf's wave does with the stream, window by window: lane l decodes bits (U - cb, U], U = top - l * cb, from
    U + warm-up (lane 0 from the true position top); every lane whose entry differs from its upper neighbour's exit decodes
    again from that exit, all at once, round after round; a pass with more symbols than rows makes the window, and the
    rest of the stream, run again in dense chunks. Returns [{"top", "cb", "rounds", "counts" (symbols per lane on the
    true path), "spill"}] per window pass. The number of rounds is not limited here: the kernel's limit is what is tested"""
    K = K or kernel_constants()
    key = (tuple(weights), bytes(stream), tuple(sorted(K.items())))
    if key in _MODEL:
        return _MODEL[key]
    CB, DENSE, ROWS, WARM = K["ZG_HP_CB"], K["ZG_HP_CB_DENSE"], K["ZG_HP_ROWS"], K["ZG_HP_WARM"]
    mb, ents, _ = huf_table(weights)
    v = int.from_bytes(stream, "little")
    T = v.bit_length() - 1
    s = bin(v)[3:] + "0" * mb                            # the T bits below the marker, the first one read first; zeros below the start
    nbs = [ents[int(s[i:i + mb], 2)][1] for i in range(T)]   # the length of the code met at position T - i

    def run(frm, U, L):
        p = frm
        while p > U:
            p -= nbs[T - p]
        entry, n = p, 0
        while p > L:
            p -= nbs[T - p]
            n += 1
        return entry, p, n

    top, cb, wins = T, CB, []
    while top > 0:
        nact = min(64, (top + cb - 1) // cb)
        UL = [(top - l * cb, max(top - l * cb - cb, 0)) for l in range(nact)]
        res = [run(U + (min(cb, WARM) if l else 0), U, L) for l, (U, L) in enumerate(UL)]
        spill = any(r[2] > ROWS for r in res)
        rounds = 0
        while True:
            need = [l for l in range(1, nact) if res[l - 1][1] != res[l][0]]
            if not need:
                break
            rounds += 1
            assert rounds <= 64 * 64, "the model does not converge"
            prev = list(res)
            for l in need:
                res[l] = run(prev[l - 1][1], *UL[l])
                spill = spill or res[l][2] > ROWS
        wins.append({"top": top, "cb": cb, "rounds": rounds, "counts": [r[2] for r in res], "spill": spill})
        if spill:
            assert cb == CB
            cb = DENSE
            continue
        top = res[nact - 1][1]
    _MODEL[key] = wins
    return wins


# ---- streams ----------------------------------------------------------------------------------------------------------------

# max_bits 11 with a 1-bit symbol; the description's last byte is 0xBA, the highest a direct description can end on (two
# weights of 11 would fill the table). Symbol k = 1 .. 9 has 12 - k bits, symbol 10 one bit, symbol 11 two; the implied symbol 12
# has 11 bits. Symbol 1's code is eleven zeros: cut short, it is a code that reaches below the stream's start
W11 = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 10]
W_DENSE = [3, 2, 1]                                     # lengths 1, 2, 3, 3: symbol 0 is "1", 1 is "01", 2 is "000", 3 is "001"


def by_len(weights):
    out = {}
    for s, (_, nb) in sorted(huf_codes(weights).items()):
        out.setdefault(nb, []).append(s)
    return out


def enc(weights, syms, drop=0):
    """the stream of syms; drop: the last code's lowest `drop` bits are left out (they must be zeros: the decoder reads zeros there)"""
    codes = huf_codes(weights)
    w = RevBits()
    for i, s in enumerate(syms):
        c, nb = codes[s]
        if drop and i == len(syms) - 1:
            assert nb > drop and c & ((1 << drop) - 1) == 0
            c, nb = c >> drop, nb - drop
        w.add(c, nb)
    return w.bytes()


def exact_lens(n, T, rng, first1=0, last1=False):
    """n code lengths of 1 .. 11 bits that sum to T; the first first1 and (last1) the last one are 1"""
    free = list(range(first1, n - (1 if last1 else 0)))
    lens, extra = [1] * n, T - n
    assert 0 <= extra <= 10 * len(free), (n, T)
    while extra:
        i = rng.choice(free)
        add = min(extra, 11 - lens[i], rng.randint(1, 10))
        lens[i] += add
        extra -= add
    return lens


def exact_stream(T, rng, n=None, first1=0, last1=False, weights=W11):
    """a stream of exactly T bits (n symbols; default about T / 4) under W11"""
    n = n or max(1, T // 4)
    bl = by_len(weights)
    return enc(weights, [rng.choice(bl[x]) for x in exact_lens(n, T, rng, first1, last1)])


def split4(n):
    """the format's share of n literals for each of four streams"""
    seg = (n + 3) // 4
    c = [min(seg, max(n - k * seg, 0)) for k in range(3)]
    return c + [n - sum(c)]


def blk(weights, streams, rng, seqs, table=True, lits=None, sf=None):
    """a Block of the given streams; its literals are serial_decode's (lits: the caller's, for a section whose count is wrong)"""
    mb = huf_table(weights)[0]
    dec = [serial_decode(weights, s, mb) for s in streams]
    if lits is None:
        lits = b"".join(d[0] for d in dec)
    sq = _simple_seqs(len(lits), rng, max(1, min(6, len(lits) // 2))) if seqs and lits else []
    b = Block(lits, sq, lit=("hufstreams", list(weights) if table else None, "direct", list(streams), sf))
    b.hs = {"weights": list(weights), "streams": list(streams), "table": table, "decoded": [d[0] for d in dec], "ends": [d[1] for d in dec],
            "max_bits": mb, "bits": [int.from_bytes(s, "little").bit_length() - 1 for s in streams]}
    return b


def frame(name, blocks, valid=True, model=False):
    """tabframes.build, then what this helper adds: where every stream starts in the frame and the byte below it (META[name]["hs"]),
    the chunk model where asked for, and for a valid frame the oracle's literals against serial_decode"""
    r = build(name, blocks, valid=valid, differs=LIBZSTD_DIFFERS)
    z, m, recs = r[1], META[name], []
    for j, b in enumerate(x for x in blocks if isinstance(x, Block)):
        h = b.hs
        ns = len(h["streams"])
        desc = len(weights_direct(h["weights"])) if h["table"] else 0
        body = desc + (6 if ns == 4 else 0) + sum(len(s) for s in h["streams"])
        at = m["lit_off"][j] + len(lit_header(2 if h["table"] else 3, len(b.lits), body, ns, b.lit[4])) + desc + (6 if ns == 4 else 0)
        starts = []
        for s in h["streams"]:
            assert z[at:at + len(s)] == s
            starts.append(at)
            at += len(s)
        rec = dict(h, starts=starts, below=[z[a - 1] for a in starts], nseq=len(b.seqs), regen=len(b.lits))
        if model:
            rec["model"] = [chunk_model(h["weights"], s) for s in h["streams"]]
        recs.append(rec)
    m["hs"] = recs
    if r[2] is not None:
        ob = [x for x in blockcheck.oracle_blocks(z) if x["type"] == 2]
        assert len(ob) == len(recs), name
        for x, rec in zip(ob, recs):
            assert x["literals"] == b"".join(rec["decoded"]), (name, "the oracle's literals are not serial_decode's")
    return r


def both(name, make, **kw):
    """every shape twice: without sequences ("_n": the block can take the direct path) and with a few simple ones ("_q")"""
    return [frame("%s_%s" % (name, "q" if q else "n"), make(q), **kw) for q in (0, 1)]


# ---- the families: each returns [(name, zst, plaintext or None)] ------------------------------------------------------------

NEVER_RESYNC = {"flat3": [1] * 7, "flat5": [1] * 31, "flat6": [1] * 63, "flat7": [1] * 127, "len3and6": [4] * 7 + [1] * 7, "flat4_control": [1] * 15}


def never_resync():
    """codes whose every misplaced decoder stays misplaced: a lane is corrected one round after the lane above it, so a full window
    needs 63 redo rounds of the 64 the loop gives. Flat codes of 3, 5, 6 and 7 bits and one of lengths 3 and 6; the flat 4-bit code
    is in step by construction (chunk and warm-up are multiples of 4) and needs none"""
    rng = random.Random(611)
    out = []
    for cname, w in NEVER_RESYNC.items():
        syms = sorted(huf_codes(w))
        for ns, n in ((1, 1000), (4, 40000)):
            lits = _lits_covering(syms, n, rng)
            cnt = [n] if ns == 1 else split4(n)
            streams = [enc(w, lits[sum(cnt[:k]):sum(cnt[:k + 1])]) for k in range(ns)]
            out += both("nr_%s_%ds" % (cname, ns), lambda q: [blk(w, streams, rng, q)], model=True)
    return out


def _dense_stream(rng, want, place, K):
    """a stream of 3-bit symbols with one run of the 1-bit symbol, placed so that under chunk_model one chunk holds exactly `want`
    symbols: in lane 0 of the first window ("lane0"), in a later lane of it ("lane") or in the second window ("window"). With
    want = rows no chunk of the stream spills; with rows + 1 the first spill is that chunk's"""
    CB, ROWS = K["ZG_HP_CB"], K["ZG_HP_ROWS"]
    n = 5200
    off = {"lane0": 0, "lane": 5 * CB, "window": 64 * CB + 3 * CB}[place]
    for k in range(4, 16):
        for i0 in range(off // 3, off // 3 + CB // 3 + 2):
            lens = [3] * n
            lens[i0:i0 + k] = [1] * k
            # symbols per chunk on the true path: the first window from position 0, the second from the first code boundary past it
            o, starts = 0, []
            for x in lens:
                starts.append(o)
                o += x
            base2 = next(s for s in starts if s >= 64 * CB)
            cnt = {}
            for s in starts:
                if s < 64 * CB:
                    key = (0, s // CB)
                elif s < base2 + 64 * CB:
                    key = (1, (s - base2) // CB)
                else:
                    break
                cnt[key] = cnt.get(key, 0) + 1
            tgt = max(cnt, key=lambda c: cnt[c])
            if cnt[tgt] != want or tgt != (off // (64 * CB), (off % (64 * CB)) // CB) or sorted(cnt.values())[-2] > ROWS - 2:
                continue
            stream = enc(W_DENSE, [0 if x == 1 else rng.choice((2, 3)) for x in lens])
            got = _dense_class(chunk_model(W_DENSE, stream, K), K)
            if got and got[:2] == (want, place):
                return stream
    raise AssertionError("no stream with a chunk of %d symbols at %s" % (want, place))


def _dense_class(wins, K):
    """(symbols in the fullest chunk, its placement, dense windows behind the one that ran again) of a modelled stream whose
    fullest full-size chunk holds exactly rows symbols and never spills, or rows + 1 and is the first to spill; else None"""
    CB, ROWS = K["ZG_HP_CB"], K["ZG_HP_ROWS"]
    full = [w for w in wins if w["cb"] == CB]
    first = next((i for i, w in enumerate(full) if w["spill"]), None)
    if first is None:
        mx = max(max(w["counts"]) for w in full)
        if mx != ROWS:
            return None
        i = next(i for i, w in enumerate(full) if max(w["counts"]) == mx)
        want = ROWS
    else:
        i, want = first, ROWS + 1
        if max(full[i]["counts"]) != want or len(full) != first + 1:
            return None
    lanes = [l for l, c in enumerate(full[i]["counts"]) if c == want]
    if len(lanes) != 1:
        return None
    place = "window" if i >= 1 else "lane0" if lanes[0] == 0 else "lane"
    return want, place, len([w for w in wins if w["cb"] != CB]) - 1


def dense_switch():
    """the switch to dense chunks: a chunk of exactly as many symbols as a lane has rows (no switch) and of one more (the window,
    and the rest of the stream, runs again in 32-bit chunks), in lane 0 of the first window, in a later lane and in the second
    window (symbols already written); runs of the 1-bit symbol: 128 symbols per chunk"""
    rng = random.Random(622)
    K = kernel_constants()
    out = []
    for want in (K["ZG_HP_ROWS"], K["ZG_HP_ROWS"] + 1):
        for place in ("lane0", "lane", "window"):
            target = _dense_stream(rng, want, place, K)
            n = len(serial_decode(W_DENSE, target, 3)[0])
            streams = [enc(W_DENSE, [rng.choice((2, 3)) for _ in range(n)]) for _ in range(4)]
            streams[1] = target
            out += both("dense_%s_%s" % ("fits" if want == K["ZG_HP_ROWS"] else "spills", place), lambda q: [blk(W_DENSE, streams, rng, q)], model=True)
    run1 = enc(W_DENSE, [0 if i % 97 else 1 + i // 97 % 3 for i in range(1000)])
    out += both("dense_runs_1s", lambda q: [blk(W_DENSE, [run1], rng, q)], model=True)
    runs4 = [enc(W_DENSE, [0 if (i + k) % 211 else 1 + i // 211 % 3 for i in range(6000)]) for k in range(4)]
    out += both("dense_runs_4s", lambda q: [blk(W_DENSE, runs4, rng, q)], model=True)
    return out


SINGLE_BITS = (1, 2, 8, 10, 11, 12, 13, 14, 127, 128, 129, 1000, 8120, 8127)     # 8127: 1016 bytes, with the description 1023
WINDOW_BITS = tuple(b + r for b in (8192, 16384, 24576) for r in (-1, 0, 1, 127, 128, 129))


def stream_lengths():
    """stream bit counts at the edges of a lane's chunk and of a window (nact from top, the window carry, a last lane whose chunk
    is one bit), every number of payload bits in the last byte, the lone marker byte 0x01 above whole bytes, max_bits 11. Single
    streams hold up to 8127 bits; the counts around one, two and three windows are those of all four streams of a frame"""
    rng = random.Random(633)
    out = []
    for T in SINGLE_BITS:
        s = exact_stream(T, rng, n=max(1, min(1023, T // 4)))
        out += both("sl_1s_T%d" % T, lambda q: [blk(W11, [s], rng, q)])
    for T in WINDOW_BITS:
        streams = [exact_stream(T, rng) for _ in range(4)]
        out += both("sl_4s_T%d" % T, lambda q: [blk(W11, streams, rng, q)])
    return out


def start_alignment():
    """the stream's start at each of the 16 byte alignments: the address arithmetic of the staging (the first staged piece, the
    position of bit 0 in it, loads that begin below the stream) for a single stream, moved by a raw block of 0 .. 15 bytes in
    front, and for streams 1 .. 3 of four, moved by the length of the stream in front. max_bits 11, the last symbol a 1-bit code
    whose peek reads 10 bits below the start; the byte there is the description's 0xBA or the 0xFF of the stream in front. These
    frames do not tell whether the bytes below the start are zeroed: a whole code selects the same entry whatever lies below
    it. The overshoot family does that, at the same 16 alignments"""
    rng = random.Random(644)
    out = []
    for p in range(16):
        s = exact_stream(300, rng, n=60, last1=True)
        pre = ("raw", rng.randbytes(p))
        out += both("sa_s0_p%d" % p, lambda q: [pre, blk(W11, [s], rng, q)])
    for j in range(16):
        streams = [exact_stream(8 * (12 + j + 3 * k) + 7, rng, n=40, first1=7, last1=True) for k in range(4)]
        out += both("sa_sk_j%d" % j, lambda q: [blk(W11, streams, rng, q)])
    return out


OVERSHOOT = (1, 5, 10)


def overshoot():
    """a last code that reaches 1, 5 and 10 bits below the stream's start (eleven zeros, cut short; the byte below the start is
    the description's 0xBA or the 0xFF of the stream in front): what it decodes to depends on the zeros the kernel stages below
    the start. In a single stream the reference makes no end check: the frame is valid when the section's count includes that
    symbol. Each valid frame has 16 such blocks, every one with its own description, and raw blocks between them sized so that
    the 16 streams start at the 16 byte alignments of the frame: the straddling 16-byte piece is zeroed for 1 .. 15 bytes, and
    not at all. With a count one short the frame is invalid. In four streams every stream must end on its last bit:
    BitstreamReadMismatch, whichever stream it is, and in front of a count that is off as well"""
    rng = random.Random(655)
    bl = by_len(W11)
    some = lambda n: [rng.choice(bl[rng.randint(1, 11)]) for _ in range(n)]
    pre = ("raw", rng.randbytes(5))
    out = []
    for d in OVERSHOOT:
        for q in (0, 1):
            name = "ov_1s_d%d_%s" % (d, "q" if q else "n")
            blocks = [blk(W11, [enc(W11, some(30) + [1], drop=d)], rng, q) for _ in range(16)]
            assert all(b.hs["ends"] == [-11 - d] for b in blocks)
            # where the streams start with empty raw blocks in front of each; a pad in front of block i moves it and every later one
            z0 = build(name, [x for b in blocks for x in (("raw", b""), b)], differs=LIBZSTD_DIFFERS)[1]
            at, starts0 = 0, []
            for b in blocks:
                at = z0.index(b.hs["streams"][0], at)
                starts0.append(at)
                at += 1
            pads, moved = [], 0
            for i, a in enumerate(starts0):
                pads.append((i - a - moved) % 16)
                moved += pads[-1]
            out.append(frame(name, [x for b, n in zip(blocks, pads) for x in (("raw", rng.randbytes(n)), b)]))
        s = enc(W11, some(30) + [1], drop=d)
        short = serial_decode(W11, s, 11)[0][:-1]
        out += both("ov_1s_d%d_short" % d, lambda q: [pre, blk(W11, [s], rng, q, lits=short)], valid=False)
        for k in range(4):
            streams = [exact_stream(8 * 11 + 7, rng, n=20, first1=7) for _ in range(4)]
            streams[k] = enc(W11, [10] * 7 + some(12) + [1], drop=d)
            fr = both("ov_4s_k%d_d%d" % (k, d), lambda q: [blk(W11, streams, rng, q)], valid=False)
            assert all(STATUS[f[0]] == 34 for f in fr), [STATUS[f[0]] for f in fr]
            out += fr
    streams = [exact_stream(8 * 11 + 7, rng, n=20, first1=7) for _ in range(4)]
    streams[1] = enc(W11, [10] * 7 + some(12) + [1], drop=5)
    lits = b"".join(serial_decode(W11, s, 11)[0] for s in streams) + b"\x00"
    out += both("ov_4s_two_defects", lambda q: [blk(W11, streams, rng, q, lits=lits)], valid=False)
    return out


def tiny_four_streams():
    """four streams of 1 .. 12 literals in the format's split, a lone 0x01 where a stream gets no symbol (the encoder uses four
    streams from 256 literals up), and splits that differ from the format's but add up (zg_k_huf_uneven). The oracle accepts
    every one of them"""
    rng = random.Random(666)
    bl = by_len(W11)
    st = lambda n: enc(W11, [rng.choice(bl[rng.randint(1, 11)]) for _ in range(n)])
    out = []
    for regen in range(1, 13):
        streams = [st(n) for n in split4(regen)]
        out += both("tiny_r%d" % regen, lambda q: [blk(W11, streams, rng, q)])
    for name, cnt in (("tiny_uneven_r8", (1, 3, 2, 2)), ("tiny_uneven_r6_empty", (0, 3, 3, 0))):
        streams = [st(n) for n in cnt]
        out += both(name, lambda q: [blk(W11, streams, rng, q)])
    return out


def groups():
    """zg_k_huf's workgroups of two waves that share a staged table: one table-carrying block and treeless blocks behind it, so
    that 1, 2, 3, 5 and 6 streams use one table slot (a lone wave in a group), and a stream of more than two windows in one group
    with a stream of at most 16 bits, in both orders"""
    rng = random.Random(677)
    out = []
    one = lambda T: [exact_stream(T, rng)]
    four = lambda T: [exact_stream(T, rng) for _ in range(4)]
    long_bits = 2 * 64 * kernel_constants()["ZG_HP_CB"] + 300
    shapes = {
        "grp_1": [one(700)],
        "grp_2": [one(700), one(90)],
        "grp_3": [one(131), one(2000), one(9)],
        "grp_5": [four(3000), one(500)],
        "grp_short_long": [one(13), four(long_bits)],                    # (13 bits, stream 0 of four) | (1, 2) | (3)
        "grp_long_short": [one(400), four(long_bits), one(16)],          # (400 bits, 0) | (1, 2) | (stream 3 of four, 16 bits)
    }
    for name, sh in shapes.items():
        out += both(name, lambda q: [blk(W11, s, rng, q, table=(i == 0)) for i, s in enumerate(sh)])
    return out


FAMILIES = {
    "never_resync": never_resync,
    "dense_switch": dense_switch,
    "stream_lengths": stream_lengths,
    "start_alignment": start_alignment,
    "overshoot": overshoot,
    "tiny_four_streams": tiny_four_streams,
    "groups": groups,
}


def _check_differs(frames):
    """the LIBZSTD_DIFFERS cap, once every family is built"""
    names = [n for _, n, _, p in frames if p is not None]
    assert set(LIBZSTD_DIFFERS) <= set(names), ("LIBZSTD_DIFFERS may hold only frames the oracle accepts", sorted(set(LIBZSTD_DIFFERS) - set(names)))
    assert len(LIBZSTD_DIFFERS) * 10 <= len(names), "LIBZSTD_DIFFERS holds more than a tenth of the valid frames"


_F = framesuite.Families(FAMILIES, _check_differs)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


def coverage(frames):
    """what the frames reach, from the writer's records and chunk_model; asserts every condition the families are there for, so that
    a generator that loses one fails here. frames is all_frames()'s list. Returns the figures"""
    K = kernel_constants()
    CB = K["ZG_HP_CB"]
    cov = {"valid": 0, "invalid": 0, "statuses": set(), "rounds": {}, "dense": {}, "runs_per_chunk": 0, "single_bits": set(), "four_bits": set(),
           "payload_bits": set(), "marker_byte_alone": False, "max_bits": {}, "align": {0: set(), 1: set()}, "below": {0: set(), 1: set()},
           "overshoot_valid": set(), "overshoot_short": set(), "overshoot_four": set(), "overshoot_align": {}, "overshoot_below": set(), "two_defects": None, "tiny": {}, "empty_streams": 0,
           "uneven": [], "group_streams": set(), "pairs": set(), "with_seq": {}, "per_family": {}}
    for fam, name, z, plain in frames:
        hs = META[name]["hs"]
        cov["valid" if plain is not None else "invalid"] += 1
        cov["per_family"][fam] = cov["per_family"].get(fam, 0) + 1
        cov["with_seq"].setdefault(fam, set()).add(any(r["nseq"] for r in hs))
        cov["max_bits"].setdefault(fam, set()).update(r["max_bits"] for r in hs)
        if plain is None:
            cov["statuses"].add(STATUS[name])
        if fam == "never_resync":
            cov["rounds"][name] = [max(w["rounds"] for w in m) for m in hs[0]["model"]]
        if fam == "dense_switch":
            for m in hs[0]["model"]:
                c = _dense_class(m, K)
                if c:
                    cov["dense"][c[:2]] = max(cov["dense"].get(c[:2], -1), c[2])
                cov["runs_per_chunk"] = max(cov["runs_per_chunk"], max(max(w["counts"]) for w in m if w["cb"] == CB))
        if fam == "stream_lengths":
            for r in hs:
                if len(set(r["bits"])) == 1:                 # (of four streams: all four have this many bits)
                    (cov["single_bits"] if len(r["bits"]) == 1 else cov["four_bits"]).add(r["bits"][0])
                cov["payload_bits"].update(b % 8 for b in r["bits"])
                cov["marker_byte_alone"] |= any(s[-1] == 1 and len(s) > 1 for s in r["streams"])
        if fam == "start_alignment":
            r = hs[0]
            one_bit = {s for s, (_, nb) in huf_codes(r["weights"]).items() if nb == 1}
            assert r["max_bits"] == 11 and all(d[-1] in one_bit and e == -11 for d, e in zip(r["decoded"], r["ends"])), name
            for k, (a, b) in enumerate(zip(r["starts"], r["below"])):
                if (len(r["starts"]) == 1) == (k == 0):       # stream 0 of the single streams, streams 1 .. 3 of the others
                    cov["align"][min(k, 1)].add(a % 16)
                    cov["below"][min(k, 1)].add(b)
        if fam == "overshoot":
            for r in hs:
                over = [(k, -e - r["max_bits"]) for k, e in enumerate(r["ends"]) if e != -r["max_bits"]]
                assert len(over) == 1, name
                k, d = over[0]
                got = sum(len(x) for x in r["decoded"])
                if len(r["ends"]) == 1:
                    cov["overshoot_valid" if plain is not None else "overshoot_short"].add(d)
                    if plain is not None:
                        cov["overshoot_align"].setdefault((d, r["nseq"] > 0), set()).add(r["starts"][0] % 16)
                        cov["overshoot_below"].add(r["below"][0])
                    assert r["regen"] == got - (plain is None), name
                elif r["regen"] == got:
                    cov["overshoot_four"].add((k, d))
                    assert STATUS[name] == 34, name
                else:
                    cov["two_defects"] = STATUS[name]
        if fam == "tiny_four_streams":
            r = hs[0]
            cnt = [len(x) for x in r["decoded"]]
            cov["empty_streams"] += sum(s == b"\x01" for s in r["streams"])
            if cnt == split4(r["regen"]):
                cov["tiny"][r["regen"]] = 0 if plain is not None else STATUS[name]
            else:
                cov["uneven"].append((tuple(cnt), 0 if plain is not None else STATUS[name]))
        if fam == "groups":
            bits = [b for r in hs for b in r["bits"]]
            cov["group_streams"].add(len(bits))
            for i in range(0, len(bits) - 1, 2):            # the host's groups: the items of a table slot in order, two at a time
                lo, hi = sorted(bits[i:i + 2])
                if lo <= 16 and hi >= 2 * 64 * CB:
                    cov["pairs"].add("short_long" if bits[i] == lo else "long_short")
    # ---- the conditions
    for cname in NEVER_RESYNC:
        for q in "nq":
            four, single = cov["rounds"]["nr_%s_4s_%s" % (cname, q)], cov["rounds"]["nr_%s_1s_%s" % (cname, q)]
            if cname == "flat4_control":
                assert max(four + single) == 0, (cname, four, single)
            else:
                assert max(four) >= 60 and max(four) < 64, (cname, four)
                assert single[0] >= 5, (cname, single)
    R = K["ZG_HP_ROWS"]
    for want in (R, R + 1):
        for place in ("lane0", "lane", "window"):
            assert (want, place) in cov["dense"], ("no chunk of %d symbols at %s" % (want, place), cov["dense"])
            assert want == R or cov["dense"][(want, place)] >= 2, ("fewer than two windows behind the switch", want, place, cov["dense"])
    assert cov["runs_per_chunk"] >= CB - 2, cov["runs_per_chunk"]
    assert cov["single_bits"] >= {1, 2, 10, 11, 12, 127, 128, 129}, cov["single_bits"]
    assert cov["four_bits"] >= {b + r for b in (8192, 16384, 24576) for r in (-1, 0, 1, 127, 128, 129)}, cov["four_bits"]
    assert cov["payload_bits"] == set(range(8)) and cov["marker_byte_alone"], cov["payload_bits"]
    assert all(11 in cov["max_bits"][f] for f in FAMILIES if f not in ("never_resync", "dense_switch")), cov["max_bits"]
    assert cov["align"][0] == set(range(16)) and cov["align"][1] == set(range(16)), cov["align"]
    assert cov["below"] == {0: {0xBA}, 1: {0xFF}}, cov["below"]
    assert cov["overshoot_valid"] == set(OVERSHOOT) == cov["overshoot_short"], (cov["overshoot_valid"], cov["overshoot_short"])
    assert set(cov["overshoot_align"]) == {(d, q) for d in OVERSHOOT for q in (False, True)}, cov["overshoot_align"]
    assert all(v == set(range(16)) for v in cov["overshoot_align"].values()) and cov["overshoot_below"] == {0xBA}, (cov["overshoot_align"], cov["overshoot_below"])
    assert cov["overshoot_four"] == {(k, d) for k in range(4) for d in OVERSHOOT}, cov["overshoot_four"]
    assert cov["two_defects"] is not None
    assert set(cov["tiny"]) >= set(range(4, 13)) and cov["empty_streams"] >= 4 and cov["uneven"], (cov["tiny"], cov["uneven"])
    assert cov["group_streams"] >= {1, 2, 3, 5} and cov["pairs"] == {"short_long", "long_short"}, (cov["group_streams"], cov["pairs"])
    assert all(v == {False, True} for v in cov["with_seq"].values()), cov["with_seq"]
    return cov
