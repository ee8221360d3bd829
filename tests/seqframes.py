"""Frames built from chosen sequences (test helper, no tests): libzstd's ZSTD_compressSequences encodes a list of (literal length,
raw offset, match length) triples we pick, so that the constants where the kernels go wrong are hit on purpose and not by chance.

frame() returns (zst, plaintext). The plaintext comes from a plain Python LZ77 execution of the sequences (the high-precision
reference); every frame is checked here against libzstd's decompressor and against the oracle before it is returned, so a
generator bug can neither pass as a decoder bug nor hide one. The families below are seeded and each names the kernel and the
constant it aims at. libzstd is 1.4.9 here; what that version accepts shapes the helper (see frame())."""
import ctypes as C
import os
import random
import sys

import framesuite
import oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import zgdata  # noqa: E402

BLOCK = 131072                       # Block_Maximum_Size == ZG_FLAT_MAX
RAND = bytes(range(256))             # uniform literals: libzstd keeps them raw
SKEW = b"eeeeeeeetttttaaaooiinnsshrdlcumwfgypbvkjxqz  \n"     # skewed alphabet: Huffman literals
RLE = b"\x5a"                        # one byte: RLE literals


class ZSTDSequence(C.Structure):
    _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]


_BOUND = False


def libzstd():
    """zgdata's libzstd with ZSTD_compressSequences bound as well"""
    global _BOUND
    L = zgdata.libzstd()
    if not _BOUND:
        L.ZSTD_compressSequences.restype = C.c_size_t
        L.ZSTD_compressSequences.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ZSTDSequence), C.c_size_t, C.c_void_p, C.c_size_t]
        L.ZSTD_getErrorName.restype = C.c_char_p
        L.ZSTD_getErrorName.argtypes = [C.c_size_t]
        _BOUND = True
    return L


def lz77(seqs, lits):
    """plain LZ77 execution: lits holds the literal bytes of all sequences in order, then the trailing literals"""
    out = bytearray()
    lp = 0
    for ll, of, ml in seqs:
        out += lits[lp:lp + ll]
        lp += ll
        assert ml >= 3 and 1 <= of <= len(out), (of, len(out))
        if of >= ml:
            out += out[len(out) - of:len(out) - of + ml]
        else:                                            # self-overlapping: the last `of` bytes repeat
            pat = bytes(out[len(out) - of:])
            out += (pat * (ml // of + 1))[:ml]
    out += lits[lp:]
    return bytes(out)


def literals(n, alphabet=RAND, seed=0):
    rng = random.Random(seed)
    if len(alphabet) == 256 and alphabet == RAND:
        return rng.randbytes(n)
    return bytes(rng.choices(alphabet, k=n))


def frame(seqs, tail=0, *, lits=RAND, seed=0, level=3, lit_mode=0, window_log=0, checksum=True, content_size=True, single_block=True):
    """seqs: [(ll, offset, ml)] with offset the raw distance; tail: trailing literals; lits: the alphabet the literal bytes are drawn
    from (seeded). single_block: one block with explicit delimiters (exactly these sequences in one block, output <= 131072 bytes);
    else no delimiters and libzstd cuts blocks every 128 KiB itself, splitting a sequence that crosses a cut (libzstd 1.4.9 rejects
    explicit delimiters in frames of more than one block). lit_mode: 0 auto, 1 Huffman, 2 uncompressed. Returns (zst, plaintext)."""
    nlit = sum(s[0] for s in seqs) + tail
    plain = lz77(seqs, literals(nlit, lits, seed))
    if single_block:
        assert len(plain) <= BLOCK, len(plain)
    L = libzstd()
    arr = (ZSTDSequence * (len(seqs) + 1))()
    for i, (ll, of, ml) in enumerate(seqs):
        arr[i].offset, arr[i].litLength, arr[i].matchLength = of, ll, ml
    n = len(seqs)
    if single_block:                                     # the block delimiter: offset 0, match 0, the trailing literals
        arr[n].offset, arr[n].litLength, arr[n].matchLength = 0, tail, 0
        n += 1
    cctx = L.ZSTD_createCCtx()
    try:
        for p, v in ((100, level), (105, 3), (1008, 1 if single_block else 0), (1009, 1), (1002, lit_mode),
                     (201, 1 if checksum else 0), (200, 1 if content_size else 0)) + (((101, window_log),) if window_log else ()):
            r = L.ZSTD_CCtx_setParameter(cctx, p, v)
            assert not L.ZSTD_isError(r), (p, v, L.ZSTD_getErrorName(r))
        cap = L.ZSTD_compressBound(len(plain)) + 1024
        dst = C.create_string_buffer(cap)
        r = L.ZSTD_compressSequences(cctx, dst, cap, arr, n, plain, len(plain))
        if L.ZSTD_isError(r):
            raise RuntimeError("ZSTD_compressSequences: %s" % L.ZSTD_getErrorName(r).decode())
        z = dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(cctx)
    assert zgdata.zstd_decompress(z, len(plain)) == plain
    d = oracle.FrameDecoder()
    st, c, _, _ = d.init(z)
    assert st == 0, st
    st, _, fin = d.decode_blocks(z[c:], oracle.STRAT_ALL)
    assert st == 0 and fin, st
    assert d.collect() == plain
    return z, plain


# ---- the families: each returns [(name, zst, plaintext)] --------------------------------------------------------------------

SHORT_OFFS = list(range(1, 17)) + [31, 32, 33, 63, 64, 65]


def short_offsets():
    """offsets 1..16, 31-33, 63-65 under matches of 3 .. 131000 bytes, alone and in dense random mixes: self-overlapping copies in
    zg_k_flatten (zg_flat4.h overlap step), the sweep's pointer chains (zg_flat1.h + zg_k_sweep), zg_k_lz and zg_k_sparse"""
    out = []
    for ml in (3, 4, 17, 255, 4096):
        seqs = [(70, SHORT_OFFS[0], ml)] + [(1 + i % 3, of, ml) for i, of in enumerate(SHORT_OFFS[1:])]
        out.append(("short_ml%d" % ml, *frame(seqs, 5, lits=SKEW, seed=ml)))
    for ml in (65536, 131000):                           # one whole match per block: single-block frames, a few back to back
        for of in (1, 2, 3, 7, 16, 33, 65):
            out.append(("short_ml%d_of%d" % (ml, of), *frame([(of + 2, of, ml)], 3, seed=of, level=1)))
    rng = random.Random(11)
    for k, (n, mlmax) in enumerate(((20000, 8), (6000, 40), (2000, 300))):
        seqs, pos = [(70, 16, 3)], 73
        while len(seqs) < n:
            ll = rng.choice((0, 0, 0, 1, 2, 5))
            ml = rng.randint(3, mlmax)
            if pos + ll + ml > BLOCK - 8:
                break
            seqs.append((ll, rng.choice(SHORT_OFFS), ml))
            pos += ll + ml
        out.append(("short_mix%d" % k, *frame(seqs, 8, lits=SKEW, seed=k, level=(1, 3, 19)[k])))
    # across blocks: multi-block frames of short-offset runs (sequences split at libzstd's cuts), the later blocks in units of their
    # own (pointer-mode flatten + sweep chains)
    seqs = [(of + 1, of, (65536, 131000)[i % 2]) for i, of in enumerate((1, 2, 3, 5, 8, 13, 16, 32, 33, 64, 65))]
    out.append(("short_long_multiblock", *frame(seqs, 10, seed=6, single_block=False)))
    seqs = [(64, 1, 3)] + [(rng.randint(0, 3), rng.choice(SHORT_OFFS), rng.randint(3, 9000)) for _ in range(120)]
    out.append(("short_multiblock", *frame(seqs, 10, lits=SKEW, seed=5, single_block=False)))
    return out


def match_lengths():
    """match lengths at the ML code edges (34/35, 131/259) and at the 15-bit split of ZG_SEQ_ML / ZG_SEQ_W1 / ZG_SEQ_W2 (32767 / 32768 /
    32769), 65535 / 65536 and the largest a block holds (131071 after one literal; 131072 with no literal in a frame's second
    block). 131074, the largest ML code 52 can say, never fits a block (Block_Maximum_Size 131072), so no valid frame holds it."""
    out = []
    small = [3, 4, 34, 35, 131, 259]
    seqs = [(40, 40, small[0])] + [(3, 17 + i, m) for i, m in enumerate(small[1:])]
    seqs += [(1, 500, 32767), (2, 5, 32768), (0, 32769, 32769)]
    out.append(("ml_edges_15bit", *frame(seqs, 7, lits=SKEW, seed=1)))
    # the same lengths among many short sequences: not a sparse frame, so zg_k_flatten's direct unit (zg_flat4.h) places them
    rng = random.Random(5)
    short = [(rng.randint(0, 4), rng.randint(1, 200), rng.randint(3, 12)) for _ in range(300)]
    seqs = [(200, 200, 8)] + short[:150] + [(1, 77, 32767), (0, 1, 32768), (3, 32769, 32769)] + short[150:]
    out.append(("ml_15bit_dense", *frame(seqs, 5, lits=SKEW, seed=6)))
    out.append(("ml_65535_65536_exact_block", *frame([(1, 1, 65535), (0, 3, 65536)], 0, seed=2)))   # 131072 bytes
    out.append(("ml_131071", *frame([(1, 1, 131071)], 0, seed=3, level=19)))
    # ML 131072 with LL 0: the second block of a frame, copying from the first (no delimiters: libzstd cuts at 131072)
    seqs = [(40, 40, 1000)] * 100 + [(BLOCK - 100 * 1040, BLOCK, BLOCK)]
    out.append(("ml_131072_ll0_second_block", *frame(seqs, 0, lits=SKEW, seed=4, single_block=False)))
    return out


def literal_lengths():
    """LL 0 with every repeat-offset rule (rep1 -> repeat code 1 means rep2, code 2 rep3, code 3 rep0 - 1) and LL > 0 with the plain
    rules (zg_k_seq's offset history, zg_k_scan), the LL code edges 15 / 16 / 63 / 64 / 65535 / 65536, and lit_start near the 17-bit
    ZG_SEQ_LIT field: a block that is all literals but one 3-byte match, a second sequence whose literals start at 131060"""
    out = []
    A, B, Cc = 300, 200, 100                             # rep history after three plain offsets: rep0 = C, rep1 = B, rep2 = A
    seqs = [(400, A, 5), (2, B, 6), (3, Cc, 7)]
    seqs += [(0, B, 4), (0, A, 5), (0, Cc - 1, 6), (0, 77, 3)]          # LL 0: rep1, rep2, rep0 - 1, and a plain offset
    seqs += [(1, 77, 4), (2, Cc - 1, 5), (3, B, 6), (0, 76, 7), (0, 77, 8)]   # LL > 0 repeats, then LL 0 -> rep1 again
    seqs += [(0, 77, 3), (0, 76, 3)] * 40                               # alternate: LL 0 rep1 forever
    out.append(("ll0_repeat_rules", *frame(seqs, 3, lits=SKEW, seed=1)))
    out.append(("ll0_repeat_rules_l19", *frame(seqs, 3, lits=SKEW, seed=1, level=19)))
    seqs = [(64, 50, 10), (15, 20, 3), (16, 20, 4), (63, 31, 5), (64, 30, 6), (65535, 77, 20), (0, 65000, 4)]
    out.append(("ll_edges", *frame(seqs, 9, lits=SKEW, seed=2)))
    out.append(("ll_65536", *frame([(65536, 65536, 300), (3, 4, 5)], 2, seed=3)))
    out.append(("ll_all_but_one_match", *frame([(131069, 131069, 3)], 0, seed=4)))
    out.append(("lit_start_131060", *frame([(131060, 5, 3), (5, 7, 4)], 0, lits=SKEW, seed=5)))
    return out


def seq_counts():
    """sequence counts at the 1/2/3-byte nbSeq forms (127/128, 0x7EFF/0x7F00/0x7F01), at and across ZG_SEQ_CH (12) / ZG_SP_S (8)
    multiples and 2048 (zg_k_seq's chunks, zg_k_sparse's steps, the 2048-sequence rounds), up to the most a block holds
    (ML 3, LL 0: 43690) — one block each"""
    out = []
    out.append(("nseq0", *frame([], 600, lits=SKEW, seed=9)))
    for n in (1, 8, 11, 12, 13, 24, 127, 128, 2047, 2048, 2049, 0x7EFF, 0x7F00, 0x7F01, (BLOCK - 64) // 3):
        rng = random.Random(n)
        seqs = [(64, 64, 3)]
        pos = 67
        while len(seqs) < n:
            ll = 0 if n > 4000 else rng.choice((0, 1, 2, 7))
            of = rng.choice((1, 2, 3, rng.randint(1, pos)))
            seqs.append((ll, of, 3))
            pos += ll + 3
        level = 19 if n in (2048, 0x7F00) else 1 if n in (127, 0x7EFF) else 3
        out.append(("nseq%d" % n, *frame(seqs[:n], BLOCK - pos if n == (BLOCK - 64) // 3 else 4, lits=SKEW, seed=n, level=level)))
    return out


def block_sizes():
    """exact 131072-byte blocks (ZG_FLAT_MAX: zg_k_flatten's per-block bound), 1- and 4-byte blocks, a run of maximum blocks in one
    frame (libzstd cuts every 131072 bytes) and a run of exact single-block frames"""
    out = []
    out.append(("block_1byte", *frame([], 1, seed=1)))
    out.append(("block_4byte", *frame([(1, 1, 3)], 0, seed=2)))
    rng = random.Random(3)
    for k in range(3):
        seqs, pos = [(100, 100, 50)], 150
        while True:
            ll, ml = rng.randint(0, 30), rng.randint(3, 200)
            if pos + ll + ml > BLOCK:
                break
            seqs.append((ll, rng.randint(1, pos), ml))
            pos += ll + ml
        out.append(("block_exact_%d" % k, *frame(seqs, BLOCK - pos, lits=SKEW, seed=k, level=(1, 3, 19)[k])))
    seqs, pos = [(100, 100, 50)], 150
    while pos < 12 * BLOCK:
        ll, ml = rng.randint(0, 40), rng.randint(3, 300)
        seqs.append((ll, rng.randint(1, min(pos, 1 << 20)), ml))
        pos += ll + ml
    out.append(("block_run_of_max", *frame(seqs, 0, lits=SKEW, seed=7, single_block=False, window_log=21)))
    return out


def far_offsets():
    """offsets of exactly the current position (back to the frame's first byte), exactly window_size and window_size - 1, and offsets
    crossing many units (zg_k_seqpost's window check, zg_k_sweep / split sweep, zg_k_exact), window logs 10, 17, 20 and 24"""
    out = []
    rng = random.Random(21)
    for wlog, nblk in ((10, 3), (17, 20), (20, 24), (24, 132)):
        W = 1 << wlog
        seqs, pos = [(64, 64, 10), (5, 79, 6)], 85          # the second reaches back to the frame's first byte
        target = nblk * BLOCK if wlog > 10 else 24 * 1024
        while pos < target:                              # dense short matches nearby; every so often a far one
            ll = rng.randint(0, 24)
            if pos + ll > W and rng.random() < 0.02:
                of = rng.choice((W, W - 1))
            elif pos + ll <= W and rng.random() < 0.01:
                of = pos + ll                            # the frame's first byte, while the frame is younger than its window
            else:
                of = rng.randint(1, min(pos + ll, 4096, W))
            ml = rng.randint(3, 64) if wlog < 24 else rng.randint(3000, 20000)
            seqs.append((ll, of, ml))
            pos += ll + ml
        seqs += [(3, W, 7), (0, W - 1, 9)]               # exactly window_size and window_size - 1 back
        out.append(("far_w%d" % wlog, *frame(seqs, 11, lits=SKEW, seed=wlog, window_log=wlog, single_block=False,
                                             level=3 if wlog < 24 else 1)))
    return out


def literal_modes():
    """raw, RLE, 1-stream and 4-stream Huffman and treeless (repeat) literals (zg_k_huf, zg_k_tables), each with levels 1, 3, 19
    so that predefined, RLE, compressed and repeat FSE modes occur for LL, OF and ML (zg_k_tables, zg_k_seq)"""
    out = []
    rng = random.Random(31)
    for level in (1, 3, 19):
        for lname, alpha, mode in (("raw", RAND, 2), ("rle", RLE, 0), ("huf", SKEW, 1)):
            # single block, few sequences with few literals: 1-stream Huffman, predefined or RLE FSE modes
            out.append(("lit_%s_small_l%d" % (lname, level), *frame([(40, 40, 9), (3, 12, 9), (2, 12, 9)], 20, lits=alpha, seed=level, level=level, lit_mode=mode)))
            # many blocks with similar statistics: 4-stream literals, treeless literals and repeat FSE modes in later blocks
            seqs, pos = [(200, 200, 20)], 220
            for _ in range(6000):
                ll, ml = rng.randint(1, 60), rng.randint(3, 40)
                seqs.append((ll, rng.randint(1, min(pos + ll, 30000)) if rng.random() < 0.7 else rng.choice((8, 16, 24)), ml))
                pos += ll + ml
            out.append(("lit_%s_multi_l%d" % (lname, level), *frame(seqs, 30, lits=alpha, seed=level + 7, level=level, lit_mode=mode, single_block=False)))
        # all sequences alike, the offsets rotating through four raw values of one offset code that never repeat a recent one:
        # RLE FSE modes for LL, OF and ML
        out.append(("fse_rle_l%d" % level, *frame([(5, (5, 6, 7, 9)[i % 4], 4) for i in range(300)], 3, lits=SKEW, seed=level, level=level)))
    return out


FAMILIES = {
    "short_offsets": short_offsets,
    "match_lengths": match_lengths,
    "literal_lengths": literal_lengths,
    "seq_counts": seq_counts,
    "block_sizes": block_sizes,
    "far_offsets": far_offsets,
    "literal_modes": literal_modes,
}

_F = framesuite.Families(FAMILIES)
family, all_frames, valid_frames = _F.family, _F.all_frames, _F.valid_frames


def window_size(z):
    d = oracle.FrameDecoder()
    d.set_max_window_size(1 << 31)
    st, _, _, _ = d.init(z)
    assert st == 0
    return d.window_size()


def coverage(frames):
    """walk each frame with the CPU harness (emu.EmuBatch): the (lit_type, nstreams) pairs and per-field FSE modes seen, the extremes
    of nseq, ML, LL, offset and block output, and how often an offset equals its frame's window size. The repeat-offset forms
    (LL == 0 or not, offset value 1..3) come from the oracle's sequences: the harness resolves them in place."""
    import emu
    cov = {"lit": set(), "fse": {"LL": set(), "OF": set(), "ML": set()}, "rep": set(), "nseq": [1 << 30, 0], "ml": [1 << 30, 0],
           "ll": [1 << 30, 0], "offset": [1 << 30, 0], "block_out_max": 0, "offset_eq_window": 0}
    for z in frames:
        e = emu.EmuBatch(z, max_window=1 << 31)
        assert e.parse_status == 0 and e.nframes == 1
        W = window_size(z)
        for b in range(e.nblocks):
            info = e.block(b)
            if info["btype"] != 2:
                continue
            cov["lit"].add((info["lit_type"], info["nstreams"]))
            n = info["nseq"]
            cov["nseq"] = [min(cov["nseq"][0], n), max(cov["nseq"][1], n)]
            if n:
                m = info["seq_modes"]
                for k, sh in (("LL", 6), ("OF", 4), ("ML", 2)):
                    cov["fse"][k].add((m >> sh) & 3)
            h = e.block_hist(b)
            end = 0
            for of, ml, mdst, lit_start in e.block_sequences(b, n):
                tag, k = of >> 30, of & 0x3FFFFFFF
                actual = of if tag == 0 else h[tag - 1] - k
                for key, v in (("ml", ml), ("ll", mdst - end), ("offset", actual)):
                    cov[key] = [min(cov[key][0], v), max(cov[key][1], v)]
                cov["offset_eq_window"] += actual == W
                end = mdst + ml
            cov["block_out_max"] = max(cov["block_out_max"], info["regen_size"] + sum(s[1] for s in e.block_sequences(b, n)))
        d = oracle.FrameDecoder()
        d.set_max_window_size(1 << 31)
        st, pos, _, _ = d.init(z)
        while st == 0 and not d.is_finished():
            st, used, fin = d.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
            pos += used
            if d.last_block_type() == 2:
                cov["rep"] |= {(ll == 0, of) for ll, _, of, _ in d.last_sequences() if of <= 3}
            if fin:
                break
        assert st == 0
    return cov
