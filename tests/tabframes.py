"""Frames built from chosen table descriptions (test helper, no tests): a block writer in Python, written from RFC 8878, that takes
Huffman weights and FSE normalised counts from the caller, so that zg_k_tables, zg_fse_build_wave and zg_k_fparse see descriptions
no encoder emits. Callers give literal bytes, (ll, offset_value, ml) sequences and the tables; the plaintext is seqframes.lz77 of
what they gave (the reference).

Every valid frame is checked before it is returned: the oracle decodes it to that plaintext, the oracle's Huffman and FSE tables
equal the ones built here entry for entry, and libzstd's decompressor gives the same bytes (except the frames of LIBZSTD_DIFFERS).
Invalid frames come back with plaintext None; STATUS[name] holds the oracle's answer for them. META[name] holds what the Python
side knows of a frame (coverage() reads it)."""
import random

import blockcheck
import framesuite
import oracle
import seqframes

MAGIC = (0xFD2FB528).to_bytes(4, "little")
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_BASE = [sum(1 << b for b in LL_BITS[:i]) for i in range(36)]
ML_BASE = [3 + sum(1 << b for b in ML_BITS[:i]) for i in range(53)]
# RFC 8878 3.1.1.3.2.2: the predefined distributions
LL_DEFAULT = (6, [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1])
OF_DEFAULT = (5, [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1])
ML_DEFAULT = (6, [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                  1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1])
FIELDS = ("LL", "OF", "ML")
DEFAULTS = {"LL": LL_DEFAULT, "OF": OF_DEFAULT, "ML": ML_DEFAULT}
MAX_LOG = {"LL": 9, "OF": 8, "ML": 9}
MAX_SYM = {"LL": 35, "OF": 31, "ML": 52}

# valid frames libzstd's decompressor does not return the plaintext for, each with its reason; checked against the frames in
# all_frames(): only frames the oracle accepts, and at most a tenth of the valid ones
LIBZSTD_DIFFERS = {
    "hws_256_weights_1s": "256 weights: the implied last symbol would be 256, libzstd rejects the table",
    "hws_256_weights_4s": "256 weights, as above, in four streams",
}

META = {}
STATUS = {}


# ---- bit writers ------------------------------------------------------------------------------------------------------------

class FwdBits:
    """forward writer (descriptions): the first value lands in the lowest bits of the first byte"""

    def __init__(self):
        self.acc = self.n = 0

    def add(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == value == 0, (value, nbits)
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


class RevBits:
    """reversed writer (streams): values are added in the order the decoder reads them; the closing 1-bit goes above the first"""

    def __init__(self):
        self.acc, self.n = 1, 0

    def add(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == value == 0, (value, nbits)
        self.acc = (self.acc << nbits) | value
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 8) // 8, "little")


# ---- FSE --------------------------------------------------------------------------------------------------------------------

def fse_desc(al, counts, forms=None):
    """normalised counts -> description bytes (RFC 4.1.1). forms, if given, collects "short" / "long" per value written"""
    w = FwdBits()
    w.add(al - 5, 4)
    remaining, i = 1 << al, 0
    while remaining > 0:
        assert i < len(counts), "counts do not fill the table"
        c = counts[i]
        value = c + 1
        mx = remaining + 1                               # values 0 .. remaining + 1
        bits = mx.bit_length()
        low = (1 << bits) - 1 - mx                       # this many values take one bit less
        if value < low:
            w.add(value, bits - 1)
            short = True
        elif value < (1 << (bits - 1)):
            w.add(value, bits)
            short = False
        else:
            w.add(value + low, bits)
            short = False
        if forms is not None:
            forms.append("short" if short else "long")
        remaining -= abs(c) if c else 0
        i += 1
        if c == 0:
            run = 0
            while i + run < len(counts) and counts[i + run] == 0:
                run += 1
            i += run
            while run >= 3:
                w.add(3, 2)
                run -= 3
            w.add(run, 2)
    assert remaining == 0 and i == len(counts), (remaining, i, len(counts))
    return w.bytes()


def fse_table(al, counts):
    """counts -> decode table [(base_line, num_bits, symbol)] (RFC 4.1.1: -1 cells from the top, the spread, the numbering)"""
    size = 1 << al
    sym = [None] * size
    high = size
    for s, c in enumerate(counts):
        if c == -1:
            high -= 1
            sym[high] = s
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos >= high:
                pos = (pos + step) & (size - 1)
    assert pos == 0 and None not in sym
    nxt = [abs(c) for c in counts]
    tab = []
    for p in range(size):
        s = sym[p]
        if p >= high:
            tab.append((0, al, s))
            continue
        x = nxt[s]
        nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        tab.append(((x << nb) - size, nb, s))
    return tab


def fse_states(tab, codes, last=None):
    """the encoder: the states a decoder passes through while it yields codes. Walked backwards: the last state is any state of
    the last code (`last`, or the first one with num_bits > 0 if there is one), and each earlier one is the one state of its
    symbol whose [base_line, base_line + 2^nb) holds the next state"""
    by_sym = {}
    for i, (_, nb, s) in enumerate(tab):
        by_sym.setdefault(s, []).append(i)
    if last is None:
        cands = by_sym[codes[-1]]
        last = next((i for i in cands if tab[i][1] > 0), cands[0])
    assert tab[last][2] == codes[-1]
    states = [last]
    for c in reversed(codes[:-1]):
        nxt = states[-1]
        hit = [i for i in by_sym[c] if tab[i][0] <= nxt < tab[i][0] + (1 << tab[i][1])]
        assert len(hit) == 1, (c, nxt, hit)
        states.append(hit[0])
    return states[::-1]


def fse_walk(tab, usable, n, rng, visited):
    """n codes chosen by walking the decode table forwards through states of usable symbols only, so that the sequences visit every
    state a block of n allows: an unvisited successor first, else the shortest way to the nearest unvisited state. Returns (codes,
    states, the set of states a walk from its first state can be in: a state outside it could only be a first state itself) or
    None if no walk of usable states exists.
    fse_states(tab, codes, states[-1]) finds the same states again (they are unique)"""
    size = len(tab)
    succ = {i: [j for j in range(tab[i][0], tab[i][0] + (1 << tab[i][1])) if tab[j][2] in usable] for i in range(size) if tab[i][2] in usable}
    live = set(succ)
    while True:                                          # drop states from which every way ends at an unusable symbol
        dead = {i for i in live if not any(j in live for j in succ[i])}
        if not dead:
            break
        live -= dead
    if not live:
        return None
    succ = {i: [j for j in succ[i] if j in live] for i in live}
    def reach(i):
        seen, queue = {i}, [i]
        while queue:
            queue = [j for q in queue for j in succ[q] if j not in seen and not seen.add(j)]
        return seen

    # the start: of the 16 widest states the one from which most can be reached (a narrow state may lead only to itself)
    cur = max(sorted(live, key=lambda i: (-tab[i][1], i))[:16], key=lambda i: (len(reach(i)), -i))
    states = [cur]
    visited.add(cur)
    while len(states) < n:
        fresh = [j for j in succ[cur] if j not in visited]
        if fresh and len(live) <= 128:                   # (small tables have corners without a way back: those are left for last)
            todo = live - visited
            fresh = [j for j in fresh if todo <= reach(j)] or [j for j in succ[cur] if todo <= reach(j)] or fresh
        if fresh:
            path = [rng.choice(fresh)]
        else:                                            # breadth first to the nearest unvisited state, if there is one left
            prev, queue, goal = {cur: None}, [cur], None
            while queue and goal is None:
                nq = []
                for i in queue:
                    for j in succ[i]:
                        if j not in prev:
                            prev[j] = i
                            nq.append(j)
                            if j not in visited and goal is None and (len(live) > 128 or live - visited <= reach(j) or not any(
                                    live - visited <= reach(x) for x in live - visited)):
                                goal = j
                queue = nq
            if goal is None:
                path = [rng.choice(succ[cur])]
            else:
                path = [goal]
                while prev[path[-1]] != cur:
                    path.append(prev[path[-1]])
                path.reverse()
        for j in path[:n - len(states)]:
            states.append(j)
            visited.add(j)
        cur = states[-1]
    return [tab[i][2] for i in states], states, reach(states[0])


# ---- Huffman ----------------------------------------------------------------------------------------------------------------

def huf_table(weights):
    """weights (of symbols 0 .. nw-1; the last symbol nw is implied) -> (max_bits, [(symbol, num_bits)], runs) as RFC 4.2.1: the
    table holds the codes of weight 1 first, each weight in symbol order. A 256th weight implies symbol 256, which a byte cannot
    hold: the oracle keeps its low 8 bits, and so does this model."""
    total = sum(1 << (w - 1) for w in weights if w)
    mb = total.bit_length()
    left = (1 << mb) - total
    assert left and left & (left - 1) == 0, "leftover is not a power of two"
    allw = list(weights) + [left.bit_length()]
    ents, runs = [], []
    for w in range(1, mb + 1):
        for s, x in enumerate(allw):
            if x == w:
                ents += [(s & 255, mb + 1 - w)] * (1 << (w - 1))
                runs.append(1 << (w - 1))
    assert len(ents) == 1 << mb
    return mb, ents, runs


def huf_codes(weights):
    """symbol -> (code, length): the code is the index of the symbol's first table entry, cut to its length"""
    mb, ents, _ = huf_table(weights)
    codes = {}
    for i, (s, nb) in enumerate(ents):
        if s not in codes:
            codes[s] = (i >> (mb - nb), nb)
    return codes


def _huf_stream(codes, data):
    """one stream: the decoder starts at the closing bit and meets the first symbol's code first"""
    w = RevBits()
    for b in data:
        w.add(*codes[b])
    return w.bytes()


def huf_encode(codes, data, nstreams):
    if nstreams == 1:
        return _huf_stream(codes, data)
    q = (len(data) + 3) // 4
    parts = [_huf_stream(codes, data[i * q:(i + 1) * q if i < 3 else len(data)]) for i in range(4)]
    assert len(data) > 3 * q - 1 and all(len(p) < 65536 for p in parts)
    return b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)


def weights_direct(weights):
    assert 1 <= len(weights) <= 128
    nib = list(weights) + [0]
    return bytes([127 + len(weights)]) + bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(weights), 2))


def weights_counts(weights, al):
    """normalised counts of a weight list for an FSE table of accuracy log al: every weight present gets at least 1, the rest goes
    by frequency, the most frequent weight takes what is left over or gives what is missing"""
    size = 1 << al
    hist = [0] * (max(weights) + 1)
    for w in weights:
        hist[w] += 1
    cnt = [max(1, h * size // len(weights)) if h else 0 for h in hist]
    top = max(range(len(hist)), key=lambda s: hist[s])
    cnt[top] += size - sum(cnt)
    assert cnt[top] >= 1 and sum(cnt) == size
    return cnt


def weights_fse(weights, al, counts=None):
    """FSE-compressed weights: header byte (compressed size), the table description, the stream of two interleaved states. The
    decoder stops when an update reads past the stream's start, so the two last states must need at least one bit"""
    counts = counts or weights_counts(weights, al)
    tab = fse_table(al, counts)
    a, b = fse_states(tab, weights[0::2]), fse_states(tab, weights[1::2])
    assert tab[a[-1]][1] > 0 and tab[b[-1]][1] > 0, "a last state of 0 bits never ends the stream"
    w = RevBits()
    w.add(a[0], al)
    w.add(b[0], al)
    for i in range(1, len(a) + len(b) - 1):              # weight i+1's state is reached from weight i-1's
        st = a if i % 2 == 1 else b
        k = (i + 1) // 2 if i % 2 == 1 else i // 2
        if k < len(st):
            prev = st[k - 1]
            w.add(st[k] - tab[prev][0], tab[prev][1])
    body = fse_desc(al, counts) + w.bytes()
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def kraft_weights(nsym, max_bits, rng):
    """nsym code lengths of a complete prefix code no longer than max_bits, as weights in random order"""
    lens = [1, 1]
    while len(lens) < nsym:
        splittable = [i for i, x in enumerate(lens) if x < max_bits]
        i = rng.choice(splittable)
        lens[i] += 1
        lens.append(lens[i])
    mb = max(lens)
    ws = [mb + 1 - x for x in lens]
    rng.shuffle(ws)
    return ws


# ---- blocks and frames ------------------------------------------------------------------------------------------------------

def lit_header(ltype, regen, comp=None, nstreams=1, sf=None):
    """literals section header. sf: the size format (None: the smallest that fits)"""
    if ltype < 2:
        if sf is None:
            sf = 0 if regen < 32 else 1 if regen < 4096 else 3
        if sf in (0, 2):
            assert regen < 32
            return bytes([ltype | (sf << 2) | (regen << 3)])
        if sf == 1:
            assert regen < 4096
            return (ltype | (1 << 2) | (regen << 4)).to_bytes(2, "little")
        return (ltype | (3 << 2) | (regen << 4)).to_bytes(3, "little")
    if sf is None:
        big = max(regen, comp)
        sf = (0 if nstreams == 1 else 1) if big < 1024 else 2 if big < 16384 else 3
    assert (sf == 0) == (nstreams == 1), (sf, nstreams)
    nb = {0: 10, 1: 10, 2: 14, 3: 18}[sf]
    assert regen < (1 << nb) and comp < (1 << nb), (regen, comp, sf)
    return (ltype | (sf << 2) | (regen << 4) | (comp << (4 + nb))).to_bytes({0: 3, 1: 3, 2: 4, 3: 5}[sf], "little")


def nbseq(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([128 + (n >> 8), n & 255])
    return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")


def _code(base, v):
    c = max(i for i, b in enumerate(base) if b <= v)
    return c, v - base[c]


class Block:
    """one compressed block. lits: all literal bytes (those of the sequences, then the trailing ones); seqs: [(ll, offset_value,
    ml)], offset_value as the format has it (1..3 the repeat offsets, else distance + 3).
    lit: ("raw"|"rle", sf) | ("huf", weights, "direct"|("fse", al[, counts]), nstreams, sf) | ("treeless", nstreams, sf) |
         ("hufbytes", description, nstreams): a description as it is, the streams a single byte (invalid frames) |
         ("hufstreams", weights or None (treeless), form, [stream bytes, ...], sf): the one or four streams as the caller wrote them;
         the description, the jump table and the header (its regen is len(lits)) are added here (tests/hufstreams.py).
    ll / of / ml: ("pre",) | ("rle", code) | ("fse", al, counts) | ("rep",) | ("bytes", description) (invalid frames).
    last: {"LL": state, ...} the last sequence's states (see fse_walk). seq_raw: the whole sequences section as it is."""

    def __init__(self, lits, seqs, lit=("raw", None), ll=("pre",), of=("pre",), ml=("pre",), last=None, seq_raw=None, junk=0):
        self.lits, self.seqs, self.lit, self.modes, self.last, self.seq_raw, self.junk = lits, seqs, lit, {"LL": ll, "OF": of, "ML": ml}, last or {}, seq_raw, junk


class _Frame:
    def __init__(self):
        self.huf = None                                  # the weights in force
        self.fse = {}                                    # field -> ("tab", al, table) | ("rle", code)
        self.hist = [1, 4, 8]
        self.expect = []                                 # per compressed block: (huf or None, {field: expectation} or None)
        self.meta = {"huf": [], "fse": [], "walks": [], "lit_off": [], "seq_off": [], "seq_desc": [], "seq_stream": []}


def _literals(fr, blk):
    kind = blk.lit[0]
    n = len(blk.lits)
    if kind == "raw":
        return lit_header(0, n, sf=blk.lit[1]) + blk.lits, None
    if kind == "rle":
        assert n and blk.lits == blk.lits[:1] * n
        return lit_header(1, n, sf=blk.lit[1]) + blk.lits[:1], None
    if kind == "hufbytes":
        body = blk.lit[1] + (b"\x01" if blk.lit[2] == 1 else b"\x01\x00" * 3 + b"\x01" * 4)
        return lit_header(2, n, len(body), blk.lit[2]) + body, None
    if kind == "hufstreams":
        _, weights, form, streams, sf = blk.lit
        assert len(streams) in (1, 4) and all(len(p) < 65536 for p in streams)
        desc = b""
        if weights is not None:
            desc = weights_direct(weights) if form == "direct" else weights_fse(weights, *form[1:])
            fr.huf = list(weights)
        assert fr.huf is not None
        body = desc + (b"".join(len(p).to_bytes(2, "little") for p in streams[:3]) if len(streams) == 4 else b"") + b"".join(streams)
        return lit_header(2 if weights is not None else 3, n, len(body), len(streams), sf) + body, huf_table(fr.huf)[:2]
    if kind == "huf":
        _, weights, form, nstreams, sf = blk.lit
        desc = weights_direct(weights) if form == "direct" else weights_fse(weights, *form[1:])
        fr.huf = list(weights)
        mb, _, runs = huf_table(weights)
        fr.meta["huf"].append({"nw": len(weights), "max_bits": mb, "run": max(runs), "desc": len(desc), "fse": form != "direct",
                               "al": None if form == "direct" else form[1], "nstreams": nstreams, "comp": None,
                               "whole_wave_runs": sum(r >= 64 for r in runs)})
        ltype = 2
    else:
        _, nstreams, sf = blk.lit
        desc, ltype = b"", 3
        assert fr.huf is not None
    body = desc + huf_encode(huf_codes(fr.huf), blk.lits, nstreams)
    if ltype == 2:
        fr.meta["huf"][-1]["comp"] = len(body)
    return lit_header(ltype, n, len(body), nstreams, sf) + body, huf_table(fr.huf)[:2]


def _sequences(fr, blk):
    if blk.seq_raw is not None:
        return blk.seq_raw, None
    n = len(blk.seqs)
    if n == 0:
        return b"\x00", None
    modes, descs = 0, b""
    for k, f in enumerate(FIELDS):
        m = blk.modes[f]
        if m[0] == "pre":
            fr.fse[f] = ("tab", DEFAULTS[f][0], fse_table(*DEFAULTS[f]))
        elif m[0] == "rle":
            modes |= 1 << (6 - 2 * k)
            descs += bytes([m[1]])
            fr.fse[f] = ("rle", m[1])
        elif m[0] == "fse":
            modes |= 2 << (6 - 2 * k)
            forms = []
            descs += fse_desc(m[1], m[2], forms)
            tab = fse_table(m[1], m[2])
            fr.fse[f] = ("tab", m[1], tab)
            fr.meta["fse"].append({"field": f, "al": m[1], "high": len(m[2]) - 1, "zero_bit": any(e[1] == 0 for e in tab),
                                   "all_low": all(c <= 0 for c in m[2]), "single": max(m[2]) == 1 << m[1], "forms": set(forms),
                                   "last_form": forms[-1], "counts": list(m[2])})
        elif m[0] == "bytes":
            modes |= 2 << (6 - 2 * k)
            descs += m[1]
            fr.fse[f] = None
        else:
            modes |= 3 << (6 - 2 * k)
    head = nbseq(n) + bytes([modes]) + descs
    if any(fr.fse.get(f) is None for f in FIELDS):       # an invalid or missing table: nothing can be encoded behind it
        return head + b"\x01" + bytes(blk.junk), None
    codes = {"LL": [], "OF": [], "ML": []}
    extra = []
    for ll, ov, ml in blk.seqs:
        lc, lx = _code(LL_BASE, ll)
        mc, mx = _code(ML_BASE, ml)
        oc = ov.bit_length() - 1
        codes["LL"].append(lc)
        codes["OF"].append(oc)
        codes["ML"].append(mc)
        extra.append(((ov - (1 << oc), oc), (mx, ML_BITS[mc]), (lx, LL_BITS[lc])))
    states = {}
    for f in FIELDS:
        if fr.fse[f][0] == "rle":
            assert set(codes[f]) == {fr.fse[f][1]}, (f, codes[f][:4], fr.fse[f])
            states[f] = None
        else:
            states[f] = fse_states(fr.fse[f][2], codes[f], blk.last.get(f))
    w = RevBits()
    for f in FIELDS:                                     # initial states: LL, OF, ML
        if states[f]:
            w.add(states[f][0], fr.fse[f][1])
    for i in range(n):
        for v, nb in extra[i]:                           # offset bits, match length bits, literal length bits
            w.add(v, nb)
        if i + 1 < n:
            for f in ("LL", "ML", "OF"):                 # state updates: LL, ML, OF
                if states[f]:
                    base, nb, _ = fr.fse[f][2][states[f][i]]
                    w.add(states[f][i + 1] - base, nb)
    expect = {f: (fr.fse[f] if fr.fse[f][0] == "rle" else (fr.fse[f][1], list(fr.fse[f][2]))) for f in FIELDS}
    fr.meta["seq_desc"].append(len(descs))
    fr.meta["seq_stream"].append(len(w.bytes()))
    return head + w.bytes(), expect


def _resolve(fr, ll, ov):
    """RFC 3.1.1.5: offset_value -> distance, updating the repeat offsets"""
    h = fr.hist
    if ov > 3:
        d = ov - 3
        fr.hist = [d, h[0], h[1]]
        return d
    k = ov - 1 + (ll == 0)
    d = h[0] - 1 if k == 3 else h[k]
    if k:
        fr.hist = [d] + [x for i, x in enumerate(h) if i != min(k, 2)][:2]
    return d


def _bh(last, btype, size):
    return (last | (btype << 1) | (size << 3)).to_bytes(3, "little")


def build(name, blocks, window_log=17, valid=True, differs=None):
    """blocks: Block | ("raw", bytes) | ("rle", byte, n) | ("bytes", block content as it is: a compressed block, invalid frames) |
    ("hdr", block type, size field, the bytes behind the header: a block header as it is, invalid frames).
    Returns (name, zst, plaintext or None). A valid frame is checked against the oracle (bytes and tables) and libzstd (differs: the
    caller's own list of frames libzstd does not return the plaintext for, in place of LIBZSTD_DIFFERS)."""
    fr = _Frame()
    z = MAGIC + bytes([0x04, (window_log - 10) << 3])    # no single segment, no content size, a checksum
    flat_seqs, flat_lits, pending = [], bytearray(), 0
    for i, b in enumerate(blocks):
        last = int(i == len(blocks) - 1)
        if isinstance(b, tuple) and b[0] == "raw":
            z += _bh(last, 0, len(b[1])) + b[1]
            flat_lits += b[1]
            pending += len(b[1])
        elif isinstance(b, tuple) and b[0] == "rle":
            z += _bh(last, 1, b[2]) + bytes([b[1]])
            flat_lits += bytes([b[1]]) * b[2]
            pending += b[2]
        elif isinstance(b, tuple) and b[0] == "hdr":
            z += _bh(last, b[1], b[2]) + b[3]
        elif isinstance(b, tuple):
            z += _bh(last, 2, len(b[1])) + b[1]
        else:
            lit, hexp = _literals(fr, b)
            seq, fexp = _sequences(fr, b)
            fr.expect.append((hexp, fexp))
            fr.meta["lit_off"].append(len(z) + 3)        # where the two sections start in the frame
            fr.meta["seq_off"].append(len(z) + 3 + len(lit))
            z += _bh(last, 2, len(lit) + len(seq)) + lit + seq
            assert len(lit) + len(seq) <= 131072
            flat_lits += b.lits
            if valid:
                for j, (ll, ov, ml) in enumerate(b.seqs):
                    flat_seqs.append((ll + (pending if j == 0 else 0), _resolve(fr, ll, ov), ml))
                    if j == 0:
                        pending = 0
                pending += len(b.lits) - sum(s[0] for s in b.seqs)
    META[name] = fr.meta
    if not valid:
        z += bytes(4)
        d = oracle.FrameDecoder()
        st, _ = d.decode_all(z, 1 << 20)
        assert st != 0, (name, "the oracle accepts a frame meant to be invalid")
        STATUS[name] = st
        return name, z, None
    plain = seqframes.lz77(flat_seqs, bytes(flat_lits))
    z += (oracle.lib().zor_xxh64(plain, len(plain), 0) & 0xFFFFFFFF).to_bytes(4, "little")
    _check_valid(name, z, plain, fr, differs)
    return name, z, plain


_LIBZSTD_MISSING = []


def _check_valid(name, z, plain, fr, differs=None):
    differs = LIBZSTD_DIFFERS if differs is None else differs
    d = oracle.FrameDecoder()
    st, out = d.decode_all(z, len(plain) + 64)
    assert st == 0 and out == plain, (name, st, len(out), len(plain))
    comp = [r for r in blockcheck.oracle_blocks(z) if r["type"] == 2]
    assert len(comp) == len(fr.expect), name
    for j, (rec, (hexp, fexp)) in enumerate(zip(comp, fr.expect)):
        if hexp:
            oents, omb = rec["huf"]
            assert omb == hexp[0] and oents == hexp[1], (name, j, "Huffman table")
        if fexp:
            for k, f in enumerate(FIELDS):
                oents, olog, orle = rec["fse"][k]
                if fexp[f][0] == "rle":
                    assert orle == fexp[f][1], (name, j, f)
                else:
                    assert orle < 0 and olog == fexp[f][0] and oents == fexp[f][1], (name, j, f, "FSE table")
    if _LIBZSTD_MISSING:
        return
    try:
        import zgdata
        zgdata.libzstd()
    except (RuntimeError, OSError) as e:
        _LIBZSTD_MISSING.append(str(e))
        print("tabframes: libzstd is absent, its cross-check is skipped (%s)" % e)
        return
    try:
        got = zgdata.zstd_decompress(z, len(plain))
    except RuntimeError:
        got = None
    if name in differs:
        assert got != plain, (name, "libzstd agrees: take it off LIBZSTD_DIFFERS")
    else:
        assert got == plain, (name, "libzstd does not return the plaintext")


# ---- helpers of the families ------------------------------------------------------------------------------------------------

def _lits_covering(symbols, n, rng):
    """n literal bytes (at least one of every symbol, shuffled)"""
    symbols = list(symbols)
    assert n >= len(symbols)
    out = symbols + [rng.choice(symbols) for _ in range(n - len(symbols))]
    rng.shuffle(out)
    return bytes(out)


def _spread_weights(nw, nsym, max_bits, rng):
    """nw weights with nsym - 1 nonzero ones spread over 0 .. nw-1 with zero-weight gaps (symbol nw - 1 always present, so that the
    count stays nw); the implied last symbol is nw. Returns (weights, symbols present)"""
    nz = kraft_weights(nsym, max_bits, rng)
    nsym = len(nz)
    last = nz.pop()                                      # the implied symbol's weight: the others must leave exactly that
    if nw < nsym - 1:
        raise ValueError
    where = sorted(rng.sample(range(nw - 1), nsym - 2)) + [nw - 1] if nsym > 1 and nw > 1 else [0]
    weights = [0] * nw
    for p, w in zip(where, nz):
        weights[p] = w
    mb, ents, _ = huf_table(weights)
    assert ents and (1 << mb) - sum(1 << (w - 1) for w in weights if w) == 1 << (last - 1)
    return weights, where + [nw]


def _simple_seqs(nlit, rng, k=6):
    """k short sequences over nlit literals: plain offsets, predefined tables"""
    seqs, used, pos = [], 0, 0
    for _ in range(k):
        ll = rng.randint(1, max(1, nlit // (k + 1)))
        pos += ll
        seqs.append((ll, rng.randint(1, pos) + 3, rng.randint(3, 12)))
        used += ll
        pos += seqs[-1][2]
    return seqs


def _huf_frames(name, weights, syms, rng, n=None, form=None, pre=()):
    """a 1-stream frame and a 4-stream frame of literals that cover syms under the table of weights"""
    out = []
    form = form or ("direct" if len(weights) <= 128 else ("fse", 6))
    usable = [s for s in syms if s < 256]
    n = n or max(len(usable) + 40, 80)
    for ns in (1, 4):
        lits = _lits_covering(usable, n, rng)
        blk = Block(lits, _simple_seqs(n, rng), lit=("huf", weights, form, ns, None))
        out.append(build("%s_%ds" % (name, ns), list(pre) + [blk]))
    return out


# ---- the families: each returns [(name, zst, plaintext or None)] ------------------------------------------------------------

NW_LIST = (1, 2, 63, 64, 65, 95, 96, 127, 128, 129, 191, 192, 193, 254, 255)


def huf_alphabets():
    """zg_k_tables' wave builder and zg_k_huf: weight counts at the k = lane + 64*k slot edges and at the direct form's limit, the
    implied last symbol anywhere, all-equal lengths, tables of 2 / 4 / 8 entries (tail copy, single 16-byte store), max_bits 11
    with a 1024-entry run and several whole-wave runs in one ballot, equal lengths at symbols 64 / 128 / 192 apart"""
    rng = random.Random(101)
    out = []
    for nw in NW_LIST:
        nsym = max(2, min(nw + 1, 2 + nw // 3))
        if nw <= 2:
            weights, syms = ([1], [0, 1]) if nw == 1 else ([0, 1], [1, 2])
        else:
            weights, syms = _spread_weights(nw, nsym, 9, rng)
        out += _huf_frames("huf_nw%d" % nw, weights, syms, rng)
    # (the weights' FSE table gives weight 0 one cell nobody uses: were weight 1 alone, every state would take 0 bits and the stream never end)
    out += _huf_frames("huf_255_equal", [1] * 255, range(256), rng, n=600, form=("fse", 6, [1, 63]))
    out += _huf_frames("huf_mb1", [1], [0, 1], rng)
    out += _huf_frames("huf_mb2", [0, 2, 0, 1], [1, 3, 4], rng)
    out += _huf_frames("huf_mb3", [3, 0, 1, 0, 0, 2], [0, 2, 5, 6], rng)
    # max_bits 11: symbol 7 has weight 11 (a run of 1024); weights 9, 8, 8, 7, 7 in slot k = 0 and 7, 7 in slot k = 1: whole-wave runs
    # that share a ballot; the rest is runs shorter than 64 (weights 1 .. 6). 2047 in all: the implied symbol 200 has weight 1
    w = [0] * 200
    for x, syms in ((11, (7,)), (9, (9,)), (8, (20, 33)), (7, (41, 50, 70, 90)), (6, (100, 110, 130, 140)), (5, (64, 128, 150, 192)),
                    (4, (0, 63, 127, 191)), (3, (1, 65, 129, 193)), (2, (2, 66, 160, 170)), (1, (3, 67, 131, 195, 197, 198, 199))):
        for sy in syms:
            w[sy] = x
    out += _huf_frames("huf_mb11_runs", w, [sy for sy, x in enumerate(w) if x] + [200], rng)
    # equal lengths at symbols that differ by 64, 128 and 192: the same lane in another slot k, so the rank crosses k.
    # 8 * 4 + 8 * 1 + 4 * 2 = 48: the implied symbol 255 takes the other 16 (weight 5), max_bits 6
    w = [0] * 255
    for sy in (3, 67, 131, 195, 40, 104, 168, 232):
        w[sy] = 3
    for sy in (10, 74, 138, 202, 63, 127, 191, 254):
        w[sy] = 1
    for sy in (20, 84, 148, 212):
        w[sy] = 2
    out += _huf_frames("huf_cross_k", w, [sy for sy, x in enumerate(w) if x] + [255], rng)
    return out


def huf_weight_streams():
    """zg_huf_read_weights: FSE-compressed weights at accuracy logs 5 and 6, streams that end on the first and on the second
    decoder (even and odd counts), 256 weights (the serial branch of zg_k_tables), descriptions of 127 and 128 bytes, the
    literals section at each of the four byte alignments, a compressed size under 136 bytes (the staged header clamped), and a
    treeless block right behind each table, one more behind a raw-literals block"""
    rng = random.Random(202)
    out = []

    def with_treeless(name, weights, syms, form, pre=(), n=None):
        usable = [s for s in syms if s < 256]
        n = n or max(len(usable) + 30, 60)
        for ns in (1, 4):
            blocks = list(pre)
            blocks.append(Block(_lits_covering(usable, n, rng), _simple_seqs(n, rng), lit=("huf", weights, form, ns, None)))
            blocks.append(Block(_lits_covering(usable, n, rng), _simple_seqs(n, rng), lit=("treeless", 5 - ns, None)))
            blocks.append(Block(rng.randbytes(40), _simple_seqs(40, rng, 3)))
            blocks.append(Block(_lits_covering(usable, n, rng), _simple_seqs(n, rng), lit=("treeless", ns, None)))
            out.append(build("%s_%ds" % (name, ns), blocks))

    for al in (5, 6):
        for nw in (40, 41, 130, 131):                    # both parities: the stream ends on the first / the second decoder
            weights, syms = _spread_weights(nw, 2 + nw // 2, 7, rng)
            with_treeless("hws_al%d_nw%d" % (al, nw), weights, syms, ("fse", al))
    # 256 weights: 255 of weight 1 and one more of weight 1 make 256 -> the implied symbol takes 256 (weight 9), max_bits 9
    # (the oracle accepts them, so they are built; it keeps the low 8 bits of the implied symbol 256: see huf_table)
    with_treeless("hws_256_weights", [1] * 256, range(256), ("fse", 6, [1, 63]), n=300)
    for want in (127, 128):
        weights, syms, form = _desc_sized(want)
        with_treeless("hws_desc%d" % want, weights, syms, form, n=500)
    for pad in range(4):                                 # a raw block of 0 .. 3 bytes in front: the section at each alignment
        weights, syms = _spread_weights(150, 40, 8, rng)
        with_treeless("hws_align%d" % pad, weights, syms, ("fse", 6), pre=[("raw", rng.randbytes(pad))])
    weights, syms = _spread_weights(12, 6, 5, rng)       # compressed size < 136
    with_treeless("hws_small_section", weights, syms, ("fse", 5), n=40)
    return out


def _desc_sized(want):
    """weights whose FSE-compressed description has exactly `want` bytes (header byte included): 255 weights of a fixed draw, and
    counts that start at the weights' frequencies (the shortest stream) and hand cells of the most frequent weight to the others,
    one at a time, which makes the stream longer step by step until the size is met. Returns (weights, symbols, form)"""
    for draw in range(64):                               # (another draw only if a walk steps over the size or ends on a 0-bit state)
        r = random.Random(1000 * want + draw)
        weights, syms = _spread_weights(255, 230, 10, r)
        counts = weights_counts(weights, 6)
        top = max(range(len(counts)), key=lambda x: counts[x])
        others = [x for x in range(len(counts)) if counts[x] and x != top]
        k = 0
        while counts[top] > 1:
            try:
                size = len(weights_fse(weights, 6, counts))
            except AssertionError:                       # a last state of 0 bits, or 128 bytes and more
                size = None
            if size == want:
                return weights, syms, ("fse", 6, list(counts))
            if size is not None and size > want:
                break
            counts[top] -= 1
            counts[others[k % len(others)]] += 1
            k += 1
    raise AssertionError("no weights description of %d bytes" % want)


def _usable(field, pos_budget):
    if field == "LL":
        return {c for c in range(36) if LL_BASE[c] <= 20}
    if field == "ML":
        return {c for c in range(53) if ML_BASE[c] <= 40}
    return {c for c in range(32) if 2 <= c <= pos_budget}


def _fse_frame(name, specs, rng, nseq=48):
    """a frame of a 2 KiB raw block (history for the offsets) and one block whose sequences walk the given tables. specs: field ->
    (al, counts) or ("rle", code) or None (predefined)"""
    hist = rng.randbytes(2048)
    nseq = max(nseq, *(3 << sp[0] for sp in specs.values() if sp and sp[0] != "rle")) if nseq >= 48 else nseq
    codes, last, walks = {}, {}, []
    modes = {}
    for f in FIELDS:
        sp = specs.get(f)
        if sp and sp[0] == "rle":
            codes[f] = [sp[1]] * nseq
            modes[f] = sp
            continue
        al, counts = sp or DEFAULTS[f]
        modes[f] = ("fse", al, counts) if sp else ("pre",)
        tab = fse_table(al, counts)
        visited = set()
        got = fse_walk(tab, _usable(f, 10), nseq, rng, visited)
        assert got, (name, f, "no usable state")
        codes[f], st, live = got
        last[f] = st[-1]
        if sp:
            walks.append({"field": f, "size": len(tab), "nseq": nseq, "live": len(live), "visited": len(visited),
                          "symbols": {tab[i][2] for i in live}, "symbols_visited": {tab[i][2] for i in visited}})
    seqs, nlit = [], 0
    for i in range(nseq):
        lc, oc, mc = codes["LL"][i], codes["OF"][i], codes["ML"][i]
        ll = LL_BASE[lc] + rng.randrange(1 << LL_BITS[lc])
        ml = ML_BASE[mc] + rng.randrange(1 << ML_BITS[mc])
        ov = (1 << oc) + rng.randrange(1 << oc)
        ov = max(ov, 4)                                  # codes 0 and 1 are kept out (_usable): repeat offsets stay with seqframes
        if ov - 3 > 2048:
            ov = (1 << oc) + 3
        seqs.append((ll, ov, ml))
        nlit += ll
    blk = Block(rng.randbytes(nlit + 7), seqs, ll=modes["LL"], of=modes["OF"], ml=modes["ML"], last=last)
    r = build(name, [("raw", hist), blk])
    META[name]["walks"] = walks
    return r


def _fill(n, size, rng, lo=1):
    """n positive counts that sum to size"""
    c = [lo] * n
    for _ in range(size - lo * n):
        c[rng.randrange(n)] += 1
    return c


def fse_shapes():
    """zg_k_fparse, zg_fse_build_wave and zg_k_seq: accuracy logs 5 and the maximum, one symbol with the whole table (0-bit states),
    the highest symbols (35 / 31 / 52, OF 29 .. 31) with prob 1 and -1, tables of low-probability cells only, a -1 cell next to
    2^al - 1, probabilities at and around powers of two, zero runs of 0 .. 4 and 6 repeats (the last ending at the highest
    symbol), final counts in the short and the long form"""
    rng = random.Random(303)
    out = []
    for f in FIELDS:
        top, mx = MAX_SYM[f], MAX_LOG[f]
        lowsym = 2 if f == "OF" else 0                   # the lowest symbol a sequence of these frames may use (_usable)
        for al in (5, mx):
            size = 1 << al
            out.append(_fse_frame("fse_%s_al%d_flat" % (f, al), {f: (al, _fill(min(16, size // 2), size, rng))}, rng))
            # one symbol owns the table: every state has 0 bits
            out.append(_fse_frame("fse_%s_al%d_single_low" % (f, al), {f: (al, [0] * lowsym + [size])}, rng, nseq=5))
            # the highest symbol with prob 1 and with prob -1; in front of it a zero run that ends exactly there
            for p in (1, -1):
                counts = _fill(8, size - 1, rng) + [0] * (top - 8) + [p]
                if f == "OF":
                    counts[0], counts[2] = 0, counts[2] + counts[0]
                out.append(_fse_frame("fse_%s_al%d_top%+d" % (f, al, p), {f: (al, counts)}, rng))
            # a -1 cell next to one symbol of 2^al - 1
            counts = [0] * lowsym + [size - 1, -1]
            out.append(_fse_frame("fse_%s_al%d_big_and_low" % (f, al), {f: (al, counts)}, rng, nseq=12))
        # every cell low-probability: 32 symbols of -1 at accuracy log 5
        out.append(_fse_frame("fse_%s_all_low" % f, {f: (5, [-1] * 32)}, rng))
        # powers of two, and one below / above
        al = mx
        size = 1 << al
        pw = [16, 15, 17, 8, 7, 9, 4, 3, 5, 2, 1, 32, 31, 33]
        counts = ([0, 0] if f == "OF" else []) + pw
        counts.append(size - sum(counts))
        out.append(_fse_frame("fse_%s_pow2" % f, {f: (al, counts)}, rng, nseq=120))
        # zero runs: repeat flags of 0, 1, 2, 3+0, 3+1 and 3+3+0 (gaps of 1, 2, 3, 4, 5 and 7 absent symbols), the last ending at
        # the highest symbol. OF has 32 symbols: its gaps are 1, 2, 3, 4, 5 and 7 too, with fewer symbols between them
        counts, gaps = ([0, 0], (1, 3, 4, 5)) if f == "OF" else ([], (1, 2, 3, 4, 5))       # (OF: the gap of 2 is symbols 0 and 1)
        for g in gaps:
            counts += [1] + [0] * g
        counts += [1] * (top + 1 - len(counts) - 8) + [0] * 7 + [1]
        counts[counts.index(1)] += 64 - sum(counts)
        assert len(counts) == top + 1
        out.append(_fse_frame("fse_%s_zero_runs" % f, {f: (6, counts)}, rng))
        # the final count in the short form (1 of 1 remaining: value 2 of 0 .. 2 needs 2 bits; -1 takes the short form) and long
        out.append(_fse_frame("fse_%s_last_short" % f, {f: (5, [0] * lowsym + [20, 11, -1])}, rng))
        out.append(_fse_frame("fse_%s_last_long" % f, {f: (5, [0] * lowsym + [10, 10, 12])}, rng))
    # one symbol with the whole table at the highest symbol: LL 35 is one literal run of 65536 bytes and ML 52 one match of 65539 (these
    # two frames are longer than 64 KiB); OF 31 is an offset past 2^31, which no frame can execute: it is in invalid_tables
    for al in (5, 9):
        blk = Block(rng.randbytes(65536 + 16), [(65536 + al, 5, 4)], ll=("fse", al, [0] * 35 + [1 << al]))
        out.append(build("fse_LL_al%d_single_high" % al, [blk]))
        blk = Block(rng.randbytes(9), [(5, 6, 65539 + al)], ml=("fse", al, [0] * 52 + [1 << al]))
        out.append(build("fse_ML_al%d_single_high" % al, [blk]))
    # OF symbols 29, 30 and 31 in a table whose sequences use only smaller codes
    counts = [0, 0] + _fill(8, 61, rng) + [0] * 19 + [1, -1, 1]
    out.append(_fse_frame("fse_OF_29_30_31", {"OF": (6, counts)}, rng))
    return out


def _three(rng, al=6):
    return {"LL": (al, _fill(12, 1 << al, rng)), "OF": (al - 1, [0, 0] + _fill(8, 1 << (al - 1), rng)), "ML": (al, _fill(14, 1 << al, rng))}


def _mode_block(rng, modes, tabs, nseq=10):
    """a block of nseq sequences under the given per-field modes. tabs: field -> ("tab", al, table) | ("rle", code) in force once the
    modes are applied. Returns the Block"""
    seqs, nlit = [], 0
    for _ in range(nseq):
        tr = []
        for f in FIELDS:
            if tabs[f][0] == "rle":
                tr.append(tabs[f][1])
            else:
                tr.append(rng.choice(sorted({e[2] for e in tabs[f][2]} & _usable(f, 10))))
        lc, oc, mc = tr
        ll = LL_BASE[lc] + (rng.randrange(1 << LL_BITS[lc]) if lc < 30 else 0)
        ml = ML_BASE[mc] + (rng.randrange(1 << ML_BITS[mc]) if mc < 44 else 0)
        ov = max(4, (1 << oc) + (rng.randrange(1 << oc) if oc < 20 else 0))
        if oc < 20 and ov - 3 > 2048:
            ov = (1 << oc) + 3
        seqs.append((ll, ov, ml))
        nlit += ll
    return Block(rng.randbytes(nlit + 3), seqs, ll=modes["LL"], of=modes["OF"], ml=modes["ML"])


def _in_force(spec):
    return ("rle", spec[1]) if spec[0] == "rle" else ("tab", spec[1], fse_table(spec[1], spec[2])) if spec[0] == "fse" else None


def fse_modes():
    """zg_k_fparse and the table lineage of zg_k_tables: all 64 (LL, OF, ML) mode triples in a second block behind compressed
    tables, repeat behind an RLE table, a predefined block, a raw block and an RLE block, the RLE bytes 35 / 31 / 52, the
    sequences section at each byte alignment, and the longest three descriptions the format allows in front of a bitstream of
    more than 336 bytes"""
    rng = random.Random(404)
    out = []
    hist = ("raw", rng.randbytes(2048))
    for triple in range(64):
        first = _three(rng)
        tabs = {f: ("tab", first[f][0], fse_table(*first[f])) for f in FIELDS}
        b1 = _mode_block(rng, {f: ("fse",) + first[f] for f in FIELDS}, tabs)
        modes = {}
        for k, f in enumerate(FIELDS):
            m = (triple >> (4 - 2 * k)) & 3
            if m == 0:
                modes[f], tabs[f] = ("pre",), ("tab", DEFAULTS[f][0], fse_table(*DEFAULTS[f]))
            elif m == 1:
                code = {"LL": 5, "OF": 6, "ML": 9}[f]
                modes[f], tabs[f] = ("rle", code), ("rle", code)
            elif m == 2:
                sp = _three(rng, 7)[f]
                modes[f], tabs[f] = ("fse",) + sp, ("tab", sp[0], fse_table(*sp))
            else:
                modes[f] = ("rep",)
        out.append(build("modes_%d%d%d" % (triple >> 4, (triple >> 2) & 3, triple & 3), [hist, b1, _mode_block(rng, modes, tabs)]))
    rle = {"LL": ("rle", 3), "OF": ("rle", 7), "ML": ("rle", 11)}
    rep = {f: ("rep",) for f in FIELDS}
    pre = {f: ("pre",) for f in FIELDS}
    pretabs = {f: ("tab", DEFAULTS[f][0], fse_table(*DEFAULTS[f])) for f in FIELDS}
    out.append(build("modes_repeat_after_rle", [hist, _mode_block(rng, rle, rle), _mode_block(rng, rep, rle)]))
    out.append(build("modes_repeat_after_predefined", [hist, _mode_block(rng, pre, pretabs), _mode_block(rng, rep, pretabs)]))
    first = _three(rng)
    tabs = {f: ("tab", first[f][0], fse_table(*first[f])) for f in FIELDS}
    b1 = _mode_block(rng, {f: ("fse",) + first[f] for f in FIELDS}, tabs)
    out.append(build("modes_repeat_across_raw_and_rle", [hist, b1, ("raw", rng.randbytes(50)), _mode_block(rng, rep, tabs), ("rle", 0x41, 77),
                                                         _mode_block(rng, rep, tabs)]))
    # the RLE bytes 35 / 31 / 52, one field at a time where a small frame can execute them: LL 35 is a literal run of 65536 bytes
    # and ML 52 a match of 65539 (these two frames are longer than 64 KiB); OF 31 is an offset past 2^31, which no frame can execute:
    # invalid_tables has it (bad_rle_of31_executes), where it must get the execution's status and not the RLE byte's
    blk = Block(rng.randbytes(65536 + 4), [(65536, 5, 4)], ll=("rle", 35))
    out.append(build("modes_rle_ll35", [blk]))
    blk = Block(rng.randbytes(9), [(5, 6, 65539)], ml=("rle", 52))
    out.append(build("modes_rle_ml52", [blk]))
    # one block with 0 .. 3 more trailing literals: nothing but the pad moves the sequences section, which so starts at each of the
    # four byte alignments (META's seq_off; test_coverage asserts the four)
    sp = _three(rng)
    tabs = {f: ("tab", sp[f][0], fse_table(*sp[f])) for f in FIELDS}
    base = _mode_block(rng, {f: ("fse",) + sp[f] for f in FIELDS}, tabs)
    for pad in range(4):
        blk = Block(base.lits + bytes(pad), base.seqs, ll=base.modes["LL"], of=base.modes["OF"], ml=base.modes["ML"])
        out.append(build("modes_align%d" % pad, [hist, blk]))
    # long descriptions at the highest accuracy logs: every other symbol absent (its value and a 2-bit repeat flag of its own, which
    # longer zero runs would share), a count of 1 on the others, the last symbol takes the rest: 43 + 34 + 62 = 139 bytes, against
    # 38 + 30 + 55 with a count of 1 everywhere. Not proven to be the longest the format can say: once a few cells are given out,
    # small values take the short form (8 bits, 7 for OF), and counts large enough for the long form use the table up sooner.
    # Behind them a bitstream of more than 336 bytes (META's seq_desc / seq_stream; test_coverage asserts both)
    long_ = {}
    for f in FIELDS:
        nsym = MAX_SYM[f] + 1
        counts = [(i + nsym) % 2 for i in range(nsym)]   # 0 1 0 1 .. or 1 0 1 0 ..: the last symbol is present
        counts[-1] = (1 << MAX_LOG[f]) - sum(counts[:-1])
        long_[f] = (MAX_LOG[f], counts)
    tabs = {f: ("tab", long_[f][0], fse_table(*long_[f])) for f in FIELDS}
    blk = _mode_block(rng, {f: ("fse",) + long_[f] for f in FIELDS}, tabs, nseq=700)
    out.append(build("modes_long_descriptions", [hist, blk]))
    return out


def _bad_huf(name, desc, nstreams=1, pre=()):
    return build(name, list(pre) + [Block(b"abcdefgh", [], lit=("hufbytes", desc, nstreams))], valid=False)


def _bad_fse(name, field, desc, rng, junk=0):
    modes = {f: ("pre",) for f in FIELDS}
    modes[field] = ("bytes", desc)
    blk = Block(rng.randbytes(30), [(3, 5, 4)] * 4, ll=modes["LL"], of=modes["OF"], ml=modes["ML"], junk=junk)
    return build(name, [("raw", rng.randbytes(100)), blk], valid=False)


def invalid_tables():
    """each must fail with the oracle's leaf: Huffman descriptions (weights 12 / 15, all zero, a leftover that is no power of two,
    max_bits 12, a header longer than the section, an FSE weight table of accuracy log 7, a stream that ends in 0 or is empty, a
    description cut short), FSE descriptions (accuracy log too high, a symbol too many, a zero run past
    the highest symbol, cuts inside a count and inside a zero-run flag, RLE bytes 36 / 32 / 53, an RLE mode with no byte left),
    and lineage and order (repeat and treeless in a first block, the third description invalid in a long section — zg_k_fparse's
    second parse —, an invalid OF description behind a valid LL one with an invalid Huffman table in front of both). A count that
    overshoots the table cannot be written: a value field holds at most what is left plus one, so the largest count it can say
    fills the table exactly. An OF table that symbol 31 owns is here as well: it is a valid table whose every offset lies past 2^31"""
    rng = random.Random(505)
    out = []
    out.append(_bad_huf("bad_huf_weight12", weights_direct([12, 1, 1])))
    out.append(_bad_huf("bad_huf_weight15", weights_direct([1, 15, 1])))
    out.append(_bad_huf("bad_huf_all_zero", weights_direct([0] * 9)))
    out.append(_bad_huf("bad_huf_leftover", weights_direct([3, 2, 1, 1, 1])))          # 4 + 2 + 3 = 9: 7 are left
    out.append(_bad_huf("bad_huf_max_bits12", weights_direct([11, 11, 10, 10, 10, 9])))  # 1024*2 + 512*3 + 256 = 3840 > 2048
    out.append(_bad_huf("bad_huf_header_past_section", bytes([100]) + bytes(10)))
    good = [2, 1, 1, 0, 3, 1, 1, 2] * 8
    out.append(_bad_huf("bad_huf_fse_al7", bytes([40, 0x02]) + bytes(39)))             # accuracy log 5 + 2
    d = bytearray(weights_fse(good, 6))
    d[-1] = 0
    out.append(_bad_huf("bad_huf_stream_ends_in_0", bytes(d)))
    d = weights_fse(good, 6)
    tl = len(fse_desc(6, weights_counts(good, 6)))
    out.append(_bad_huf("bad_huf_empty_stream", bytes([tl]) + d[1:1 + tl]))
    d = weights_direct([1, 2, 3, 4, 4, 1, 2, 3, 3, 2, 1])
    out.append(build("bad_huf_description_cut", [("bytes", lit_header(2, 8, len(d) - 1, 1) + d[:-1] + b"\x00")], valid=False))
    for f in FIELDS:
        top, mx = MAX_SYM[f], MAX_LOG[f]
        w = FwdBits()
        w.add(mx + 1 - 5, 4)
        out.append(_bad_fse("bad_fse_%s_log" % f, f, w.bytes() + bytes(8), rng))
        out.append(_bad_fse("bad_fse_%s_one_symbol_too_many" % f, f, fse_desc(5, [16] + [0] * top + [16]), rng))
        out.append(_bad_fse("bad_fse_%s_zero_run_past_top" % f, f, fse_desc(5, [16] + [0] * (top + 6) + [16]), rng))
        d = fse_desc(6, _fill(20, 64, rng))
        out.append(build("bad_fse_%s_cut_in_count" % f, [_cut_block(f, d[:3], rng)], valid=False))
        d = fse_desc(5, [31, 0, 0, 0, 0, 0, 0, 0, 1])    # 4 + 6 bits, the zero's 2 bits, then flags: the cut falls inside them
        out.append(build("bad_fse_%s_cut_in_zero_run" % f, [_cut_block(f, d[:1] + bytes([d[1] & 0x3F | 0xC0]), rng)], valid=False))
        out.append(_bad_rle("bad_rle_%s_byte%d" % (f, top + 1), f, bytes([top + 1]), rng))
        out.append(_bad_rle("bad_rle_%s_no_byte" % f, f, b"", rng))
    blk = Block(rng.randbytes(30), [(3, (1 << 31) + 5, 4)] * 2, of=("fse", 5, [0] * 31 + [32]))
    out.append(build("bad_of31_owns_the_table", [("raw", rng.randbytes(100)), blk], valid=False))
    # the RLE byte 31 for OF is a valid byte (32 is not): the sequences decode, and the offset past 2^31 fails in execution
    blk = Block(rng.randbytes(30), [(3, (1 << 31) + 5, 4)] * 2, of=("rle", 31))
    out.append(build("bad_rle_of31_executes", [("raw", rng.randbytes(100)), blk], valid=False))
    assert STATUS["bad_rle_of31_executes"] >= 50, STATUS["bad_rle_of31_executes"]
    # lineage and order
    blk = Block(rng.randbytes(30), [(3, 5, 4)] * 4, ll=("rep",))
    blk2 = Block(rng.randbytes(30), [(3, 5, 4)] * 4, of=("rep",), ml=("rep",))
    fr = _Frame()
    for name, b in (("bad_repeat_in_first_block_ll", blk), ("bad_repeat_in_first_block_of_ml", blk2)):
        out.append(build(name, [("raw", rng.randbytes(64)), ("bytes", _raw_compressed(b, rng))], valid=False))
    lit = lit_header(3, 8, 2, 1) + b"\x55\x01"
    out.append(build("bad_treeless_in_first_block", [("raw", rng.randbytes(3)), ("bytes", lit + b"\x00")], valid=False))
    # the third description invalid in a section of more than 336 bytes: the staged row holds LL and OF whole, ML fails there and
    # is parsed again from the section itself
    ll_d = fse_desc(9, _fill(36, 512, rng, 3))
    of_d = fse_desc(8, _fill(29, 256, rng, 3))
    w = FwdBits()
    w.add(MAX_LOG["ML"] + 1 - 5, 4)
    sec = bytes([20, 0xA8]) + ll_d + of_d + w.bytes() + rng.randbytes(400)
    out.append(build("bad_third_description_long_section", [("raw", rng.randbytes(64)), ("bytes", lit_header(0, 5) + b"hello" + sec)], valid=False))
    ml_bad = fse_desc(5, [16] + [0] * 52 + [16])
    sec = bytes([20, 0xA8]) + ll_d + of_d + ml_bad + rng.randbytes(400)
    out.append(build("bad_third_description_symbols_long_section", [("raw", rng.randbytes(64)), ("bytes", lit_header(0, 5) + b"hello" + sec)], valid=False))
    # an invalid Huffman table in front of a valid LL and an invalid OF description: the literals error wins
    hd = weights_direct([12, 1, 1]) + b"\x01"
    w = FwdBits()
    w.add(MAX_LOG["OF"] + 1 - 5, 4)
    sec = bytes([4, 0xA0]) + fse_desc(6, _fill(12, 64, rng)) + w.bytes() + bytes(6)
    out.append(build("bad_huf_before_bad_of", [("raw", rng.randbytes(9)), ("bytes", lit_header(2, 8, len(hd), 1) + hd + sec)], valid=False))
    good_h = weights_direct([1, 1]) + _huf_stream(huf_codes([1, 1]), b"\x00\x01\x02\x02\x01\x00\x02\x02")
    out.append(build("bad_of_behind_good_huf", [("raw", rng.randbytes(9)), ("bytes", lit_header(2, 8, len(good_h), 1) + good_h + sec)], valid=False))
    return out


def _raw_compressed(blk, rng):
    """the content of a compressed block whose tables are not there: raw literals, the modes of blk, a short junk stream"""
    modes = 0
    for k, f in enumerate(FIELDS):
        modes |= {"pre": 0, "rle": 1, "fse": 2, "rep": 3}[blk.modes[f][0]] << (6 - 2 * k)
    return lit_header(0, len(blk.lits)) + blk.lits + bytes([len(blk.seqs), modes]) + b"\x5a\x01"


def _cut_block(field, desc, rng):
    """a last block whose sequences section ends inside the description of field (the fields in front are predefined)"""
    k = FIELDS.index(field)
    return ("bytes", lit_header(0, 6) + b"zgpu!!" + bytes([3, 2 << (6 - 2 * k)]) + desc)


def _bad_rle(name, field, byte, rng):
    k = FIELDS.index(field)
    tail = b"\x5a\x33\x01" if byte else b""
    return build(name, [("raw", rng.randbytes(40)), ("bytes", lit_header(0, 6) + b"zgpu!!" + bytes([3, 1 << (6 - 2 * k)]) + byte + tail)], valid=False)


FAMILIES = {
    "huf_alphabets": huf_alphabets,
    "huf_weight_streams": huf_weight_streams,
    "fse_shapes": fse_shapes,
    "fse_modes": fse_modes,
    "invalid_tables": invalid_tables,
}


def _check_differs(frames):
    """the LIBZSTD_DIFFERS cap, once every family is built"""
    names = [n for _, n, _, p in frames if p is not None]
    assert set(LIBZSTD_DIFFERS) <= set(names), "LIBZSTD_DIFFERS may hold only frames the oracle accepts"
    assert len(LIBZSTD_DIFFERS) * 10 <= len(names), "LIBZSTD_DIFFERS holds more than a tenth of the valid frames"


_F = framesuite.Families(FAMILIES, _check_differs)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


def coverage(frames):
    """what the frames reach, from the Python side (META, STATUS): frames is all_frames()'s list"""
    cov = {"nw": set(), "max_bits": set(), "largest_run": 0, "whole_wave_runs": 0, "huf_fse_al": set(), "desc_bytes": set(), "weight_parity": set(),
           "al": {f: set() for f in FIELDS}, "high": {f: 0 for f in FIELDS}, "zero_bit": False, "all_low": False, "single": False,
           "last_forms": set(), "states": [0, 0], "statuses": set(), "valid": 0, "invalid": 0, "lit_align": set(), "seq_align": set(),
           "min_comp": 1 << 20, "long_desc": None, "walks_short": [], "status_of": dict(STATUS)}
    for _, name, _, plain in frames:
        m = META[name]
        if plain is None:
            cov["statuses"].add(STATUS[name])
            cov["invalid"] += 1
            continue
        cov["valid"] += 1
        for h in m["huf"]:
            cov["nw"].add(h["nw"])
            cov["max_bits"].add(h["max_bits"])
            cov["largest_run"] = max(cov["largest_run"], h["run"])
            cov["whole_wave_runs"] = max(cov["whole_wave_runs"], h["whole_wave_runs"])
            cov["desc_bytes"].add(h["desc"])
            if h["fse"]:
                cov["huf_fse_al"].add(h["al"])
                cov["weight_parity"].add(h["nw"] % 2)
        for t in m["fse"]:
            cov["al"][t["field"]].add(t["al"])
            cov["high"][t["field"]] = max(cov["high"][t["field"]], t["high"])
            cov["zero_bit"] |= t["zero_bit"]
            cov["all_low"] |= t["all_low"]
            cov["single"] |= t["single"]
            cov["last_forms"].add(t["last_form"])
        for wk in m["walks"]:
            cov["states"][0] += wk["visited"]
            cov["states"][1] += wk["live"]
            if wk["nseq"] >= 3 * wk["size"] and (wk["visited"] != wk["live"] or wk["symbols"] != wk["symbols_visited"]):
                cov["walks_short"].append((name, wk["field"], wk["visited"], wk["live"]))
        if name.startswith("hws_align"):                 # (the block that carries the table: the first compressed one)
            cov["lit_align"].add(m["lit_off"][0] & 3)
        if name.startswith("modes_align"):
            cov["seq_align"].add(m["seq_off"][0] & 3)
        if name.startswith("hws_small_section"):
            cov["min_comp"] = min(cov["min_comp"], m["huf"][0]["comp"])
        if name == "modes_long_descriptions":
            cov["long_desc"] = (m["seq_desc"][0], m["seq_stream"][0])
    return cov
