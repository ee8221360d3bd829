"""Frames built from chosen sequence bitstreams (test helper, no tests): the FSE-coded stream of a sequences section at the bit rates
and stream positions no encoder reaches, so that zg_k_seq (zstd-rs_amd/csrc/zg_kernels.hip: the 512-byte LDS ring and its 16-byte
mirror, the mover wave that lands pieces one phase late, ZG_SEQ_MARGIN, the FAST form that checks nothing per step, the CAREFUL
form of the last ZG_SEQ_CH sequences, the packed tables) and zg_k_seqpost's extra-bit read (three dwords at pa & ~3, sh <= 31, the
so >= 32 branch) see them. Built on tests/tabframes.py: Block, fse_table, fse_states, RevBits and build, so every valid frame is
checked when it is built against its plaintext (seqframes.lz77 of what the writer was given), the oracle's bytes and tables, and
libzstd (except the frames of LIBZSTD_DIFFERS); every invalid one comes back with plaintext None and the oracle's status in STATUS.

serial_sequences is the plain reference of the operation, written from RFC 8878 3.1.1.3.2 and the reference's loop
(sequence_section_decoder.rs:154-221). coverage() computes from its per-sequence bit counts what the families reach.

The tables that make a step cost the maximum: accuracy logs 9 / 8 / 9, every symbol the sequences use with a count of 1 or -1 (one
cell, all `al` state bits), the rest of the table with a filler symbol no sequence uses: a misread state almost surely lands on the
filler and shifts every later bit count. A sequence of codes 35 / 31 / 52 takes 9 + 9 + 8 + 16 + 16 + 31 = 89 bits; no valid frame
can hold one (an offset past 2^31). The highest valid rate here is LL code 30 / 31, ML code 52 and OF code 26: 79 / 80 bits.

Limits found (the oracle decides, see LABNOTES.md "seqstreams"): window log 27 is accepted under the default 128 MiB limit, so
offset code 26 is reached over 64 MiB of RLE blocks (4 bytes of input per 128 KiB); the literals header's 20-bit size is the only
bound on an RLE literals section, so MAX_RLE_REGEN = 2^20 - 1 literals per block, and a block may regenerate far more than 128 KiB
(60 matches of code 52 are about 6 MiB). libzstd 1.4.9 decodes such a block as long as its literals section stays within 128 KiB
(mix_11_hi_13: 13 matches of code 52, 1.3 MiB) and rejects it otherwise: those frames are on LIBZSTD_DIFFERS, each with that one
reason."""
import os
import random
import re

import blockcheck
import framesuite
from tabframes import DEFAULTS, FIELDS, LL_BASE, LL_BITS, MAX_LOG, META, ML_BASE, ML_BITS, STATUS, Block, build, fse_desc, fse_table, nbseq

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zstd-rs_amd", "csrc", "zg_kernels.hip")

EXTRA_PADDING, UNSUPPORTED_OFFSET, NOT_ENOUGH_BYTES, EXTRA_BITS = 44, 45, 46, 47     # oracle/zstd_oracle.h
MAX_RLE_REGEN = (1 << 20) - 1
MAX_SEQ_BITS = 9 + 9 + 8 + 16 + 16 + 31
HI_BITS = 9 + 9 + 8 + 26 + 16 + 11                       # LL code 30, ML code 52, OF code 26
BIG_BLOCK = "the literals section of a block regenerates more than 128 KiB: libzstd rejects it"

# valid frames libzstd's decompressor does not return the plaintext for; all_frames() checks that these are frames the oracle
# accepts, at most a fifth of the valid ones, and every one for the one reason BIG_BLOCK
LIBZSTD_DIFFERS = {n: BIG_BLOCK for n in ("mrv_w27", "mrv_w25", "burst_low_high_low", "burst_high_low_high", "burst_zero_bit_states",
                                          "ring_hi_offsets", "mix_03_hi_49")}


def kernel_constants():
    """the ring and phase sizes of zg_k_seq, read out of its source"""
    out = framesuite.defines(_SRC, ("ZG_SEQ_CH", "ZG_SEQ_CMAX", "ZG_SEQ_RING", "ZG_SEQ_G"))
    m = re.search(r"^#define\s+ZG_SEQ_MARGIN\s+\((\d+) \* ZG_SEQ_CMAX \+ (\d+)\)", open(_SRC).read(), re.M)
    assert m, "ZG_SEQ_MARGIN has another form"
    out["ZG_SEQ_MARGIN"] = int(m.group(1)) * out["ZG_SEQ_CMAX"] + int(m.group(2))
    assert out["ZG_SEQ_CMAX"] * 8 >= out["ZG_SEQ_CH"] * MAX_SEQ_BITS, "a phase of 89-bit sequences does not fit ZG_SEQ_CMAX"
    return out


K = kernel_constants()
CH, G, RING = K["ZG_SEQ_CH"], K["ZG_SEQ_G"], K["ZG_SEQ_RING"]


# ---- the reference ----------------------------------------------------------------------------------------------------------

def serial_sequences(tables, nseq, stream):
    """one sequences bitstream, sequence by sequence (RFC 8878 3.1.1.3.2; sequence_section_decoder.rs:26-40 and :154-221): skip to
    the closing 1-bit; initial states LL, OF, ML; per sequence the codes of the three states, the extra bits offset, match length,
    literal length, then (not after the last) the state updates LL, ML, OF, and NotEnoughBytes once bits_remaining is negative;
    ExtraBits if any are left at the end. Bits below the stream's start read as zeros. tables: field -> ("tab", al, [(base_line,
    num_bits, symbol)]) | ("rle", code). Returns {"status": 0 or the oracle's status number, "seqs": [(ll, ml, offset_value)],
    "bits": bits each sequence consumed, "remaining": bits_remaining at the end, "first": bit position of the first sequence,
    "reads": [(q_ll, LL extra bits, ML extra bits, OF code)] per sequence, q_ll the bit position of the lowest extra bit,
    "failed_at": the sequence a failure was met at}"""
    out = {"status": 0, "seqs": [], "bits": [], "remaining": None, "first": None, "reads": [], "failed_at": None}
    if not stream or stream[-1] == 0:
        out["status"] = EXTRA_PADDING
        return out
    v = int.from_bytes(stream, "little")
    pos = v.bit_length() - 1

    def get(n):
        nonlocal pos
        pos -= n
        return ((v >> pos) if pos >= 0 else (v << -pos)) & ((1 << n) - 1)

    state = {}
    for f in ("LL", "OF", "ML"):
        if tables[f][0] == "tab":
            state[f] = get(tables[f][1])
    out["first"] = pos

    def code(f):
        return tables[f][1] if tables[f][0] == "rle" else tables[f][2][state[f]][2]

    for i in range(nseq):
        start = pos
        lc, mc, oc = code("LL"), code("ML"), code("OF")
        if oc > 31:
            out["status"], out["failed_at"] = UNSUPPORTED_OFFSET, i
            break
        ov = get(oc) + (1 << oc)
        ml = ML_BASE[mc] + get(ML_BITS[mc])
        ll = LL_BASE[lc] + get(LL_BITS[lc])
        out["reads"].append((pos, LL_BITS[lc], ML_BITS[mc], oc))
        out["seqs"].append((ll, ml, ov))
        if i + 1 < nseq:
            for f in ("LL", "ML", "OF"):
                if tables[f][0] == "tab":
                    base, nb, _ = tables[f][2][state[f]]
                    state[f] = base + get(nb)
        out["bits"].append(start - pos)
        if pos < 0:
            out["status"], out["failed_at"] = NOT_ENOUGH_BYTES, i
            break
    out["remaining"] = pos
    if out["status"] == 0 and pos > 0:
        out["status"] = EXTRA_BITS
    return out


# ---- tables -----------------------------------------------------------------------------------------------------------------

def full_counts(field, used, low=(), filler=0):
    """counts of an accuracy log MAX_LOG[field] table in which every symbol of `used` has one cell (count 1; the ones in `low` -1:
    a low-probability cell at the table's top) and so takes all state bits; the filler symbol has the rest"""
    counts = [0] * (max(max(used), filler) + 1)
    for s in used:
        counts[s] = -1 if s in low else 1
    assert filler not in used
    counts[filler] = (1 << MAX_LOG[field]) - len(used)
    return ("fse", MAX_LOG[field], counts)


def _shared_counts(field, cheap, full):
    """cheap: symbols that share the table evenly (few state bits each); full: symbols of one cell"""
    size = 1 << MAX_LOG[field]
    counts = [0] * (max(cheap + full) + 1)
    for s in full:
        counts[s] = 1
    each = (size - len(full)) // len(cheap)
    for s in cheap:
        counts[s] = each
    counts[cheap[0]] += size - sum(counts)
    return ("fse", MAX_LOG[field], counts)


# HI: the highest valid rate and the 89-bit codes; NR: the highest rate that keeps a block of 60 sequences under 128 KiB (libzstd
# accepts it); MOD: full state bits and small values; MIX: cheap symbols next to one-cell symbols (bursts)
HI = {"LL": full_counts("LL", [30, 31, 34, 35], low=[31]), "OF": full_counts("OF", [1, 2, 20, 24, 26, 31], low=[26]), "ML": full_counts("ML", [51, 52], low=[52])}
NR = {"LL": full_counts("LL", [24, 25, 26, 27], low=[25]), "OF": full_counts("OF", [1, 2, 14, 15, 16], low=[15]), "ML": full_counts("ML", [42, 43, 44, 45, 46], low=[44])}
MOD = {"LL": full_counts("LL", list(range(1, 16)), low=[3, 9], filler=0), "OF": full_counts("OF", [2, 3, 4, 5], low=[4]),
       "ML": full_counts("ML", list(range(1, 12)), low=[5])}
MIX = {"LL": _shared_counts("LL", [1, 2, 3, 4], [30, 31]), "OF": _shared_counts("OF", [8, 9, 10, 11], [26]), "ML": _shared_counts("ML", [1, 2, 3, 4], [52])}
REJ = {"LL": full_counts("LL", [35]), "OF": full_counts("OF", [31]), "ML": full_counts("ML", [52])}


def in_force(modes, prev=None):
    """modes (field -> Block mode) -> field -> ("tab", al, table) | ("rle", code), as serial_sequences takes them"""
    out = dict(prev or {})
    for f in FIELDS:
        m = modes[f]
        if m[0] == "pre":
            out[f] = ("tab", DEFAULTS[f][0], fse_table(*DEFAULTS[f]))
        elif m[0] == "rle":
            out[f] = ("rle", m[1])
        elif m[0] == "fse":
            out[f] = ("tab", m[1], fse_table(m[1], m[2]))
    return out


def _desc_len(modes):
    return sum(len(fse_desc(m[1], m[2])) if m[0] == "fse" else 1 if m[0] == "rle" else 0 for m in (modes[f] for f in FIELDS))


# ---- sequences --------------------------------------------------------------------------------------------------------------

def _val(base, bits, c, rng, mask=-1):
    return base[c] + (rng.randrange(1 << bits[c]) & mask)


def hi_seqs(n, pos, rng, of_code=26, ll_codes=(30, 31), ml_mask=0xFFFF):
    """n sequences at the highest valid rate: LL code 30 / 31 with random extra bits, ML code 52, the given OF code with extra bits
    random below what the output so far (pos bytes) allows. Returns (seqs, pos after them)"""
    seqs = []
    for _ in range(n):
        ll = _val(LL_BASE, LL_BITS, rng.choice(ll_codes), rng)
        pos += ll
        span = min(1 << of_code, pos + 3 - (1 << of_code))               # distance = offset_value - 3 <= pos
        assert span > 0, (pos, of_code)
        ml = _val(ML_BASE, ML_BITS, 52, rng, ml_mask)
        seqs.append((ll, (1 << of_code) + rng.randrange(span), ml))
        pos += ml
    return seqs, pos


def table_seqs(n, pos, rng, T, lo_of=2, window=1 << 17):
    """n sequences that draw their codes from the one-cell symbols of the table set T (OF codes from lo_of up, offsets within
    the output so far and the window)"""
    use = {f: [s for s, c in enumerate(T[f][2]) if abs(c) == 1] for f in FIELDS}
    seqs = []
    for _ in range(n):
        ll = _val(LL_BASE, LL_BITS, rng.choice(use["LL"]), rng)
        pos += ll
        ocs = [c for c in use["OF"] if c >= lo_of and (1 << c) - 3 <= min(pos, window) and c < 31]
        oc = rng.choice(ocs)
        span = min(1 << oc, min(pos, window) + 4 - (1 << oc))
        ov = max((1 << oc) + rng.randrange(span), 4)
        ml = _val(ML_BASE, ML_BITS, rng.choice(use["ML"]), rng)
        seqs.append((ll, ov, ml))
        pos += ml
    return seqs, pos


def cheap_seqs(n, pos, rng):
    """n sequences of MIX's cheap symbols: about 2 + 2 + 2 state bits and 8 .. 11 offset bits"""
    seqs = []
    for _ in range(n):
        ll = rng.randint(1, 4)
        pos += ll
        oc = rng.choice([c for c in (8, 9, 10, 11) if (1 << c) - 3 <= pos])
        span = min(1 << oc, pos + 4 - (1 << oc))
        ml = rng.randint(4, 7)
        seqs.append((ll, (1 << oc) + rng.randrange(span), ml))
        pos += ml
    return seqs, pos


def rle_history(nbytes, rng, piece=131072):
    """RLE blocks of a random byte each, nbytes in all"""
    out = []
    while nbytes:
        n = min(piece, nbytes)
        out.append(("rle", rng.randrange(256), n))
        nbytes -= n
    return out


def sblock(seqs, T, rng, tail=5, lit="rle", prev=None):
    """a Block of seqs under the table set T (field -> Block mode); RLE literals (any count up to MAX_RLE_REGEN) or raw ones"""
    n = sum(s[0] for s in seqs) + tail
    assert n <= MAX_RLE_REGEN
    lits = bytes([rng.randrange(256)]) * n if lit == "rle" else rng.randbytes(n)
    b = Block(lits, seqs, lit=(lit, None), ll=T["LL"], of=T["OF"], ml=T["ML"])
    b.regen, b.lit_regen = n + sum(s[2] for s in seqs), n
    return b


def frame(name, blocks, window_log=17, valid=True):
    """tabframes.build, then what this helper adds: per compressed block the tables in force, where its bitstream lies in the
    frame, and serial_sequences of it (META[name]["ss"])"""
    r = build(name, blocks, window_log=window_log, valid=valid, differs=LIBZSTD_DIFFERS)
    z, m, recs, tabs = r[1], META[name], [], {}
    for j, b in enumerate(x for x in blocks if isinstance(x, Block)):
        end = m["lit_off"][j] + (int.from_bytes(z[m["lit_off"][j] - 3:m["lit_off"][j]], "little") >> 3)
        if b.seq_raw is not None:
            tabs, nseq, at = b.ss["tables"], b.ss["nseq"], m["seq_off"][j] + b.ss["stream_at"]
        else:
            tabs, nseq = in_force(b.modes, tabs), len(b.seqs)
            at = m["seq_off"][j] + len(nbseq(nseq)) + 1 + _desc_len(b.modes)
        if nseq == 0:
            continue
        ss = serial_sequences(tabs, nseq, z[at:end])
        recs.append(dict(ss, at=at, end=end, nseq=nseq, tables=tabs, block=j, regen=getattr(b, "regen", None), lit_regen=getattr(b, "lit_regen", None)))
        if r[2] is not None:
            assert ss["status"] == 0 and ss["remaining"] == 0, (name, j, ss["status"], ss["remaining"])
            assert [(ll, ov, ml) for ll, ml, ov in ss["seqs"]] == list(b.seqs), (name, j, "serial_sequences does not return what was written")
    m["ss"] = recs
    m["frame_len"] = len(z)
    return r


_OB = {}


def oracle_blocks(name, z):
    """blockcheck.oracle_blocks of a valid frame, once per frame"""
    if name not in _OB:
        _OB[name] = blockcheck.oracle_blocks(z)
    return _OB[name]


# ---- the families: each returns [(name, zst, plaintext or None)] ------------------------------------------------------------

NSEQ_LIST = (1, 2, 11, 12, 13, 24, 25, 36, 37, 48, 49, 60)
HIST27 = (64 << 20) + 131072
HIST25 = (16 << 20) + 131072


def _so_block(rng, pos, so, of_code):
    """a block of 3 sequences whose middle one has LL code 35 with ML code 52 (so == 32) or ML code 51 (so == 31) and the given OF
    code: with code 26 the 16 + 16 + 26 = 58 bits that are the widest field zg_k_seqpost reads in a valid frame"""
    a, pos = hi_seqs(1, pos, rng, of_code=20)
    ll = _val(LL_BASE, LL_BITS, 35, rng)
    pos += ll
    span = min(1 << of_code, pos + 3 - (1 << of_code))
    assert span > 0, (pos, of_code)
    mid = (ll, (1 << of_code) + rng.randrange(span), _val(ML_BASE, ML_BITS, 52 if so == 32 else 51, rng))
    pos += mid[2]
    c, pos = hi_seqs(1, pos, rng, of_code=20)
    return a + [mid] + c, pos


def max_rate_valid():
    """ZG_SEQ_CMAX, ZG_SEQ_MARGIN and the three-phase request -> land -> read pipeline of the mover at the highest rate a valid
    frame can sustain: every sequence of a block takes 79 or 80 bits (all 26 state bits, OF code 26, ML code 52, LL code 30 / 31
    over RLE literals, the extra bits random) except its last, which updates no state. mrv_w27: window log 27, 64 MiB + 128 KiB of
    RLE blocks, then one block for every nseq of NSEQ_LIST (the last sequence and the FAST -> CAREFUL switch at every phase
    position), a block whose middle sequence has LL code 35, ML code 52 and OF code 26 (zg_k_seqpost's so == 32, a field of 58 bits)
    and one with LL code 35 and ML code 51 (so == 31). mrv_w25: the same with OF code 24 under window log 25, for nseq 49 and 60. mrv_nr_n*: one block of
    each nseq at the highest rate that stays under 128 KiB (about 55 bits), which libzstd decodes too"""
    rng = random.Random(711)
    out = []
    for name, wl, hist, oc, counts in (("mrv_w27", 27, HIST27, 26, NSEQ_LIST), ("mrv_w25", 25, HIST25, 24, (49, 60))):
        blocks, pos = rle_history(hist, rng), hist
        for n in counts:
            seqs, pos = hi_seqs(n, pos, rng, of_code=oc)
            blocks.append(sblock(seqs, HI, rng))
            pos += 5
        for so in (32, 31):
            seqs, pos = _so_block(rng, pos, so, oc)
            blocks.append(sblock(seqs, HI, rng))
            pos += 5
        out.append(frame(name, blocks, window_log=wl))
    for n in NSEQ_LIST:
        seqs, _ = table_seqs(n, 70000, rng, NR, lo_of=14)
        out.append(frame("mrv_nr_n%d" % n, rle_history(70000, rng, 10000) + [sblock(seqs, NR, rng, lit="raw")]))
    return out


def _rej_seqs(n, rng):
    return [(_val(LL_BASE, LL_BITS, 35, rng), (1 << 31) + rng.randrange(1 << 31), _val(ML_BASE, ML_BITS, 52, rng)) for _ in range(n)]


def max_rate_rejected():
    """ZG_SEQ_CMAX exactly: every sequence takes all 89 bits (codes 35 / 31 / 52, random extra bits), 4 x ZG_SEQ_CH + 1 of them
    and once 301; the stream ends on bit 0, so the status is the execution's (an offset past 2^31), not the bitstream's. The second
    kind: 4 x ZG_SEQ_CH executable sequences at the NR rate and a failing last one: offset 0 (repeat code 3 with no literals
    behind a distance of 1), and an offset one byte past everything decoded so far"""
    rng = random.Random(722)
    out = []
    for n in (4 * CH + 1, 301):
        b = Block(bytes([7]) * 200000, _rej_seqs(n, rng), lit=("rle", None), ll=REJ["LL"], of=REJ["OF"], ml=REJ["ML"])
        out.append(frame("mrr_all89_n%d" % n, [("raw", rng.randbytes(300)), b], valid=False))
    for kind in ("zero_offset", "past_the_data"):
        seqs, pos = table_seqs(4 * CH - 1, 70000, rng, NR, lo_of=14)
        ll = _val(LL_BASE, LL_BITS, 24, rng)
        seqs.append((ll, 4, 700))                                     # a distance of 1: the repeat offsets are now [1, ..]
        pos += ll + 700
        if kind == "zero_offset":
            seqs.append((0, 3, 700))                                  # repeat code 3 without literals: offset 1 - 1
        else:
            ll = _val(LL_BASE, LL_BITS, 25, rng)
            d = pos + ll + 1
            assert (d + 3).bit_length() - 1 == 16
            seqs.append((ll, d + 3, 700))
        # (LL code 0 for the sequence without literals: the table gets that cell, the filler moves to symbol 1)
        T = dict(NR, LL=full_counts("LL", [0, 24, 25, 26, 27], low=[25], filler=1))
        out.append(frame("mrr_last_%s" % kind, rle_history(70000, rng, 10000) + [sblock(seqs, T, rng, lit="raw")], valid=False))
    return out


def bursts():
    """the mover's request arithmetic when the rate changes between phases (want = p0 - ZG_SEQ_MARGIN after a phase that moved
    little or much): 300 sequences of about 20 bits, 4 x ZG_SEQ_CH at the highest valid rate, 300 cheap ones again, in one stream;
    the reverse order; and 0-bit states (an ML table that symbol 52 owns, LL as RLE mode) next to a full-rate OF chain, then all
    three fields without state bits: a sequence that takes its extra bits only"""
    rng = random.Random(733)
    out = []
    for name, order in (("burst_low_high_low", "lhl"), ("burst_high_low_high", "hlh")):
        blocks, pos, seqs = rle_history(HIST25, rng), HIST25, []
        for k in order:
            s, pos = cheap_seqs(300, pos, rng) if k == "l" else hi_seqs(4 * CH, pos, rng, of_code=24)
            seqs += s
        T = dict(MIX, OF=_shared_counts("OF", [8, 9, 10, 11], [24]))
        blocks.append(sblock(seqs, T, rng))
        out.append(frame(name, blocks, window_log=25))
    blocks, pos = rle_history(4 << 20, rng), 4 << 20
    seqs, pos = hi_seqs(4 * CH + 3, pos, rng, of_code=20, ll_codes=(30,))
    T = {"LL": ("rle", 30), "OF": HI["OF"], "ML": ("fse", 5, [0] * 52 + [32])}
    blocks.append(sblock(seqs, T, rng))
    pos += 5
    seqs, pos = hi_seqs(2 * CH + 5, pos, rng, of_code=20, ll_codes=(30,))
    T = {"LL": ("rle", 30), "OF": ("rle", 20), "ML": ("fse", 9, [0] * 52 + [512])}
    blocks.append(sblock(seqs, T, rng))
    out.append(frame("burst_zero_bit_states", blocks, window_log=23))
    return out


RING_COPIES = RING
HI_OFFSETS = 16


def ring_phases():
    """the ring's wrap (ZG_SEQ_RING, the mirror store of zg_ring_put) at every position of a stream: ring_mod is one block of 220
    sequences with all 26 state bits and small values (a stream of more than ZG_SEQ_RING bytes, a few KiB of output) in a frame
    of odd length: ring_submit() repeats it ZG_SEQ_RING times, so in one submit the stream's start, and with it its top, takes
    every residue mod ZG_SEQ_RING relative to the first copy's, whatever the alignment of the device buffer. ring_hi_offsets:
    16 blocks of 3 x ZG_SEQ_CH + 1 sequences at the highest valid rate in one frame, raw blocks between them sized so that the 16
    streams start at the 16 residues mod 16 (the 16-byte pieces of the prologue and of the mover; ML's extra bits are cut to 12
    there to keep the frame small: the bit counts are the same). ring_nr_p*: the NR block behind a raw block of 0 .. 15 bytes:
    decoded alone, each has its stream near the front of the source buffer, where the floorA clamp applies"""
    rng = random.Random(744)
    out = []
    seqs, _ = table_seqs(220, 64, rng, MOD, lo_of=2)
    for tail in (5, 6):
        r = frame("ring_mod", [("raw", rng.randbytes(64)), sblock(seqs, MOD, random.Random(1), tail=tail, lit="raw")])
        if len(r[1]) % 2:
            break
    assert len(r[1]) % 2 == 1
    out.append(r)
    hist = rle_history(HIST27, rng)
    pos, blks = HIST27, []
    for _ in range(HI_OFFSETS):
        seqs, pos = hi_seqs(3 * CH + 1, pos, rng, ml_mask=0xFFF)
        blks.append(sblock(seqs, HI, rng))
        pos += 5
    lay = lambda pads: hist + [x for b, n in zip(blks, pads) for x in (("raw", bytes(n)), b)]
    # where the streams start with empty raw blocks in front of each (a layout run without the history, which the oracle refuses; an
    # RLE block takes 4 bytes); a pad in front of block i moves it and every later one
    frame("ring_hi_layout", lay([0] * HI_OFFSETS)[len(hist):], window_log=27, valid=False)
    pads, moved = [], 0
    for i, rec in enumerate(META.pop("ring_hi_layout")["ss"]):
        pads.append((i - rec["at"] - 4 * len(hist) - moved) % 16)
        moved += pads[-1]
    del STATUS["ring_hi_layout"]
    out.append(frame("ring_hi_offsets", lay(pads), window_log=27))
    for p in range(16):
        seqs, _ = table_seqs(3 * CH + 2, 70000 + p, rng, NR, lo_of=14)
        out.append(frame("ring_nr_p%d" % p, [("raw", rng.randbytes(p))] + rle_history(70000, rng, 10000) + [sblock(seqs, NR, rng, lit="raw")]))
    return out


def ring_submit():
    """(the bytes of ZG_SEQ_RING copies of ring_mod, its plaintext, the number of copies)"""
    _, z, plain = family("ring_phases")[0]
    return z * RING_COPIES, plain, RING_COPIES


def _raw_section(nseq_claimed, modes_byte, descs, stream):
    return nbseq(nseq_claimed) + bytes([modes_byte]) + descs + stream


def stream_ends():
    """the end of a stream at every position relative to the FAST / CAREFUL switch (left > ZG_SEQ_CH) and to the ring's prologue:
    one valid NR stream of 60 sequences kept byte for byte under other sequence counts (47, 48, 59: bits left over; 61, 72, 73,
    0x7F00, 0x7F01: the stream runs out in the CAREFUL form, at the switch, and in a FAST phase with thousands of sequences
    left); random streams of 1, 2, 3, 15, 16 and 17 bytes under a count of 30 and of 1 (the initial states alone are longer than
    the first three); the closing bit at each position of the last byte, a last byte of 0 and an empty stream"""
    rng = random.Random(755)
    out = []
    hist = rle_history(70000, rng, 10000)
    seqs, _ = table_seqs(60, 70000, rng, NR, lo_of=14)
    base = sblock(seqs, NR, rng, lit="raw")
    r = frame("se_base_n60", hist + [base])
    out.append(r)
    rec = META["se_base_n60"]["ss"][0]
    stream = r[1][rec["at"]:rec["end"]]
    descs = b"".join(fse_desc(NR[f][1], NR[f][2]) for f in FIELDS)
    tabs = in_force({f: NR[f] for f in FIELDS})

    def variant(name, n, st):
        sec = _raw_section(n, 0xA8, descs, st)
        b = Block(base.lits, [], lit=("raw", None), seq_raw=sec)
        b.ss = {"tables": tabs, "nseq": n, "stream_at": len(sec) - len(st)}
        fr = frame(name, hist + [b], valid=False)
        want = serial_sequences(tabs, n, st)["status"]
        assert want == 0 or STATUS[name] == want, (name, STATUS[name], want, "serial_sequences and the oracle differ on the bitstream's status")
        return fr

    for n in (47, 48, 59, 61, 72, 73, 0x7F00, 0x7F01):
        out.append(variant("se_count_%d" % n, n, stream))
    for nb in (1, 2, 3, 15, 16, 17):
        st = rng.randbytes(nb - 1) + bytes([rng.randrange(128, 256)])
        for n in (30, 1):
            out.append(variant("se_bytes%d_count%d" % (nb, n), n, st))
    for k in range(8):
        st = rng.randbytes(40) + bytes([(1 << k) | rng.randrange(1 << k)])
        for n in (20, 1):
            out.append(variant("se_closing_bit%d_count%d" % (k, n), n, st))
    out.append(variant("se_last_byte_0", 5, stream[:-1] + b"\x00"))
    out.append(variant("se_empty_stream", 5, b""))
    return out


def workgroup_mixes():
    """a workgroup of zg_k_seq: ZG_SEQ_G blocks that are adjacent in a submit (mix_submit(): one frame each, in this order), of 1 to
    480 sequences, at the MOD, NR, highest valid and 89-bit rates, valid and rejected: quads that finish at once or after one
    phase, quads that fail in a FAST phase and in the CAREFUL one, and wave neighbours that run on for 40 phases more"""
    rng = random.Random(766)
    out = []
    hist = lambda: rle_history(70000, rng, 10000)

    def mod(name, n):
        seqs, _ = table_seqs(n, 70000, rng, MOD, lo_of=2)
        return frame(name, hist() + [sblock(seqs, MOD, rng, lit="raw")])

    def nr(name, n):
        seqs, _ = table_seqs(n, 70000, rng, NR, lo_of=14)
        return frame(name, hist() + [sblock(seqs, NR, rng, lit="raw")])

    def hi(name, n):
        seqs, _ = hi_seqs(n, 4 << 20, rng, of_code=20)
        return frame(name, rle_history(4 << 20, rng) + [sblock(seqs, HI, rng)], window_log=23)

    def cut(name, n, claimed, drop):
        """an NR stream of n sequences cut by `drop` bytes at its low end under a claimed count"""
        seqs, _ = table_seqs(n, 70000, rng, NR, lo_of=14)
        base = sblock(seqs, NR, rng, lit="raw")
        r = frame(name, hist() + [base])
        rec = META[name]["ss"][0]
        st = r[1][rec["at"] + drop:rec["end"]]
        descs = b"".join(fse_desc(NR[f][1], NR[f][2]) for f in FIELDS)
        sec = _raw_section(claimed, 0xA8, descs, st)
        b = Block(base.lits, [], lit=("raw", None), seq_raw=sec)
        b.ss = {"tables": in_force({f: NR[f] for f in FIELDS}), "nseq": claimed, "stream_at": len(sec) - len(st)}
        return frame(name, hist() + [b], valid=False)

    out.append(mod("mix_00_mod_1", 1))
    out.append(nr("mix_01_nr_120", 120))
    out.append(mod("mix_02_mod_2", 2))
    out.append(hi("mix_03_hi_49", 4 * CH + 1))
    b = Block(bytes([9]) * 200000, _rej_seqs(4 * CH + 1, rng), lit=("rle", None), ll=REJ["LL"], of=REJ["OF"], ml=REJ["ML"])
    out.append(frame("mix_04_all89_49", [("raw", rng.randbytes(40)), b], valid=False))
    out.append(mod("mix_05_mod_12", CH))
    out.append(cut("mix_06_runs_out_fast", 100, 100, 300))
    out.append(mod("mix_07_mod_300", 300))
    out.append(cut("mix_08_runs_out_careful", 30, 30, 3))
    out.append(nr("mix_09_nr_13", CH + 1))
    out.append(cut("mix_10_extra_bits", 40, 39, 0))
    out.append(hi("mix_11_hi_13", CH + 1))
    out.append(mod("mix_12_mod_5", 5))
    out.append(nr("mix_13_nr_100", 100))
    out.append(mod("mix_14_mod_480", 480))
    out.append(nr("mix_15_nr_25", 2 * CH + 1))
    assert len(out) == G, "one frame per block of a workgroup"
    return out


FAMILIES = {
    "max_rate_valid": max_rate_valid,
    "max_rate_rejected": max_rate_rejected,
    "bursts": bursts,
    "ring_phases": ring_phases,
    "stream_ends": stream_ends,
    "workgroup_mixes": workgroup_mixes,
}
LARGE = ("mrv_w27", "mrv_w25", "ring_hi_offsets", "burst_low_high_low", "burst_high_low_high")     # histories of 16 and 64 MiB


def _check_differs(frames):
    """LIBZSTD_DIFFERS, once every family is built"""
    names = [n for _, n, _, p in frames if p is not None]
    assert set(LIBZSTD_DIFFERS) <= set(names), ("LIBZSTD_DIFFERS may hold only frames the oracle accepts", sorted(set(LIBZSTD_DIFFERS) - set(names)))
    assert len(LIBZSTD_DIFFERS) * 5 <= len(names), "LIBZSTD_DIFFERS holds more than a fifth of the valid frames"
    for n, reason in LIBZSTD_DIFFERS.items():
        assert reason == BIG_BLOCK and max(r["lit_regen"] for r in META[n]["ss"]) > 131072, (n, "on LIBZSTD_DIFFERS for another reason")
    for n in names:
        assert n in LIBZSTD_DIFFERS or all(r["lit_regen"] <= 131072 for r in META[n]["ss"]), n


_F = framesuite.Families(FAMILIES, _check_differs)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


def mix_submit():
    """the frames of workgroup_mixes in the order that makes their blocks one workgroup"""
    return family("workgroup_mixes")


def submit_offsets(frames):
    """name -> where the frame starts when the frames are one submit in this order (their bytes joined)"""
    out, at = {}, 0
    for _, name, z, _ in frames:
        out[name] = at
        at += len(z)
    return out


def _windows(bits, n):
    """(the largest sum of n consecutive entries from any start, from a start that is a multiple of ZG_SEQ_CH)"""
    if len(bits) < n:
        return 0, 0
    sums = [sum(bits[i:i + n]) for i in range(len(bits) - n + 1)]
    return max(sums), max(sums[::CH])


def coverage(frames, offsets=None):
    """what the frames reach, from serial_sequences' records: frames is all_frames()'s list. Every figure that concerns a kernel is
    kept apart for valid and for rejected frames ("valid" / "rejected"), since zg_k_seq decodes both and zg_k_seqpost runs on the
    blocks of valid frames only.

    window_bits / four_window_bits: the most bits ZG_SEQ_CH and 4 x ZG_SEQ_CH consecutive sequences of a block take, from any
    start; phase_bits / four_phase_bits: the same from a start that is a multiple of ZG_SEQ_CH, which is how zg_k_seq cuts its
    phases. The second is the smaller one, so the lower bounds the CPU test asserts on it hold for the first too.

    pairs, so, sh, field_bits (the widest LL + ML + OF extra-bit field), field_bits_at_sh31: what zg_k_seqpost's read meets. pa is
    the byte address of a sequence's lowest extra bit; only pa & 3 matters, and device buffers are aligned to far more than 4
    bytes, so pa is taken relative to the start of the source buffer: the frame's own start for a frame decoded alone (offsets
    None), or offsets[name] (submit_offsets) for the frames of a shared submit. The widest field a valid frame can hold is 16 + 16
    + 26 = 58 bits (an offset code above 26 needs a window the oracle refuses); the 63 bits the read is built for occur in
    rejected frames only, that is in this model and never in the kernel. Returns the figures; the CPU test asserts the targets"""
    two = lambda v: {"valid": v(), "rejected": v()}
    cov = {"valid": 0, "invalid": 0, "statuses": set(), "phase_bits": two(int), "four_phase_bits": two(int), "window_bits": two(int),
           "four_window_bits": two(int), "pairs": two(set), "so": two(set), "sh": two(set), "field_bits": two(int), "field_bits_at_sh31": two(int),
           "nseq_mod": two(set), "residues": set(), "hi_residues16": set(), "runs_out": set(), "max_regen": 0, "max_lit_regen": 0, "max_nseq": 0,
           "seq_bits": two(int), "min_seq_bits": 1 << 30, "per_family": {}}
    for fam, name, z, plain in frames:
        kind = "valid" if plain is not None else "rejected"
        cov["valid" if plain is not None else "invalid"] += 1
        cov["per_family"][fam] = cov["per_family"].get(fam, 0) + 1
        if plain is None:
            cov["statuses"].add(STATUS[name])
        base = offsets[name] if offsets else 0
        for rec in META[name]["ss"]:
            bits = rec["bits"]
            if rec["status"] == NOT_ENOUGH_BYTES:
                i = rec["failed_at"]
                cov["runs_out"].add("fast" if rec["nseq"] - i // CH * CH > CH else "careful")
            if rec["status"] in (NOT_ENOUGH_BYTES, EXTRA_PADDING, UNSUPPORTED_OFFSET):
                continue
            for key, akey, n in (("window_bits", "phase_bits", CH), ("four_window_bits", "four_phase_bits", 4 * CH)):
                anywhere, aligned = _windows(bits, n)
                cov[key][kind], cov[akey][kind] = max(cov[key][kind], anywhere), max(cov[akey][kind], aligned)
            cov["seq_bits"][kind] = max([cov["seq_bits"][kind]] + bits)
            cov["min_seq_bits"] = min([cov["min_seq_bits"]] + bits)
            cov["nseq_mod"][kind].add(rec["nseq"] % CH)
            cov["max_nseq"] = max(cov["max_nseq"], rec["nseq"])
            if rec["regen"]:
                cov["max_regen"], cov["max_lit_regen"] = max(cov["max_regen"], rec["regen"]), max(cov["max_lit_regen"], rec["lit_regen"])
            for q_ll, xl, xm, oc in rec["reads"]:
                if q_ll < 0:
                    continue
                pa = base + rec["at"] + (q_ll >> 3)
                sh = (pa & 3) * 8 + (q_ll & 7)
                cov["pairs"][kind].add((pa & 3, q_ll & 7))
                cov["so"][kind].add(xl + xm)
                cov["sh"][kind].add(sh)
                cov["field_bits"][kind] = max(cov["field_bits"][kind], xl + xm + oc)
                if sh == 31:
                    cov["field_bits_at_sh31"][kind] = max(cov["field_bits_at_sh31"][kind], xl + xm + oc)
            if name == "ring_hi_offsets":
                cov["hi_residues16"].add(rec["at"] % 16)
        if name == "ring_mod":
            rec, L = META[name]["ss"][0], META[name]["frame_len"]
            assert rec["end"] - rec["at"] > RING
            cov["residues"] = {(k * L) % RING for k in range(RING_COPIES)}      # relative to the first copy's stream start (and top)
    return cov
