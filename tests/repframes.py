"""Frames built from chosen repeat codes (test helper, no tests): the symbolic offset history of zg_k_seqpost (8 sequences per
thread stepped directly, wave shuffles, the wave maps through LDS, the carry from one pass to the next), of zg_k_scan (blocks per
thread, wave scan, cross-wave maps, the carry from one chunk of blocks to the next) and zg_sym_resolve in every executor, on
frames no encoder emits: blocks of repeat codes only, runs of "repeat offset 1 minus one", repeat codes that read what was set
blocks earlier at the scan's edges, frames of more blocks than one chunk, offsets that become 0 only across a block boundary.

The reference is plain Python: step() is the history rule of RFC 8878 3.1.1.5, the plaintext is seqframes.lz77 of the distances
it gives. The generator (_Gen) tracks history and position itself, so that a valid frame never reaches offset 0 or an offset
beyond the bytes produced. Frames are written by tabframes.build, which checks every valid one against the oracle and libzstd
(LIBZSTD_DIFFERS: the frames libzstd treats differently; none so far). META[name] holds what the Python model knows of a frame:
the history at every block start, every block's map in symbolic form, which blocks open with a sequence that depends on older
blocks; coverage() reads it. The sizes the families aim at come out of the kernel sources (kernel_constants)."""
import itertools
import os
import random
import re

import framesuite
import oracle
import seqframes
import tabframes
from tabframes import STATUS, Block

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "zstd-rs_amd", "csrc")

LIBZSTD_DIFFERS = {}
META = {}
GOOD = {}          # invalid frames: the plaintext of the blocks in front of the one that fails


def kernel_constants():
    """zg_k_seqpost's threads and sequences per thread, and zg_launch_scan's forms [(largest nblocks or None, T, I)], read out of
    zg_kernels.hip so that a retune moves the frames"""
    src = os.path.join(_CSRC, "zg_kernels.hip")
    out = framesuite.defines(src, ("ZG_SP_T", "ZG_SP_S"))
    text = open(src).read()
    body = text[text.index("void zg_launch_scan("):]
    body = body[:body.index("zg_k_scanf")]
    forms = re.findall(r"(?:max_frame_blocks <= (\d+)u\) )?hipLaunchKernelGGL\(\(zg_k_scan<(\d+), (\d+)>\)", body)
    assert len(forms) == 3 and forms[0][0] and forms[1][0] and not forms[2][0], "zg_launch_scan has another form: tests/repframes.py reads it"
    out["SCAN"] = [(int(a) if a else None, int(t), int(i)) for a, t, i in forms]
    return out


K = kernel_constants()
S = K["ZG_SP_S"]                       # 8: sequences a thread steps directly
WAVE = 64 * S                          # 512: sequences of a wave
PASS = K["ZG_SP_T"] * S                # 2048: sequences of a pass
SCAN_I = K["SCAN"][2][2]               # 8: blocks a thread of the chunked scan composes
CHUNK = K["SCAN"][2][1] * SCAN_I       # 8192: blocks of a chunk
SCAN_LIMITS = (K["SCAN"][0][0], K["SCAN"][1][0], CHUNK)           # 64, 1024, 8192: nblocks at which the scan changes form
NSEQ = sorted({1, 2 * PASS + 1} | {m + d for m in (S, 2 * S, WAVE, PASS) for d in (-1, 0, 1)})
CHAIN = sorted({1, 2} | {m + d for m in (S, WAVE, PASS) for d in (-1, 0, 1)})
NBLOCKS = sorted({1, 2, CHUNK + 8, 2 * CHUNK + 1} | {m + d for m in SCAN_LIMITS for d in (-1, 0, 1)})
EDGES = (SCAN_I, 64, 64 * SCAN_I, CHUNK)                          # a thread's, a wave's (one and SCAN_I blocks per thread), a chunk's blocks
BAD_AT = (1, SCAN_I, 64 * SCAN_I, CHUNK, CHUNK + 1, CHUNK + 7)


# ---- the reference ----------------------------------------------------------------------------------------------------------

def eff(ll, ov):
    """the repeat code as if literals were present: 1 .. 3 the slots, 4 "slot 0 minus one"; 0 for a new offset"""
    return 0 if ov > 3 else ov + (ll == 0)


def step(h, ll, ov):
    """RFC 8878 3.1.1.5: (distance, history behind the sequence)"""
    c = eff(ll, ov)
    if c == 0:
        return ov - 3, [ov - 3, h[0], h[1]]
    if c == 1:
        return h[0], list(h)
    if c == 2:
        return h[1], [h[1], h[0], h[2]]
    if c == 3:
        return h[2], [h[2], h[0], h[1]]
    return h[0] - 1, [h[0] - 1, h[0], h[1]]


def sym_step(m, ll, ov):
    """the same on symbolic slots: (0, value) a constant, (t, k) slot t - 1 of the history in front of the block, minus k"""
    c = eff(ll, ov)
    if c == 0:
        return [(0, ov - 3), m[0], m[1]]
    if c == 1:
        return list(m)
    if c == 2:
        return [m[1], m[0], m[2]]
    if c == 3:
        return [m[2], m[0], m[1]]
    t, v = m[0]
    return [(0, v - 1) if t == 0 else (t, v + 1), m[0], m[1]]


IDENT = [(1, 0), (2, 0), (3, 0)]


def encode(c, rng, of_codes=(0, 1)):
    """an effective repeat code as (ll, offset_value); of_codes: the offset codes the block's table has (0: value 1, 1: values 2, 3)"""
    forms = {1: [(1, 1)], 2: [(1, 2), (0, 1)], 3: [(1, 3), (0, 2)], 4: [(0, 3)]}[c]
    forms = [f for f in forms if (0 if f[1] == 1 else 1) in of_codes]
    assert forms, (c, of_codes)
    ll, ov = rng.choice(forms)
    return (rng.randint(1, 2) if ll else 0), ov


# ---- the generator ----------------------------------------------------------------------------------------------------------

class _Gen:
    def __init__(self, name, seed):
        self.name, self.rng = name, random.Random(seed)
        self.blocks, self.hist, self.pos = [], [1, 4, 8], 0
        self.made = [-2, -2, -2]             # the block in which each slot's value was made (a new offset or a decrement); -2: the frame's initial history
        self.lits, self.seqs, self.pending = bytearray(), [], 0
        self.meta = {"hist_at": [], "maps": [], "pairs": set(), "deps": set(), "dep_open": set(), "bad_block": None, "of_modes": set()}

    def _start(self):
        self.meta["hist_at"].append(list(self.hist))

    def raw(self, n):
        self._start()
        data = self.rng.randbytes(n)
        self.blocks.append(("raw", data))
        self.lits += data
        self.pending += n
        self.pos += n

    def rle(self, n):
        self._start()
        byte = self.rng.randrange(256)
        self.blocks.append(("rle", byte, n))
        self.lits += bytes([byte]) * n
        self.pending += n
        self.pos += n

    def comp(self, seqs, of=("pre",), tail=None, bad=False):
        """a compressed block of raw literals and the sequences [(ll, offset_value, ml)]. bad: the block is meant to fail; nothing
        is tracked behind it"""
        self._start()
        bi = len(self.blocks)
        tail = self.rng.randint(0, 3) if tail is None else tail
        lits = self.rng.randbytes(sum(s[0] for s in seqs) + tail)
        self.blocks.append(Block(lits, list(seqs), of=of))
        self.meta["of_modes"].add(of[0])
        if bad:
            self.meta["bad_block"] = bi
            return
        m, placed = list(IDENT), [-1, -1, -1]
        for i, (ll, ov, ml) in enumerate(seqs):
            c = eff(ll, ov)
            self.pos += ll
            d, self.hist = step(self.hist, ll, ov)
            assert 1 <= d <= self.pos, (self.name, bi, i, d, self.pos)
            self.pos += ml
            self.seqs.append((ll + (self.pending if i == 0 else 0), d, ml))
            m = sym_step(m, ll, ov)
            if c:
                self.meta["pairs"].add((i % S, c))
                slot = 0 if c == 4 else c - 1
                j = placed[slot]
                if j >= 0:
                    for kind, width in (("thread", S), ("wave", WAVE), ("pass", PASS)):
                        if i // width != j // width:
                            self.meta["deps"].add((kind, i - j))
                if i == 0 and self.made[slot] <= bi - 2:
                    self.meta["dep_open"].add(bi)
            if c in (0, 4):
                self.made = [bi, self.made[0], self.made[1]]
                placed = [i, placed[0], placed[1]]
            elif c == 2:
                self.made = [self.made[1], self.made[0], self.made[2]]
                placed = [i, placed[0], placed[2]]
            elif c == 3:
                self.made = [self.made[2], self.made[0], self.made[1]]
                placed = [i, placed[0], placed[1]]
        if seqs:
            self.pending = 0
            self.meta["maps"].append(m)
        self.lits += lits
        self.pending += len(lits) - sum(s[0] for s in seqs)
        self.pos += tail

    # ---- block kinds ----
    def new_offsets(self, offs, of=("pre",)):
        """a block that sets the given offsets with new-offset sequences, the last one ends in slot 0"""
        self.comp([(self.rng.randint(1, 2), d + 3, self.rng.randint(3, 6)) for d in offs], of=of)

    def pick_new(self, n, hi=250):
        return [self.rng.randint(2, max(2, min(self.pos, hi))) for _ in range(n)]

    def rand_rep(self, n, allow4=True, of=("pre",), of_codes=(0, 1)):
        """n repeat codes, each chosen among those that are valid where it stands"""
        seqs, h, pos = [], list(self.hist), self.pos
        for i in range(n):
            ok = []
            for c in (1, 2, 3, 4):
                if c == 4 and (not allow4 or h[0] < 6):
                    continue
                for ll, ov in {1: [(1, 1)], 2: [(1, 2), (0, 1)], 3: [(1, 3), (0, 2)], 4: [(0, 3)]}[c]:
                    if (0 if ov == 1 else 1) not in of_codes:
                        continue
                    ll = self.rng.randint(1, 2) if ll else 0
                    d, _ = step(h, ll, ov)
                    if 1 <= d <= pos + ll:
                        ok.append((ll, ov))
            assert ok, (self.name, len(self.blocks), h, pos)
            ll, ov = self.rng.choice(ok)
            ml = self.rng.randint(3, 6)
            _, h = step(h, ll, ov)
            pos += ll + ml
            seqs.append((ll, ov, ml))
        self.comp(seqs, of=of)

    def use_all(self):
        """a closing block that reads each slot once, so that the history behind the block in front shows in the bytes"""
        self.comp([(1, 1, 3), (2, 2, 4), (1, 3, 5), (1, 1, 3)])

    def finish(self, valid=True):
        name, z, plain = tabframes.build(self.name, self.blocks, valid=valid, differs=LIBZSTD_DIFFERS)
        self.meta["nblocks"] = len(self.blocks)
        self.meta["hist_end"] = list(self.hist)
        META[name] = self.meta
        mine = seqframes.lz77(self.seqs, bytes(self.lits)) if valid else None
        if valid:
            assert plain == mine, (name, "the model's plaintext differs from the writer's")
        else:                                            # what the model produced in front of the failing block must be what the oracle holds
            k = self.meta["bad_block"]
            # (the flat lists hold the good blocks only: comp(bad=True) adds nothing)
            GOOD[name] = seqframes.lz77(self.seqs, bytes(self.lits))
            d = oracle.FrameDecoder()
            st, c, _, _ = d.init(z)
            assert st == 0
            st, _, _ = d.decode_blocks(z[c:], oracle.STRAT_ALL)
            assert st == STATUS[name] and d.blocks_decoded() == k, (name, st, d.blocks_decoded(), k)
            assert d.held()[:len(GOOD[name])] == GOOD[name], (name, "the oracle holds other bytes for the good blocks")
        return name, z, plain


# ---- the families: each returns [(name, zst, plaintext or None)] ------------------------------------------------------------

PERIODS = {3: [2, 3, 4], 5: [3, 1, 4, 2, 3], 7: [4, 2, 3, 1, 3, 2, 4]}
OF_REP_FSE = ("fse", 5, [12, 20])                 # an offset table of the two codes the repeat offsets have


def _perm_frame(name, seed, codes, of=("pre",), of_codes=(0, 1)):
    g = _Gen(name, seed)
    dec = sum(c == 4 for c in codes)
    g.raw(dec + 120)
    g.new_offsets([dec + 90, dec + 40, dec + 3])      # three distinct offsets, none of which a run of decrements can bring to 0
    g.comp([encode(c, g.rng, of_codes) + (g.rng.randint(3, 6),) for c in codes], of=of)
    g.use_all()
    return g.finish()


def perm_blocks():
    """zg_k_seqpost: a block that sets three distinct offsets, then a block of repeat codes only of 1 .. 2 * PASS + 1 sequences around
    S, 2 S, WAVE and PASS; code strings of periods 3, 5 and 7 (coprime to S: every code at every index mod S, every "repeats what
    i - 1 / i - 2 / i - 3 put in front" across a thread, a wave and a pass boundary); the identity (code 1 with literals) and pure
    slot swaps (codes 2 and 3 only: the block's map is a permutation of the three symbols); RLE and FSE offset tables"""
    out = []
    for n in NSEQ:
        for p, pat in PERIODS.items():
            out.append(_perm_frame("perm_n%d_p%d" % (n, p), 1000 * n + p, [pat[i % p] for i in range(n)]))
    for n in (S + 1, WAVE + 1, PASS + 1):
        rng = random.Random(n)
        out.append(_perm_frame("perm_n%d_identity" % n, 11 * n, [1] * n))
        out.append(_perm_frame("perm_n%d_identity_of_rle" % n, 12 * n, [1] * n, of=("rle", 0), of_codes=(0,)))
        out.append(_perm_frame("perm_n%d_swaps" % n, 13 * n, [rng.choice((2, 3)) for _ in range(n)]))
        out.append(_perm_frame("perm_n%d_swaps_of_rle" % n, 14 * n, [rng.choice((2, 3)) for _ in range(n)], of=("rle", 1), of_codes=(1,)))
        out.append(_perm_frame("perm_n%d_p7_of_fse" % n, 15 * n, [PERIODS[7][i % 7] for i in range(n)], of=OF_REP_FSE))
    return out


def _chain(g, n, pre=None, post=(), of=("pre",)):
    """n times LL 0 with repeat code 3, behind an optional swap (code 2 or 3 with literals: the run then decrements what was in slot
    1 or 2) and in front of swaps that move the decremented values on"""
    seqs = [(1, pre, 3)] if pre else []
    seqs += [(0, 3, g.rng.randint(3, 4)) for _ in range(n)]
    seqs += [(1, c, 3) for c in post]
    g.comp(seqs, of=of)


def dec_chains():
    """LL 0 with repeat code 3, n times in a row, n around S, WAVE and PASS: from an offset of n + 1 set in the block in front (the
    map ends in "slot 0 minus n" and the last distance is 1), from an offset set in the same block (constants), behind a swap
    (slots 1 and 2 minus n: tags 2 and 3 with k > 1), in front of swaps, and two or three such blocks in a row (compose adds the k)"""
    out = []
    for n in CHAIN:
        for pre in (None, 2, 3):
            g = _Gen("dec_n%d_%s" % (n, "slot%d" % (pre - 1) if pre else "prev"), 2000 * n + (pre or 0))
            g.raw(n + 60)
            g.new_offsets([n + 1 + (pre == 3) * 8, n + 1 + (pre == 2) * 5, n + 1] if pre else [n + 30, n + 20, n + 1])
            _chain(g, n, pre, post=() if pre is None else (2,) if pre == 2 else (3, 2))
            g.use_all()
            out.append(g.finish())
        g = _Gen("dec_n%d_same_block" % n, 2000 * n + 7)
        g.raw(n + 60)
        g.new_offsets([n + 30, n + 20, n + 10])
        g.comp([(2, n + 1 + 3, 3)] + [(0, 3, 3)] * n + [(1, 2, 3), (1, 3, 3)])
        g.use_all()
        out.append(g.finish())
    for runs, pre, of in (((S - 1, S + 1), None, ("pre",)), ((WAVE - 1, 2), 2, ("pre",)), ((WAVE, WAVE + 1, S), 3, ("rle", 1)),
                          ((PASS, PASS + 1), None, OF_REP_FSE), ((PASS + 1, 1, WAVE), 2, ("pre",))):
        tot = sum(runs)
        g = _Gen("dec_rows_%s_%s" % ("_".join(map(str, runs)), "slot%d" % (pre - 1) if pre else "prev"), 3000 + tot)
        g.raw(tot + 60)
        g.new_offsets([tot + 9, tot + 5, tot + 1] if not pre else [tot + 1 + (pre == 3) * 8, tot + 1 + (pre == 2) * 5, tot + 1])
        for k, n in enumerate(runs):
            _chain(g, n, pre if k == 0 else None, of=of)     # (the swap in front has offset_value 2 or 3: the RLE table's code 1)
        g.use_all()
        out.append(g.finish())
    return out


def _kind(g, kind, of=("pre",)):
    if kind == "one":                                    # exactly one new offset: one constant slot, two symbolic
        g.comp([(1, 1, 3), (2, g.pick_new(1)[0] + 3, 4), (1, 1, 3)])
    elif kind == "two":                                  # exactly two: two constants, one symbolic
        a, b = g.pick_new(2)
        g.comp([(1, a + 3, 3), (1, 1, 4), (2, b + 3, 3)])
    elif kind == "three":
        g.new_offsets(g.pick_new(3))
    elif kind == "perm":
        g.rand_rep(g.rng.randint(1, 5), of=of)
    elif kind == "raw":
        g.raw(g.rng.randint(1, 4))
    elif kind == "rle":
        g.rle(g.rng.randint(1, 4))
    elif kind == "noseq":
        g.comp([], tail=g.rng.randint(1, 3))
    else:
        raise ValueError(kind)


def mixed_maps():
    """zg_k_scan's compose on maps of constant and symbolic slots: blocks with exactly one and exactly two new offsets in every order
    before and after blocks of repeat codes only, with raw, RLE and zero-sequence compressed blocks (identity maps) between them"""
    out = []
    for order in itertools.permutations(("one", "two", "perm")):
        for v, of in enumerate((("pre",), OF_REP_FSE)):
            g = _Gen("mixed_%s%s" % ("_".join(order), "_of_fse" if v else ""), 4000 + v + sum(map(ord, "".join(order))))
            g.raw(200)
            g.new_offsets([77, 150, 31])
            for rep in range(3):
                for kind, sep in zip(order, ("raw", "rle", "noseq") if rep != 1 else ("noseq", "raw", "rle")):
                    _kind(g, kind, of=of if kind == "perm" else ("pre",))
                    if rep:
                        _kind(g, sep)
                g.rand_rep(3, of=of)
            g.use_all()
            out.append(g.finish())
    return out


def initial_history():
    """the frame's initial history 1, 4, 8 read by repeat codes before any new offset, in the first block, behind a raw and behind an
    RLE block; the second block goes on permuting it"""
    out = []
    for lead in ("first", "raw", "rle"):
        for v, of in enumerate((("pre",), ("rle", 1))):
            g = _Gen("initial_%s%s" % (lead, "_of_rle" if v else ""), 5000 + v + len(lead))
            if lead == "raw":
                g.raw(5)
            if lead == "rle":
                g.rle(3)
            if v == 0:
                g.comp([(10, 1, 4), (2, 2, 3), (1, 3, 5), (0, 3, 3), (0, 1, 3), (1, 3, 4)])    # distances 1, 4, 8, 7, 8, 4
            else:
                g.comp([(10, 3, 4), (2, 2, 3), (0, 2, 5), (0, 3, 3)], of=of)                   # 8, 1, 4, 3
            g.rand_rep(S + 1, of=of, of_codes=(0, 1) if v == 0 else (1,))
            g.new_offsets(g.pick_new(1))
            g.use_all()
            out.append(g.finish())
    return out


def _edge(i):
    """is block i one of those that must open with a history-dependent sequence: a multiple of an edge, the one before, the one after"""
    return any(i % m in (0, 1, m - 1) for m in EDGES)


def _scan_frame(name, n, seed):
    g = _Gen(name, seed)
    for i in range(n):
        near = i % SCAN_I in (0, 1, SCAN_I - 1)          # (every other edge is a multiple of SCAN_I)
        if i == 0:
            g.comp([(9, 3, 4), (1, 2, 3)])               # the initial 8, then 1
        elif near:
            g.rand_rep(g.rng.randint(1, 3), allow4=False)
        elif i % SCAN_I == SCAN_I - 2:                   # nothing new right in front of an edge block: what that reads is two blocks old
            _kind(g, g.rng.choice(("raw", "rle", "noseq")))
        else:
            _kind(g, g.rng.choice(("raw", "raw", "rle", "noseq", "one", "one", "two", "three", "perm")))
    return g.finish()


def scan_edges():
    """zg_k_scan: frames of 1 block to two chunks and one, around the sizes at which zg_launch_scan changes the kernel form, built
    from the block kinds above; a repeat code whose value is two or more blocks old opens every block at a multiple of a thread's,
    a wave's and a chunk's blocks, the block before and the block after"""
    return [_scan_frame("scan_%d" % n, n, 6000 + n) for n in NBLOCKS]


def _filler(g, i):
    if i % 16 == 5:
        g.comp([(1, 1, 3)])
    else:
        _kind(g, ("raw", "rle", "noseq", "raw")[i % 4])


def invalid():
    """frames the oracle refuses: an offset that becomes 0 only across a block boundary (the block in front leaves rep0 = 1, the next
    opens with LL 0 and repeat code 3, or does so behind 2048 good sequences) at the scan's edges; the same inside one block; on
    the frame's initial rep0 = 1; a repeat of an offset larger than the bytes produced so far; a zero offset behind such a repeat"""
    out = []
    for at in BAD_AT:
        for behind in (0, PASS):
            g = _Gen("bad_zero_across_block_%d_seq%d" % (at, behind), 7000 + at + behind)
            if at > 1:
                g.raw(40)
            for i in range(1, at - 1):
                _filler(g, i)
            g.comp([(9, 5 + 3, 3), (2, 1 + 3, 3)])                           # the block in front leaves 1, 5
            good = []
            for k in range(behind // 4):                                     # swap twice, stay, stay: rep0 is 1 again
                good += [(1, 2, 3), (0, 1, 3), (1, 1, 3), (2, 1, 4)]
            g.comp(good + [(0, 3, 3), (1, 1, 3)], bad=True)
            for i in range(at + 1, max(at + 1, CHUNK + 8 if at >= CHUNK else at + 3)):
                g.blocks.append(("raw", b"zz"))
            out.append(g.finish(valid=False))
    g = _Gen("bad_zero_in_block", 7101)
    g.raw(20)
    g.comp([(1, 1 + 3, 3), (0, 3, 3)], bad=True)
    out.append(g.finish(valid=False))
    g = _Gen("bad_zero_on_initial_history", 7102)
    g.comp([(0, 3, 3)], tail=4, bad=True)
    out.append(g.finish(valid=False))
    g = _Gen("bad_repeat_out_of_reach", 7103)
    g.comp([(5, 3, 3)], bad=True)                                             # the initial 8 with 5 bytes produced
    out.append(g.finish(valid=False))
    g = _Gen("bad_repeat_out_of_reach_second_block", 7104)
    g.raw(2)
    g.comp([(1, 2, 3)], bad=True)                                             # the initial 4 with 3 bytes produced
    out.append(g.finish(valid=False))
    g = _Gen("bad_zero_behind_out_of_reach", 7105)
    g.raw(3)
    g.comp([(1, 3, 3), (1, 1 + 3, 3), (0, 3, 3)], bad=True)                   # the initial 8 with 4 bytes produced, then 1, then 1 - 1
    out.append(g.finish(valid=False))
    return out


FAMILIES = {
    "perm_blocks": perm_blocks,
    "dec_chains": dec_chains,
    "mixed_maps": mixed_maps,
    "initial_history": initial_history,
    "scan_edges": scan_edges,
    "invalid": invalid,
}

_F = framesuite.Families(FAMILIES)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


def big(name):
    """the frames of more blocks than one chunk of zg_k_scan"""
    return META[name]["nblocks"] > CHUNK


def coverage(frames):
    """what the frames reach, from the Python model (META): frames is all_frames()'s list. Every valid frame counts"""
    cov = {"valid": 0, "invalid": 0, "per_family": {}, "pairs": set(), "deps": set(), "max_k": {1: 0, 2: 0, 3: 0}, "shapes": set(),
           "permutations": set(), "nblocks": set(), "edges_missing": [], "edges_open": 0, "statuses": set(), "bad_blocks": set(),
           "of_modes": {}, "run_k": {1: set(), 2: set(), 3: set()}}
    for fam, name, _, plain in frames:
        m = META[name]
        cov["per_family"][fam] = cov["per_family"].get(fam, 0) + 1
        if plain is None:
            cov["invalid"] += 1
            cov["statuses"].add(STATUS[name])
            cov["bad_blocks"].add(m["bad_block"])
            continue
        cov["valid"] += 1
        cov["pairs"] |= m["pairs"]
        cov["deps"] |= m["deps"]
        cov["of_modes"].setdefault(fam, set()).update(m["of_modes"])
        for mp in m["maps"]:
            nsym = sum(t != 0 for t, _ in mp)
            cov["shapes"].add(nsym)
            for t, k in mp:
                if t:
                    cov["max_k"][t] = max(cov["max_k"][t], k)
            for slot, (t, k) in enumerate(mp):
                if t and (slot == 0 or t != 1):             # tag 1: where the issue's run ends, slot 0; tags 2 and 3: wherever the swaps left the run
                    cov["run_k"][t].add(k)
            if nsym == 3 and all(k == 0 for _, k in mp):
                cov["permutations"].add(tuple(t for t, _ in mp))
        if fam == "scan_edges":
            cov["nblocks"].add(m["nblocks"])
            want = [i for i in range(m["nblocks"]) if _edge(i)]
            cov["edges_open"] += len(want)
            cov["edges_missing"] += [(name, i) for i in want if i not in m["dep_open"]]
    return cov
