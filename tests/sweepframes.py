"""Frames built at the edges of zg_k_sweep and the split sweep (test helper, no tests): zg_sweep_body and zg_launch_sweep in
zg_kernels.hip exist only as HIP (the CPU harness resolves the scratch with a plain serial model, tests/emu/zg_emu_flat.cpp), so
these frames are what aims at them. They come from tabframes.build: raw literals, predefined FSE tables, the window log a
parameter; the plaintext is seqframes.lz77 of the sequences asked for, checked there against the oracle and libzstd (except the
names of SWEEP_LIBZSTD_DIFFERS). Every frame is (name, zst, plaintext).

What the layout rests on, each read out of the source by constants() and asserted by tests/test_sweepframes_cpu.py from the
harness's plan (emu.Plan: the same BatchBuilder::finish, flat_slots 256):
  * a batch is ZG_SW_BATCH = 4 * ZG_SW_T * ZG_SW_B = 2048 bytes of a unit (zg_kernels.h);
  * BatchBuilder::finish (zg_host_parse.cpp) never plans fewer than 4 blocks per unit (`if (ub < 4) ub = 4;`, `if (ubf < 4) ubf = 4;`),
    and a frame's own share is ubf = ceil(ub * blocks with sequences / blocks). Every unit here is four blocks: its program in one
    to four blocks with sequences, empty Raw blocks for the rest. A frame's first unit is direct (resolved to bytes by zg_flat4.h,
    no step) while the frame has at most direct_max_units = 32 units (zg_host_parse.h); every later unit with a sequence is a
    pointer-mode unit with a sweep step of its own;
  * a frame goes to zg_k_sparse, and has no step at all, when it has at most sparse_max = 2048 sequences and at most
    sparse_per_block = 4 per block (zg_host_parse.h); every frame here but mx_sparse stays off it by filler sequences in its
    first unit;
  * the sweep is split when window_max / 2048 + 2 batches plus 65536 bytes are less than unit_blocks_used * 131072
    (zg_launch_sweep): with units of four blocks, for windows up to 256 KiB. The heads of `group` = 16 steps share a launch
    (ZgSweepTuning, zg_kernels.h), and Batch::launch_sweep hands over 80 events, two of them not for groups, so more than
    78 * 16 steps raise the group to 17.

The families, each with the lines it aims at:
  groups        the value selection of a 4-byte group: `nD` / `nB` / `nC` (one gather per distinct effective offset), `sw` / `sy` / `sz`
                (which gather a byte takes), the byte masks of `v`, and `fun` (alignbit by ((lowb - e) & 3) * 8). The key of a group
                is (which bytes have e != 0, which of those e are equal): 52 on paper, KEYS the 44 a frame can hold (IMPOSSIBLE:
                the 8 with a run of one or two match bytes between literals inside the group, since Match_Length >= 3). A seeded
                search over unit-local programs (LL 0 .. 3, ML 3 .. 7, offsets 1 .. 8, to earlier bytes of the unit, in front of the
                unit; e by parent chasing, e(x) = off + e(x - off)) picks units until all are there but the one of four literals; every unit is a multiple of 4
                long and the frames groups_r0 .. r3 start them at output residues 0 .. 3 (`lowb`) by 0 .. 3 extra bytes in the
                direct unit. A unit written by hand adds the group of four literals, e = 1 .. 5, an e that lands on the last byte in front of the unit and one on
                the frame's first byte; groups_far (window log 21, two units of Raw blocks) one e above 2^20. Sources are random
                literals, so a wrong lane is a wrong byte.
  unit_ends     the end of a unit: `if (... (size & 3u) && n4 >= b0 * BG && n4 < (b0 + nbatch) * BG && t < (size & 3u))` (the byte tail,
                by "the workgroup that would hold their group"), `g < n4` in load_og and the batch that ends inside a group
                (`nb_all = (n4 + BG - 1) / BG`). Units of SMALL_SIZES and of 2048 k + r bytes, k 1 and 2, r -4 .. 4, once in the middle of
                the frame (the unit behind starts unaligned and copies the last three bytes) and once as its last unit; the last
                bytes are literals, the end of a match from in front of the unit, or the end of a match whose source is a literal
                of the unit (ENDS). A unit of 1 or 2 bytes cannot hold a match (Match_Length >= 3): it is a unit without
                sequences and has no step; 3 bytes are one match.
  tails_heads   `sd.head = sd.size > w ? (sd.size - w) / 2048 : 0`, `b0 = blockIdx.x * nbatch + (part == 1 ? sd.head : 0)`,
                `if (part == 2u && b0 >= sd.head) return;` and the grids of zg_launch_sweep (tails: window_max / 2048 + 2 batches and
                one workgroup more, heads: slices - window_min / 2048). Window logs 10 and 11; units of W + d bytes, d of HEAD_EDGES,
                so that head is 0, 1 and 2 batches on both sides of each step; a unit of 1 byte, one of W - 1 bytes and one of Raw
                blocks between long ones. Every unit is a relay: all its bytes but a few fresh literals are matches whose sources
                lie in the last W bytes in front of the unit (its tail directly, its head directly or through the unit's own
                earlier bytes), so a step that runs early or a head launched before the tail it reads leaves other bytes. In every
                unit a match of offset exactly W (or W - 1: the frames *_wm1) starts at the unit's first byte, at its last head
                byte (frames *_lh) or first tail byte (*_ft), and one ends at its last byte.
  head_groups   `gs`, `need()` and the event indices of zg_launch_sweep: relay frames of 15, 16, 17, 18 and 33 pointer-mode units (the
                16 steps whose heads share a launch) and hg_big with 78 * 16 + 2, where gs becomes 17. Every unit is W + 2048 bytes
                or a little more and starts with a match of offset W: a head byte that reads the tail of the step in front. hg_33 and
                hg_big have more than direct_max_units units, so their first unit is a pointer-mode unit too and is counted.
  mixed         submits (submits()): windows of 1, 128 and 256 KiB together (`window_max` sizes the tail grids, `window_min` the head
                grids, sd.head is per frame), the same with a frame that declares 1 MiB (no split), frames of 1, 2, 3 and 9
                pointer-mode units (the step lists shrink), a sparse frame and a frame of one block among them.
  beyond_window two frames that differ in one offset, W and W + 1 for W of 1 KiB: the match is the first of a head and reads the last
                head byte of the unit in front, the one read the split does not order. zg_k_seqpost reports it (`far`), Batch::sync
                repeats the sweep as a plain chain (sweep_mode 2)."""
import functools
import os
import random
import re

import framesuite
import tabframes
from tabframes import Block

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zstd-rs_amd", "csrc")

# valid frames libzstd does not return the plaintext for, each with its reason
SWEEP_LIBZSTD_DIFFERS = {
}


@functools.lru_cache(None)
def constants():
    """what the layout takes from the source: {batch, min_unit_blocks, sparse_max, sparse_per_block, direct_max_units, group, events}"""
    k = framesuite.defines(os.path.join(_CSRC, "zg_kernels.h"), ("ZG_SW_T", "ZG_SW_B"))
    out = {"batch": 4 * k["ZG_SW_T"] * k["ZG_SW_B"]}

    def grab(fname, pattern, what):
        m = re.search(pattern, open(os.path.join(_CSRC, fname)).read())
        assert m, "%s: %s has another form, tests/sweepframes.py relies on it" % (fname, what)
        return int(m.group(1))

    out["min_unit_blocks"] = grab("zg_host_parse.cpp", r"if \(ub < (\d+)\) ub = \1;", "the least blocks per unit")
    assert grab("zg_host_parse.cpp", r"if \(ubf < (\d+)\) ubf = \1;", "the least blocks per unit of a frame") == out["min_unit_blocks"]
    out["sparse_max"] = grab("zg_host_parse.h", r"uint32_t sparse_max = (\d+);", "sparse_max")
    out["sparse_per_block"] = grab("zg_host_parse.h", r"uint32_t sparse_per_block = (\d+);", "sparse_per_block")
    out["direct_max_units"] = grab("zg_host_parse.h", r"uint32_t direct_max_units = (\d+);", "direct_max_units")
    out["group"] = grab("zg_kernels.h", r"struct ZgSweepTuning \{[^}]*\bgroup = (\d+)", "the steps whose heads share a launch")
    out["events"] = grab("zg_engine.cpp", r"split \? (\d+)u : 0u", "the events handed to zg_launch_sweep")
    return out


BATCH = constants()["batch"]
UB = constants()["min_unit_blocks"]
BLOCK = 131072

# ---- the keys of a 4-byte group -------------------------------------------------------------------------------------------------


def group_key(e4):
    """(0 for a literal byte, else 1 + the index of the byte's e among the group's distinct nonzero e in order of appearance) x 4"""
    seen, out = [], []
    for e in e4:
        if e == 0:
            out.append(0)
        else:
            if e not in seen:
                seen.append(e)
            out.append(1 + seen.index(e))
    return tuple(out)


def _all_keys():
    keys = set()
    for a in range(5):
        for b in range(5):
            for c in range(5):
                for d in range(5):
                    keys.add(group_key((a, b, c, d)))
    return keys


def _impossible(key):
    """a run of one or two match bytes with a literal on both sides inside the group: no match is shorter than 3 bytes"""
    m = "".join("M" if k else "L" for k in key)
    return "LML" in m or m == "LMML"


IMPOSSIBLE = frozenset(k for k in _all_keys() if _impossible(k))
KEYS = frozenset(_all_keys() - IMPOSSIBLE)
assert len(_all_keys()) == 52 and len(IMPOSSIBLE) == 8 and len(KEYS) == 44


def loads_of(q):
    """which of the gathers A, B, C, D zg_sweep_body issues for a group with the effective offsets q = (x, y, z, w), and the e of each
    (`ux`, `nD`, `nB`, `nC`): one per distinct nonzero e, A for byte 0's, D for byte 3's, then B, then C"""
    x, y, z, w = q
    out = {}
    if x:
        out["A"] = x
    if w and not (x and w == x):
        out["D"] = w
    if y and not (x and y == x) and not (w and y == w):
        out["B"] = y
    if z and not (x and z == x) and not (w and z == w) and not (y and z == y):
        out["C"] = z
    return out


# ---- the layout -----------------------------------------------------------------------------------------------------------------

class Lay:
    """a frame laid out unit by unit (four blocks each) with its output positions known. units: [(start, size, kind)], kind "first",
    "ptr" or "noseq"; aims: [(what, position of the match, distance)]"""

    def __init__(self, seed, front=64, lead=0, fill=None, nunits=8):
        """the first unit: a block of `fill` short matches (a multiple of 4 bytes long), then front + lead random Raw bytes in the
        other blocks. fill None: enough for nunits units behind it to stay off zg_k_sparse whatever they hold"""
        c = constants()
        self.rng = rng = random.Random(seed)
        self.blocks, self.units, self.aims, self.pos, self.nseq = [], [], [], 0, 0
        if fill is None:
            fill = min(c["sparse_per_block"] * UB * (nunits + 1) + 8, c["sparse_max"] + 1)
        assert front % 4 == 0 and fill >= 1
        seqs, p = [], 0
        for i in range(fill):
            p += 1 if i else 8
            seqs.append((1 if i else 8, rng.randint(1, min(p, 512)) + 3, 3))       # (512: inside the smallest window)
            p += 3
        self.blocks.append(Block(rng.randbytes(8 + fill - 1 + 5), seqs))                 # 4 * fill + 12 bytes
        rest = front + lead
        for _ in range(UB - 1):
            n = min(rest, BLOCK) if len(self.blocks) < UB - 1 else rest
            self.blocks.append(("raw", rng.randbytes(n)))
            rest -= n
        assert rest == 0 and n <= BLOCK
        self.pos = p + 5 + front + lead
        self.nseq = fill
        self.units.append((0, self.pos, "first"))

    def unit(self, prog, tail=0, split=1):
        """a unit of the sequences prog [(ll, distance, ml)] and `tail` literals behind them, in `split` blocks with sequences"""
        rng, start, p = self.rng, self.pos, self.pos
        for ll, d, ml in prog:
            p += ll
            assert ml >= 3 and 1 <= d <= p, (ll, d, ml, p)
            p += ml
        split = max(1, min(split, UB, len(prog)))
        per = (len(prog) + split - 1) // split
        chunks = [prog[i:i + per] for i in range(0, len(prog), per)]
        for i, ch in enumerate(chunks):
            nl = sum(s[0] for s in ch) + (tail if i == len(chunks) - 1 else 0)
            self.blocks.append(Block(rng.randbytes(nl), [(ll, d + 3, ml) for ll, d, ml in ch]))
        self.blocks += [("raw", b"")] * (UB - len(chunks))
        self.nseq += len(prog)
        self.pos = p + tail
        self.units.append((start, self.pos - start, "ptr"))
        return start

    def raw_unit(self, sizes):
        """a unit of Raw blocks only: no sequences, no step"""
        sizes = list(sizes) + [0] * (UB - len(sizes))
        assert len(sizes) == UB
        self.blocks += [("raw", self.rng.randbytes(n)) for n in sizes]
        self.units.append((self.pos, sum(sizes), "noseq"))
        self.pos += sum(sizes)

    def build(self, name, window_log=17, pad4=False):
        c = constants()
        if pad4 and self.pos % 4:                        # the frame a multiple of 4 long: the frames behind it in a submit keep their residues
            assert self.blocks[-1] == ("raw", b"")
            n = 4 - self.pos % 4
            self.blocks[-1] = ("raw", self.rng.randbytes(n))
            s, size, kind = self.units[-1]
            self.units[-1] = (s, size + n, kind)
            self.pos += n
        assert len(self.blocks) == UB * len(self.units)
        assert self.nseq > c["sparse_max"] or self.nseq > c["sparse_per_block"] * len(self.blocks), (name, "would go to zg_k_sparse")
        r = tabframes.build(name, self.blocks, window_log=window_log, differs=SWEEP_LIBZSTD_DIFFERS)
        assert len(r[2]) == self.pos, name
        LAYOUT[name] = {"units": list(self.units), "aims": list(self.aims), "window": 1 << window_log}
        return r


LAYOUT = {}                                              # name -> what the generator meant: the units, the aimed matches, the window


def rand_prog(rng, size, reach, maxll=3, maxml=7):
    """a unit-local program of exactly `size` bytes: LL 0 .. maxll, ML 3 .. maxml, distances 1 .. 8, to earlier bytes of the unit, or up to
    `reach` bytes in front of the unit. Returns (prog, tail)"""
    prog, x = [], 0
    while size - x >= 3:
        r = size - x
        ll = rng.randint(0, min(maxll, r - 3))
        ml = rng.randint(3, min(maxml, r - ll))
        x += ll
        kind = rng.randrange(3)
        if kind == 0 and x + reach >= 1:
            d = rng.randint(1, min(8, x + reach))
        elif kind == 1 and x >= 1:
            d = rng.randint(1, x)
        else:
            d = x + rng.randint(1, reach)
        prog.append((ll, d, ml))
        x += ml
    return prog, size - x


def local_e(prog, tail):
    """the effective offsets of a unit-local program by parent chasing: e(x) = d + e(x - d) while x - d is a match byte of the unit"""
    e = []
    for ll, d, ml in prog:
        e += [0] * ll
        for _ in range(ml):
            x = len(e)
            e.append(d + (e[x - d] if x - d >= 0 else 0))
    return e + [0] * tail


def keys_of(e):
    return {group_key(e[g:g + 4]) for g in range(0, len(e) - 3, 4)}


@functools.lru_cache(None)
def key_programs():
    """programs of 96 bytes from a seeded search, kept while they add a key, until all of KEYS but the all-literal one are there"""
    rng = random.Random(4401)
    want = KEYS - {(0, 0, 0, 0)}                         # (four literals in a group: LL <= 3 here; the unit written by hand starts with them)
    have, kept = set(), []
    for _ in range(200000):
        prog, tail = rand_prog(rng, 96, 32)
        new = (keys_of(local_e(prog, tail)) & want) - have
        if new:
            have |= new
            kept.append((prog, tail))
            if have == want:
                return kept
    raise AssertionError(("the search misses", sorted(want - have)))


def _special(lay):
    """the unit written by hand: e = 1, 2, 3, 4 in one group (a match of distance 1 behind four literals), e = 5 from a literal, an e
    that lands on the last byte in front of the unit and one on the frame's first byte"""
    s = lay.pos
    prog = [(4, 1, 4), (6, 5, 3)]                        # x = 4 .. 7: e = 1 .. 4; x = 14 .. 16: e = 5
    prog.append((3, 20 + 1, 3))                          # x = 20: the last byte in front of the unit
    prog.append((1, s + 24, 3))                          # x = 24: the frame's first byte
    lay.aims += [("in_front", s + 20, 21), ("first_byte", s + 24, s + 24)]
    lay.unit(prog, 1)                                    # 28 bytes


def groups():
    out = []
    progs = key_programs()
    for r in range(4):
        lay = Lay(4410 + r, front=64, lead=r, nunits=len(progs) + 1)
        _special(lay)
        for i, (prog, tail) in enumerate(progs):
            lay.unit(prog, tail, split=1 + i % 3)
        out.append(lay.build("groups_r%d" % r, pad4=True))
    lay = Lay(4420, front=64, nunits=3)
    lay.raw_unit([BLOCK] * UB)
    lay.raw_unit([BLOCK] * UB)
    s = lay.pos
    prog, tail = rand_prog(lay.rng, 60, 32)
    far = s + 64 - (lay.units[0][1] - 40)                # into the random Raw bytes of the first unit
    assert far > 1 << 20
    lay.aims.append(("far", s + 64, far))
    lay.unit(prog + [(4 + tail, far, 8)], 0)
    out.append(lay.build("groups_far", window_log=21))
    return out


SMALL_SIZES = (1, 2, 3, 4, 5, 7, 8)
BIG_SIZES = tuple(BATCH * k + r for k in (1, 2) for r in range(-4, 5))
ENDS = ("lit", "front", "own")


def end_fits(n, end):
    """can a unit of n bytes end that way? 1 and 2 bytes hold no match at all, 3 bytes are one match with nothing in front of it"""
    if n < 3:
        return end == "lit"
    if n == 3:
        return end == "front"
    return True


def _end_unit(lay, n, end):
    """a unit of n bytes whose last bytes are literals ("lit": min(3, n - 3) of them), the end of a match from in front of the unit
    ("front") or the end of a match whose source is a literal of the unit ("own")"""
    rng = lay.rng
    if n < 3:
        lay.raw_unit([n])
        return
    if end == "lit":
        t = min(3, n - 3)
        prog, tail = rand_prog(rng, n - t, 32, maxml=24)
        lay.unit(prog, tail + t, split=2)
    elif end == "front":
        prog, tail = rand_prog(rng, n - 3, 32, maxml=24) if n > 3 else ([], 0)
        lay.unit(prog + [(tail, n - 3 + rng.randint(1, 32), 3)], 0, split=2)
    else:
        if n < 6:
            lay.unit([(n - 3, 1, 3)], 0)
        else:
            prog, tail = rand_prog(rng, n - 6, 32, maxml=24)
            lay.unit(prog + [(tail + 3, 3, 3)], 0, split=2)


def unit_ends():
    out = []
    for i, n in enumerate(SMALL_SIZES + BIG_SIZES):
        for end in ENDS:
            if not end_fits(n, end):
                continue
            lay = Lay(4500 + 3 * i + ENDS.index(end), front=64, lead=i % 4, nunits=3)
            _end_unit(lay, n, end)
            prog, tail = rand_prog(lay.rng, 37, 32)      # the unit behind: starts where that one ends, and copies its last 3 bytes
            lay.unit([(0, 3, 3)] + prog, tail) if n >= 3 else lay.unit(prog, tail)
            _end_unit(lay, n, end)
            out.append(lay.build("end_%d_%s" % (n, end)))
    return out


HEAD_EDGES = (-1, 0, 1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH, 2 * BATCH + 1)


def head_of(size, w):
    """the model of sd.head: whole batches of the unit in front of its last w bytes"""
    return (size - w) // BATCH if size > w else 0


def relay_prog(rng, size, w, aims, ml=(8, 48)):
    """a unit of `size` bytes that only passes on what lies in the last w bytes in front of it: matches with a distance of x + 1 .. w
    at unit position x < w (the source in front of the unit), of w / 2 .. w behind that (the source the unit's own earlier bytes), a
    fresh literal now and then; aims [(x, distance, ml)] are placed as they are. Returns (prog, tail)"""
    prog, x, ll = [], 0, 0
    for ax, ad, aml in sorted(aims) + [(size, None, 0)]:
        assert ax >= x, (ax, x)
        while x < ax:
            r = ax - x
            if r < 3:
                ll, x = ll + r, ax
                break
            if r >= 8 and rng.random() < 0.1:
                ll, x, r = ll + 1, x + 1, r - 1
            m = min(r, rng.randint(*ml))
            d = rng.randint(x + 1, w) if x < w else rng.randint(w // 2, w)
            prog.append((ll, d, m))
            ll, x = 0, x + m
        if ad is not None:
            prog.append((ll, ad, aml))
            ll, x = 0, x + aml
    return prog, ll


def _relay_unit(lay, size, w, dist, mid="lh", split=1, ml=(8, 48)):
    """a relay unit with matches of distance `dist` at its first byte, at its last head byte ("lh") or first tail byte ("ft") and
    ending at its last byte"""
    s, h = lay.pos, head_of(size, w)
    at = [0, size - 3]
    if h:
        at.append(h * BATCH - 1 if mid == "lh" else h * BATCH)
    at = sorted(set(a for a in at if a >= 0))
    aims = [(a, dist, 3) for i, a in enumerate(at) if i == 0 or a >= at[i - 1] + 3]
    names = {0: "first", size - 3: "last", h * BATCH - 1: "last_head", h * BATCH: "first_tail"} if h else {0: "first", size - 3: "last"}
    lay.aims += [(names[a], s + a, d) for a, d, _ in aims]
    prog, tail = relay_prog(lay.rng, size, w, aims, ml)
    lay.unit(prog, tail, split=split)


def tails_heads():
    out = []
    for wlog in (10, 11):
        w = 1 << wlog
        for dname, dist in (("w", w), ("wm1", w - 1)):
            for mid in ("lh", "ft"):
                lay = Lay(4600 + wlog * 8 + (dist != w) * 2 + (mid == "ft"), front=w + 64, nunits=14)
                e = HEAD_EDGES
                order = [e[0], e[1], e[2], e[3], "one", e[4], e[5], "wm1", e[6], "noseq", e[7], e[8], e[1]]
                for i, d in enumerate(order):
                    if d == "one":
                        lay.raw_unit([1])
                    elif d == "noseq":
                        lay.raw_unit([100, 0, 150, 50])
                    else:
                        _relay_unit(lay, w - 1 if d == "wm1" else w + d, w, dist, mid, split=1 + i % 4)
                out.append(lay.build("th_w%d_%s_%s" % (wlog, dname, mid), window_log=wlog))
    return out


HEAD_GROUP_UNITS = (15, 16, 17, 18, 33)


def big_units():
    c = constants()
    return (c["events"] - 2) * c["group"] + 2


def _relay_frame(name, seed, pointer_units, wlog=10, size=None, ml=(8, 48), split=None, dist=None, window_log=None):
    """a frame of `pointer_units` pointer-mode units, all relays of W + 2048 bytes or a little more (a head of one batch). A frame of
    more than direct_max_units units has no direct unit: its first unit is a pointer-mode unit as well"""
    w = 1 << wlog
    relays = pointer_units if pointer_units + 1 <= constants()["direct_max_units"] else pointer_units - 1
    lay = Lay(seed, front=w + 64, nunits=relays)
    for i in range(relays):
        _relay_unit(lay, (size or w + BATCH) + i % 3, w, dist or w, "lh" if i % 2 else "ft", split=split or 1 + i % 4, ml=ml)
    return lay.build(name, window_log=window_log or wlog)


def head_groups():
    return [_relay_frame("hg_%d" % n, 4700 + n, n) for n in HEAD_GROUP_UNITS]


@functools.lru_cache(None)
def head_groups_big():
    """the frame of 78 * 16 + 2 pointer-mode units, one block with sequences and three empty ones each (a frame's unit is
    ceil(ub * blocks with sequences / blocks) blocks, 4 at least: with a block with sequences in four the units stay at 4 blocks)"""
    return _relay_frame("hg_big", 4790, big_units(), ml=(200, 500), split=1)


def mixed():
    out = [_relay_frame("mx_w10", 4801, 3, 10, (1 << 10) + BATCH + 7)]
    out.append(_relay_frame("mx_w17", 4802, 3, 17, (1 << 17) + 2 * BATCH + 5, ml=(256, 2048), split=4))
    out.append(_relay_frame("mx_w18", 4803, 3, 18, (1 << 18) + BATCH + 3, ml=(256, 2048), split=4))
    out.append(_relay_frame("mx_w20", 4804, 3, 10, window_log=20))
    for n in (1, 2, 3, 9):
        out.append(_relay_frame("mx_p%d" % n, 4810 + n, n))
    rng = random.Random(4820)
    blocks = [Block(rng.randbytes(40), [(30, 20 + 3, 5), (2, 9 + 3, 4)])]
    for i in range(7):
        blocks += [("raw", rng.randbytes(300 + i)), Block(rng.randbytes(9), [(4, 200 + i + 3, 6 + i)])]
    out.append(tabframes.build("mx_sparse", blocks, window_log=10, differs=SWEEP_LIBZSTD_DIFFERS))
    seqs = [(2, rng.randint(1, 20) + 3, rng.randint(3, 9)) for _ in range(12)]
    out.append(tabframes.build("mx_one_block", [Block(rng.randbytes(20 + 2 * 12 + 5), [(20, 7 + 3, 4)] + seqs)], differs=SWEEP_LIBZSTD_DIFFERS))
    return out


def beyond_window():
    """[first][A: W + 2048 bytes][B: its first match of distance W (bw_w) or W + 1 (bw_w1), in its head][C]: W + 1 back from B's first
    byte lies A's byte W + 2047 - W = 2047, the last of A's head"""
    out = []
    w = 1 << 10
    for name, dist in (("bw_w", w), ("bw_w1", w + 1)):
        lay = Lay(4900, front=w + 64, nunits=3)
        _relay_unit(lay, w + BATCH, w, w, "ft", split=2)
        s = lay.pos
        prog, tail = relay_prog(lay.rng, w + BATCH + 9, w, [(0, dist, 3)])
        lay.aims.append(("beyond" if dist > w else "exact", s, dist))
        lay.unit(prog, tail, split=3)
        _relay_unit(lay, w + BATCH, w, w, "lh")
        out.append(lay.build(name, window_log=10))
    return out


FAMILIES = {
    "groups": groups,
    "unit_ends": unit_ends,
    "tails_heads": tails_heads,
    "head_groups": head_groups,
    "mixed": mixed,
    "beyond_window": beyond_window,
}


def _check_differs(frames):
    names = [n for _, n, _, p in frames]
    assert set(SWEEP_LIBZSTD_DIFFERS) <= set(names)
    assert len(SWEEP_LIBZSTD_DIFFERS) * 10 <= len(names), "SWEEP_LIBZSTD_DIFFERS holds more than a tenth of the frames"


_F = framesuite.Families(FAMILIES, _check_differs)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames
SMALL_FAMILIES = ("groups", "unit_ends", "tails_heads", "beyond_window")          # (whose frames the CPU tests also flatten on the emulator)


SUBMITS = ("groups", "groups_far", "unit_ends", "tails_heads", "head_groups", "mixed_windows", "mixed_windows_1m", "mixed_counts",
           "beyond_window_w", "beyond_window_w1", "beyond_window")


@functools.lru_cache(None)
def submits():
    """name -> (the sweep_mode() expected with no switch set, [(name, zst, plaintext)]): 0 a plain chain, 1 split into tails and
    heads, 2 split and repeated as a plain chain. The submits the GPU tests run and the CPU tests read the plan of"""
    by = {n: (n, z, p) for _, n, z, p in all_frames()}
    pick = lambda *names: [by[n] for n in names]         # noqa: E731
    out = {
        "groups": (1, [f for f in family("groups") if f[0] != "groups_far"]),
        "groups_far": (0, pick("groups_far")),
        "unit_ends": (1, family("unit_ends")),
        "tails_heads": (1, family("tails_heads")),
        "head_groups": (1, family("head_groups")),
        "mixed_windows": (1, pick("mx_w10", "mx_w17", "mx_w18")),
        "mixed_windows_1m": (0, pick("mx_w10", "mx_w17", "mx_w18", "mx_w20")),
        "mixed_counts": (1, pick("mx_p1", "mx_p2", "mx_sparse", "mx_p3", "mx_one_block", "mx_p9")),
        "beyond_window_w": (1, pick("bw_w")),
        "beyond_window_w1": (2, pick("bw_w1")),
        "beyond_window": (2, family("beyond_window")),
    }
    assert tuple(out) == SUBMITS
    return out


# ---- what the frames reach ------------------------------------------------------------------------------------------------------

def plan_of(frames, **kw):
    """the harness's plan of the frames in one submit (BatchBuilder::finish with flat_slots 256) as [(frame, out_base, [(first block in
    the frame, blocks, noseq)])] and the emu.Plan itself"""
    import emu
    plan = emu.Plan(b"".join(z for _, z, _ in frames), **kw)
    assert len(plan.frames) == len(frames)
    out, base = [], 0
    for f, (name, z, plain) in enumerate(frames):
        fb, nb, fu, nu = plan.frames[f][:4]
        units = [(plan.units[u][1] - fb, plan.units[u][2], plan.units[u][3]) for u in range(fu, fu + nu)]
        assert all(plan.units[u][0] == f for u in range(fu, fu + nu))
        out.append((f, base, units))
        base += len(plain)
    return out, plan


def coverage(frames):
    """the frames [(name, zst, plaintext)] as one submit, from the harness's plan and lz_model.expected_scratch on its units: per lowb
    (the output residue of a unit's first byte) the group keys reached, per load A .. D the shifts (lowb - e) & 3, the e values, the
    sizes of pointer-mode units, the (s - W, head) pairs, the pointer-mode units per frame, the sparse frames, whether every byte
    behind a frame's first unit that a match wrote lies in a pointer-mode unit; per frame the unit bounds and the e array"""
    import numpy as np
    import lz_model
    per_frame, plan = plan_of(frames)
    cov = {"keys": {r: set() for r in range(4)}, "shifts": {k: set() for k in "ABCD"}, "e": set(), "e_max": 0, "sizes": set(),
           "s_minus_w": set(), "pointer_units": {}, "sparse": [], "tail_sizes": set(), "frames": {}, "steps": len(plan.steps)}
    for (f, base, units), (name, z, plain) in zip(per_frame, frames):
        e, bounds = lz_model.expected_scratch(z, [u[0] for u in units])
        w = LAYOUT[name]["window"] if name in LAYOUT else None
        sparse = bool(plan.frames[f][6])
        if sparse:
            cov["sparse"].append(name)
        cov["frames"][name] = {"e": e, "bounds": bounds, "units": units, "base": base, "sparse": sparse}
        n = 0
        for i, (fb, nb, noseq) in enumerate(units):
            a, b = bounds[i], bounds[i + 1]
            if noseq or sparse:
                continue
            n += 1
            size, lowb = b - a, (base + a) & 3
            cov["sizes"].add(size)
            if w:
                cov["s_minus_w"].add((size - w, head_of(size, w)))
            q = e[a:a + (size & ~3)].reshape(-1, 4)
            for row in np.unique(q, axis=0):
                row = tuple(int(v) for v in row)
                cov["keys"][lowb].add(group_key(row))
                for load, ev in loads_of(row).items():
                    cov["shifts"][load].add((lowb - ev) & 3)
            if size & 3:
                cov["tail_sizes"].add(size & 3)
            cov["e"] |= set(int(v) for v in np.unique(e[a:b])[:4096])
            cov["e_max"] = max(cov["e_max"], int(e[a:b].max()) if size else 0)
        cov["pointer_units"][name] = n
    return cov
