"""The cases and the plain model behind tests/test_zxprobe_cpu.py (the CPU emulator, tests/emu/zg_simt.h) and tests/test_gpu_zxprobe.py (an
MI355X, zg_kernels.hip): every zx_* primitive the kernel bodies are written against, one primitive and one workgroup of 64 or 256 threads per
case (zstd-rs_amd/csrc/zg_zxprobe.h says what a thread does with its eight operand words and four result words). The model is written from the
ISA's and HIP's rules in plain Python integers, not from either definition under test:
  __shfl / __shfl_up / __shfl_xor (amd_warp_functions.h, width 64): ds_bpermute_b32 from lane (l & 63), from lane - delta where that is >= 0 else
  the caller's own value, from lane ^ mask where that is < 64 else the caller's own value; ds_bpermute_b32 from a lane that is off in EXEC reads 0;
  __ballot counts the lanes that are on. DPP: the model tests/test_prefix_scans_cpu.py already holds (dpp, KSTEPS, scan_add) — not a second
  one. Raw buffers (stride 0, no swizzle): a byte is in range when offset < num_records, a dword when offset + 4 <= num_records, each dword of
  a wide access by itself; out of range reads 0 and writes nothing. v_alignbit_b32 shifts by S2[4:0]. v_pk_sub_i16 / v_pk_ashrrev_i16 work on
  the two halves by themselves. Cases are seeded: the same list every time."""
import os
import random
import re
import struct

from test_prefix_scans_cpu import KSTEPS, dpp, scan_add

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "zstd-rs_amd", "csrc", "zg_zxprobe.h")
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
K_IN, K_OUT = 8, 4
OUT_FILL = 0xEEEEEEEE                # what a result word holds that no thread wrote
GUARD = 256
ZX_OOB = 0x80000000
NULL_RES = 1
SIZES = (0, 1, 3, 4, 5, 7, 8, 11, 12, 13, 16, 17, 64)


def _ops():
    src = open(HEADER).read()
    names = re.search(r"enum Op : uint32_t \{(.*?)\};", src, re.S).group(1)
    names = [n.split("=")[0].strip() for n in names.replace("\n", " ").split(",") if n.strip()]
    assert names[-1] == "kOps"
    return {n[1:]: i for i, n in enumerate(names[:-1])}


OP = _ops()                          # "Ballot" -> 0, ...
COLLECTIVES = ("Ballot", "Any", "Shfl", "ShflUp", "ShflXor", "Shfl63", "Scan64", "Lane64", "XorSum64")
LOADS = {"Ld8": 0, "Ld32": 1, "Ld64": 2, "Ld96": 3, "Ld128": 4}      # -> dwords (0: a byte)
STORES = ("St8", "St32")
UP_DELTAS = (0, 1, 2, 4, 8, 16, 32, 63, 64)
XOR_MASKS = (1, 2, 4, 8, 16, 32, 63)


class Case:
    def __init__(self, name, op, threads, inp, arena=None, res_off=GUARD, res_bytes=0, flags=0):
        assert len(inp) == threads * K_IN and all(0 <= w <= M32 for w in inp)
        self.name, self.op, self.threads, self.inp = name, OP[op], threads, list(inp)
        self.opname, self.flags, self.res_off, self.res_bytes = op, flags, res_off, res_bytes
        self.arena = bytes(arena) if arena is not None else bytes(_arena_bytes(random.Random(len(name)), 2 * GUARD))
        self.out0 = [OUT_FILL] * (threads * K_OUT)

    def a(self, t):
        return self.inp[t * K_IN:(t + 1) * K_IN]


def _arena_bytes(rng, n):
    """n bytes, none of them 0: a byte read from outside the resource never looks like the 0 of a refused access"""
    return bytearray(rng.randrange(1, 256) for _ in range(n))


def _words(rows, threads):
    """rows[t]: the operand words of thread t (shorter rows are padded with 0)"""
    assert len(rows) == threads
    return [int(w) for r in rows for w in (list(r) + [0] * K_IN)[:K_IN]]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def _bperm(vals, on, src):
    """ds_bpermute_b32 in one wave: lane l (on) reads lane src[l] & 63; a lane that is off gives 0"""
    return [(vals[src[l] & 63] if on[src[l] & 63] else 0) if on[l] else None for l in range(64)]


def _shfl(vals, on, idx):
    return _bperm(vals, on, [i & 63 for i in idx])


def _shfl_up(vals, on, delta):
    got = _bperm(vals, on, [l - delta[l] if l - delta[l] >= 0 else l for l in range(64)])
    return got


def _shfl_xor(vals, on, mask):
    return _bperm(vals, on, [l ^ mask[l] if (l ^ mask[l]) < 64 else l for l in range(64)])


def _lo(v):
    return [x & M32 for x in v]


def _hi(v):
    return [(x >> 32) & M32 for x in v]


def _join(lo, hi, on):
    return [(hi[l] << 32 | lo[l]) if on[l] else 0 for l in range(64)]


def _wave_collective(op, a, on):
    """one wave: a[l] the operand words of lane l, on[l] whether it got to the primitive; -> per lane None or the result words it stores"""
    v32 = [a[l][1] for l in range(64)]
    v64 = [a[l][2] << 32 | a[l][1] for l in range(64)]
    if op in ("Ballot", "Any"):
        mask = sum(1 << l for l in range(64) if on[l] and a[l][1] & 1)
        res = [mask & M32, mask >> 32] if op == "Ballot" else [1 if mask else 0]
        return [res if on[l] else None for l in range(64)]
    if op == "Shfl":
        r = _shfl(v32, on, [a[l][2] for l in range(64)])
    elif op == "Shfl63":
        r = _shfl(v32, on, [63] * 64)
    elif op == "ShflUp":
        r = _shfl_up(v32, on, [a[l][2] for l in range(64)])
    elif op == "ShflXor":
        r = _shfl_xor(v32, on, [a[l][2] for l in range(64)])
    elif op == "Lane64":
        idx = [a[l][3] for l in range(64)]
        r = _join(_shfl(_lo(v64), on, idx), _shfl(_hi(v64), on, idx), on)
    elif op == "Scan64":                                 # zg_seektab.h: scan64
        v, o = list(v64), 1
        while o < 64:
            t = _join(_shfl_up(_lo(v), on, [o] * 64), _shfl_up(_hi(v), on, [o] * 64), on)
            v = [(v[l] + t[l]) & M64 if l >= o else v[l] for l in range(64)]
            o <<= 1
        r = v
    elif op == "XorSum64":                               # zg_seekmany.h: seekmany_prefix
        v = list(v64)
        for sh in (32, 16, 8, 4, 2, 1):
            t = _join(_shfl_xor(_lo(v), on, [sh] * 64), _shfl_xor(_hi(v), on, [sh] * 64), on)
            v = [(v[l] + t[l]) & M64 for l in range(64)]
        r = v
    else:
        raise ValueError(op)
    if op in ("Lane64", "Scan64", "XorSum64"):
        return [[r[l] & M32, r[l] >> 32] if on[l] else None for l in range(64)]
    return [[r[l]] if on[l] else None for l in range(64)]


def _dword(c, arena, off):
    """a dword of the resource at byte offset off: in range exactly when off + 4 <= bytes"""
    if off + 4 > c.res_bytes:
        return 0
    return int.from_bytes(arena[c.res_off + off:c.res_off + off + 4], "little")


def dwords_in_range(c, off, k):
    return sum(1 for j in range(k) if off + 4 * j + 4 <= c.res_bytes)


def _sub16(x, y):
    return (x - y) & 0xFFFF


def model(c):
    """(the result words, the arena) after the case, by the rules in this module's docstring"""
    op, T = c.opname, c.threads
    out, arena = list(c.out0), bytearray(c.arena)
    A = [c.a(t) for t in range(T)]

    def put(t, words):
        out[t * K_OUT:t * K_OUT + len(words)] = words

    if op in COLLECTIVES:
        for w in range(T // 64):
            a = A[64 * w:64 * w + 64]
            res = _wave_collective(op, a, [not x[0] for x in a])
            for l in range(64):
                if res[l] is not None:
                    put(64 * w + l, res[l])
    elif op.startswith("ScanSrc") or op in ("ScanAdd", "Shr1"):
        for w in range(T // 64):
            a = A[64 * w:64 * w + 64]
            assert not any(x[0] for x in a), "DPP: every lane active"
            v, fill = [x[1] for x in a], [x[2] for x in a]
            if op == "ScanAdd":
                r = [[x] for x in scan_add(v)]
            elif op == "Shr1":
                r = [[x] for x in dpp(v, 0x138, 0xF, fill)]
            else:
                ctrl, rows = KSTEPS[int(op[-1])]
                takes = dpp([1] * 64, ctrl, rows, [0] * 64)
                r = [[x, k] for x, k in zip(dpp(v, ctrl, rows, fill), takes)]
            for l in range(64):
                put(64 * w + l, r[l])
    elif op in LOADS:
        for t in range(T):
            if A[t][0]:
                continue
            off = A[t][1]
            if op == "Ld8":
                put(t, [arena[c.res_off + off] if off < c.res_bytes else 0])
            else:
                put(t, [_dword(c, arena, off + 4 * j) for j in range(LOADS[op])])
    elif op in STORES:
        n, hit = (1, set()) if op == "St8" else (4, set())
        for t in range(T):
            off = A[t][1]
            if A[t][0] or off + n > c.res_bytes:
                continue
            assert not hit & set(range(off, off + n)), "two stores to one byte"
            hit |= set(range(off, off + n))
            arena[c.res_off + off:c.res_off + off + n] = (A[t][2] & (0xFF if n == 1 else M32)).to_bytes(n, "little")
    elif op == "Alignbit":
        for t in range(T):
            put(t, [((A[t][1] << 32 | A[t][2]) >> (A[t][3] & 31)) & M32])
    elif op == "PkSub16":
        for t in range(T):
            x, y = A[t][1], A[t][2]
            put(t, [_sub16(x & 0xFFFF, y & 0xFFFF) | _sub16(x >> 16, y >> 16) << 16])
    elif op == "PkSign16":
        for t in range(T):
            x = A[t][1]
            put(t, [(0xFFFF if x & 0x8000 else 0) | (0xFFFF0000 if x & 0x80000000 else 0)])
    elif op == "Bfi":
        for t in range(T):
            m, x, y = A[t][1:4]
            put(t, [(x & m) | (y & ~m & M32)])
    elif op in ("Gst32u", "Gst128"):
        n, hit = (4, set()) if op == "Gst32u" else (16, set())
        for t in range(T):
            if A[t][0]:
                continue
            at = A[t][1]
            assert at + n <= len(arena) and not hit & set(range(at, at + n))
            hit |= set(range(at, at + n))
            arena[at:at + n] = struct.pack("<%dI" % (n // 4), *A[t][2:2 + n // 4])
    elif op == "Gld128":
        for t in range(T):
            if not A[t][0]:
                put(t, list(struct.unpack("<4I", arena[A[t][1]:A[t][1] + 16])))
    elif op in ("OrLds", "MinLds", "MinLds64", "AddLds", "CasLds"):
        w = [A[t][7] << 32 | A[t][6] if op == "MinLds64" else A[t][7] for t in range(64)]
        contenders = set()
        for t in range(T):
            if A[t][0]:
                continue
            i, v = A[t][1], A[t][2]
            if op == "OrLds":
                w[i] |= v
            elif op == "MinLds":
                w[i] = min(w[i], v)
            elif op == "MinLds64":
                w[i] = min(w[i], A[t][3] << 32 | v)
            elif op == "AddLds":
                w[i] = (w[i] + v) & M32
            else:
                assert i not in contenders, "zx_cas_lds: one contender per word"
                contenders.add(i)
                if w[i] == v:
                    w[i] = A[t][3]
        for t in range(T):
            put(t, [w[t & 63] & M32, w[t & 63] >> 32] if op == "MinLds64" else [w[t & 63]])
    elif op in ("MinGlb", "MaxGlb"):
        for t in range(T):
            if A[t][0]:
                continue
            at = A[t][1]
            old = int.from_bytes(arena[at:at + 4], "little")
            arena[at:at + 4] = (min if op == "MinGlb" else max)(old, A[t][2]).to_bytes(4, "little")
    elif op in ("PubWave", "PubBarrier", "PubBarrierVm", "PubFence"):
        for t in range(T):
            put(t, [A[A[t][2]][1]])
            if op in ("PubBarrierVm", "PubFence"):
                arena[4 * t:4 * t + 4] = A[t][1].to_bytes(4, "little")
    else:
        raise ValueError(op)
    return out, bytes(arena)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
RETURNS = {                                              # which lanes of a wave return before the primitive
    "none": lambda l: False,
    "odd": lambda l: l % 2 == 1,
    "40..63": lambda l: l >= 40,
    "all but 0": lambda l: l != 0,
    "all but 63": lambda l: l != 63,
    "whole": lambda l: True,
}
WAVES_OF_4 = [("odd", "whole", "40..63", "none"), ("all but 63", "whole", "none", "all but 0"), ("none", "whole", "odd", "all but 63")]


def _val(rng, i):
    """a 32-bit value; every other one has its top bit set"""
    return rng.randrange(1 << 32) | (0x80000000 if i % 2 == 0 else 0)


def _collective_cases(rng):
    cases = []

    def add(op, tag, row):
        """row(rng, lane, wave) -> the operand words behind a[0]"""
        shapes = [(64, (p,)) for p in ("none", "odd", "40..63", "all but 0", "all but 63")]
        shapes.append((256, WAVES_OF_4[len(cases) % 3]))
        for T, pats in shapes:
            rows = [[1 if RETURNS[pats[t // 64]](t % 64) else 0] + row(rng, t % 64, t // 64) for t in range(T)]
            cases.append(Case("%s %s T=%d returns %s" % (op, tag, T, "/".join(pats)), op, T, _words(rows, T)))

    for name, pred in (("random", lambda r, l: r.randrange(2)), ("zeros", lambda r, l: 0), ("ones", lambda r, l: 1),
                       ("only where odd", lambda r, l: l % 2), ("only 40..63", lambda r, l: int(l >= 40)), ("only lane 63", lambda r, l: int(l == 63))):
        for op in ("Ballot", "Any"):
            add(op, name, lambda r, l, w, pred=pred: [pred(r, l) | (r.randrange(1 << 31) << 1)])   # (only bit 0 is the predicate)
    for d in UP_DELTAS:
        add("ShflUp", "delta %d" % d, lambda r, l, w, d=d: [_val(r, l), d])
    add("ShflUp", "delta per wave", lambda r, l, w: [_val(r, l), (1, 63, 64, 16)[w]])
    for x in XOR_MASKS:
        add("ShflXor", "mask %d" % x, lambda r, l, w, x=x: [_val(r, l), x])
    for k in range(2):
        # a per-lane index: 0 .. 127, the caller's own lane, lane 0 and lane 63, returned sources among them
        add("Shfl", "index per lane %d" % k, lambda r, l, w: [_val(r, l), l if l % 5 == 0 else 64 + l if l % 7 == 0 else r.choice((0, 63, r.randrange(128)))])
    add("Shfl63", "wave total", lambda r, l, w: [_val(r, l)])
    for k in range(2):
        add("Scan64", "carries %d" % k, lambda r, l, w: [r.choice((M32, _val(r, l))), r.randrange(1 << 32)])
        add("Lane64", "index per lane %d" % k, lambda r, l, w: [_val(r, l), _val(r, l + 1), r.choice((l, 63, 0, r.randrange(128)))])
        add("XorSum64", "carries %d" % k, lambda r, l, w: [r.choice((M32, _val(r, l))), r.randrange(1 << 32)])
    return cases


def _dpp_cases(rng):
    cases = []
    for T in (64, 256):
        for s in range(6):
            for tag, fill in (("fill 0", lambda: 0), ("fill per lane", lambda: rng.randrange(1, 1 << 32))):
                rows = [[0, _val(rng, t), fill()] for t in range(T)]
                cases.append(Case("ScanSrc%d %s T=%d" % (s, tag, T), "ScanSrc%d" % s, T, _words(rows, T)))
        for tag, fill in (("fill 0", lambda: 0), ("fill per lane", lambda: rng.randrange(1, 1 << 32))):
            cases.append(Case("Shr1 %s T=%d" % (tag, T), "Shr1", T, _words([[0, _val(rng, t), fill()] for t in range(T)], T)))
        for tag, v in (("wraps", lambda t: _val(rng, t)), ("all ones", lambda t: M32), ("one per lane", lambda t: 1),
                       ("row edges", lambda t: 0x80000000 if t % 64 in (15, 16, 31, 32, 47, 48, 63) else 0)):
            cases.append(Case("ScanAdd %s T=%d" % (tag, T), "ScanAdd", T, _words([[0, v(t)] for t in range(T)], T)))
    return cases


def _offsets(nbytes, align, wide):
    """every offset from 0 to nbytes + 20 and the four around ZX_OOB; for the wide accesses only those that make a dword-aligned ADDRESS, in
    range or not (the emulator's and the bodies' rule): zx_ld8, zx_ld32 and zx_st8 alone take the others"""
    offs = [o for o in range(nbytes + 21) if not wide or (align + o) % 4 == 0]
    return offs + [ZX_OOB, ZX_OOB + 4, ZX_OOB + 8, ZX_OOB + 12]


def _buffer_cases(rng):
    cases = []
    for op in list(LOADS) + list(STORES):
        wide = op not in ("Ld8", "Ld32", "St8")
        for i, nbytes in enumerate(SIZES):
            for align in [a for a in range(16) if (a + i) % 4 == 0]:     # over the 13 sizes: each of the 16 alignments of the base, per primitive
                offs = _offsets(nbytes, align, wide)
                T = 64 if len(offs) <= 64 else 256
                rng.shuffle(offs)
                res_off = GUARD + align
                arena = _arena_bytes(rng, (res_off + nbytes + GUARD + 15) // 16 * 16)
                rows = [[0, offs[t], _val(rng, t)] if t < len(offs) else [1, ZX_OOB, 0] for t in range(T)]
                cases.append(Case("%s bytes=%d base%%16=%d" % (op, nbytes, align), op, T, _words(rows, T), arena, res_off, nbytes))
        offs = _offsets(0, 0, wide)
        rows = [[0, offs[t], _val(rng, t)] if t < len(offs) else [1, 0, 0] for t in range(64)]
        cases.append(Case("%s null resource" % op, op, 64, _words(rows, 64), _arena_bytes(rng, 2 * GUARD), 0, 0, NULL_RES))
    return cases


def _integer_cases(rng):
    cases = []
    sh = list(range(32)) + [32, 33, 63, 255]
    rows = [[0, _val(rng, t), rng.randrange(1 << 32), sh[t] if t < len(sh) else rng.randrange(1 << 32)] for t in range(64)]
    cases.append(Case("Alignbit shifts", "Alignbit", 64, _words(rows, 64)))
    rows = [[0, rng.choice((0, M32, _val(rng, t))), rng.choice((0, M32, _val(rng, t))), rng.choice(sh)] for t in range(256)]
    cases.append(Case("Alignbit random", "Alignbit", 256, _words(rows, 256)))
    halves = (0, 1, 0x7FFF, 0x8000, 0xFFFF)
    pairs = [(x, y) for x in halves for y in halves]                      # a half of a against a half of b: every pairing, in both halves
    quads = [((hx << 16 | lx), (hy << 16 | ly)) for lx, ly in pairs for hx, hy in pairs]
    for k in range(0, len(quads), 256):
        part = quads[k:k + 256]
        rows = [[0, *part[t]] if t < len(part) else [0, rng.randrange(1 << 32), rng.randrange(1 << 32)] for t in range(256)]
        cases.append(Case("PkSub16 halves %d" % (k // 256), "PkSub16", 256, _words(rows, 256)))
    rows = [[0, (pairs[t][0] << 16 | pairs[t][1])] if t < len(pairs) else [0, rng.randrange(1 << 32)] for t in range(64)]
    cases.append(Case("PkSign16 halves", "PkSign16", 64, _words(rows, 64)))
    rows = [[0, rng.randrange(1 << 32)] for t in range(256)]
    cases.append(Case("PkSign16 random", "PkSign16", 256, _words(rows, 256)))
    masks = (0, M32, 0xFFFF, 0xFFFF0000, 0x80000000, 1)
    rows = [[0, masks[t] if t < len(masks) else rng.randrange(1 << 32), rng.randrange(1 << 32), rng.randrange(1 << 32)] for t in range(64)]
    cases.append(Case("Bfi", "Bfi", 64, _words(rows, 64)))
    return cases


def _memory_cases(rng):
    cases = []
    arena = _arena_bytes(rng, 4096)
    rows = [[0, 512 + 48 * t + t % 16, _val(rng, t)] for t in range(64)]  # every address mod 16, four times
    cases.append(Case("Gst32u every address mod 16", "Gst32u", 64, _words(rows, 64), arena))
    rows = [[t % 3 == 2, 16 * (2 * t + 1) if t else 4096 - 16, *[_val(rng, t + k) for k in range(4)]] for t in range(64)]
    cases.append(Case("Gst128", "Gst128", 64, _words(rows, 64), arena))
    rows = [[t % 5 == 4, rng.choice((0, 4096 - 16, 16 * rng.randrange(256)))] for t in range(256)]
    cases.append(Case("Gld128", "Gld128", 256, _words(rows, 256), arena))
    for op in ("OrLds", "MinLds", "MinLds64", "AddLds"):
        for T in (64, 256):
            # many threads on few words (and some words nobody touches); the words start at a[6], a[7] of the first 64 threads
            rows = [[t % 7 == 3, rng.choice((0, 1, 2, 31, 63)), _val(rng, t) >> rng.randrange(32), rng.randrange(1 << 32) >> rng.randrange(32), 0, 0,
                     rng.randrange(1 << 32), rng.randrange(1 << 32) >> rng.randrange(8)] for t in range(T)]
            cases.append(Case("%s contended T=%d" % (op, T), op, T, _words(rows, T)))
    for op in ("MinGlb", "MaxGlb"):
        for T in (64, 256):
            rows = [[t % 7 == 3, rng.choice((0, 4, 512, 4092)), _val(rng, t) >> rng.randrange(32)] for t in range(T)]
            cases.append(Case("%s contended T=%d" % (op, T), op, T, _words(rows, T), arena))
    for T in (64, 256):
        perm = list(range(64))
        rng.shuffle(perm)
        init = [rng.randrange(1 << 32) for _ in range(64)]
        # one contender per word: half of them compare with what the word holds, the others with something else
        rows = [[t >= 64 or t % 9 == 8, perm[t % 64], init[perm[t % 64]] ^ (t % 2), _val(rng, t), 0, 0, 0, init[t % 64]] for t in range(T)]
        cases.append(Case("CasLds one contender T=%d" % T, "CasLds", T, _words(rows, T)))
    for op in ("PubWave", "PubBarrier", "PubBarrierVm", "PubFence"):
        for T in (64, 256):
            rows = [[0, _val(rng, t), (t & ~63) | rng.randrange(64) if op == "PubWave" else rng.randrange(T)] for t in range(T)]
            cases.append(Case("%s T=%d" % (op, T), op, T, _words(rows, T), _arena_bytes(rng, 2048)))
    return cases


def all_cases():
    rng = random.Random(0x5A58)
    return _collective_cases(rng) + _dpp_cases(rng) + _buffer_cases(rng) + _integer_cases(rng) + _memory_cases(rng)


def coverage(cases):
    """what the cases reach, for the assertions the suites make of them: {primitive: ...}"""
    cov = {"ops": {c.opname for c in cases}, "dwords": {}, "bases": {}, "sizes": {}, "threads": {}}
    for c in cases:
        cov["threads"].setdefault(c.opname, set()).add(c.threads)
        if c.opname in LOADS or c.opname in STORES:
            k = LOADS.get(c.opname, 1) or 1
            if not c.flags:
                cov["bases"].setdefault(c.opname, set()).add(c.res_off % 16)
                cov["sizes"].setdefault(c.opname, set()).add(c.res_bytes)
            if c.opname not in ("Ld8", "St8"):
                for t in range(c.threads):
                    if not c.a(t)[0]:
                        cov["dwords"].setdefault(c.opname, set()).add(dwords_in_range(c, c.a(t)[1], k))
    return cov


def write_cases(path, cases, wants):
    """the file tests/emu/zg_emu_zxprobe.cpp's main reads"""
    with open(path, "wb") as f:
        f.write(b"ZXPC" + struct.pack("<I", len(cases)))
        for c, (out, arena) in zip(cases, wants):
            f.write(struct.pack("<6I", c.op, c.threads, c.flags, c.res_off, c.res_bytes, len(c.arena)))
            f.write(struct.pack("<%dI" % len(c.inp), *c.inp) + struct.pack("<%dI" % len(c.out0), *c.out0) + c.arena)
            f.write(struct.pack("<%dI" % len(out), *out) + arena)
