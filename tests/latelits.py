"""Frames whose literals verdict arrives after the position scan (test helper, no tests): a submit that runs its Huffman streams
behind zg_k_scan (ZG_FLAG_LIT_DIRECT; BatchBuilder::finish, "literals after the scan?") learns of a literal-stream error — 30
UninitHuf, 31 MissingJump, 32 MissingBytes, 33 ExtraPadding, 34 BitstreamMismatch, 35 CountMismatch — when the frames are laid
out already. zg_k_merge and zg_k_litfix (zg_kernels.hip) then have to rank it against what every other stage found, cut the frame
at the right block and leave the stages behind them nothing to do there. These frames put one such defect L next to one defect D of
every other stage, in the block in front, in the same block and in the block behind, and at the block indices where zg_k_litfix's
loop (stride 256, lim = good_blocks + 1) can go wrong.

Built on tabframes.build: blocks of a handful of bytes, one direct-weights table of five symbols (W). A failing block is written
here byte by byte (lit_section, seq_section); its valid twin is a tabframes.Block of the same streams and sequences. The oracle
decides every verdict, the failing block and the bytes held; compose() also predicts verdict and block from the reference's
order — within a block: block header, literals header, tree description, streams in order, sequences header, FSE descriptions,
bitstream, execution; across blocks: block order — and asserts that the oracle agrees, so that a defect that did not land where it
was meant to cannot pass as coverage. STATUS[name], GOOD[name] (the bytes of the good blocks) and META[name]["bad_block"] are what
the tests compare with."""
import zlib
import random

import framesuite
import oracle
import tabframes
from hufstreams import enc, split4
from tabframes import META, STATUS, Block, FwdBits, lit_header, nbseq, weights_direct

GOOD = {}
W = [2, 2, 1, 1]                                        # symbols 0, 1 and the implied 4 have two bits, 2 and 3 three; symbol 2 is 000
# literals in front of an offset that must be OffsetTooBig: more than the 1 KiB window, in a compressed block (the reference counts
# the literals and matches of compressed blocks, decode_buffer.rs:76 / :108 / :149, not the bytes of Raw and RLE blocks)
BIG_RAW = 1100
MAX_BLOCK = 131072
FAR = 60000                                             # an offset no frame here reaches

# the literal defects: kind -> [(variant name, streams, the stream that carries it or None)]
L_VARIANTS = {
    30: [("l30_1s", 1, None), ("l30_4s", 4, None)],
    31: [("l31", 4, None)],
    32: [("l32", 4, None)],
    33: [("l33_1s", 1, 0)] + [("l33_4s_k%d" % k, 4, k) for k in range(4)],
    34: [("l34_4s_k%d" % k, 4, k) for k in range(4)],
    35: [("l35_1s", 1, None), ("l35_4s", 4, None)],
}
TWO_DEFECTS = [("l34k2_33k1", 4, None), ("l33k2_34k1", 4, None)]       # the rank word: the earlier stream's verdict wins
VARIANT = {v[0]: (kind,) + v[1:] for kind, vs in L_VARIANTS.items() for v in vs}
VARIANT.update({"l34k2_33k1": (33, 4, None), "l33k2_34k1": (34, 4, None)})

# the other stages' defects: stage -> codes ("47h": status 47 found by the host, a section of zero sequences with a byte behind it)
D_STAGES = {"walk": [20, 21], "tree": [36], "seqhdr": [24, "47h"], "fse": [40, 41, 43], "bitstream": [44, 46, 47], "seqpost": [50, 51],
            "exact": [53, 52]}
STAGE_OF = {c: s for s, cs in D_STAGES.items() for c in cs}
_ORDER = {"walk": (0,), "tree": (2,), "seqhdr": (4,), "fse": (5,), "bitstream": (6,), "seqpost": (7,), "exact": (7,)}
RELATIONS = ("front", "same", "behind")
# what the host's walk finds itself (block headers, a treeless section with no table in force, the sequences section header): it ends
# the walk of a whole submit there, so META[name]["host"] frames can only be a submit's last frame (a few of them the host lets
# pass: a treeless section behind a tree description that fails counts as having a table)
HOST_FINDS = (20, 21, 24, "47h")

# what the format does not allow, each with its reason (coverage() asserts that exactly these cells are absent)
SKIPPED_VARIANTS = {
    "l34_1s": "the reference makes no end check on a single stream (literals_section_decoder.rs:143-147): it runs into the count, 35",
    "d42": "MissingByteForModes: a nonzero sequence count always has its mode byte checked as part of the header (24); seq_host_status never carries 42",
    "d43_by_host": "the RLE byte is read with the FSE descriptions, on the device: seq_host_status never carries 43; 43 is in the fse stage here",
}


def skip_reason(kind, q, stage, rel):
    """why no frame can hold literal defect `kind` in a block without (q = 0) or with (1) sequences next to a defect of `stage` in
    relation `rel`; None if one can"""
    if rel != "same":
        return None
    if stage == "walk":
        return "a block has one header: a reserved or an oversized block has no literals section"
    if stage == "tree":
        return "a treeless section carries no tree description" if kind == 30 else None
    if stage == "seqhdr":
        return "the host stops at the sequences header: the block has no sequences as the host sees it" if q else None
    return None if q else "the defect lies in the sequences section or its execution: the block has sequences"


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _status(code):
    return 47 if code == "47h" else code


# ---- sections, byte by byte -------------------------------------------------------------------------------------------------

SEQS = [(2, 5, 4), (3, 6, 3), (2, 4, 5), (1, 5, 3)]     # four sequences over 8 literals, every offset inside the block


def _valid_seq_section(lits, seqs):
    return tabframes._sequences(tabframes._Frame(), Block(lits, seqs))[0] if seqs else b"\x00"


def seq_section(code):
    """a sequences section that carries defect `code` (predefined tables, written for 12 literals)"""
    s = _valid_seq_section(bytes(12), SEQS)
    assert s[0] == 4 and s[1] == 0
    if code == 24:
        return b""
    if code == "47h":
        return b"\x00\x55"
    if code == 40:
        w = FwdBits()
        w.add(tabframes.MAX_LOG["LL"] + 1 - 5, 4)
        return nbseq(4) + bytes([2 << 6]) + w.bytes() + bytes(8) + b"\x01"
    if code == 41:
        return nbseq(4) + bytes([3 << 6]) + b"\x5a\x01"
    if code == 43:
        return bytes([3, 1 << 6, 36]) + b"\x5a\x33\x01"
    if code == 44:
        return s[:-1] + b"\x00"
    if code == 46:
        return bytes([s[0] + 8]) + s[1:]
    if code == 47:
        return bytes([s[0] - 1]) + s[1:]
    if code == 50:
        return _valid_seq_section(bytes(14), [(7, 5, 3), (7, 5, 3)])
    if code == 51:
        return _valid_seq_section(bytes(12), [(1, 1 + 3, 3), (0, 3, 3)])
    if code in (52, 53):
        return _valid_seq_section(bytes(12), [(2, FAR + 3, 3)])
    raise ValueError(code)


BAD_DESC = weights_direct([12, 1, 1])                   # a weight of 12: status 36


def lit_section(ltype, regen, streams, desc=b"", jump=None, payload=None):
    """a Huffman literals section as it is: the description, the jump table of four streams (jump: another one), the streams
    (payload: other bytes behind the description)"""
    ns = len(streams)
    if payload is None:
        jt = b"".join(len(p).to_bytes(2, "little") for p in streams[:3]) if ns == 4 else b""
        payload = (jump if jump is not None else jt) + b"".join(streams)
    body = desc + payload
    return lit_header(ltype, regen, len(body), ns) + body


def lblock(var, q, seed, defect=True, dcode=None):
    """the block of literal defect `var` without (q = 0) or with sequences; dcode: a defect of another stage in the same block.
    defect False: the valid twin, a tabframes.Block of the same streams, literals and sequences"""
    kind, ns, k = VARIANT[var]
    rng = random.Random(seed)
    counts = split4(rng.randint(13, 24)) if ns == 4 else [rng.randint(8, 14)]         # (the format's split: libzstd decodes by it)
    syms = [[rng.choice((0, 1, 2, 3, 4)) for _ in range(c)] for c in counts]
    streams = [enc(W, s) for s in syms]
    lits = bytes(x for s in syms for x in s)
    seqs = tabframes._simple_seqs(len(lits), rng, 3) if q else []
    if not defect:
        return Block(lits, seqs, lit=("hufstreams", list(W), "direct", streams, None))
    desc, ltype, regen, jump, payload = weights_direct(W), 2, len(lits), None, None
    if dcode == 36:
        assert kind != 30
        desc = BAD_DESC
    zero = lambda j: streams.__setitem__(j, streams[j] + b"\x00")
    short = lambda j: streams.__setitem__(j, enc(W, syms[j] + [2], drop=1))
    if kind == 30:
        desc, ltype = b"", 3
    elif kind == 31:
        payload = b"\x02\x00\x02\x00"
    elif kind == 32:
        jump = b"".join(len(p).to_bytes(2, "little") for p in streams[:2]) + (len(streams[2]) + 40).to_bytes(2, "little")
    elif var == "l34k2_33k1":
        short(2), zero(1)
    elif var == "l33k2_34k1":
        zero(2), short(1)
    elif kind == 33:
        zero(k)
    elif kind == 34:
        short(k)
    elif kind == 35:
        regen += 1
    if dcode is not None and dcode != 36:
        sec = seq_section(dcode)
    else:
        sec = _valid_seq_section(lits, seqs)
    return ("bytes", lit_section(ltype, regen, streams, desc, jump, payload) + sec)


def dblock(code, seed, defect=True):
    """a block of its own for defect `code` of another stage; defect False: its valid twin"""
    rng = random.Random(seed)
    lits = rng.randbytes(12)
    if code in (20, 21):
        return (("hdr", 3, 0, b"") if code == 20 else ("hdr", 0, MAX_BLOCK + 1, b"")) if defect else ("raw", lits[:1])
    if code == 36:
        if not defect:
            return lblock("l33_1s", 0, seed, False)
        return ("bytes", lit_section(2, 8, [b"\x01"], BAD_DESC) + b"\x00")
    if not defect:
        return Block(lits, [] if code in (24, "47h") else list(SEQS))
    return ("bytes", lit_header(0, 12) + lits + seq_section(code))


def _stages(spec):
    """[(place in the reference's order within the block, status)] of a block spec"""
    if spec[0] in ("raw", "V", "big"):
        return []
    if spec[0] == "D":
        return [(_ORDER[STAGE_OF[spec[1]]], _status(spec[1]))]
    _, var, q, dcode = spec
    kind, ns, k = VARIANT[var]
    if var == "l34k2_33k1":
        out = [((3, 1, 0), 33), ((3, 2, 1), 34)]
    elif var == "l33k2_34k1":
        out = [((3, 1, 1), 34), ((3, 2, 0), 33)]
    else:
        out = [({30: (2,), 31: (3, -1), 32: (3, -1), 33: (3, k, 0), 34: (3, k, 1), 35: (3, 4)}[kind], kind)]
    if dcode is not None:
        out.append((_ORDER[STAGE_OF[dcode]], _status(dcode)))
    return out


def predict(specs):
    """(status, failing block) by the reference's order: the first block with a defect, the defect it meets first there"""
    for i, s in enumerate(specs):
        st = _stages(s)
        if st:
            return min(st)[1], i
    return 0, len(specs)


def _render(spec, seed, defect):
    if spec[0] == "raw":
        return ("raw", random.Random(seed).randbytes(spec[1]))
    if spec[0] == "big":
        return Block(random.Random(seed).randbytes(BIG_RAW), [])
    if spec[0] == "V":                                  # a block spec that stands for its valid twin
        return _render(spec[1:], seed, False)
    if spec[0] == "D":
        return dblock(spec[1], seed, defect)
    return lblock(spec[1], spec[2], seed, defect, spec[3])


TWINS = {}                                              # valid frames by their bytes: name -> (name, zst, plaintext)


def compose(name, specs, info, twin=True):
    """the frame of the block specs ("raw", n) | ("big",) | ("V", a spec: its valid twin) | ("L", variant, q, code of a defect in the same block or None) | ("D", code): built,
    predicted and checked against the oracle. info goes to META[name] with the prediction. The valid twin (every block without its
    defect) is kept in TWINS"""
    big = any(s[0] == "D" and s[1] == 52 or s[0] == "L" and s[3] == 52 for s in specs)
    wl = 10 if big else 17
    seeds = [_seed(name, i) for i in range(len(specs))]
    want, at = predict(specs)
    if twin:
        v = tabframes.build("v_" + name, [_render(s, sd, False) for s, sd in zip(specs, seeds)], window_log=wl)
        if v[1] in TWINS:
            del META[v[0]]
        else:
            TWINS[v[1]] = v
    if not want:
        r = tabframes.build(name, [_render(s, sd, False) for s, sd in zip(specs, seeds)], window_log=wl)
        META[name].update(info, nblocks=len(specs))
        return r
    r = tabframes.build(name, [_render(s, sd, True) for s, sd in zip(specs, seeds)], window_log=wl, valid=False)
    GOOD[name] = tabframes.build("_front", [_render(s, sd, False) for s, sd in zip(specs[:at], seeds)] + [("raw", b"")], window_log=wl)[2]
    del META["_front"]
    d = oracle.FrameDecoder()
    st, c, _, _ = d.init(r[1])
    assert st == 0, name
    st, _, _ = d.decode_blocks(r[1][c:], oracle.STRAT_ALL)
    assert (st, d.blocks_decoded()) == (want, at) and STATUS[name] == want, (name, "oracle", st, d.blocks_decoded(), "predicted", want, at)
    assert d.held()[:len(GOOD[name])] == GOOD[name], (name, "the oracle holds other bytes for the good blocks")
    host = any(s[0] == "D" and s[1] in HOST_FINDS or s[0] == "L" and (VARIANT[s[1]][0] == 30 or s[3] in HOST_FINDS) for s in specs)
    META[name].update(info, bad_block=at, nblocks=len(specs), host=host,
                      l_wins=specs[at][0] == "L" and 30 <= want <= 35)
    return r


# ---- the families -----------------------------------------------------------------------------------------------------------

class _Rot:
    """the variants of a kind in turn"""

    def __init__(self):
        self.n = {}

    def next(self, kind):
        v = L_VARIANTS[kind]
        self.n[kind] = self.n.get(kind, -1) + 1
        return v[self.n[kind] % len(v)][0]


def _front(kind, code, j):
    """one or two valid blocks in front of both: raw bytes (more literals than the window for OffsetTooBig), and in every other frame a
    compressed block without sequences behind them, of raw literals in front of UninitHuf (no Huffman table may be in force there)
    and of Huffman literals else (no FSE table may be in force in front of a repeat mode that must fail)"""
    out = [("big",) if code == 52 else ("raw", 5 + j % 7)]
    if j % 2:
        out.append(("V", "D", 24) if kind == 30 else ("V", "L", "l35_1s", 0, None))
    return out


def alone():
    """every variant of every literal defect, the two-defect blocks included, in a block without and with sequences, behind one
    valid block and in front of one"""
    out = []
    for var in [v[0] for vs in L_VARIANTS.values() for v in vs] + [v[0] for v in TWO_DEFECTS]:
        for q in (0, 1):
            name = "alone_%s_%s" % (var, "q" if q else "n")
            out.append(compose(name, [("raw", 9), ("L", var, q, None), ("raw", 2)], {"variant": var, "q": q}))
    return out


def pairs():
    """one literal defect and one defect of another stage: in the block in front, in the same block where the format allows it, in
    the block behind; one or two valid blocks in front of both, one behind"""
    out, rot, j = [], _Rot(), 0
    for kind in L_VARIANTS:
        for q in (0, 1):
            for stage, codes in D_STAGES.items():
                for code in codes:
                    for rel in RELATIONS:
                        if skip_reason(kind, q, stage, rel):
                            continue
                        var = rot.next(kind)
                        j += 1
                        name = "pair_%s_%s_d%s_%s" % (var, "q" if q else "n", code, rel)
                        mid = {"front": [("D", code), ("L", var, q, None)], "same": [("L", var, q, code)], "behind": [("L", var, q, None), ("D", code)]}[rel]
                        out.append(compose(name, _front(kind, code, j) + mid + [("raw", 2)],
                                           {"cell": (kind, q, stage, rel), "code": code, "variant": var}))
    return out


GEO_N = (1, 2, 257, 600)
GEO_AT = (0, 1, 255, 256, 257, 511, 512)


def _geo(name, n, put, info, twin=True):
    specs = [("raw", 1)] * n
    if any(s[0] == "D" and s[1] == 52 for s in put.values()):
        specs[0] = ("big",)
    for i, s in put.items():
        assert 0 <= i < n and (i or specs[0] == ("raw", 1))
        specs[i] = s
    return compose(name, specs, dict(info, n=n, put=sorted(put)), twin)


def geometry():
    """zg_k_litfix's loop and lim, in frames of one-byte raw blocks around the blocks that matter: a literal defect at the block
    indices around the stride of 256, two of them one stride apart, one next to a defect found before the scan (the three sides of
    lim = good_blocks + 1) and two blocks from an offset too far, which the flatten finds after zg_k_litfix"""
    out = []
    vars_ = [v[0] for kd in (31, 32, 33, 34, 35) for v in L_VARIANTS[kd]] + [v[0] for v in TWO_DEFECTS]
    j = 0
    for n in GEO_N:
        out.append(_geo("geo_n%d_control" % n, n, {n // 2: ("V", "L", "l33_4s_k1", n % 2, None)}, {"what": "control"}, twin=False))
        for at in sorted(set(a for a in GEO_AT + (n - 1,) if a < n)):
            var, j = vars_[j % len(vars_)], j + 1
            out.append(_geo("geo_n%d_at%d" % (n, at), n, {at: ("L", var, j % 2, None)}, {"what": "at", "at": at}))
    for a, b, va, vb in ((40, 300, "l33_4s_k0", "l35_4s"), (40, 300, "l35_1s", "l33_4s_k3"), (300, 552, "l34_4s_k2", "l32")):
        out.append(_geo("geo_two_%s_at%d_%s_at%d" % (va, a, vb, b), 600, {a: ("L", va, 0, None), b: ("L", vb, 1, None)}, {"what": "two", "at": (a, b)}))
    for n, i, code in ((600, 300, 46), (600, 256, 51), (257, 1, 46)):
        for side in (-1, 0, 1):
            var, j = vars_[j % len(vars_)], j + 1
            put = {i: ("L", var, 1, code)} if side == 0 else {i: ("L", var, j % 2, None), i + side: ("D", code)}
            out.append(_geo("geo_lim_n%d_at%d_d%d_%+d" % (n, i, code, side), n, put, {"what": "lim", "side": side, "code": code}))
    for i, code in ((300, 52), (257, 53)):
        for side in (-2, 2):
            var, j = vars_[j % len(vars_)], j + 1
            out.append(_geo("geo_far_at%d_d%d_%+d" % (i, code, side), 600, {i: ("L", var, j % 2, None), i + side: ("D", code)},
                            {"what": "far", "side": side, "code": code}))
    return out


def valid():
    """the same blocks without their defect: every invalid frame's twin of its own shape (twins of equal bytes once)"""
    for fam in ("alone", "pairs", "geometry"):
        family(fam)
    return list(TWINS.values())


FAMILIES = {"alone": alone, "pairs": pairs, "geometry": geometry, "valid": valid}
_F = framesuite.Families(FAMILIES)
family, all_frames, valid_frames, invalid_frames = _F.family, _F.all_frames, _F.valid_frames, _F.invalid_frames


def with_content_size(z, n):
    """the frame with an 8-byte Frame_Content_Size of n in its header (tabframes' header: descriptor 0x04, window byte). The reference
    never checks the value; a submit whose frames all declare one is sized in advance (Batch::sync's presized branch)"""
    assert z[:4] == tabframes.MAGIC and z[4] == 0x04
    return z[:4] + bytes([0xC4, z[5]]) + n.to_bytes(8, "little") + z[6:]


def coverage(frames):
    """asserts the matrix the families are there for; frames is all_frames()'s list. Returns the figures"""
    cov = {"cells": set(), "skipped": {}, "codes": set(), "variants": set(), "geo_at": set(), "geo_n": set(), "two": set(), "lim": set(),
           "far": set(), "controls": set(), "statuses": set(), "l_wins": 0, "d_wins_by_order": 0, "d_wins_same_block": 0, "valid": 0,
           "invalid": 0, "per_family": {}}
    for fam, name, z, plain in frames:
        m = META[name]
        cov["per_family"][fam] = cov["per_family"].get(fam, 0) + 1
        cov["valid" if plain is not None else "invalid"] += 1
        if fam == "geometry" and m.get("what") == "control":
            assert plain is not None, name
            cov["controls"].add(m["n"])
        if plain is None:
            cov["statuses"].add(STATUS[name])
            if "variant" in m:
                cov["variants"].add((m["variant"], m.get("q", m.get("cell", (0, 0))[1])))
        if fam == "pairs":
            kind, q, stage, rel = m["cell"]
            cov["cells"].add(m["cell"])
            cov["codes"].add(m["code"])
            won = STATUS[name] == kind and m["l_wins"]
            assert won == (rel == "behind" or rel == "same" and stage not in ("walk", "tree")), (name, STATUS[name])
            cov["l_wins"] += won
            cov["d_wins_by_order"] += (not won) and rel == "front"
            cov["d_wins_same_block"] += (not won) and rel == "same"
        if fam == "geometry" and plain is None:
            cov["geo_n"].add(m["n"])
            if m["what"] == "at":
                cov["geo_at"].add((m["n"], m["at"]))
                assert m["bad_block"] == m["at"], name
            elif m["what"] == "two":
                cov["two"].add(m["at"])
                assert m["bad_block"] == min(m["at"]), name
            elif m["what"] in ("lim", "far"):
                cov[m["what"]].add((m["code"], m["side"]))
                assert (m["bad_block"] == min(m["put"])) and (STATUS[name] == m["code"]) == (m["side"] < 0), name
    for kind in L_VARIANTS:
        for q in (0, 1):
            for stage in D_STAGES:
                for rel in RELATIONS:
                    why = skip_reason(kind, q, stage, rel)
                    if why:
                        cov["skipped"][(kind, q, stage, rel)] = why
                        assert (kind, q, stage, rel) not in cov["cells"]
                    else:
                        assert (kind, q, stage, rel) in cov["cells"], ("no frame for", kind, q, stage, rel)
    assert cov["codes"] == set(STAGE_OF), cov["codes"]
    assert cov["variants"] >= {(v, q) for v in VARIANT for q in (0, 1)}, cov["variants"]
    assert cov["geo_at"] == {(n, a) for n in GEO_N for a in GEO_AT + (n - 1,) if a < n}, cov["geo_at"]
    assert cov["controls"] == set(GEO_N) and cov["two"] == {(40, 300), (300, 552)}, (cov["controls"], cov["two"])
    assert cov["lim"] == {(c, s) for c in (46, 51) for s in (-1, 0, 1)} and cov["far"] == {(c, s) for c in (52, 53) for s in (-2, 2)}, (cov["lim"], cov["far"])
    assert cov["statuses"] >= {30, 31, 32, 33, 34, 35} | {_status(c) for c in STAGE_OF}, cov["statuses"]
    assert cov["l_wins"] and cov["d_wins_by_order"] and cov["d_wins_same_block"]
    cov["skipped_variants"] = dict(SKIPPED_VARIANTS)
    return cov
