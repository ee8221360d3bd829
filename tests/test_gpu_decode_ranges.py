"""zgpu_decode_ranges_device_src / zgpu_frames_seek_device (Context.decode_ranges_device_src, frames_seek_device, decode_tensor_ranges) on
the GPU: plaintext bytes [begin, begin + len) of multi-frame entries that lie in device memory, written to device memory, with only the
frames that hold the range decoded. The expectation of every case comes from the oracle: a small pure-Python chain walker (select, below)
computes the selection S = entry[src_lo:src_hi] and plain_lo by the rule of zg_seek.h, oracle_alone(S) gives the status and the bytes, a
taken frame that declares a size and decodes to another length gives zgpu.E_CONTENT_SIZE_MISMATCH, and the destination must hold
out[begin - plain_lo:][:len] — with guard bytes, everything behind `written` and every byte of a failed entry's slot untouched (Arena.check
compares the whole arena)."""
import ctypes as C
import random
import time

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import zgpu
from devmem import ALL, Arena, RawSources, Sources, oracle_alone
from golden_io import read_manifest, read_pack

pytestmark = pytest.mark.gpu
TOP = 2 ** 64 - 1


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


# ---- the model: the header chain and the selection rule, in Python -------------------------------------------------------------------------
class F:
    def __init__(self, begin, end, kind, fcs=None, fcs_at=0, fcs_len=0, block_at=0, desc=0):
        self.begin, self.end, self.kind, self.fcs, self.fcs_at, self.fcs_len, self.block_at, self.desc = begin, end, kind, fcs, fcs_at, fcs_len, block_at, desc


def chain(z, p=0):
    """the frames of z from p on: kind 'skip', 'frame', or 'broken' (the last one: the chain could not go on in it)"""
    out, n = [], len(z)
    while p < n:
        b = p
        if n - p < 4:
            return out + [F(b, p, "broken")]
        magic = int.from_bytes(z[p:p + 4], "little")
        if 0x184D2A50 <= magic <= 0x184D2A5F:
            if n - p < 8:
                return out + [F(b, p, "broken")]
            sl = int.from_bytes(z[p + 4:p + 8], "little")
            p += 8
            if sl > n - p:
                return out + [F(b, p, "broken")]
            p += sl
            out.append(F(b, p, "skip"))
            continue
        if magic != 0xFD2FB528 or n - p < 5:
            return out + [F(b, p, "broken")]
        d = z[p + 4]
        single, did, fc = (d >> 5) & 1, d & 3, d >> 6
        fl = [single, 2, 4, 8][fc]
        hs = 5 + (0 if single else 1) + (4 if did == 3 else did) + fl
        if n - p < hs:
            return out + [F(b, p, "broken")]
        fcs = int.from_bytes(z[p + hs - fl:p + hs], "little") + (256 if fl == 2 else 0) if fl else None
        fcs_at = p + hs - fl
        p += hs
        first = p
        while True:
            if n - p < 3:
                return out + [F(b, p, "broken", fcs)]
            h = int.from_bytes(z[p:p + 3], "little")
            last, typ, size = h & 1, (h >> 1) & 3, h >> 3
            content = 1 if typ == 1 else size
            if typ == 3 or size > (128 << 10) or n - (p + 3) < content:
                return out + [F(b, p, "broken", fcs)]
            p += 3 + content
            if last:
                if d & 4:
                    if n - p < 4:
                        return out + [F(b, n, "broken", fcs)]
                    p += 4
                break
        out.append(F(b, p, "frame", fcs, fcs_at, fl, first, d))
    return out


def select(z, begin, n, anchor=(0, 0)):
    """(src_lo, src_hi, plain_lo, flags, taken frames) by the rule of zg_seek.h"""
    p, pos = anchor
    end = min(begin + n, TOP)
    lo = plo = None
    opened, taken, at = False, [], p
    for f in chain(z, p):
        at = f.end
        if f.kind == "broken":
            if lo is None:
                lo, plo = f.begin, pos
            return lo, len(z), plo, 2 | (1 if opened else 0), taken
        if f.kind == "skip":
            continue
        if lo is None and f.fcs is not None and pos + f.fcs <= begin:
            pos += f.fcs
            continue
        if lo is None:
            lo, plo = f.begin, pos
        taken.append(f)
        if f.fcs is not None:
            pos = min(pos + f.fcs, TOP)
        else:
            opened = True
        if not opened and pos >= end:
            return lo, f.end, plo, 0, taken
    if lo is None:
        return at, at, pos, 4, []
    return lo, at, plo, 1 if opened else 0, taken


_CACHE = {}


def _decode(z, dict_raw=None):
    key = (z, dict_raw)
    if key not in _CACHE:
        _CACHE[key] = oracle_alone(z, zgpu.plaintext_bound(z) + 64, dict_raw)
    return _CACHE[key]


def expect(z, rg, cap=None, dict_raw=None, anchor=(0, 0)):
    """(status, bytes or None) the call must answer for range rg of entry z; cap None: room enough"""
    begin, n = rg
    if n == 0:
        return 0, b""
    lo, hi, plo, flags, taken = select(z, begin, n, anchor)
    if flags & 4:
        return 0, b""
    st, out = _decode(z[lo:hi], dict_raw)
    if st:
        return st, None
    for f in taken:
        if f.fcs is not None and len(_decode(z[f.begin:f.end], dict_raw)[1]) != f.fcs:
            return zgpu.E_CONTENT_SIZE_MISMATCH, None
    clip = out[begin - plo:][:n]
    if cap is not None and len(clip) > cap:
        return zgpu.E_TARGET_TOO_SMALL, None
    return 0, clip


def run_and_check(c, z, ranges, src=None, caps=None, anchors=None, shifts=None, dict_raw=None, entries=None, **kw):
    """ranges[i] of entries[i] (default: all of the one entry z, its source pointer repeated) in ONE call, checked against the model"""
    n = len(ranges)
    entries = entries or [z] * n
    s = src or Sources([z] if entries == [z] * n else entries)
    ptrs = s.ptrs * n if len(s.ptrs) == 1 else s.ptrs
    lens = s.lens * n if len(s.lens) == 1 else s.lens
    exps = [expect(e, rg, None if caps is None else caps[i], dict_raw, anchors[i] if anchors and anchors[i] else (0, 0))
            for i, (e, rg) in enumerate(zip(entries, ranges))]
    if caps is None:
        caps = [(len(d) if d is not None else 4096) + (7 if i % 2 else 0) for i, (_, d) in enumerate(exps)]
    a = Arena(caps, shifts)
    res, seeks = c.decode_ranges_device_src(ptrs, lens, ranges, a.ptrs, caps, anchors=anchors, **kw)
    for i, ((st, d), r, k) in enumerate(zip(exps, res, seeks)):
        assert r.status == st, (i, ranges[i], r, k, st)
        assert r.written == (len(d) if st == 0 else 0), (i, ranges[i], r, k)
        if ranges[i][1] and not k.status:
            lo, hi, plo, flags, taken = select(entries[i], ranges[i][0], ranges[i][1], anchors[i] if anchors and anchors[i] else (0, 0))
            assert (k.src_lo, k.src_hi, k.plain_lo, k.flags) == (lo, hi, plo, flags), (i, ranges[i], k)
            if st == 0:
                assert r.nframes == len(taken), (i, r, k)
    a.check([d for _, d in exps])
    assert s.unchanged()
    return a, res, seeks, exps


# ---- 1: many ranges over one mixed entry ---------------------------------------------------------------------------------------------------
def _mixed_entry():
    import zgdata
    from test_walk_cpu import skippable
    rng = random.Random(0x3A9E)
    sizes = [0, 1, 70000, 300, 0, 65536, 131, 40000, 2, 17] + [rng.randint(0, 70000) for _ in range(30)]
    parts, plains = [], []
    for k, n in enumerate(sizes):
        text = zgdata.text_like(max(n, 1), seed=0x100 + k)[:n]
        parts.append(zgdata.zstd_compress(text, checksum=(k % 3 != 1), content_size=(k not in (31, 37))))
        plains.append(text)
        if k in (3, 18, 33):
            parts.append(skippable(bytes([k]) * (k * 7)))
    return b"".join(parts), plains


def _mixed_ranges(z):
    fr = [f for f in chain(z) if f.kind == "frame"]
    bounds, pos = [0], 0
    for f in fr:
        pos += f.fcs or 0
        bounds.append(pos)
    total = bounds[-1]
    rgs = []
    for k, b in enumerate(bounds):
        rgs += [(max(b - 1, 0), 2), (b, 1), (b + 1, 1)]         # across every boundary, and the single bytes on either side of it
    rgs += [(5, 60000), (70001, 300), (bounds[7], bounds[9] - bounds[7]), (0, total), (0, TOP), (bounds[20] + 3, 1 << 63),
            (total - 1, 1), (total, 1), (total + 5, 9), (12345, 0), (0, 1), (bounds[12], bounds[13] - bounds[12])]
    return rgs


def test_many_ranges_over_one_mixed_entry(ctx):
    z, plains = _mixed_entry()
    assert _decode(z) == (0, b"".join(plains))
    rgs = _mixed_ranges(z)
    assert 120 <= len(rgs) <= 150
    a, res, seeks, exps = run_and_check(ctx, z, rgs, hash_max=ALL)
    st, n = ctx.ranges_stats(), len(rgs)
    assert st["seek_launches"] == 1 and st["seek_bytes_downloaded"] == 64 * n and st["input_bytes_to_host"] == 0
    assert ctx.frames_submits() == 1
    assert st["bytes_written"] == sum(r.written for r in res) and st["frames_decoded"] == sum(r.nframes for r in res)
    assert any(k.open_ended for k in seeks) and any(k.frames_taken == 1 for k in seeks) and any(k.frames_taken > 30 for k in seeks)
    assert all(r.status == 0 for r in res) and all(r.checksum_mismatches == 0 for r in res)


# ---- 2: golden frames ----------------------------------------------------------------------------------------------------------------------
def _golden_entries(n=12):
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = [x for x in sorted(man) if man[x]["size"] <= 300000]
    rng = random.Random(0x601D)
    return [b"".join(pack[x] for x in rng.sample(names, 5)) for _ in range(n)]


def test_golden_frames_random_ranges(ctx):
    rng = random.Random(0x7A46)
    entries, rgs = [], []
    for z in _golden_entries():
        total = sum(f.fcs or 0 for f in chain(z) if f.kind == "frame")
        for _ in range(4):
            entries.append(z)
            b = rng.randint(0, total + 3)
            rgs.append((b, rng.choice([1, 17, 5000, 200000, 1 << 63])))
    a, res, seeks, exps = run_and_check(ctx, None, rgs, entries=entries, hash_max=ALL)
    assert any(k.open_ended for k in seeks) and any(not k.open_ended and k.frames_taken for k in seeks)
    assert sum(r.status == 0 and r.written > 0 for r in res) > 10
    assert ctx.ranges_stats()["seek_launches"] == 1 and ctx.ranges_stats()["input_bytes_to_host"] == 0


# ---- 3: defects ----------------------------------------------------------------------------------------------------------------------------
def _six_frames():
    import zgdata
    plains = [zgdata.text_like(20000 + 111 * k, seed=0x660 + k) for k in range(6)]
    return b"".join(zgdata.zstd_compress(p) for p in plains), plains


def _edit(z, at, f):
    b = bytearray(z)
    b[at] = f(b[at])
    return bytes(b)


def test_defects(ctx):
    z, plains = _six_frames()
    fr = chain(z)
    assert [f.kind for f in fr] == ["frame"] * 6 and all(f.fcs == len(p) for f, p in zip(fr, plains))
    off = [sum(len(p) for p in plains[:k]) for k in range(7)]
    mid = (off[3] + 100, 5000)                                     # inside frame 3
    body1 = _edit(z, fr[1].block_at + 3 + 40, lambda x: x ^ 0xFF)  # (a) a body byte of frame 1
    assert _decode(z[fr[1].begin:fr[1].end]) != _decode(body1[fr[1].begin:fr[1].end])
    head1 = _edit(z, fr[1].block_at, lambda x: x | 6)              # (b) frame 1's first block: the reserved type
    body3 = _edit(z, fr[3].block_at + 3, lambda x: x ^ 0xFF)       # (c) the literals section header of frame 3's first block
    trunc = z[:len(z) - 100]                                       # (d)
    lie3 = _edit(z, fr[3].fcs_at, lambda x: (x + 1) & 255)         # (e) frame 3 declares one byte more
    lie1 = _edit(z, fr[1].fcs_at, lambda x: (x + 5) & 255)         # (f) frame 1 declares five bytes more: everything behind it shifts
    assert chain(lie3)[3].fcs == len(plains[3]) + 1 and chain(lie1)[1].fcs == len(plains[1]) + 5
    entries = [z, body1, head1, z, body3, z, trunc, trunc, lie3, lie1, lie1, z, z]
    rgs = [mid, mid, mid, mid, mid, mid, (off[5] + 7, 100), (off[0] + 7, 100), mid, mid, (off[2] + 2, 4), (off[3] - 1, 2), (off[6] + 5, 9)]
    a, res, seeks, exps = run_and_check(ctx, None, rgs, entries=entries, hash_max=ALL)
    good = plains[3][100:5100]
    assert exps[0] == exps[1] == exps[3] == exps[5] == (0, good)                     # (a): the defect is not seen
    assert res[1].status == 0
    assert exps[2][0] not in (0, zgpu.E_CONTENT_SIZE_MISMATCH) and seeks[2].broken and seeks[2].src_lo == fr[1].begin and seeks[2].src_hi == len(z)   # (b)
    assert exps[4][0] not in (0, zgpu.E_CONTENT_SIZE_MISMATCH) and res[4].written == 0                       # (c)
    assert exps[6][0] != 0 and seeks[6].broken and exps[7] == (0, plains[0][7:107]) and not seeks[7].broken   # (d)
    assert res[8].status == zgpu.E_CONTENT_SIZE_MISMATCH                                                     # (e)
    assert exps[9] == (0, plains[3][95:5095]) and res[9].status == 0                                    # (f): shifted by the lie
    assert res[10].status == zgpu.E_CONTENT_SIZE_MISMATCH                                                    # ... and taken, the lie is found
    assert exps[11] == (0, plains[2][-1:] + plains[3][:1]) and res[11].nframes == 2
    assert exps[12] == (0, b"") and seeks[12].nothing and seeks[12].frames_skipped == 6  # the range lies behind the plaintext


# ---- 4: verify -----------------------------------------------------------------------------------------------------------------------------
def test_verify_acts_on_the_taken_frames_only(ctx):
    z, plains = _six_frames()
    fr = chain(z)
    off = [sum(len(p) for p in plains[:k]) for k in range(7)]
    bad3 = _edit(z, fr[3].end - 1, lambda x: x ^ 0x40)             # frame 3's Content_Checksum
    bad1 = _edit(z, fr[1].end - 1, lambda x: x ^ 0x40)             # frame 1's
    rgs = [(off[3] + 10, 3000)] * 3
    s = Sources([bad3, bad1, z])
    caps = [3000] * 3
    a = Arena(caps)
    res, seeks = ctx.decode_ranges_device_src(s.ptrs, s.lens, rgs, a.ptrs, caps, verify=True)
    assert [(r.status, r.written) for r in res] == [(zgpu.E_CHECKSUM_MISMATCH, 0), (0, 3000), (0, 3000)]
    assert (res[0].checksums, res[0].checksum_mismatches) == (1, 1)
    want = plains[3][10:3010]
    a.check([None, want, want])
    # without the flag the mismatch is counted, and the bytes are written
    a = Arena(caps)
    res, _ = ctx.decode_ranges_device_src(s.ptrs, s.lens, rgs, a.ptrs, caps, hash_max=ALL)
    assert [(r.status, r.checksum_mismatches) for r in res] == [(0, 1), (0, 0), (0, 0)]
    a.check([want] * 3)


# ---- 5: destinations and pointers ----------------------------------------------------------------------------------------------------------
def test_destinations_and_pointers(ctx):
    z, plains = _six_frames()
    whole = b"".join(plains)
    off = [sum(len(p) for p in plains[:k]) for k in range(7)]
    rng = random.Random(0xD57)
    rgs = [(rng.randint(0, len(whole) - 1), rng.choice([1, 15, 16, 17, 33, 4097, 30001])) for _ in range(36)]
    raw = RawSources([b"\x00" * 5, z], [3, 11])                    # the entry ends flush with its allocation
    try:
        shifts = [j % 18 for j in range(36)]
        assert set(shifts) == set(range(18))
        a, res, seeks, exps = run_and_check(ctx, None, rgs, entries=[z] * 36, src=type("S", (), {
            "ptrs": [raw.ptrs[1]], "lens": [raw.lens[1]], "unchanged": raw.unchanged})(), shifts=shifts)
        assert all(r.status == 0 for r in res)
        assert all(d == whole[b:b + n] for (b, n), (_, d) in zip(rgs, exps))
    finally:
        raw.free()
    # caps one byte short, exact, and pointers the contract refuses
    s = Sources([z])
    host_buf = C.create_string_buffer(z, len(z))
    pinned = torch.empty(4096, dtype=torch.uint8).pin_memory()
    rg = (off[2] - 10, 500)
    caps = [499, 500, 500, 500, 500, 500, 500]
    a = Arena(caps)
    ptrs, dsts = s.ptrs * 7, list(a.ptrs)
    ptrs[2] = C.addressof(host_buf)                                # a host pointer as source
    dsts[3] = pinned.data_ptr()                                    # ... as destination
    anchors = [None, None, None, None, (len(z) + 1, 0), (0, rg[0] + 1), None]
    res, seeks = ctx.decode_ranges_device_src(ptrs, s.lens * 7, [rg] * 7, dsts, caps, anchors=anchors)
    assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL, 0, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, 0]
    assert [k.status for k in seeks] == [0, 0, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, 0]
    assert all(k.key() == (0,) * 5 + (zgpu.E_BAD_ARG,) + (0,) * 5 for k in seeks[2:6])
    want = whole[rg[0]:rg[0] + 500]
    a.check([None, want, None, None, None, None, want])
    assert s.unchanged() and host_buf.raw == z


# ---- 6: anchors ----------------------------------------------------------------------------------------------------------------------------
def test_anchors_from_the_frame_table(ctx):
    z, plains = _mixed_entry()
    rgs = [r for r in _mixed_ranges(z) if r[1]]
    s = Sources([z])
    _, _, frames = ctx.frames_table_device(s.ptrs, s.lens)
    anchors = [zgpu.anchor_before(frames, b) for b, _ in rgs]
    assert sum(a != (0, 0) for a in anchors) > len(rgs) // 2
    a1, res1, seeks1, _ = run_and_check(ctx, z, rgs, src=s)
    a2, res2, seeks2, _ = run_and_check(ctx, z, rgs, src=s, anchors=anchors)
    assert torch.equal(a1.t, a2.t)
    smaller = 0
    for i, (x, y, p, q) in enumerate(zip(res1, res2, seeks1, seeks2)):
        assert (x.status, x.written, x.nframes, x.checksums, x.calculated_checksum) == (y.status, y.written, y.nframes, y.checksums, y.calculated_checksum), i
        assert (p.src_lo, p.src_hi, p.plain_lo, p.bound, p.flags) == (q.src_lo, q.src_hi, q.plain_lo, q.bound, q.flags) and q.nblocks <= p.nblocks, i
        smaller += q.nblocks < p.nblocks
    assert smaller > len(rgs) // 2
    near_end = [i for i, (b, _) in enumerate(rgs) if anchors[i][1] > 500000]
    assert near_end and all(seeks2[i].nblocks < seeks1[i].nblocks and seeks2[i].frames_skipped == 0 for i in near_end)


# ---- 7: dictionaries -----------------------------------------------------------------------------------------------------------------------
def test_dictionary_entries_shared_and_alone():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:48]
    entries = [b"".join(pack[n] for n in names[k:k + 6]) for k in range(0, 48, 6)]
    rgs = []
    for k, z in enumerate(entries):
        sizes = [man[n]["size"] for n in names[6 * k:6 * k + 6]]
        rgs.append((sum(sizes[:3]) - 20 + k, sizes[3] // 2 + 40))   # from the end of frame 2 into frame 3
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, seeks, exps = run_and_check(c, None, rgs, entries=entries, dict_raw=rawd, hash_max=ALL)
            assert all(r.status == 0 and r.written == rg[1] for r, rg in zip(res, rgs))
            assert all(k.frames_skipped == 2 and k.frames_taken == 2 for k in seeks)
            alone, st = c.frames_device_stats()["entries_alone"], c.ranges_stats()
            if shared:
                assert alone == 0 and st["input_bytes_to_host"] == 0
            else:
                assert alone == len(entries)
                assert st["input_bytes_to_host"] == sum(k.src_hi - k.src_lo for k in seeks) < sum(len(z) for z in entries)
            assert st["bytes_written"] == sum(rg[1] for rg in rgs)
    finally:
        c.close()


def _set_fcs(z, f, delta):
    v = int.from_bytes(z[f.fcs_at:f.fcs_at + f.fcs_len], "little") + delta
    assert f.fcs_len and 0 <= v < 1 << (8 * f.fcs_len)
    return z[:f.fcs_at] + v.to_bytes(f.fcs_len, "little") + z[f.fcs_at + f.fcs_len:]


def test_an_entry_has_one_verdict_in_a_shared_submit_and_alone():
    """The verdict order of a range — decode and walk, ContentSizeMismatch per frame, TargetTooSmall by the clipped count, then the checksum
    verdict of ZGPU_DEVICE_VERIFY — does not depend on whether the entry's dictionary frames stay in the submit or the entry is decoded alone:
    two taken frames whose false sizes compensate, a taken frame that declares less than it holds, and a corrupted Content_Checksum with caps
    one byte short and exact."""
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:6]
    z = b"".join(pack[n] for n in names)
    sizes = [man[n]["size"] for n in names]
    fr = chain(z)
    assert [f.kind for f in fr] == ["frame"] * 6 and [f.fcs for f in fr] == sizes and all(f.desc & 4 for f in fr)
    rg = (sum(sizes[:3]) - 20, sizes[3] // 2 + 40)                 # frames 2 and 3 are taken
    both = _set_fcs(_set_fcs(z, fr[2], +1), fr[3], -1)             # the selection declares what it holds; neither frame does
    under = _set_fcs(z, fr[3], -1)
    badsum = _edit(z, fr[3].end - 1, lambda x: x ^ 0x40)
    want = b"".join(_decode(z[f.begin:f.end], rawd)[1] for f in fr)[rg[0]:rg[0] + rg[1]]
    assert len(want) == rg[1]
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, seeks, exps = run_and_check(c, None, [rg] * 3, entries=[both, under, z], dict_raw=rawd, hash_max=ALL)
            assert [r.status for r in res] == [zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_CONTENT_SIZE_MISMATCH, 0], shared
            assert c.frames_device_stats()["entries_alone"] == (0 if shared else 3)
            s = Sources([badsum, badsum, z, badsum])
            caps = [rg[1] - 1, rg[1], rg[1], rg[1] - 1]
            a = Arena(caps)
            res, _ = c.decode_ranges_device_src(s.ptrs, s.lens, [rg] * 4, a.ptrs, caps, verify=True)
            assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL, zgpu.E_CHECKSUM_MISMATCH, 0, zgpu.E_TARGET_TOO_SMALL], shared
            assert all(r.written == 0 for r in (res[0], res[1], res[3])) and res[2].written == rg[1]
            a.check([None, None, want, None])
            assert s.unchanged()
            st = c.ranges_stats()                                  # every entry is counted once, delivered or not: 4 x the two taken frames
            assert st["frames_decoded"] == 8 and st["bytes_written"] == rg[1], (shared, st)
    finally:
        c.close()


# ---- 8: selectivity ------------------------------------------------------------------------------------------------------------------------
def test_selectivity_on_512_frames_of_128k(ctx):
    import zgdata
    size, n = 128 << 10, 512
    texts = [zgdata.text_like(size, seed=0x512 + k) for k in range(8)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    z = b"".join(comp[k % 8] for k in range(n))
    src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
    total, mib = n * size, 1 << 20

    def plain(b, m):
        out, k = [], b // size
        while len(b"".join(out)) < m + size:
            out.append(texts[k % 8])
            k += 1
        return b"".join(out)[b % size:][:m]

    _, _, frames = ctx.frames_table_device([src.data_ptr()], [len(z)])
    rows = {}
    for name, b in (("front", 4321), ("middle", total // 2 + 4321), ("end", total - mib)):
        for anchored in (False, True):
            anchor = zgpu.anchor_before(frames, b) if anchored else (0, 0)
            dst = torch.full((mib + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, seeks = ctx.decode_ranges_device_src([src.data_ptr()], [len(z)], [(b, mib)], [dst.data_ptr() + 256], [mib], anchors=[anchor])
            wall = (time.perf_counter() - t0) * 1e3
            st = ctx.ranges_stats()
            assert (res[0].status, res[0].written) == (0, mib), (name, res[0], seeks[0])
            got = dst.cpu().numpy().tobytes()
            assert got[256:256 + mib] == plain(b, mib) and got[:256] == b"\xa5" * 256 and got[256 + mib:] == b"\xa5" * 256
            assert st["frames_decoded"] <= 10 and st["plaintext_decoded"] <= mib + (mib >> 2) + size, (name, st)
            assert st["seek_launches"] == 1 and st["input_bytes_to_host"] == 0 and st["bytes_written"] == mib
            rows[(name, anchored)] = (st["seek_us"], round(wall, 2), st["frames_decoded"], seeks[0].nblocks)
    assert rows[("end", True)][3] < rows[("end", False)][3]
    print("decode_ranges, 512 x 128 KiB, 1 MiB range: (seek us, whole call ms, frames decoded, block headers read)")
    for k, v in rows.items():
        print("  ", k, v)


# ---- 9: equivalence ------------------------------------------------------------------------------------------------------------------------
def test_tensor_call_and_seek_alone_agree_with_the_decode_call(ctx):
    z, plains = _mixed_entry()
    rgs = _mixed_ranges(z)
    s = Sources([z])
    n = len(rgs)
    a, res, seeks, exps = run_and_check(ctx, z, rgs, src=s)
    alone = ctx.frames_seek_device(s.ptrs * n, s.lens * n, rgs)
    st = ctx.ranges_stats()
    assert (st["seek_launches"], st["seek_bytes_downloaded"], st["frames_decoded"], st["bytes_written"]) == (1, 64 * n, 0, 0)
    assert [k.key() for k in alone] == [k.key() for k in seeks]
    view = s.t[s.offs[0]:s.offs[0] + len(z)]
    outs, res2, seeks2 = ctx.decode_tensor_ranges([view] * n, rgs)
    assert [k.key() for k in seeks2] == [k.key() for k in seeks]
    for i, (t, r, r2, (stt, d)) in enumerate(zip(outs, res, res2, exps)):
        assert (r2.status, r2.written, r2.nframes, r2.checksums) == (r.status, r.written, r.nframes, r.checksums), i
        assert t.cpu().numpy().tobytes() == (d or b""), i
        assert t.data_ptr() % 256 == 0
    assert s.unchanged()
