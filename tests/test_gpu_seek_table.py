"""zgpu_decode_ranges_seek_table_device_src / zgpu_frames_seek_table_device (Context.decode_ranges_seek_table_device_src,
frames_seek_table_device, decode_tensor_ranges(seek_table=True)) on the GPU: plaintext bytes [begin, begin + len) of entries in the seekable
format that lie in device memory, selected through the seek table at the entry's end (zg_k_seektab, a wave per entry). The expectation of
every case comes from the oracle on the selection that tests/seektabs.py's model of the rule computes: S = entry[src_lo:src_hi],
_oracle_alone(S) gives the status and the bytes, a selection that decodes to another total than the table promises (or a frame that declares
a size and decodes to another) gives zgpu.E_CONTENT_SIZE_MISMATCH, an unusable table zgpu.E_SEEK_TABLE, and the destination must hold
out[begin - plain_lo:][:len] — with guard bytes, everything behind `written` and every byte of a failed entry's slot untouched."""
import ctypes as C
import random
import struct
import time

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import seektabs
import zgpu
from devmem import ALL, Arena, RawSources, Sources
from golden_io import read_manifest, read_pack
from seektabs import U64, model
from test_gpu_decode_ranges import _decode, _edit, chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def seekable(frames, sizes, lie=None, checksums=None):
    """the frames and their seek table; lie(csizes, dsizes) may falsify the table"""
    cs, ds = [len(f) for f in frames], list(sizes)
    if lie:
        lie(cs, ds)
    return b"".join(frames) + zgpu.seek_table_frame(cs, ds, checksums)


def expect(z, rg, cap=None, dict_raw=None):
    """(status, bytes or None) the call must answer for range rg of entry z; cap None: room enough"""
    begin, n = rg
    rec, _ = model(z, begin, n)
    if n == 0 or (rec[5] == 0 and rec[10] & 4):
        return 0, b""
    if rec[5]:
        return rec[5], None
    lo, hi, plo, bound = rec[:4]
    st, out = _decode(z[lo:hi], dict_raw)
    if st:
        return st, None
    for f in chain(z[lo:hi]):
        if f.kind == "frame" and f.fcs is not None and len(_decode(z[lo + f.begin:lo + f.end], dict_raw)[1]) != f.fcs:
            return zgpu.E_CONTENT_SIZE_MISMATCH, None
    if len(out) != bound:
        return zgpu.E_CONTENT_SIZE_MISMATCH, None
    clip = out[begin - plo:][:n]
    if cap is not None and len(clip) > cap:
        return zgpu.E_TARGET_TOO_SMALL, None
    return 0, clip


def run_and_check(c, entries, ranges, src=None, caps=None, shifts=None, dict_raw=None, **kw):
    """ranges[i] of entries[i] in ONE call (src: the entries' Sources; default: one copy per distinct entry), checked against the model"""
    n = len(ranges)
    if src is None:
        distinct = list(dict.fromkeys(entries))
        s = Sources(distinct)
        at = {z: j for j, z in enumerate(distinct)}
        ptrs, lens = [s.ptrs[at[z]] for z in entries], [s.lens[at[z]] for z in entries]
    else:
        s, ptrs, lens = src, src.ptrs, src.lens
    exps = [expect(e, rg, None if caps is None else caps[i], dict_raw) for i, (e, rg) in enumerate(zip(entries, ranges))]
    if caps is None:
        caps = [(len(d) if d is not None else 4096) + (7 if i % 2 else 0) for i, (_, d) in enumerate(exps)]
    a = Arena(caps, shifts)
    res, seeks = c.decode_ranges_seek_table_device_src(ptrs, lens, ranges, a.ptrs, caps, **kw)
    for i, ((st, d), r, k) in enumerate(zip(exps, res, seeks)):
        assert k.key() == model(entries[i], *ranges[i])[0], (i, ranges[i], k)
        assert r.status == st, (i, ranges[i], r, k, st)
        assert r.written == (len(d) if st == 0 else 0), (i, ranges[i], r, k)
    a.check([d for _, d in exps])
    assert s.unchanged()
    return a, res, seeks, exps


# ---- 1: unsized frames, the real seekable case -----------------------------------------------------------------------------------------------
def _unsized_entry():
    import zgdata
    from test_walk_cpu import skippable
    rng = random.Random(0x5EE4)
    sizes = [0, 1, 20000, 300] + [rng.randint(0, 20000) for _ in range(66)]
    frames, ds, plains = [], [], []
    for k, n in enumerate(sizes):
        text = zgdata.text_like(max(n, 1), seed=0x700 + k)[:n]
        frames.append(zgdata.zstd_compress(text, checksum=(k % 3 == 0), content_size=False))
        ds.append(n)
        plains.append(text)
        if k in (5, 40):
            frames.append(skippable(bytes([k]) * (k * 3)))
            ds.append(0)
    return seekable(frames, ds), ds, plains


def test_unsized_frames_every_boundary_in_one_call(ctx):
    z, ds, plains = _unsized_entry()
    assert len(plains) == 70 and len(ds) == 72 and all(f.fcs is None for f in chain(z) if f.kind == "frame")
    whole = b"".join(plains)
    rgs = seektabs.boundary_ranges(ds)
    n = len(rgs)
    a, res, seeks, exps = run_and_check(ctx, [z] * n, rgs, hash_max=ALL)
    st = ctx.ranges_stats()
    assert st["seek_launches"] == 1 and st["seek_bytes_downloaded"] == 64 * n and st["input_bytes_to_host"] == 0
    assert ctx.frames_submits() == 1
    assert all(r.status == 0 and r.checksum_mismatches == 0 for r in res)
    assert all(d == whole[b:b + m] for (b, m), (_, d) in zip(rgs, exps))
    assert st["bytes_written"] == sum(r.written for r in res) and st["frames_decoded"] == sum(r.nframes for r in res)
    assert any(k.frames_taken == 1 for k in seeks) and any(k.frames_taken >= 70 for k in seeks) and any(k.nothing for k in seeks)
    assert any(k.frames_skipped // 64 != (k.frames_skipped + k.frames_taken - 1) // 64 for k in seeks if k.frames_taken)
    # the tensor call agrees
    s = Sources([z])
    view = s.t[s.offs[0]:s.offs[0] + len(z)]
    outs, res2, seeks2 = ctx.decode_tensor_ranges([view] * 9, rgs[60:69], seek_table=True)
    assert [k.key() for k in seeks2] == [k.key() for k in seeks[60:69]]
    assert [t.cpu().numpy().tobytes() for t in outs] == [d for _, d in exps[60:69]]


# ---- 2: the point of the feature --------------------------------------------------------------------------------------------------------------
def test_the_table_selects_where_the_header_chain_is_open_ended(ctx):
    import zgdata
    size, nf = 16 << 10, 64
    texts = [zgdata.text_like(size, seed=0x160 + k) for k in range(nf)]
    z = seekable([zgdata.zstd_compress(t, content_size=False) for t in texts], [size] * nf)
    whole = b"".join(texts)
    rg = (37 * size + 5000, 20 << 10)
    a, res, seeks, exps = run_and_check(ctx, [z], [rg])
    st = ctx.ranges_stats()
    assert exps[0] == (0, whole[rg[0]:rg[0] + rg[1]]) and res[0].status == 0
    assert st["frames_decoded"] <= 3 and st["plaintext_decoded"] <= 48 << 10, st
    # the header chain cannot skip a frame that declares no size: it takes the first one and everything behind it. This is why the table is needed
    s = Sources([z])
    a = Arena([rg[1]])
    res, seeks = ctx.decode_ranges_device_src(s.ptrs, s.lens, [rg], a.ptrs, [rg[1]])
    st = ctx.ranges_stats()
    assert res[0].status == 0 and seeks[0].open_ended and (seeks[0].src_lo, seeks[0].frames_skipped) == (0, 0)
    assert st["frames_decoded"] == nf and st["plaintext_decoded"] == nf * size, st
    a.check([whole[rg[0]:rg[0] + rg[1]]])


# ---- 3: agreement with zg_k_seek --------------------------------------------------------------------------------------------------------------
def test_agreement_with_the_header_chain_on_sized_frames(ctx):
    import zgdata
    rng = random.Random(0xA62E)
    sizes = [rng.choice([0, 1, 77, 3000]) for _ in range(140)]
    sizes[0], sizes[70] = 5, 0
    frames = [zgdata.zstd_compress(zgdata.text_like(max(n, 1), seed=0x900 + k)[:n], checksum=bool(k % 2)) for k, n in enumerate(sizes)]
    z = seekable(frames, sizes)
    front = b"".join(frames)                                       # the header chain runs over the frames alone: the table frame is the table call's
    assert all(f.kind == "frame" and f.fcs == n for f, n in zip(chain(front), sizes))
    rgs = [r for r in seektabs.boundary_ranges(sizes)]
    n = len(rgs)
    s = Sources([z])
    by_table = ctx.frames_seek_table_device(s.ptrs * n, s.lens * n, rgs)
    st = ctx.ranges_stats()
    assert (st["seek_launches"], st["seek_bytes_downloaded"], st["frames_decoded"], st["bytes_written"]) == (1, 64 * n, 0, 0)
    by_chain = ctx.frames_seek_device(s.ptrs * n, [len(front)] * n, rgs)
    for rg, t, k in zip(rgs, by_table, by_chain):
        assert t.key() == model(z, *rg)[0], (rg, t)
        assert (t.src_lo, t.src_hi, t.plain_lo, t.plain_seen, t.flags) == (k.src_lo, k.src_hi, k.plain_lo, k.plain_seen, k.flags), (rg, t, k)
    assert sum(t.frames_taken > 0 for t in by_table) > 200


# ---- 4: wave-step edges on the device ----------------------------------------------------------------------------------------------------------
def _edge_entries():
    from test_seek_cpu import sized_frame
    rng = random.Random(0xED6E)
    entries, shifts, rgs = [], [], []
    for nf in (1, 63, 64, 65, 129):
        for checksums in (False, True):
            for align in range(4):
                ds = [rng.randint(0, 20) for _ in range(nf)]
                frames = [sized_frame(bytes([65 + k % 26]) * d, checksum=bool(k % 5 == 0)) for k, d in enumerate(ds)]
                z = seekable(frames, ds, checksums=[k * 2654435761 & 0xFFFFFFFF for k in range(nf)] if checksums else None)
                tab = sum(len(f) for f in frames)
                for rg in ((max(sum(ds) - 2, 0), 5), (sum(ds[:nf // 2]), 3)):
                    entries.append(z)
                    shifts.append((align - tab) % 4)
                    rgs.append(rg)
    return entries, shifts, rgs


def test_wave_step_edges_alignments_and_a_flush_end(ctx):
    entries, shifts, rgs = _edge_entries()
    assert len(entries) == 80
    for count in (1, 65):
        e, sh, rg = entries[-count:], shifts[-count:], rgs[-count:]
        run_and_check(ctx, e, rg, src=Sources(e, sh))
    e, sh, rg = entries[:65], shifts[:65], rgs[:65]
    a, res, seeks, exps = run_and_check(ctx, e, rg, src=Sources(e, sh))
    assert all(r.status == 0 for r in res) and sum(r.written > 0 for r in res) > 50
    # entries in an allocation of the runtime's own, the last one ending flush with it, at each alignment
    for k in (33, 62, 79):
        raw = RawSources([b"\x00" * 5, entries[k]], [3, shifts[k]])
        try:
            src = type("S", (), {"ptrs": [raw.ptrs[1]], "lens": [raw.lens[1]], "unchanged": raw.unchanged})()
            a, res, seeks, exps = run_and_check(ctx, [entries[k]], [rgs[k]], src=src)
            assert res[0].status == 0
        finally:
            raw.free()


# ---- 5: false tables --------------------------------------------------------------------------------------------------------------------------
def _six_unsized():
    import zgdata
    plains = [zgdata.text_like(9000 + 111 * k, seed=0x770 + k) for k in range(6)]
    return [zgdata.zstd_compress(p, checksum=True, content_size=False) for p in plains], plains


def test_false_tables_become_a_status(ctx):
    frames, plains = _six_unsized()
    sizes = [len(p) for p in plains]
    good = seekable(frames, sizes)
    n, tab = len(good), sum(len(f) for f in frames)
    off = [sum(sizes[:k]) for k in range(7)]
    mid = (off[3] + 100, 5000)

    def put(at, v):
        return good[:at] + v + good[at + len(v):]
    entries = [
        good,
        put(n - 1, b"\x00"),                                       # NONE
        good[:16],
        put(n - 5, b"\x40"),                                       # RESERVED_BITS
        put(n - 9, struct.pack("<I", 0x8000001)),                  # TOO_LARGE
        put(n - 9, struct.pack("<I", 7000)),
        put(tab + 4, struct.pack("<I", 6 * 8 + 8)),                # BAD_FRAME
        put(tab, b"\x50"),
        seekable(frames, sizes, lie=lambda cs, ds: cs.__setitem__(5, cs[5] + 1)),        # PAST_TABLE: src_hi one byte behind the table's begin
        seekable(frames, sizes, lie=lambda cs, ds: ds.__setitem__(3, ds[3] + 1)),        # a decompressed size off by one, taken
        seekable(frames, sizes, lie=lambda cs, ds: ds.__setitem__(3, ds[3] - 1)),
        seekable(frames, sizes, lie=lambda cs, ds: cs.__setitem__(2, cs[2] + 9)),        # src_lo lands inside frame 3
        seekable(frames, sizes, lie=lambda cs, ds: cs.__setitem__(3, cs[3] - 4)),        # src_hi cuts frame 3's checksum off
        seekable(frames, sizes, lie=lambda cs, ds: ds.__setitem__(1, ds[1] + 5)),        # a false size in front of the range: shifts, silently
        good,
    ]
    rgs = [mid] * len(entries)
    rgs[8] = (off[5] + 1, 10)
    a, res, seeks, exps = run_and_check(ctx, entries, rgs, hash_max=ALL)
    whys = [zgpu.SEEKTAB_NONE, zgpu.SEEKTAB_NONE, zgpu.SEEKTAB_RESERVED_BITS, zgpu.SEEKTAB_TOO_LARGE, zgpu.SEEKTAB_TOO_LARGE,
            zgpu.SEEKTAB_BAD_FRAME, zgpu.SEEKTAB_BAD_FRAME, zgpu.SEEKTAB_PAST_TABLE]
    for i, why in enumerate(whys, 1):
        assert (res[i].status, res[i].written, seeks[i].status, seeks[i].why) == (zgpu.E_SEEK_TABLE, 0, zgpu.E_SEEK_TABLE, why), (i, res[i], seeks[i])
        assert seeks[i].key() == (0,) * 5 + (zgpu.E_SEEK_TABLE, 0, 0, 0, why, 0)
    want = plains[3][100:5100]
    assert exps[0] == exps[14] == (0, want) and res[0].status == res[14].status == 0     # the others of the call are unaffected
    assert res[9].status == res[10].status == zgpu.E_CONTENT_SIZE_MISMATCH
    assert exps[11][0] not in (0, zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_SEEK_TABLE) and res[11].status == exps[11][0]   # the oracle's verdict on those bytes
    assert res[12].status == exps[12][0]
    assert exps[13] == (0, plains[3][95:5095]) and res[13].status == 0
    # a range with an anchor: the table is the index, there is nothing to anchor
    s = Sources([good])
    srcs, lens = (C.c_void_p * 2)(s.ptrs[0], s.ptrs[0]), (C.c_size_t * 2)(n, n)
    rg, out = (zgpu.RangeC * 2)(zgpu.RangeC(mid[0], mid[1], 0, 1), zgpu.RangeC(mid[0], mid[1], 0, 0)), (zgpu.SeekC * 2)()
    assert ctx.L.zgpu_frames_seek_table_device(ctx.h, srcs, lens, 2, rg, out) == 0
    assert zgpu.Seek(out[0]).key() == (0,) * 5 + (zgpu.E_BAD_ARG,) + (0,) * 5 and zgpu.Seek(out[1]).key() == model(good, *mid)[0]
    rg[0] = zgpu.RangeC(mid[0], mid[1], 8, 0)
    a = Arena([5000, 5000])
    dsts, caps, rr = (C.c_void_p * 2)(*a.ptrs), (C.c_size_t * 2)(5000, 5000), (zgpu.RangeResultC * 2)()
    assert ctx.L.zgpu_decode_ranges_seek_table_device_src(ctx.h, srcs, lens, 2, rg, dsts, caps, None, rr) == 0
    assert (rr[0].d.r.status, rr[0].seek.status, rr[1].d.r.status, rr[1].d.r.written) == (zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, 0, 5000)
    a.check([None, want])


# ---- 6: capacities and verify -----------------------------------------------------------------------------------------------------------------
def test_capacities_and_verify(ctx):
    frames, plains = _six_unsized()
    sizes = [len(p) for p in plains]
    off = [sum(sizes[:k]) for k in range(7)]
    ends = [sum(len(f) for f in frames[:k + 1]) for k in range(6)]
    good = seekable(frames, sizes)
    bad3 = _edit(good, ends[3] - 1, lambda x: x ^ 0x40)            # frame 3's Content_Checksum
    bad1 = _edit(good, ends[1] - 1, lambda x: x ^ 0x40)            # frame 1's: in front of the range
    body1 = _edit(good, ends[0] + 40, lambda x: x ^ 0xFF)          # a body byte of frame 1
    rg = (off[3] - 10, 3000)                                       # frames 2 and 3
    want = b"".join(plains)[rg[0]:rg[0] + 3000]
    entries, caps = [good, good, bad3, bad1, body1, bad3], [2999, 3000, 3000, 3000, 3000, 2999]
    s = Sources(entries)
    a = Arena(caps)
    res, seeks = ctx.decode_ranges_seek_table_device_src(s.ptrs, s.lens, [rg] * 6, a.ptrs, caps, verify=True)
    assert [(r.status, r.written) for r in res] == [(zgpu.E_TARGET_TOO_SMALL, 0), (0, 3000), (zgpu.E_CHECKSUM_MISMATCH, 0), (0, 3000), (0, 3000),
                                                    (zgpu.E_TARGET_TOO_SMALL, 0)]
    assert (res[2].checksums, res[2].checksum_mismatches) == (2, 1) and all(k.frames_taken == 2 for k in seeks)
    a.check([None, want, None, want, want, None])
    assert s.unchanged()
    # without the flag the mismatch is counted, and the bytes are written
    a, res, seeks, exps = run_and_check(ctx, entries[2:5], [rg] * 3, hash_max=ALL)
    assert [(r.status, r.checksum_mismatches) for r in res] == [(0, 1), (0, 0), (0, 0)]


# ---- 7: dictionaries ----------------------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_shared_and_alone():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:24]
    entries, rgs = [], []
    for k in range(0, 24, 6):
        sizes = [man[n]["size"] for n in names[k:k + 6]]
        frames = [pack[n] for n in names[k:k + 6]]
        entries.append(seekable(frames, sizes))
        rgs.append((sum(sizes[:3]) - 20 + k, sizes[3] // 2 + 40))   # from the end of frame 2 into frame 3
    sizes = [man[n]["size"] for n in names[:6]]
    entries.append(seekable([pack[n] for n in names[:6]], sizes, lie=lambda cs, ds: ds.__setitem__(2, ds[2] + 1)))
    rgs.append(rgs[0])
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, seeks, exps = run_and_check(c, entries, rgs, dict_raw=rawd, hash_max=ALL)
            assert [r.status for r in res] == [0, 0, 0, 0, zgpu.E_CONTENT_SIZE_MISMATCH], shared
            assert all(r.written == rg[1] for r, rg in zip(res[:4], rgs)) and all(k.frames_skipped == 2 and k.frames_taken == 2 for k in seeks)
            alone, st = c.frames_device_stats()["entries_alone"], c.ranges_stats()
            assert alone == (0 if shared else 5) and (st["input_bytes_to_host"] == 0) == bool(shared)
            got.append(([(r.status, r.written, r.nframes) for r in res], a.t.cpu().numpy().tobytes()))
        assert got[0] == got[1]
    finally:
        c.close()


# ---- 8: what it costs (printed; LABNOTES "seek_table" holds a run's values) ----------------------------------------------------------------------
def test_selectivity_on_512_frames_of_128k(ctx):
    import zgdata
    size, n = 128 << 10, 512
    texts = [zgdata.text_like(size, seed=0x512 + k) for k in range(8)]
    total, mib = n * size, 1 << 20

    def plain(b, m):
        out, k = [], b // size
        while sum(len(x) for x in out) < m + size:
            out.append(texts[k % 8])
            k += 1
        return b"".join(out)[b % size:][:m]

    rows = {}
    for sized in (True, False):
        comp = [zgdata.zstd_compress(t, content_size=sized) for t in texts]
        z = seekable([comp[k % 8] for k in range(n)], [size] * n)
        src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
        ptr, ln = [src.data_ptr()], [len(z)]
        frames = ctx.frames_table_device(ptr, ln)[2] if sized else None
        for name, b in (("front", 4321), ("middle", total // 2 + 4321), ("end", total - mib - size)):
            for how in ("table", "chain", "chain anchored"):
                if how == "chain anchored" and not sized:
                    continue
                dst = torch.full((mib + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if how == "table":
                    res, seeks = ctx.decode_ranges_seek_table_device_src(ptr, ln, [(b, mib)], [dst.data_ptr() + 256], [mib])
                else:
                    anchor = zgpu.anchor_before(frames, b) if how == "chain anchored" else (0, 0)
                    res, seeks = ctx.decode_ranges_device_src(ptr, ln, [(b, mib)], [dst.data_ptr() + 256], [mib], anchors=[anchor])
                wall = (time.perf_counter() - t0) * 1e3
                st = ctx.ranges_stats()
                assert (res[0].status, res[0].written) == (0, mib), (sized, name, how, res[0], seeks[0])
                got = dst.cpu().numpy().tobytes()
                assert got[256:256 + mib] == plain(b, mib) and got[:256] == b"\xa5" * 256 and got[256 + mib:] == b"\xa5" * 256
                assert st["seek_launches"] == 1 and st["input_bytes_to_host"] == 0 and st["bytes_written"] == mib
                if how == "table":
                    assert st["frames_decoded"] <= 9 and st["plaintext_decoded"] <= mib + size, (sized, name, st)
                    assert seeks[0].key() == model(z, b, mib)[0]
                elif not sized:
                    assert seeks[0].open_ended and st["frames_decoded"] == n
                rows[("sized" if sized else "unsized", name, how)] = (st["seek_us"], round(wall, 2), st["frames_decoded"])
    print("seek_table, 512 x 128 KiB, 1 MiB range: (seek kernel us, whole call ms, frames decoded)")
    for k, v in rows.items():
        print("  ", k, v)
