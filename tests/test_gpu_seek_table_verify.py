"""ZGPU_DEVICE_VERIFY_SEEK_TABLE on the GPU (Context.decode_ranges_seek_table_device_src(verify_table=True), decode_tensor_ranges(seek_table=True,
verify_table=True)): the Checksum fields of an entry's seek table enforced on the device by zg_k_seeksums. Small on purpose: frames of 0 - 20
plaintext bytes, each call a few milliseconds. The expectation of every case comes from the oracle on the selection that tests/seektabs.py's
model computes (test_gpu_seek_table.expect: the answer without the flag) plus tests/seeksums.py's model of the rule on the frames of that
selection: a table that does not vouch for them gives zgpu.E_SEEK_CHECKSUM_MISMATCH behind every other verdict, written = nframes = 0, the
counts the model says, and — destinations lie in an Arena with guard bytes — every byte of the failed entry's slot untouched, as is every
byte behind `written` of the others."""
import ctypes as C
import random
import struct

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import seeksums
import zgpu
from devmem import Arena, RawSources, Sources, xxh32, xxh64
from golden_io import read_manifest, read_pack
from seektabs import model as seek_model
from test_gpu_decode_ranges import _decode, _edit, chain
from test_gpu_seek_table import expect, seekable
from test_seek_cpu import sized_frame
from test_walk_cpu import skippable

pytestmark = pytest.mark.gpu
BAD = zgpu.E_SEEK_CHECKSUM_MISMATCH


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def checked_frame(payload):
    """sized_frame with a Content_Checksum that holds"""
    return sized_frame(payload, checksum=True)[:-4] + struct.pack("<I", xxh32(payload))


def payload(k, n):
    return bytes((37 * k + 11 * i + 1) & 0xFF for i in range(n))


def table(frames, plains, flip=(), checksums=True, lie=None):
    """the frames and a seek table whose Checksum fields are those of plains (None: a skippable frame, entered with size 0 and checksum 0);
    flip: rows whose checksum gets one false bit"""
    sums = [(xxh32(p) if p is not None else 0) ^ (0x100 if k in flip else 0) for k, p in enumerate(plains)]
    return seekable(frames, [len(p) if p is not None else 0 for p in plains], lie=lie, checksums=sums if checksums else None)


def expect_verified(z, rg, cap=None, dict_raw=None, hash_max=0, verify=False):
    """(status, bytes or None, counts or None): expect()'s answer, then the checksum verdict of verify, then the table's, which ranks last.
    counts: (checksums, checksum_mismatches, checksums_unverified) of an entry the table failed"""
    st, data = expect(z, rg, cap, dict_raw)
    rec = seek_model(z, *rg)[0]
    if st or rg[1] == 0 or rec[7] == 0:
        return st, data, None
    lo, hi, first, taken = rec[0], rec[1], rec[6], rec[7]
    frames, digests = [], []
    for f in chain(z[lo:hi]):
        if f.kind != "frame":
            continue
        plain = _decode(z[lo + f.begin:lo + f.end], dict_raw)[1]
        if verify and z[lo + f.begin + 4] & 4 and z[lo + f.end - 4:lo + f.end] != struct.pack("<I", xxh32(plain)):
            return zgpu.E_CHECKSUM_MISMATCH, None, None
        hashed = hash_max == 0 or len(plain) <= hash_max
        frames.append((f.begin, f.end - f.begin, len(digests) if hashed else None))
        if hashed:
            digests.append(xxh64(plain))
    if not frames:
        return st, data, None
    srec = seeksums.model(z, first, taken, frames, digests)[0]
    assert srec[5] == 0
    if seeksums.vouched(srec, len(frames)):
        return 0, data, (srec[2], 0, 0)
    return BAD, None, seeksums.failed_counts(srec, len(frames))


def run(c, entries, ranges, src=None, caps=None, shifts=None, dict_raw=None, hash_max=0, verify=False, flag=True):
    """ranges[i] of entries[i] in ONE call with the flag, checked against the models; (arena, results, expectations)"""
    s = src or Sources(entries, shifts)
    exps = [expect_verified(e, rg, None if caps is None else caps[i], dict_raw, hash_max, verify) if flag else expect(e, rg, None, dict_raw) + (None,)
            for i, (e, rg) in enumerate(zip(entries, ranges))]
    if caps is None:   # room for what the entry yields without the flag: TARGET_TOO_SMALL would rank in front of the table's verdict
        room = [expect(e, rg, None, dict_raw)[1] for e, rg in zip(entries, ranges)]
        caps = [(len(d) if d is not None else 64) + (7 if i % 2 else 0) for i, d in enumerate(room)]
    a = Arena(caps)
    res, seeks = c.decode_ranges_seek_table_device_src(s.ptrs, s.lens, ranges, a.ptrs, caps, hash_max=hash_max, verify=verify, verify_table=flag)
    for i, ((st, d, counts), r, k) in enumerate(zip(exps, res, seeks)):
        assert k.key() == seek_model(entries[i], *ranges[i])[0], (i, k)        # the selection's record stays, failed or not
        assert r.status == st, (i, ranges[i], r, st, counts)
        assert r.written == (len(d) if st == 0 else 0), (i, r)
        if st == BAD:
            assert (r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified) == (0,) + counts, (i, r, counts)
            assert (r.checksum_from_data, r.calculated_checksum, r.first_hashed) == (0, 0, 0), (i, r)
    a.check([x[1] for x in exps])
    assert s.unchanged()
    return a, res, exps


def six(n=20):
    plains = [payload(k, n) for k in range(6)]
    return [sized_frame(p) for p in plains], plains


# ---- 1: the case no existing check catches -------------------------------------------------------------------------------------------------------
def test_two_swapped_frames_of_equal_size(ctx):
    frames, plains = six()
    good = table(frames, plains)
    sw = list(frames)
    sw[2], sw[3] = sw[3], sw[2]
    swapped = b"".join(sw) + good[len(b"".join(frames)):]           # the table of the original order
    assert len(swapped) == len(good) and swapped != good
    rg = (25, 70)                                                   # frames 1 .. 4
    swapped_plain = b"".join(plains[k] for k in (0, 1, 3, 2, 4, 5))[25:95]
    # sizes, total and (absent) content checksums all agree: without the flag nothing is noticed
    a, res, exps = run(ctx, [good, swapped], [rg, rg], flag=False)
    assert [r.status for r in res] == [0, 0] and exps[1][1] == swapped_plain != exps[0][1]
    for order in ([good, swapped, good], [swapped, good, good]):
        a, res, exps = run(ctx, order, [rg] * 3)
        bad = order.index(swapped)
        assert [r.status for r in res] == [BAD if i == bad else 0 for i in range(3)]
        assert (res[bad].checksums, res[bad].checksum_mismatches, res[bad].checksums_unverified) == (4, 2, 0)
        st = ctx.ranges_stats(verify_table=True)
        assert (st["compare_launches"], st["compare_bytes_downloaded"], st["frames_compared"], st["entries_failed_table"]) == (1, 96, 12, 1)
        assert st["input_bytes_to_host"] == 0 and ctx.frames_device_stats(verify=True)["entries_failed_verify"] == 0


# ---- 2: wave-step edges ------------------------------------------------------------------------------------------------------------------------------
def _edge(taken, align, flip=(), rng=None):
    """an entry of taken + 2 frames whose rows 1 .. taken are the selection, its table at `align` mod 4 (the shift), the range"""
    rng = rng or random.Random(taken * 8 + align)
    plains = [payload(k, rng.randint(1, 20)) for k in range(taken + 2)]
    frames = [checked_frame(p) if k % 5 == 0 else sized_frame(p) for k, p in enumerate(plains)]
    z = table(frames, plains, flip=[1 + k for k in flip])
    tab = sum(len(f) for f in frames)
    return z, (align - tab) % 4, (len(plains[0]), sum(len(p) for p in plains[1:taken + 1]))


def test_wave_step_edges_alignments_and_a_flush_end(ctx):
    entries, shifts, rgs, want = [], [], [], []
    for taken in (1, 63, 64, 65, 129):
        for align in range(4):
            z, sh, rg = _edge(taken, align)
            entries.append(z); shifts.append(sh); rgs.append(rg); want.append(0)
    for taken, rows in ((1, (0,)), (65, (0, 63, 64)), (129, (0, 63, 64, 128))):
        for k in rows:
            z, sh, rg = _edge(taken, k % 4, flip=(k,))
            entries.append(z); shifts.append(sh); rgs.append(rg); want.append(BAD)
    a, res, exps = run(ctx, entries, rgs, shifts=shifts)
    assert [r.status for r in res] == want
    assert all(seek_model(z, *rg)[0][6:8] == (1, t) for z, rg, t in zip(entries[::4][:5], rgs[::4][:5], (1, 63, 64, 65, 129)))
    assert all((r.checksum_mismatches, r.checksums_unverified) == (1, 0) for r, w in zip(res, want) if w)
    st = ctx.ranges_stats(verify_table=True)
    assert st["compare_launches"] == 1 and st["compare_bytes_downloaded"] == 32 * len(entries) and st["entries_failed_table"] == 8
    # an entry that ends flush with an allocation of the runtime's own: a good one and one whose last row differs
    for flip in ((), (128,)):
        z, sh, rg = _edge(129, 3, flip=flip)
        raw = RawSources([b"\x00" * 5, z], [3, sh])
        try:
            src = type("S", (), {"ptrs": [raw.ptrs[1]], "lens": [raw.lens[1]], "unchanged": raw.unchanged})()
            a, res, exps = run(ctx, [z], [rg], src=src)
            assert res[0].status == (BAD if flip else 0)
        finally:
            raw.free()


# ---- 3: what is deliberately not seen or not compared -----------------------------------------------------------------------------------------------
def test_rows_that_are_not_looked_at_and_the_empty_frame(ctx):
    frames, plains = six()
    skip = skippable(b"xyz")
    fr, pl = frames[:3] + [skip] + frames[3:], plains[:3] + [None] + plains[3:]
    rg = (45, 50)                                                   # frames 2 .. 4 of the six, the skippable frame's row between them
    in_front = table(fr, pl, flip=(0, 1))                           # false checksums in rows in front of the range
    in_skip = table(fr, pl, flip=(3,))                              # ... and in the skippable frame's row inside it
    behind = table(fr, pl, flip=(6,))
    taken = table(fr, pl, flip=(4,))
    assert seek_model(in_skip, *rg)[0][6:8] == (2, 4)
    # a zero-size zstd frame is a decoded frame like any other: its row must hold the XXH64 of nothing
    empty = sized_frame(b"")
    fe, pe = frames[:3] + [empty] + frames[3:], plains[:3] + [b""] + plains[3:]
    with_empty, false_empty = table(fe, pe), table(fe, pe, flip=(3,))
    assert xxh32(b"") == seeksums.EMPTY_XXH32 == 0x51D8E999
    assert struct.unpack_from("<I", with_empty, sum(len(f) for f in fe) + 8 + 3 * 12 + 8)[0] == 0x51D8E999
    a, res, exps = run(ctx, [in_front, in_skip, behind, taken, with_empty, false_empty], [rg] * 6)
    assert [r.status for r in res] == [0, 0, 0, BAD, 0, BAD]
    assert (res[3].checksums, res[3].checksum_mismatches) == (3, 1) and (res[5].checksums, res[5].checksum_mismatches) == (4, 1)
    assert exps[0][1] == b"".join(plains)[45:95] == exps[4][1]


# ---- 4: tables without checksums ------------------------------------------------------------------------------------------------------------------------
def test_a_table_without_checksums_vouches_for_nothing(ctx):
    frames, plains = six()
    bare, good = table(frames, plains, checksums=False), table(frames, plains)
    rg = (25, 70)
    a, res, exps = run(ctx, [bare, good, bare], [rg, rg, (5, 0)])
    assert [r.status for r in res] == [BAD, 0, 0]                   # (a range of length 0 reads nothing and asks nothing of the table)
    assert (res[0].checksums, res[0].checksum_mismatches, res[0].checksums_unverified) == (0, 0, 4)
    a, res, exps = run(ctx, [bare, good], [rg, rg], flag=False)
    assert [r.status for r in res] == [0, 0]


# ---- 5: ranks ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_verdict_ranks_last(ctx):
    plains = [payload(k, 20) for k in range(6)]
    frames = [checked_frame(p) for p in plains]
    rg = (25, 70)
    flipped = table(frames, plains, flip=(2,))
    ends = [sum(len(f) for f in frames[:k + 1]) for k in range(6)]
    false_size = table(frames, plains, flip=(2,), lie=lambda cs, ds: ds.__setitem__(3, ds[3] + 1))
    bad_content = _edit(flipped, ends[3] - 1, lambda x: x ^ 0x40)   # frame 3's Content_Checksum
    reserved = _edit(flipped, ends[0] + 6, lambda x: x | 6)         # frame 1's block: the reserved type
    entries = [flipped, false_size, bad_content, reserved, flipped]
    caps = [69, 70, 70, 70, 70]
    a, res, exps = run(ctx, entries, [rg] * 5, caps=caps, verify=True)
    assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL, zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_CHECKSUM_MISMATCH, zgpu.E_RESERVED_BLOCK, BAD]
    assert (res[2].checksums, res[2].checksum_mismatches) == (4, 1) and (res[4].checksums, res[4].checksum_mismatches) == (4, 1)
    st, dv = ctx.ranges_stats(verify_table=True), ctx.frames_device_stats(verify=True)
    assert st["entries_failed_table"] == 1 and dv["entries_failed_verify"] == 1 and st["compare_launches"] == 1


# ---- 6: bounded hashing -----------------------------------------------------------------------------------------------------------------------------
def test_a_frame_longer_than_hash_max_passes_uncompared(ctx):
    sizes = [10, 10, 20, 10, 7, 10]
    plains = [payload(k, n) for k, n in enumerate(sizes)]
    frames = [sized_frame(p) for p in plains]
    rg = (10, 45)                                                   # frames 1 .. 4
    long_false, short_false = table(frames, plains, flip=(2,)), table(frames, plains, flip=(4,))
    a, res, exps = run(ctx, [long_false, short_false, long_false], [rg, rg, (25, 3)], hash_max=10)
    assert [r.status for r in res] == [0, BAD, 0]
    assert (res[1].checksums, res[1].checksum_mismatches, res[1].checksums_unverified) == (3, 1, 1)
    st = ctx.ranges_stats(verify_table=True)
    assert st["frames_compared"] == sum(x[2][0] for x in exps) == 3 + 3 + 0
    # with no bound (hash_max 0) the long frame is compared
    a, res, exps = run(ctx, [long_false], [rg])
    assert res[0].status == BAD and ctx.ranges_stats(verify_table=True)["frames_compared"] == 4


# ---- 7: the flag on the wrong call ------------------------------------------------------------------------------------------------------------------
def test_the_flag_is_refused_where_there_is_no_table_and_with_no_hash():
    frames, plains = six()
    z = table(frames, plains)
    c = zgpu.Context(0)                                             # a context of its own: its counters have never been written
    try:
        s, a = Sources([z]), Arena([64])
        n = 1
        srcs, lens, dsts, caps = (C.c_void_p * n)(*s.ptrs), (C.c_size_t * n)(*s.lens), (C.c_void_p * n)(*a.ptrs), (C.c_size_t * n)(64)
        host = (C.c_char_p * n)(z)
        rg, res, dres = (zgpu.RangeC * n)(zgpu.RangeC(25, 30, 0, 0)), (zgpu.RangeResultC * n)(), (zgpu.DeviceEntryResultC * n)()
        for flags in (4, 6):
            o = C.byref(zgpu.DeviceOptsC(0, flags, 0))
            assert c.L.zgpu_decode_frames_device(c.h, C.cast(host, C.POINTER(C.c_void_p)), lens, n, dsts, caps, o, dres) == zgpu.E_BAD_ARG
            assert c.L.zgpu_decode_frames_device_src(c.h, srcs, lens, n, dsts, caps, o, dres) == zgpu.E_BAD_ARG
            assert c.L.zgpu_decode_ranges_device_src(c.h, srcs, lens, n, rg, dsts, caps, o, res) == zgpu.E_BAD_ARG
        with pytest.raises(zgpu.ZgpuError) as e:
            c.decode_ranges_seek_table_device_src(s.ptrs, s.lens, [(25, 30)], a.ptrs, [64], no_hash=True, verify_table=True)
        assert e.value.status == zgpu.E_BAD_ARG
        every = [c.ranges_stats(verify_table=True), c.frames_device_stats(verify=True), c.frames_device_src_stats(), c.frames_dict_stats()]
        assert all(v == 0 for d in every for v in d.values()) and c.frames_submits() == 0, every
        a.check([None])
        # the same context then serves the call that has a table
        res, seeks = c.decode_ranges_seek_table_device_src(s.ptrs, s.lens, [(25, 30)], a.ptrs, [64], verify_table=True)
        assert (res[0].status, res[0].written) == (0, 30)
        a.check([b"".join(plains)[25:55]])
    finally:
        c.close()


# ---- 8: dictionary frames ---------------------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_shared_and_alone_agree():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:12]
    entries, rgs = [], []
    for k, flip in ((0, ()), (6, ()), (0, (3,)), (6, (2,)), (0, (1,))):
        fr = [pack[n] for n in names[k:k + 6]]
        pl = [_decode(f, rawd)[1] for f in fr]
        assert [len(p) for p in pl] == [man[n]["size"] for n in names[k:k + 6]]
        entries.append(table(fr, pl, flip=flip))
        rgs.append((sum(len(p) for p in pl[:3]) - 20, len(pl[3]) // 2 + 40))   # from the end of frame 2 into frame 3
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, exps = run(c, entries, rgs, dict_raw=rawd)
            assert [r.status for r in res] == [0, 0, BAD, BAD, 0], shared            # (a false checksum in a row in front of the range is not seen)
            assert all((r.checksums, r.checksum_mismatches, r.checksums_unverified) == (2, 1, 0) for r in res[2:4])
            alone, st = c.frames_device_stats()["entries_alone"], c.ranges_stats(verify_table=True)
            assert alone == (0 if shared else 5) and (st["input_bytes_to_host"] == 0) == bool(shared)
            assert st["compare_launches"] == (1 if shared else 0) and st["entries_failed_table"] == 2 and st["frames_compared"] == 10
            got.append(([(r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified) for r in res],
                        a.t.cpu().numpy().tobytes()))
        assert got[0] == got[1]
    finally:
        c.close()


# ---- 9: stats and the tensor call -------------------------------------------------------------------------------------------------------------------
def test_stats_and_the_tensor_call(ctx):
    frames, plains = six()
    good, flipped = table(frames, plains), table(frames, plains, flip=(3,))
    whole = b"".join(plains)
    entries = [good, flipped, good, good[:len(good) - 1] + b"\x00", good]
    rgs = [(25, 70), (25, 70), (5, 0), (25, 70), (500, 3)]          # a range of length 0, an entry without a table, a range behind the plaintext
    a, res, exps = run(ctx, entries, rgs)
    assert [r.status for r in res] == [0, BAD, 0, zgpu.E_SEEK_TABLE, 0]
    st = ctx.ranges_stats(verify_table=True)
    # one compare launch for the submit; only the entries of which frames were decoded have a wave, 32 bytes each
    assert (st["compare_launches"], st["compare_bytes_downloaded"], st["frames_compared"], st["entries_failed_table"]) == (1, 64, 8, 1)
    assert st["input_bytes_to_host"] == 0 and st["seek_launches"] == 1 and ctx.frames_submits() == 1
    assert ctx.ranges_stats() == {k: v for k, v in list(st.items())[:8]}
    # without the flag: no compare launch, the same bytes
    a, res, exps = run(ctx, entries[:2], rgs[:2], flag=False)
    st = ctx.ranges_stats(verify_table=True)
    assert [r.status for r in res] == [0, 0] and (st["compare_launches"], st["compare_bytes_downloaded"], st["frames_compared"]) == (0, 0, 0)
    # the tensor call agrees
    s = Sources([good, flipped])
    views = [s.t[o:o + n] for o, n in zip(s.offs, s.lens)]
    outs, res2, seeks2 = ctx.decode_tensor_ranges(views, rgs[:2], seek_table=True, verify_table=True)
    assert [r.status for r in res2] == [0, BAD] and [t.cpu().numpy().tobytes() for t in outs] == [whole[25:95], b""]
    assert (res2[1].checksums, res2[1].checksum_mismatches, res2[1].checksums_unverified) == (4, 1, 0)
    outs, res2, seeks2 = ctx.decode_tensor_ranges(views, rgs[:2], seek_table=True)
    assert [r.status for r in res2] == [0, 0] and [t.cpu().numpy().tobytes() for t in outs] == [whole[25:95]] * 2
    with pytest.raises(ValueError):
        ctx.decode_tensor_ranges(views, rgs[:2], verify_table=True)
