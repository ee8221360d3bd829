"""Seek index handles on the GPU (zgpu_seek_index_create_device, zgpu_frames_seek_indexed_device, zgpu_gather_ranges_indexed_device_src;
Context.seek_index, frames_seek_indexed_device, gather_ranges_indexed_device_src, gather_tensor_ranges(index=...)): per entry the prefix sums
of its rows built once on the device — from its seek table, or from its header chain where every frame declares its size — and reused by any
number of gather calls. No expectation comes from the calls under test: a table-kind entry must answer what the existing seek-table calls
answer, field for field and byte for byte; a declared-kind entry's rows are tests/seekidx.py's model (parsed from the bytes in Python), its
records that model's rule and what frames_seek_device answers, its groups tests/seekmany.py's model of the contract, and a group's status and
bytes the oracle's on the rows the group takes, held to the sizes the frames declare. Destinations have guard bytes and odd alignments
(devmem.Arena), and every byte of a failed range's slot and behind `written` must be untouched."""
import os
import random
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import seekidx
import seekmany
import seektabs
import zgpu
from devmem import ALL, Arena, Sources, full_key, xxh32
from golden_io import read_manifest, read_pack
from seekidx import U64
from test_gpu_decode_ranges import _decode, _edit, chain
from test_gpu_gather_ranges import BAD_ARG_REC, Rec, _eight_frames, group_verdict, range_verdicts, run_checked
from test_gpu_seek_table import _unsized_entry, seekable
from test_walk_cpu import skippable

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: the workload generators
pytestmark = pytest.mark.gpu
FIVE = (0, 1, 2, 4)   # src_lo, src_hi, plain_lo, plain_seen of a Seek key; flag bit 2 besides


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def _eight_declared(size=4096, checksum=False):
    """_eight_frames' plaintexts, every frame declaring its size"""
    import zgdata
    plains = [zgdata.text_like(size, seed=0x3A0 + k) for k in range(8)]
    return [zgdata.zstd_compress(p, checksum=checksum, content_size=True) for p in plains], plains


def _six_declared():
    import zgdata
    plains = [zgdata.text_like(9000 + 111 * k, seed=0x770 + k) for k in range(6)]
    return [zgdata.zstd_compress(p, checksum=True, content_size=True) for p in plains], plains


def expectations(entries, ranges, caps=None, dict_raw=None, group_status=None, indexed=None, now=None):
    """(records, groups, group_of, [(status, bytes or None)]) of declared-kind entries. indexed: the bytes the index was built from (default:
    entries); now: the bytes the entries hold when the gather runs (default: the same)"""
    indexed = indexed or entries
    now = now or entries
    idx = [seekidx.index(z) for z in indexed]
    recs = []
    for r in ranges:
        if r[0] >= len(entries) or (len(r) > 3 and r[3]):
            recs.append(BAD_ARG_REC)
            continue
        why, C_, D_ = idx[r[0]]
        if why:
            recs.append((0,) * 5 + (zgpu.E_FRAME_INDEX, 0, 0, 0, why, 0) if r[2] else (0,) * 11)
        else:
            recs.append(seekidx.record(C_, D_, len(indexed[r[0]]), r[1], r[2]))
    grps, group_of = seekmany.groups(ranges, [Rec(k) for k in recs])
    decoded = [group_verdict(now[e], idx[e][1], idx[e][2], a, b, dict_raw) for e, a, b, _ in grps]
    return recs, grps, group_of, range_verdicts(ranges, recs, grps, group_of, decoded, lambda e, a: idx[e][2][a], caps, group_status)


def run_indexed(c, index, s, entries, ranges, caps=None, lens=None, **kw):
    """the ranges in ONE indexed gather call, checked against the models; (arena, results, seeks, expectations, groups)"""
    gkw = {k: kw.pop(k) for k in ("dict_raw", "group_status", "indexed", "now") if k in kw}
    recs, grps, group_of, exps = expectations(entries, ranges, caps, **gkw)
    a, res, seeks = run_checked(lambda ptrs, cp: c.gather_ranges_indexed_device_src(index, s.ptrs, lens or s.lens, ranges, ptrs, cp, **kw), s, ranges, recs, exps, caps)
    return a, res, seeks, exps, grps


def with_skippables(frames):
    """skippable frames at positions 0, 3 and at the end"""
    return b"".join([skippable(b"front" * 5)] + frames[:2] + [skippable(b"")] + frames[2:] + [skippable(b"behind" * 7)])


# ---- 1: the table kind is the existing call ---------------------------------------------------------------------------------------------------
def test_table_kind_equals_the_seek_table_call(ctx):
    z, ds, plains = _unsized_entry()
    unusable = z[:len(z) - 5] + b"\x40" + z[len(z) - 4:]
    total = sum(ds)
    ranges = [(0, b, n) for b, n in seektabs.boundary_ranges(ds)] + [(1, 5, 10), (1, 0, 0), (2, 0, 1), (0, 3, 4, 1)]
    caps = [(min(r[2], max(total - r[1], 0)) if r[0] == 0 else 16) + (7 if j % 2 else 0) for j, r in enumerate(ranges)]
    shifts = [j % 5 for j in range(len(ranges))]
    s = Sources([z, unusable], [3, 9])
    a_old, a_new = Arena(caps, shifts), Arena(caps, shifts)
    old, old_seeks = ctx.gather_ranges_seek_table_device_src(s.ptrs, s.lens, ranges, a_old.ptrs, caps, hash_max=ALL)
    st_old = ctx.gather_ranges_stats()
    with ctx.seek_index(s.ptrs, s.lens, kind="seek_table") as ix:
        i0, i1 = ix.infos
        tab = len(z) - (72 * 8 + 17)
        assert (i0.status, i0.kind, i0.nrows, i0.len, i0.compressed, i0.plaintext) == (0, zgpu.INDEX_SEEK_TABLE, 72, len(z), tab, total), i0
        assert (i1.status, i1.why, i1.nrows, i1.compressed, i1.plaintext) == (zgpu.E_SEEK_TABLE, zgpu.SEEKTAB_RESERVED_BITS, 0, 0, 0), i1
        bs = ix.stats()
        assert ix.device_bytes == bs["device_bytes"] == 16 * 73 and bs["rows"] == 72 and bs["input_bytes_to_host"] == 0 and bs["launches"] == 3, bs
        new, new_seeks = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a_new.ptrs, caps, hash_max=ALL)
        st = ctx.gather_ranges_stats()
        only = ctx.frames_seek_indexed_device(ix, ranges)
        st_seek = ctx.gather_ranges_stats()
    assert [full_key(r) for r in new] == [full_key(r) for r in old]
    assert [k.key() for k in new_seeks] == [k.key() for k in old_seeks] == [k.key() for k in only]
    assert a_new.t.cpu().numpy().tobytes() == a_old.t.cpu().numpy().tobytes() and s.unchanged()
    assert sum(r.status == 0 and r.written > 0 for r in new) > 100 and sum(r.status == zgpu.E_BAD_ARG for r in new) == 2
    # no locate, no prefix pass: one find launch and the decode
    assert (st["seek_launches"], st["seek_us"], st["seek_bytes_downloaded"], st["prefix_launches"], st["prefix_us"], st["prefix_scratch_bytes"]) == (0,) * 6, st
    assert st["find_launches"] == 1 and (st_old["seek_launches"], st_old["prefix_launches"], st_old["find_launches"]) == (1, 2, 1)
    for k in ("groups_decoded", "frames_decoded", "plaintext_decoded", "bytes_written", "frames_skipped", "input_bytes_to_host"):
        assert st[k] == st_old[k], (k, st, st_old)
    assert (st_seek["find_launches"], st_seek["seek_launches"], st_seek["prefix_launches"], st_seek["frames_decoded"]) == (1, 0, 0, 0), st_seek


# ---- 2: the declared kind ---------------------------------------------------------------------------------------------------------------------
def test_declared_kind_equals_the_seek_table_gather_on_the_same_frames(ctx):
    size = 4096
    sized, plains = _eight_declared()
    unsized, plains2 = _eight_frames()
    assert plains == plains2
    whole = b"".join(plains)
    za, zb = with_skippables(sized), seekable(unsized, [size] * 8)
    ranges = [(0, 2 * size + 61 * k, 60) for k in range(64)]                       # 64 records inside frame 2
    ranges += [(0, 5 * size - 10, 20), (0, 5 * size - 3, 6), (0, 7 * size - 1, 2)]   # pairs that straddle 4|5, and 6|7
    ranges += [(0, 8 * size - 1, 5), (0, 8 * size, 1), (0, 0, 0), (0, size, 1)]
    random.Random(5).shuffle(ranges)
    sa, sb = Sources([za], [5]), Sources([zb])
    with ctx.seek_index(sa.ptrs, sa.lens, kind="declared") as ix:
        info = ix.infos[0]
        assert (info.status, info.kind, info.nrows, info.len, info.compressed, info.plaintext) == (0, zgpu.INDEX_DECLARED, 11, len(za), len(za), 8 * size)
        bs = ix.stats()
        assert (bs["launches"], bs["device_bytes"], bs["rows"], bs["input_bytes_to_host"]) == (2, 16 * 12, 11, 0) and bs["bytes_downloaded"] == 48 + 32, bs
        a, res, seeks, exps, grps = run_indexed(ctx, ix, sa, [za], ranges, hash_max=ALL)
        st = ctx.gather_ranges_stats()
        only = ctx.frames_seek_indexed_device(ix, ranges)
    assert [k.key() for k in only] == [k.key() for k in seeks]
    assert all(r.status == 0 for r in res) and [d for _, d in exps] == [whole[b:b + n] for _, b, n in ranges]
    # rows: 0 skip, 1-2 frames 0-1, 3 skip, 4-9 frames 2-7, 10 skip. The groups: frame 1; frame 2; frames 4-5; frames 6-7 — and the range that runs past
    # the plaintext takes every row to the end, the skippable frame behind frame 7 too (last = nrows - 1)
    assert [(g[1], g[2]) for g in grps] == [(2, 2), (4, 4), (6, 7), (8, 10)]
    assert (st["frames_decoded"], st["plaintext_decoded"], st["groups_decoded"]) == (6, 6 * size, 4), st
    assert (st["seek_launches"], st["prefix_launches"], st["find_launches"], st["input_bytes_to_host"]) == (0, 0, 1, 0), st
    # the same frames, unsized, behind a correct seek table: the existing call
    b = Arena(a.caps, [j % 5 for j in range(len(ranges))])
    old, old_seeks = ctx.gather_ranges_seek_table_device_src(sb.ptrs, sb.lens, ranges, b.ptrs, b.caps, hash_max=ALL)
    assert [(r.status, r.written) for r in old] == [(r.status, r.written) for r in res]
    assert [(k.plain_lo, k.plain_seen) for k in old_seeks] == [(k.plain_lo, k.plain_seen) for k in seeks]
    assert b.t.cpu().numpy().tobytes() == a.t.cpu().numpy().tobytes()
    # ... and the header chain's own selection, range by range
    m = len(ranges)
    by_chain = ctx.frames_seek_device(sa.ptrs * m, sa.lens * m, [r[1:3] for r in ranges])
    for k, c in zip(seeks, by_chain):
        assert tuple(k.key()[i] for i in FIVE) == tuple(c.key()[i] for i in FIVE) and k.nothing == c.nothing, (k, c)


# ---- 3: one handle, many calls ------------------------------------------------------------------------------------------------------------------
def test_one_handle_serves_many_calls_and_a_copy_of_the_entry(ctx):
    size = 4096
    sized, plains = _eight_declared()
    whole = b"".join(plains)
    z = with_skippables(sized)
    s = Sources([z], [7])
    ix = ctx.seek_index(s.ptrs, s.lens, kind="declared")
    try:
        built = ix.stats()
        calls = [[(0, 100, 50), (0, size - 3, 10)], [(0, 3 * size + 9, 2 * size), (0, 3 * size + 20, 7), (0, 0, 1)], [(0, 7 * size + 1, U64), (0, 5, 5)]]
        for n, ranges in enumerate(calls):
            src = s if n < 2 else Sources([b"\x11" * 64, z], [0, 2])            # the third call: the entry copied elsewhere
            if n == 2:
                assert src.ptrs[1] != s.ptrs[0]
                caps = [size, 5]
                a = Arena(caps, [1, 2])
                res, seeks = ctx.gather_ranges_indexed_device_src(ix, src.ptrs[1:], src.lens[1:], ranges, a.ptrs, caps, hash_max=ALL)
                assert [(r.status, r.written) for r in res] == [(0, size - 1), (0, 5)]
                a.check([whole[7 * size + 1:], whole[5:10]])
                assert src.unchanged()
            else:
                a, res, seeks, exps, _ = run_indexed(ctx, ix, src, [z], ranges, hash_max=ALL)
                assert [d for _, d in exps] == [whole[b:b + n_] for _, b, n_ in ranges] and all(r.status == 0 for r in res)
            assert ix.stats() == built and built["launches"] == 2          # the index is never rebuilt
            assert ctx.gather_ranges_stats()["find_launches"] == 1
    finally:
        ix.close()
    assert ix.h is None and ix not in ctx._indexes
    with pytest.raises(ValueError):
        ctx.frames_seek_indexed_device(ix, [(0, 0, 1)])


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refused_entries_and_arguments(ctx):
    import zgdata
    size = 4096
    sized, plains = _eight_declared()
    whole = b"".join(plains)
    good = b"".join(sized)
    one_unsized = sized[0] + zgdata.zstd_compress(plains[1], checksum=False, content_size=False) + sized[2]
    trunc = good[:len(good) - 100]
    why_trunc = seekidx.index(trunc)[0]
    assert why_trunc in range(1, 9) and seekidx.index(one_unsized)[0] == seekidx.INDEX_UNSIZED
    entries = [good, one_unsized, trunc, with_skippables(sized), b""]
    s = Sources(entries, [0, 3, 1, 6, 0])
    ix = ctx.seek_index(s.ptrs, s.lens, kind="declared")
    try:
        assert [(i.status, i.why, i.nrows, i.plaintext) for i in ix.infos] == [
            (0, 0, 8, 8 * size), (zgpu.E_FRAME_INDEX, zgpu.INDEX_UNSIZED, 0, 0), (zgpu.E_FRAME_INDEX, why_trunc, 0, 0), (0, 0, 11, 8 * size), (0, 0, 0, 0)]
        assert ix.device_bytes == 16 * (9 + 12 + 1)
        ranges = [(0, 10, 20), (1, 10, 20), (2, 10, 20), (3, size + 1, size), (1, 0, 0), (2, 8 * size, 9), (4, 0, 5), (5, 0, 1), (0, 7, 7, 9)]
        a, res, seeks, exps, _ = run_indexed(ctx, ix, s, entries, ranges, hash_max=ALL)
        bad = zgpu.E_FRAME_INDEX
        assert [r.status for r in res] == [0, bad, bad, 0, 0, bad, 0, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG]
        assert [d for _, d in exps] == [whole[10:30], None, None, whole[size + 1:2 * size + 1], b"", None, b"", None, None]
        assert (seeks[1].why, seeks[2].why, seeks[6].nothing) == (zgpu.INDEX_UNSIZED, why_trunc, True)
        # lens[i] off by one: that entry's ranges only
        lens = list(s.lens)
        lens[0] -= 1
        caps = [20, 20, size]
        b = Arena(caps)
        res, seeks = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, lens, [(0, 10, 20), (0, 5, 0), (3, size + 1, size)], b.ptrs, caps)
        assert [(r.status, r.written) for r in res] == [(zgpu.E_BAD_ARG, 0), (0, 0), (0, size)] and seeks[0].key() == BAD_ARG_REC
        b.check([None, b"", whole[size + 1:2 * size + 1]])
        # the wrong n, and a handle of a second context, fail the call
        with pytest.raises(zgpu.ZgpuError) as err:
            ctx.gather_ranges_indexed_device_src(ix, s.ptrs[:4], s.lens[:4], [(0, 10, 20)], b.ptrs[:1], caps[:1])
        assert err.value.status == zgpu.E_BAD_ARG
        c2 = zgpu.Context(0)
        try:
            for call in (lambda: c2.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, [(0, 10, 20)], b.ptrs[:1], caps[:1]),
                         lambda: c2.frames_seek_indexed_device(ix, [(0, 10, 20)])):
                with pytest.raises(zgpu.ZgpuError) as err:
                    call()
                assert err.value.status == zgpu.E_BAD_ARG
        finally:
            c2.close()
        b.check([None, b"", whole[size + 1:2 * size + 1]])
        # an entry that is no device memory: its own status, the others are indexed
        with ctx.seek_index([s.ptrs[0], 0x10], [s.lens[0], 64], kind="declared") as ix2:
            assert [(i.status, i.nrows) for i in ix2.infos] == [(0, 8), (zgpu.E_BAD_ARG, 0)]
    finally:
        ix.close()
    assert s.unchanged()


# ---- 5: AUTO --------------------------------------------------------------------------------------------------------------------------------------
def test_auto_takes_the_table_and_the_chain_only_where_there_is_none(ctx):
    size = 4096
    sized, plains = _eight_declared()
    unsized, _ = _eight_frames()
    whole = b"".join(plains)
    seekable_z = seekable(unsized, [size] * 8)
    declared_z = with_skippables(sized)
    reserved = seekable(sized, [size] * 8)
    reserved = reserved[:len(reserved) - 5] + b"\x40" + reserved[len(reserved) - 4:]   # a table that is there and malformed: the chain is not asked
    entries = [seekable_z, declared_z, reserved]
    s = Sources(entries, [1, 4, 2])
    with ctx.seek_index(s.ptrs, s.lens) as ix:
        assert [(i.status, i.why, i.kind, i.nrows) for i in ix.infos] == [
            (0, 0, zgpu.INDEX_SEEK_TABLE, 8), (0, 0, zgpu.INDEX_DECLARED, 11), (zgpu.E_SEEK_TABLE, zgpu.SEEKTAB_RESERVED_BITS, zgpu.INDEX_SEEK_TABLE, 0)]
        assert ix.device_bytes == 16 * (9 + 12) and ix.stats()["launches"] == 5          # locate, total, prefix; summary, rows
        ranges = [(0, size - 5, 10), (1, size - 5, 10), (2, size - 5, 10), (1, 3 * size, size), (0, 3 * size, size), (2, 0, 0)]
        caps = [10, 17, 10, size, size + 3, 0]
        a = Arena(caps, [0, 1, 2, 3, 4, 0])
        res, seeks = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a.ptrs, caps, hash_max=ALL)
        assert [(r.status, r.written) for r in res] == [(0, 10), (0, 10), (zgpu.E_SEEK_TABLE, 0), (0, size), (0, size), (0, 0)]
        assert seeks[2].why == zgpu.SEEKTAB_RESERVED_BITS and seeks[2].key()[:5] == (0,) * 5
        a.check([whole[size - 5:size + 5]] * 2 + [None, whole[3 * size:4 * size], whole[3 * size:4 * size], b""])
        old = ctx.frames_seek_table_many_device(s.ptrs[:1], s.lens[:1], [r for r in ranges if r[0] == 0])
        assert [k.key() for k in old] == [seeks[0].key(), seeks[4].key()]
    assert s.unchanged()


# ---- 6: verdicts inside groups ----------------------------------------------------------------------------------------------------------------------
def test_defects_fail_exactly_the_groups_that_hold_them(ctx):
    frames, plains = _six_declared()
    sizes = [len(p) for p in plains]
    good = b"".join(frames)
    fr = chain(good)
    off = seekmany.prefixes(sizes, sizes)[1]
    bad = None
    for at, f in ((fr[3].block_at + 3, lambda x: x ^ 0xFF), (fr[3].block_at + 3 + 40, lambda x: x ^ 0xFF), (fr[3].block_at, lambda x: x ^ 2),
                  (fr[3].block_at, lambda x: x ^ 4)):                # a byte of frame 3's first block that the oracle rejects
        cand = _edit(good, at, f)
        if _decode(cand[fr[3].begin:fr[3].end])[0] != 0 and seekidx.index(cand)[0] == 0:
            bad = cand
            break
    assert bad is not None
    ranges = [(0, 100, 50), (0, off[1] + 7, 1000), (0, off[3] - 5, 10), (0, off[3] + 100, 300), (0, off[2] + 9, 90), (0, off[5] + 1, sizes[5] - 1)]
    s = Sources([bad])
    with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
        a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [bad], ranges, hash_max=ALL)
    assert [(g[1], g[2], g[3]) for g in grps] == [(0, 0, [0]), (1, 1, [1]), (2, 3, [2, 3, 4]), (5, 5, [5])]
    want = _decode(bad[fr[2].begin:fr[3].end])[0]
    assert want != 0 and [r.status for r in res] == [0, 0, want, want, want, 0]
    assert [e[1] for e in exps][:2] == [plains[0][100:150], plains[1][7:1007]]
    # a frame whose declared size is false; the index is built after the edit, so the index itself is consistent: everything behind shifts by one
    lie3 = _edit(good, fr[3].fcs_at, lambda x: (x + 1) & 255)
    why, C_, D_ = seekidx.index(lie3)
    assert why == 0 and D_[4] == off[4] + 1 and chain(lie3)[3].fcs == sizes[3] + 1
    ranges = [(0, D_[3] + 5, 100), (0, D_[4] - 2, 4), (0, D_[1], 10), (0, D_[5] + 3, 10), (0, D_[4], 9)]
    s = Sources([lie3], [3])
    with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
        assert ix.infos[0].plaintext == sum(sizes) + 1
        a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [lie3], ranges)
    csm = zgpu.E_CONTENT_SIZE_MISMATCH
    assert [r.status for r in res] == [csm, csm, 0, 0, csm] and [(g[1], g[2]) for g in grps] == [(1, 1), (3, 4), (5, 5)]
    assert [exps[2][1], exps[3][1]] == [plains[1][:10], plains[5][3:13]]


def test_too_small_and_the_option_flags(ctx):
    frames, plains = _six_declared()                               # every frame carries a Content_Checksum
    sizes = [len(p) for p in plains]
    good = b"".join(frames)
    ends = seekmany.prefixes([len(f) for f in frames], sizes)[0]
    off = seekmany.prefixes(sizes, sizes)[1]
    s = Sources([good], [2])
    with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
        # a destination that is too small fails its own range only
        ranges = [(0, off[3] + 10, 500), (0, off[3] + 700, 500), (0, off[3] + 1500, 500)]
        a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [good], ranges, caps=[500, 499, 507])
        assert len(grps) == 1 and [(r.status, r.written) for r in res] == [(0, 500), (zgpu.E_TARGET_TOO_SMALL, 0), (0, 500)]
        assert full_key(res[1]) == (zgpu.E_TARGET_TOO_SMALL, 0, 0, 0, 0, 0, 0, 0, 0)
        # verify_table on a declared-kind entry: there is no table to enforce
        a = Arena([500] * 3)
        res, seeks = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges[:2] + [(0, 5, 0)], a.ptrs, a.caps, verify_table=True)
        assert [(r.status, r.written) for r in res] == [(zgpu.E_BAD_ARG, 0)] * 2 + [(0, 0)] and seeks[0].key() == BAD_ARG_REC
        a.check([None, None, b""])
        with pytest.raises(zgpu.ZgpuError):
            ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, [], [], [], no_hash=True, verify=True)
    # verify=True with a flipped stored checksum fails the group that holds that frame
    bad3 = _edit(good, ends[4] - 1, lambda x: x ^ 0x40)            # frame 3's Content_Checksum
    ranges = [(0, off[3] + 1, 9), (0, off[3] - 1, 2), (0, off[2] + 50, 50), (0, off[1] + 50, 50), (0, off[4], 77), (0, off[3] + 99, 1)]
    caps = [9, 2, 50, 50, 77, 0]                                   # the last one: too small ranks in front of the checksum verdict
    verdict = lambda e, a, b: zgpu.E_CHECKSUM_MISMATCH if a <= 3 <= b else 0   # noqa: E731
    s = Sources([bad3])
    with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
        a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [bad3], ranges, caps=caps, group_status=verdict, verify=True)
        cm = zgpu.E_CHECKSUM_MISMATCH
        assert [r.status for r in res] == [cm, cm, cm, 0, 0, zgpu.E_TARGET_TOO_SMALL]
        assert (res[0].checksums, res[0].checksum_mismatches) == (2, 1)
        a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [bad3], ranges[:5], hash_max=ALL)   # without the flag: counted, and written
        assert [(r.status, r.checksum_mismatches) for r in res] == [(0, 1), (0, 1), (0, 1), (0, 0), (0, 0)]
    # verify_table on a table-kind entry: the existing verdicts
    frames, plains = _eight_frames(size=2000)
    sums = [xxh32(p) ^ (0x100 if k == 5 else 0) for k, p in enumerate(plains)]   # row 5's checksum: one false bit
    z = seekable(frames, [2000] * 8, checksums=sums)
    ranges = [(0, 5 * 2000 + 5, 10), (0, 5 * 2000 - 1, 2), (0, 4 * 2000 + 7, 3), (0, 6 * 2000, 2000), (0, 100, 3000), (0, 5 * 2000 + 800, 10)]
    caps = [10, 2, 3, 2000, 3000, 9]
    s = Sources([z])
    a_old, a_new = Arena(caps), Arena(caps)
    old, _ = ctx.gather_ranges_seek_table_device_src(s.ptrs, s.lens, ranges, a_old.ptrs, caps, verify_table=True)
    with ctx.seek_index(s.ptrs, s.lens, kind="auto") as ix:
        new, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a_new.ptrs, caps, verify_table=True)
    tb = zgpu.E_SEEK_CHECKSUM_MISMATCH
    assert [r.status for r in new] == [tb, tb, tb, 0, 0, zgpu.E_TARGET_TOO_SMALL] and [full_key(r) for r in new] == [full_key(r) for r in old]
    assert a_new.t.cpu().numpy().tobytes() == a_old.t.cpu().numpy().tobytes()
    st = ctx.gather_ranges_stats()
    assert st["entries_failed_table"] == 1 and st["frames_compared"] == 5 and st["compare_launches"] == 1, st


# ---- 7: a stale index -------------------------------------------------------------------------------------------------------------------------------
def test_a_stale_index_is_a_status_never_a_fault(ctx):
    import zgdata
    sized, plains = _eight_declared()
    a0 = b"".join(sized)
    other = [zgdata.zstd_compress(zgdata.text_like(n, seed=0xB00 + k), checksum=False, content_size=True) for k, n in enumerate((1000, 9000, 300, 12000, 5000))]
    b0 = b"".join(other)
    if len(b0) + 8 <= len(a0):
        za, zb = a0, b0 + skippable(bytes(len(a0) - len(b0) - 8))
    else:
        za, zb = a0 + skippable(bytes(len(b0) - len(a0) - 8)), b0
    assert len(za) == len(zb) and seekidx.index(za)[0] == 0 and seekidx.index(zb)[0] == 0
    why, C_, D_ = seekidx.index(za)
    assert set(C_[1:-1]).isdisjoint(seekidx.index(zb)[1])          # other frame boundaries: every group of A starts inside a frame of B, or ends in one
    nz = [k for k in range(len(D_) - 1) if D_[k + 1] > D_[k]]      # the rows that are frames
    calls = [[(0, D_[k] + o, n) for k in nz for o, n in ((0, 1), (5, 3))] + [(0, 7, 0)],      # every row a group of its own
             [(0, D_[k + 1] - 6, 20) for k in nz[:-1:2]] + [(0, D_[-1] - 1, 9)],               # pairs of rows
             [(0, 0, D_[-1]), (0, 3, 0)]]                                                      # every row in one group
    s = Sources([za], [4])
    ix = ctx.seek_index(s.ptrs, s.lens, kind="declared")
    try:
        s.t[s.offs[0]:s.offs[0] + len(zb)] = torch.frombuffer(bytearray(zb), dtype=torch.uint8).to("cuda:0")   # the same tensor now holds entry B
        torch.cuda.synchronize()
        s.host = s.host[:s.offs[0]] + zb + s.host[s.offs[0] + len(zb):]
        for n, part in enumerate(calls):
            a, res, seeks, exps, grps = run_indexed(ctx, ix, s, [za], part, indexed=[za], now=[zb])
            assert len(grps) == (len(nz), (len(nz) + 1) // 2, 1)[n], (n, grps)
            assert all(r.status != 0 for r, rg in zip(res, part) if rg[2]), [r.status for r in res]
            assert all(d is None for (_, d), rg in zip(exps, part) if rg[2])
    finally:
        ix.close()


# ---- 8: dictionary frames ---------------------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_shared_and_alone():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:4]
    sizes = [man[n]["size"] for n in names]
    z = b"".join(pack[n] for n in names)
    why, C_, D_ = seekidx.index(z)
    assert why == 0 and D_ == seekmany.prefixes(sizes, sizes)[1]      # four frames compressed with one dictionary, each declaring its size
    ranges = [(0, D_[3] - 20, 40), (0, D_[3] + 1, max(1, min(sizes[3] - 1, 30))), (0, D_[0], min(sizes[0], 9)), (0, D_[1], sizes[1])]
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        s = Sources([z], [3])
        ix = c.seek_index(s.ptrs, s.lens, kind="declared")
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, seeks, exps, grps = run_indexed(c, ix, s, [z], ranges, dict_raw=rawd, hash_max=ALL)
            assert [r.status for r in res] == [0] * 4 and all(d is not None and len(d) == r[2] for (_, d), r in zip(exps, ranges)), shared
            alone, st = c.frames_device_stats()["entries_alone"], c.gather_ranges_stats()
            assert alone == (0 if shared else len(grps)) and (st["input_bytes_to_host"] == 0) == bool(shared), (shared, alone, st)
            got.append(([full_key(r)[:3] for r in res], a.t.cpu().numpy().tobytes()))
        assert got[0] == got[1]
    finally:
        c.close()                                                      # (with the index still open: the context closes it first)
    assert ix.h is None


# ---- 9: the torch surface ---------------------------------------------------------------------------------------------------------------------------
def test_torch_surface_round_trip_and_close_with_a_live_index():
    size = 4096
    sized, plains = _eight_declared()
    unsized, _ = _eight_frames()
    whole = b"".join(plains)
    z, other = with_skippables(sized), seekable(unsized[:3], [size] * 3)
    s = Sources([z, other])
    views = [s.t[o:o + n] for o, n in zip(s.offs, s.lens)]
    ranges = [(0, 4000, 200), (1, 8190, 100), (0, size * 8 - 5, 50), (0, 9, 0), (1, 1 << 20, 4), (0, 12000, 1), (5, 0, 1)]
    want = [whole[4000:4200], whole[8190:8290], whole[-5:], b"", b"", whole[12000:12001], b""]
    c = zgpu.Context(0)
    try:
        ix = c.seek_index_tensors(views)
        assert [i.kind for i in ix.infos] == [zgpu.INDEX_DECLARED, zgpu.INDEX_SEEK_TABLE] and len(ix) == 2 and c._indexes == [ix]
        outs, res, seeks = c.gather_tensor_ranges(views, ranges, index=ix)
        assert [t.cpu().numpy().tobytes() for t in outs] == want
        assert [r.status for r in res] == [0] * 6 + [zgpu.E_BAD_ARG]
        assert c.gather_ranges_stats()["prefix_launches"] == 0
        buf, offs, res2, _ = c.gather_tensor_ranges(views, ranges, packed=True, index=ix)
        assert offs == [0, 200, 300, 350, 350, 350, 351, 351]
        packed = buf.cpu().numpy().tobytes()
        assert [packed[o:o + r.written] for o, r in zip(offs, res2)] == want and [full_key(r) for r in res2] == [full_key(r) for r in res]
        # without the index the call is what it was (entry 1 only: entry 0 has no table)
        outs, res, _ = c.gather_tensor_ranges(views, [(1, 8190, 100), (0, 5, 5)])
        assert [t.cpu().numpy().tobytes() for t in outs] == [whole[8190:8290], b""] and [r.status for r in res] == [0, zgpu.E_SEEK_TABLE]
        assert c.gather_ranges_stats()["prefix_launches"] == 2
    finally:
        c.close()
    assert ix.h is None and c._indexes == [] and s.unchanged()
