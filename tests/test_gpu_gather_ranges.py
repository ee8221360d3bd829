"""zgpu_gather_ranges_seek_table_device_src / zgpu_frames_seek_table_many_device (Context.gather_ranges_seek_table_device_src,
frames_seek_table_many_device, gather_tensor_ranges) on the GPU: m ranges over n seekable entries in device memory, each table scanned once,
each frame decoded once, each range's bytes in its own destination. No expectation comes from the call under test: the records are
tests/seektabs.py's model (and what frames_seek_table_device answers for the same range), the groups are tests/seekmany.py's model of the
contract, and a group's status and bytes are the oracle's on the rows the group takes — for a range alone in its group that is
test_gpu_seek_table.expect, checked as well. Destinations have guard bytes and odd alignments (devmem.Arena), and every byte of a failed
range's slot and behind `written` must be untouched."""
import os
import random
import struct
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import seekmany
import seektabs
import zgpu
from devmem import ALL, Arena, Sources, full_key, xxh32
from golden_io import read_manifest, read_pack
from seektabs import U64, model
from test_gpu_decode_ranges import _decode, _edit, chain
from test_gpu_seek_table import _six_unsized, _unsized_entry, expect, seekable

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: the workload generators
pytestmark = pytest.mark.gpu
BAD_ARG_REC = (0,) * 5 + (zgpu.E_BAD_ARG,) + (0,) * 5


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def rows(z):
    """(csizes, dsizes) of a usable table, from the entry's own bytes"""
    nf, desc = struct.unpack_from("<IB", z, len(z) - 9)
    es = 12 if desc & 0x80 else 8
    tab = len(z) - (nf * es + 17)
    pairs = [struct.unpack_from("<II", z, tab + 8 + k * es) for k in range(nf)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def record(entries, r):
    """the model's record of range r = (entry, begin, len[, pad])"""
    if r[0] >= len(entries) or (len(r) > 3 and r[3]):
        return BAD_ARG_REC
    return model(entries[r[0]], r[1], r[2])[0]


class Rec:
    def __init__(self, key):
        self.status, self.frames_skipped, self.frames_taken = key[5], key[6], key[7]


def group_verdict(z, C_, D_, gfirst, glast, dict_raw=None):
    """(status, bytes or None) of rows [gfirst, glast] of an entry whose rows have the prefixes C_, D_, on the bytes z holds NOW: the oracle on
    those bytes, held to the sizes the frames declare and to the promise of the table or index — what test_gpu_seek_table.expect demands of
    a selection"""
    lo, hi = C_[gfirst], C_[glast + 1]
    st, out = _decode(z[lo:hi], dict_raw)
    if st:
        return st, None
    for f in chain(z[lo:hi]):
        if f.kind == "frame" and f.fcs is not None and len(_decode(z[lo + f.begin:lo + f.end], dict_raw)[1]) != f.fcs:
            return zgpu.E_CONTENT_SIZE_MISMATCH, None
    if len(out) != D_[glast + 1] - D_[gfirst]:
        return zgpu.E_CONTENT_SIZE_MISMATCH, None
    return 0, out


def group_decode(z, gfirst, glast, dict_raw=None):
    """group_verdict on the entry's own seek table"""
    return group_verdict(z, *seekmany.prefixes(*rows(z)), gfirst, glast, dict_raw)


def range_verdicts(ranges, recs, grps, group_of, decoded, d_lo, caps=None, group_status=None):
    """[(status, bytes or None)] per range, from its record, its group's (status, bytes) in decoded and where that group's plaintext begins,
    d_lo(entry, gfirst). group_status(entry, gfirst, glast): a checksum verdict the test knows of (it ranks behind TARGET_TOO_SMALL), or 0"""
    out = []
    for j, (r, k) in enumerate(zip(ranges, recs)):
        if k[5]:
            out.append((k[5], None))
        elif group_of[j] is None:
            out.append((0, b""))
        else:
            e, a, b, _ = grps[group_of[j]]
            st, data = decoded[group_of[j]]
            clip = data[r[1] - d_lo(e, a):][:r[2]] if data is not None else None
            small = clip is not None and caps is not None and len(clip) > caps[j]
            st = seekmany.verdict(decode=st, small=small, checksum=group_status(e, a, b) if group_status and not st else 0)
            out.append((st, clip if st == 0 else None))
    return out


def expectations(entries, ranges, caps=None, dict_raw=None, group_status=None):
    """(records, groups, group_of, [(status, bytes or None)]); group_status: as range_verdicts takes it"""
    recs = [record(entries, r) for r in ranges]
    grps, group_of = seekmany.groups(ranges, [Rec(k) for k in recs])
    decoded = [group_decode(entries[e], a, b, dict_raw) for e, a, b, _ in grps]
    out = range_verdicts(ranges, recs, grps, group_of, decoded, lambda e, a: seekmany.prefixes(*rows(entries[e]))[1][a], caps, group_status)
    for e, a, b, members in grps:
        if len(members) == 1 and not (group_status and group_status(e, a, b)):   # alone in its group: today's call, the existing expectation
            j = members[0]
            assert out[j] == expect(entries[e], ranges[j][1:3], None if caps is None else caps[j], dict_raw), (j, ranges[j])
    return recs, grps, group_of, out


def run_checked(call, s, ranges, recs, exps, caps=None, shifts=None):
    """call(dst_ptrs, caps) -> (results, seeks): ONE gather call of the ranges on the sources s into an arena with guard bytes, checked against
    the models' records and expectations; (arena, results, seeks)"""
    if caps is None:
        caps = [(len(d) if d is not None else 96) + (7 if j % 2 else 0) for j, (_, d) in enumerate(exps)]
    a = Arena(caps, shifts if shifts is not None else [j % 5 for j in range(len(ranges))])
    res, seeks = call(a.ptrs, caps)
    for j, ((st, d), r, k) in enumerate(zip(exps, res, seeks)):
        assert k.key() == recs[j], (j, ranges[j], k, recs[j])
        assert r.status == st, (j, ranges[j], r, k, st)
        assert r.written == (len(d) if st == 0 else 0), (j, ranges[j], r, k)
    a.check([d for _, d in exps])
    assert s.unchanged()
    return a, res, seeks


def run_gather(c, entries, ranges, caps=None, shifts=None, dict_raw=None, group_status=None, src=None, **kw):
    """the ranges in ONE call, checked against the models; (arena, results, seeks, expectations, groups, group_of)"""
    s = src or Sources(entries)
    recs, grps, group_of, exps = expectations(entries, ranges, caps, dict_raw, group_status)
    a, res, seeks = run_checked(lambda ptrs, cp: c.gather_ranges_seek_table_device_src(s.ptrs, s.lens, ranges, ptrs, cp, **kw), s, ranges, recs, exps, caps, shifts)
    return a, res, seeks, exps, grps, group_of


# ---- 1: records -------------------------------------------------------------------------------------------------------------------------------
def test_records_equal_the_single_range_call_and_the_model(ctx):
    rng = random.Random(0x6A7E)
    nf = 2 * 2048 + 3                                              # two chunks of the prefix passes and three rows
    cs = [rng.randint(0, 9) for _ in range(nf)]
    ds = [rng.choice([0, 1, 50, 3000, 70000]) for _ in range(nf)]
    filler = bytes(rng.getrandbits(8) for _ in range(sum(cs)))     # the seek calls touch no frame
    good = filler + zgpu.seek_table_frame(cs, ds, [k for k in range(nf)])
    lie = list(cs)
    lie[3000] += 1 << 20                                           # ranges that reach row 3000 lead past the table; the others do not
    past = filler + zgpu.seek_table_frame(lie, ds)
    unusable = good[:-1] + b"\x00"
    entries = [good, unusable, past]
    D = seekmany.prefixes(cs, ds)[1]
    ranges = []
    for e in range(3):
        for _ in range(80):
            k = rng.randrange(nf)
            ranges.append((e, D[k] + rng.randint(-1, 1) if D[k] else 0, rng.choice([1, 2, 5000, 200000])))
        ranges += [(e, D[2047], 1), (e, D[2048], 1), (e, D[2048] - 1, 2), (e, D[4096], D[-1]), (e, 0, U64), (e, D[-1], 1), (e, D[-1] + 9, 5),
                   (e, 7, 0), (e, U64, U64), (e, D[2990], 1), (e, D[2990], D[3001] - D[2990])]
    ranges += [(3, 0, 1), (7, 5, 0), (2 ** 32 - 1, 0, 9), (0, 0, 1, 1), (1, 5, 0, 0xFFFFFFFF)]
    rng.shuffle(ranges)
    m = len(ranges)
    s = Sources(entries, [3, 0, 9])
    seeks = ctx.frames_seek_table_many_device(s.ptrs, s.lens, ranges)
    st = ctx.gather_ranges_stats()
    want = [record(entries, r) for r in ranges]
    assert [k.key() for k in seeks] == want
    # one locate launch, two prefix launches, one find launch, whatever m is; the unusable table gets no scratch
    assert (st["seek_launches"], st["prefix_launches"], st["find_launches"], st["groups_decoded"]) == (1, 2, 1, 0), st
    assert st["prefix_scratch_bytes"] == 2 * 16 * (nf + 1) and st["seek_bytes_downloaded"] == 32 * 3 + 64 * m, st
    assert st["frames_decoded"] == 0 and st["bytes_written"] == 0
    # the existing call, the entry's pointer repeated once per range
    ok = [j for j, r in enumerate(ranges) if r[0] < 3 and not (len(r) > 3 and r[3])]
    single = ctx.frames_seek_table_device([s.ptrs[ranges[j][0]] for j in ok], [s.lens[ranges[j][0]] for j in ok], [ranges[j][1:3] for j in ok])
    assert [k.key() for k in single] == [seeks[j].key() for j in ok]
    whys = set(k.why for k in seeks)
    assert whys == {0, zgpu.SEEKTAB_NONE, zgpu.SEEKTAB_PAST_TABLE}
    assert sum(k.status == 0 and k.frames_taken > 0 for e, k in zip(ranges, seeks) if e[0] == 2) > 20     # only some ranges of `past` fail
    assert sum(k.status == zgpu.E_BAD_ARG for k in seeks) == 5 and any(k.nothing for k in seeks)
    assert s.unchanged()


# ---- 2: every boundary in one call --------------------------------------------------------------------------------------------------------------
def test_unsized_frames_every_boundary_in_one_call(ctx):
    z, ds, plains = _unsized_entry()
    whole = b"".join(plains)
    ranges = [(0, b, n) for b, n in seektabs.boundary_ranges(ds)]
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges, hash_max=ALL)
    assert all(r.status == 0 and r.checksum_mismatches == 0 for r in res)
    assert all(d == whole[b:b + n] for (_, b, n), (_, d) in zip(ranges, exps))
    st = ctx.gather_ranges_stats()
    is_frame = [d > 0 or k not in (6, 42) for k, d in enumerate(ds)]           # rows 6 and 42 are the skippable frames
    assert sum(is_frame) == 70
    assert (st["frames_decoded"], st["plaintext_decoded"]) == seekmany.work(grps, is_frame, ds), (st, grps)
    assert st["groups_decoded"] == len(grps) and st["input_bytes_to_host"] == 0 and ctx.frames_submits() == 1
    assert st["bytes_written"] == sum(r.written for r in res)
    assert (st["seek_launches"], st["prefix_launches"], st["find_launches"]) == (1, 2, 1)


# ---- 3: dedup ---------------------------------------------------------------------------------------------------------------------------------
def _eight_frames(size=4096, checksum=False):
    import zgdata
    plains = [zgdata.text_like(size, seed=0x3A0 + k) for k in range(8)]
    return [zgdata.zstd_compress(p, checksum=checksum, content_size=False) for p in plains], plains


def test_frames_shared_by_many_ranges_are_decoded_once(ctx):
    frames, plains = _eight_frames()
    size = 4096
    z = seekable(frames, [size] * 8)
    ranges = [(0, 2 * size + 61 * k, 60) for k in range(64)]                       # 64 records inside frame 2
    ranges += [(0, 5 * size - 10, 20), (0, 5 * size - 3, 6), (0, 7 * size - 1, 2)]   # pairs that straddle 4|5, and 6|7
    random.Random(3).shuffle(ranges)
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges, hash_max=ALL)
    st = ctx.gather_ranges_stats()
    assert [(g[1], g[2]) for g in grps] == [(2, 2), (4, 5), (6, 7)]
    assert (st["frames_decoded"], st["plaintext_decoded"], st["groups_decoded"]) == (5, 5 * size, 3) == seekmany.work(grps, [True] * 8, [size] * 8) + (3,)
    assert st["bytes_written"] == sum(r[2] for r in ranges)
    new_bytes = a.t.cpu().numpy().tobytes()
    # the existing call with the pointer repeated: the same bytes, every range's frames decoded again
    s = Sources([z])
    m = len(ranges)
    b = Arena(a.caps, [j % 5 for j in range(m)])
    old, _ = ctx.decode_ranges_seek_table_device_src(s.ptrs * m, s.lens * m, [r[1:] for r in ranges], b.ptrs, b.caps, hash_max=ALL)
    st_old = ctx.ranges_stats()
    assert (st_old["frames_decoded"], st_old["plaintext_decoded"]) == (64 + 2 + 2 + 2, 70 * size)
    assert b.t.cpu().numpy().tobytes() == new_bytes and [r.written for r in old] == [r.written for r in res]


# ---- 4: the group rule --------------------------------------------------------------------------------------------------------------------------
def test_ranges_that_share_a_frame_share_its_fate(ctx):
    frames, plains = _six_unsized()
    sizes = [len(p) for p in plains]
    good = seekable(frames, sizes)
    fr = chain(good)
    off = seekmany.prefixes(sizes, sizes)[1]
    bad = None
    for bit in (2, 4, 1):                                          # one bit of frame 3's first block header: a block type the oracle rejects
        cand = _edit(good, fr[3].block_at, lambda x: x ^ bit)
        if _decode(cand[fr[3].begin:fr[3].end])[0] != 0:
            bad = cand
            break
    assert bad is not None
    ranges = [(0, 100, 50),                        # frame 0, alone
              (0, off[1] + 7, 1000),               # frame 1, alone
              (0, off[3] - 5, 10),                 # frames 2 and 3
              (0, off[3] + 100, 300),              # frame 3
              (0, off[2] + 9, 90),                 # frame 2 only: no byte of frame 3, the fate of frame 3
              (0, off[5] + 1, sizes[5] - 1)]       # frame 5, alone
    a, res, seeks, exps, grps, group_of = run_gather(ctx, [bad], ranges, hash_max=ALL)
    assert [(g[1], g[2], g[3]) for g in grps] == [(0, 0, [0]), (1, 1, [1]), (2, 3, [2, 3, 4]), (5, 5, [5])]
    want = _decode(bad[fr[2].begin:fr[3].end])[0]
    assert want != 0 and [r.status for r in res] == [0, 0, want, want, want, 0]
    assert [e[1] for e in exps][:2] == [plains[0][100:150], plains[1][7:1007]]
    # a range alone in its group: field for field what the existing call gives for it
    alone = [0, 1, 5]
    s = Sources([bad])
    b = Arena([a.caps[j] for j in alone])
    old, old_seeks = ctx.decode_ranges_seek_table_device_src(s.ptrs * 3, s.lens * 3, [ranges[j][1:] for j in alone], b.ptrs, b.caps, hash_max=ALL)
    assert [full_key(r) for r in old] == [full_key(res[j]) for j in alone]
    assert [k.key() for k in old_seeks] == [seeks[j].key() for j in alone]
    b.check([exps[j][1] for j in alone])


# ---- 5: TARGET_TOO_SMALL is a range's own -------------------------------------------------------------------------------------------------------
def test_a_range_that_is_too_small_does_not_disturb_its_group(ctx):
    frames, plains = _six_unsized()
    sizes = [len(p) for p in plains]
    z = seekable(frames, sizes)
    off = seekmany.prefixes(sizes, sizes)[1]
    ranges = [(0, off[3] + 10, 500), (0, off[3] + 700, 500), (0, off[3] + 1500, 500)]
    caps = [500, 499, 507]
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges, caps=caps)
    assert len(grps) == 1 and [r.status for r in res] == [0, zgpu.E_TARGET_TOO_SMALL, 0] and [r.written for r in res] == [500, 0, 500]
    assert full_key(res[1]) == (zgpu.E_TARGET_TOO_SMALL, 0, 0, 0, 0, 0, 0, 0, 0)
    assert ctx.gather_ranges_stats()["bytes_written"] == 1000
    # every range of a group too small
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges, caps=[499, 0, 499])
    assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL] * 3


# ---- 6: false tables ----------------------------------------------------------------------------------------------------------------------------
def test_false_tables_fail_the_groups_that_hold_the_row(ctx):
    frames, plains = _six_unsized()
    sizes = [len(p) for p in plains]
    good = seekable(frames, sizes)
    lied = seekable(frames, sizes, lie=lambda cs, ds: ds.__setitem__(3, ds[3] + 1))      # row 3 promises one byte more
    unusable = good[:len(good) - 5] + b"\x40" + good[len(good) - 4:]
    off = seekmany.prefixes(sizes, sizes)[1]
    ranges = [(0, off[3] + 5, 100), (0, off[4] - 2, 4), (0, off[1], 10), (0, off[5] + 3, 10),      # lied: the first two hold row 3
              (1, 5, 10), (1, off[3], 10), (2, off[3] + 5, 100), (2, 0, 1), (1, 0, 0)]
    a, res, seeks, exps, grps, _ = run_gather(ctx, [lied, unusable, good], ranges)
    csm, tab = zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_SEEK_TABLE
    assert [r.status for r in res] == [csm, csm, 0, 0, tab, tab, 0, 0, 0]
    assert all(seeks[j].why == zgpu.SEEKTAB_RESERVED_BITS for j in (4, 5))
    assert exps[6][1] == plains[3][5:105] and res[2].written == 10


# ---- 7: checksums -------------------------------------------------------------------------------------------------------------------------------
def test_verify_fails_the_groups_that_hold_the_frame(ctx):
    frames, plains = _six_unsized()                                # every frame carries a Content_Checksum
    sizes = [len(p) for p in plains]
    ends = seekmany.prefixes([len(f) for f in frames], sizes)[0]
    off = seekmany.prefixes(sizes, sizes)[1]
    good = seekable(frames, sizes)
    bad3 = _edit(good, ends[4] - 1, lambda x: x ^ 0x40)            # frame 3's Content_Checksum
    ranges = [(0, off[3] + 1, 9), (0, off[3] - 1, 2), (0, off[2] + 50, 50), (0, off[1] + 50, 50), (0, off[4], 77), (0, off[3] + 99, 1)]
    caps = [9, 2, 50, 50, 77, 0]                                   # the last one: too small ranks in front of the checksum verdict
    verdict = lambda e, a, b: zgpu.E_CHECKSUM_MISMATCH if a <= 3 <= b else 0   # noqa: E731
    a, res, seeks, exps, grps, _ = run_gather(ctx, [bad3], ranges, caps=caps, group_status=verdict, verify=True)
    bad = zgpu.E_CHECKSUM_MISMATCH
    assert [r.status for r in res] == [bad, bad, bad, 0, 0, zgpu.E_TARGET_TOO_SMALL]
    assert (res[0].checksums, res[0].checksum_mismatches) == (2, 1) and ctx.frames_device_stats(verify=True)["entries_failed_verify"] == 1
    # without the flag the mismatch is counted and the bytes are written
    a, res, seeks, exps, grps, _ = run_gather(ctx, [bad3], ranges[:5], hash_max=ALL)
    assert [(r.status, r.checksum_mismatches) for r in res] == [(0, 1), (0, 1), (0, 1), (0, 0), (0, 0)]


def test_verify_table_fails_the_groups_that_hold_the_row(ctx):
    frames, plains = _eight_frames(size=2000)
    sums = [xxh32(p) ^ (0x100 if k == 5 else 0) for k, p in enumerate(plains)]   # row 5's checksum: one false bit
    z = seekable(frames, [2000] * 8, checksums=sums)
    ranges = [(0, 5 * 2000 + 5, 10), (0, 5 * 2000 - 1, 2), (0, 4 * 2000 + 7, 3), (0, 6 * 2000, 2000), (0, 100, 3000), (0, 5 * 2000 + 800, 10)]
    caps = [10, 2, 3, 2000, 3000, 9]
    bad = zgpu.E_SEEK_CHECKSUM_MISMATCH
    verdict = lambda e, a, b: bad if a <= 5 <= b else 0   # noqa: E731
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges, caps=caps, group_status=verdict, verify_table=True)
    assert [(g[1], g[2]) for g in grps] == [(0, 1), (4, 5), (6, 6)]
    assert [r.status for r in res] == [bad, bad, bad, 0, 0, zgpu.E_TARGET_TOO_SMALL]
    assert (res[0].nframes, res[0].checksums, res[0].checksum_mismatches, res[0].checksums_unverified) == (0, 2, 1, 0)
    st = ctx.gather_ranges_stats()
    assert st["entries_failed_table"] == 1 and st["frames_compared"] == 5 and st["compare_launches"] == 1, st
    # the flag's contradictions are the sibling's
    with pytest.raises(zgpu.ZgpuError):
        ctx.gather_ranges_seek_table_device_src([0], [0], [], [], [], no_hash=True, verify_table=True)


# ---- 8: dictionary frames -------------------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_shared_and_alone():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:12]
    entries, ranges = [], []
    for e, k in enumerate(range(0, 12, 6)):
        sizes = [man[n]["size"] for n in names[k:k + 6]]
        entries.append(seekable([pack[n] for n in names[k:k + 6]], sizes))
        off = seekmany.prefixes(sizes, sizes)[1]
        ranges += [(e, off[3] - 20, 40), (e, off[3] + 1, max(1, min(sizes[3] - 1, 30))), (e, off[0], min(sizes[0], 9)), (e, off[5], sizes[5])]
    sizes = [man[n]["size"] for n in names[:6]]
    entries.append(seekable([pack[n] for n in names[:6]], sizes, lie=lambda cs, ds: ds.__setitem__(2, ds[2] + 1)))
    off = seekmany.prefixes(sizes, sizes)[1]
    ranges += [(2, off[3] - 20, 40), (2, off[0], min(sizes[0], 9))]
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            a, res, seeks, exps, grps, _ = run_gather(c, entries, ranges, dict_raw=rawd, hash_max=ALL)
            assert [r.status for r in res] == [0] * 8 + [zgpu.E_CONTENT_SIZE_MISMATCH, 0], shared
            alone, st = c.frames_device_stats()["entries_alone"], c.gather_ranges_stats()
            assert alone == (0 if shared else len(grps)) and (st["input_bytes_to_host"] == 0) == bool(shared), (shared, alone, st)
            got.append(([full_key(r)[:3] for r in res], a.t.cpu().numpy().tobytes()))
        assert got[0] == got[1]
    finally:
        c.close()


# ---- 9: submits -----------------------------------------------------------------------------------------------------------------------------------
def test_groups_spread_over_several_submits(ctx, monkeypatch):
    frames, plains = _eight_frames(size=60000)
    z = seekable(frames, [60000] * 8)
    ranges = [(0, k * 60000 + 100 * k, 500) for k in range(8)] + [(0, 3 * 60000 + 7, 9), (0, 6 * 60000 - 4, 8)]
    a, res, seeks, exps, grps, _ = run_gather(ctx, [z], ranges)
    assert ctx.frames_submits() == 1 and len(grps) == 7
    monkeypatch.setenv("ZGPU_FRAMES_SUBMIT_BYTES", str(256 << 10))
    c = zgpu.Context(0, dev=True)
    try:
        a2, res2, seeks2, _, _, _ = run_gather(c, [z], ranges)
        assert c.frames_submits() >= 3 and c.gather_ranges_stats()["groups_decoded"] == 7
        assert [full_key(r) for r in res2] == [full_key(r) for r in res] and a2.t.cpu().numpy().tobytes() == a.t.cpu().numpy().tobytes()
    finally:
        c.close()


# ---- 10: the torch helper -------------------------------------------------------------------------------------------------------------------------
def test_gather_tensor_ranges_round_trip(ctx):
    frames, plains = _eight_frames()
    whole = b"".join(plains)
    z = seekable(frames, [4096] * 8)
    other = seekable(frames[:3], [4096] * 3)
    s = Sources([z, other])
    views = [s.t[o:o + n] for o, n in zip(s.offs, s.lens)]
    ranges = [(0, 4000, 200), (1, 8190, 100), (0, 4096 * 8 - 5, 50), (0, 9, 0), (1, 1 << 20, 4), (0, 12000, 1), (5, 0, 1)]
    want = [whole[4000:4200], whole[8190:8290], whole[-5:], b"", b"", whole[12000:12001], b""]
    outs, res, seeks = ctx.gather_tensor_ranges(views, ranges)
    assert [t.cpu().numpy().tobytes() for t in outs] == want
    assert [r.status for r in res] == [0] * 6 + [zgpu.E_BAD_ARG] and [k.key() for k in seeks] == [record([z, other], r) for r in ranges]
    buf, offs, res2, _ = ctx.gather_tensor_ranges(views, ranges, packed=True)
    assert offs == [0, 200, 300, 350, 350, 350, 351, 351]         # a slot has the room the table promises its range at the most
    packed = buf.cpu().numpy().tobytes()
    assert [packed[o:o + r.written] for o, r in zip(offs, res2)] == want
    assert [full_key(r) for r in res2] == [full_key(r) for r in res]
    assert s.unchanged()
