"""The record index on the GPU (zgpu_seek_index_records_device, _records_of, _read_records, _set_records, zgpu_seek_index_record_ranges_device,
zgpu_gather_records_indexed_device_src; zg_k_recs_count / _scan / _emit / _find, zg_records.h; SeekIndex.records, record_offsets, set_records,
records_infos, Context.record_ranges, gather_records_indexed_device_src). No expectation comes from the calls under test: plaintext is the
oracle's decode (test_gpu_seek_index_measured.Shard holds every frame against the oracle), an entry's offsets are tests/records.py's —
numpy.flatnonzero(plain == d) + 1 with O[0] = 0 in front and O[R] = L behind an open tail —, delivered bytes are slices of that plaintext,
and a gather by number is held, field for field, against the gather by bytes on the model's ranges. Everything is compared for equality.
Destinations have guard bytes and odd alignments (devmem.Arena)."""
import os
import random
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import records
import tabframes
import zgpu
from devmem import Arena, Sources, full_key, oracle_alone
from golden_io import read_manifest, read_pack
from test_gpu_seek_index_measured import Shard, _flip_in_huffman_stream, _text_frames
from test_gpu_seek_table import seekable
from test_walk_cpu import skippable

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: the workload generators
pytestmark = pytest.mark.gpu
NL, STRIP = 0x0A, zgpu.RECORDS_STRIP
SIZES = (0, 1, 17, 4096, 70000, 131073)   # the last one: more than one block
CLOSED, OPEN, EMPTY = range(3)


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def _frames(seed, open_tail, content_size):
    """[(frame, plaintext or None)]: text_like frames of SIZES with skippable frames between them; no frame but the last ends in a newline,
    so a record straddles every boundary; the last byte of the entry is a newline unless open_tail"""
    import zgdata
    out = []
    for k, n in enumerate(SIZES):
        p = bytearray(zgdata.text_like(max(n, 1), seed=seed + k)[:n])
        if n:
            p[-1] = ord("x")
        if k == len(SIZES) - 1 and not open_tail:
            p[-1] = NL
        out.append((zgdata.zstd_compress(bytes(p), checksum=False, content_size=content_size), bytes(p)))
        if k % 2:
            out.append((skippable(b"between" * (k + 1)), None))
    return out


class Kind:
    """the three entries — closed last record, open tail, length 0 — as one kind of handle indexes them"""

    def __init__(self, name):
        self.name = name
        declared = name != "measured"
        self.shards = [Shard(_frames(0x900, False, declared)), Shard(_frames(0xA00, True, declared))]
        assert sum(p.count(b"\n") for sh in self.shards for _, p in sh.frames if p) > 1000      # (text_like has real newlines)
        self.entries = [sh.z for sh in self.shards] + [b""]
        if name == "seek_table":
            self.entries = [seekable([z for z, _ in sh.frames], sh.ds) for sh in self.shards] + [b""]
        self.plains = [sh.plain for sh in self.shards] + [b""]
        self.model = [records.offsets(p, NL) for p in self.plains]
        assert [t for _, t in self.model] == [False, True, False]

    def index(self, ctx, s):
        if self.name == "measured":
            ix = ctx.seek_index_measured(s.ptrs, s.lens)
        else:
            ix = ctx.seek_index(s.ptrs, s.lens, kind="auto" if self.name == "seek_table" else self.name)   # (an entry of length 0 has no table: its chain indexes it)
        want = {"seek_table": zgpu.INDEX_SEEK_TABLE, "declared": zgpu.INDEX_DECLARED, "measured": zgpu.INDEX_MEASURED}[self.name]
        kinds = [want, want, zgpu.INDEX_DECLARED if self.name == "seek_table" else want]
        assert [(i.status, i.kind, i.plaintext) for i in ix.infos] == [(0, kd, len(p)) for kd, p in zip(kinds, self.plains)], ix.infos
        return ix


@pytest.fixture(scope="module", params=["seek_table", "declared", "measured"])
def kind(request):
    return Kind(request.param)


# ---- 1: the pass ----------------------------------------------------------------------------------------------------------------------------------
def test_the_pass_leaves_the_models_offsets(ctx, kind):
    s = Sources(kind.entries, [1, 2, 0])
    for run_bytes in (60000, 0):
        with kind.index(ctx, s) as ix:
            assert ix.records_stats()["records_offset_bytes"] == 0 and [r.state for r in ix.records_infos()] == [0, 0, 0]
            ix.hash(s.ptrs, s.lens, run_bytes=run_bytes)
            hashed = ix.stats(sums=True)
            infos = ix.records(s.ptrs, s.lens, run_bytes=run_bytes)
            for e, (O, tail) in enumerate(kind.model):
                got = ix.record_offsets(e)
                assert got == O, (kind.name, run_bytes, e, len(got), len(O), [(i, a, b) for i, (a, b) in enumerate(zip(got, O)) if a != b][:4])
                assert (infos[e].status, infos[e].state, infos[e].delimiter, infos[e].flags, infos[e].nrecords) == (
                    0, zgpu.RECORDS_FOUND, NL, int(tail), len(O) - 1), (e, infos[e])
                assert ix.record_offsets(e, 1, 2) == O[1:3] and ix.record_offsets(e, len(O) - 1) == O[-1:] and ix.record_offsets(e, len(O) + 5) == []
            st = ix.records_stats()
            held = sum(len(O) - 1 for O, _ in kind.model)
            assert st["records_submits"] == hashed["hash_submits"] and st["records_held"] == held, (st, hashed)
            assert st["records_offset_bytes"] == sum(8 * len(O) for O, _ in kind.model) and st["records_chunks"] > 0 and st["records_bytes_downloaded"] > 0
            assert {k: st[k] for k in hashed} == hashed                       # (a caller that asks for 14 gets what it always got)
            if run_bytes:                                                     # at least three runs per shard, a record straddling each cut
                assert hashed["hash_runs"] >= 6, hashed
                for sh, (O, _) in zip(kind.shards, kind.model):
                    cuts = [sh.D[k] for k in range(1, len(sh.ds)) if sh.zstd[k] and sh.ds[k] and 0 < sh.D[k] < sh.D[-1]]
                    assert len([c for c in cuts if c not in set(O)]) >= 3
            print("\n%s run_bytes=%d: %d records, %d chunks, side pass %d us, %d bytes back" % (
                kind.name, run_bytes, held, st["records_chunks"], st["records_us"], st["records_bytes_downloaded"]))
    assert s.unchanged()


# ---- 2: gather by number equals gather by bytes ------------------------------------------------------------------------------------------------------
def _record_sets(sh, O):
    """(first, count): the first record, the last, one that straddles a frame boundary, one count that spans several frames, behind the end, none"""
    R = len(O) - 1
    inner = [sh.D[k] for k in range(1, len(sh.ds)) if sh.ds[k] and 0 < sh.D[k] < sh.D[-1]]
    straddle = max(r for r in range(R) if O[r] < inner[1])                  # the record that holds the byte in front of that boundary
    assert O[straddle] < inner[1] < O[straddle + 1]
    span_lo = max(r for r in range(R) if O[r] < inner[-2])
    span_hi = min(r for r in range(R + 1) if O[r] > inner[-1])
    return [(0, 1), (R - 1, 1), (straddle, 1), (span_lo, span_hi - span_lo), (R, 3), (R + 7, 1), (5, 0), (R - 2, 1 << 63), (3, (1 << 64) - 1)]


def test_gather_by_number_equals_gather_by_bytes(ctx, kind):
    s = Sources(kind.entries, [3, 1, 0])
    with kind.index(ctx, s) as ix:
        ix.records(s.ptrs, s.lens)
        recs = []
        for e in (CLOSED, OPEN):
            for first, count in _record_sets(kind.shards[e], kind.model[e][0]):
                recs += [(e, first, count), (e, first, count, STRIP)]
        recs += [(EMPTY, 0, 1), (EMPTY, 0, 0, STRIP)]
        want = []
        for r in recs:
            O, tail = kind.model[r[0]]
            want.append((r[0],) + records.find(O, tail, r[1], r[2], r[3] if len(r) > 3 else 0))
        ranges, statuses = ctx.record_ranges(ix, recs)
        assert ranges == want and statuses == [0] * len(recs)
        fs = ctx.gather_records_stats()
        assert (fs["record_find_launches"], fs["record_find_bytes_downloaded"]) == (1, 24 * len(recs)), fs
        exp = [kind.plains[e][b:b + n] for e, b, n in want]
        assert any(n and kind.plains[e][b + n - 1] != NL for (e, b, n), r in zip(want, recs) if len(r) > 3)      # a delimiter was stripped
        caps = [len(x) + (5 if j % 2 else 0) for j, x in enumerate(exp)]
        a = Arena(caps, [j % 7 for j in range(len(recs))])
        res, seeks = ctx.gather_records_indexed_device_src(ix, s.ptrs, s.lens, recs, a.ptrs, a.caps)
        fs = ctx.gather_records_stats()
        assert (fs["record_find_launches"], fs["record_find_bytes_downloaded"]) == (1, 24 * len(recs)), fs
        assert [(r.status, r.written) for r in res] == [(0, len(x)) for x in exp]
        a.check(exp)
        b = Arena(caps, [j % 7 for j in range(len(recs))])
        res0, seeks0 = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, want, b.ptrs, b.caps)
        assert [full_key(r) for r in res] == [full_key(r) for r in res0] and [k.key() for k in seeks] == [k.key() for k in seeks0]
        assert ctx.gather_records_stats()["record_find_launches"] == 0          # (the byte gather has no lookup)
        b.check(exp)
        # ZGPU_E_TARGET_TOO_SMALL is one range's own
        small = list(caps)
        j = 6                                                                   # (CLOSED, span, no strip): several frames
        assert len(exp[j]) > 70000
        small[j] = len(exp[j]) - 1
        c = Arena(small, [j % 7 for j in range(len(recs))])
        res, _ = ctx.gather_records_indexed_device_src(ix, s.ptrs, s.lens, recs, c.ptrs, c.caps)
        assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL if q == j else 0 for q in range(len(recs))]
        c.check([None if q == j else x for q, x in enumerate(exp)])
    assert s.unchanged()


# ---- 3: delimiters 0x00 and 0xFF, the pass run again ---------------------------------------------------------------------------------------------
def test_binary_delimiters_and_a_second_pass_replaces_the_first(ctx):
    import zgdata
    rng = random.Random(0xB1A)
    plains = [bytes(rng.choice((0x00, 0x01, 0xFE, 0xFF, 0x0A)) for _ in range(n)) for n in (5000, 1, 20011, 333)]
    sh = Shard([(zgdata.zstd_compress(p, checksum=False, content_size=True), p) for p in plains])
    s = Sources([sh.z], [5])
    with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
        for d in (0x00, 0xFF, b"\n", 0x01):
            info = ix.records(s.ptrs, s.lens, delimiter=d, run_bytes=6000)[0]
            dv = d if isinstance(d, int) else d[0]
            O, tail = records.offsets(sh.plain, dv)
            assert ix.record_offsets(0) == O and (info.state, info.delimiter, info.nrecords, info.flags) == (1, dv, len(O) - 1, int(tail)), (d, info)
            assert ix.records_stats()["records_offset_bytes"] == 8 * len(O)
            ranges, st = ctx.record_ranges(ix, [(0, 7, 3), (0, len(O) - 2, 5, STRIP)])
            assert st == [0, 0] and ranges == [(0,) + records.find(O, tail, 7, 3), (0,) + records.find(O, tail, len(O) - 2, 5, STRIP)]
    assert s.unchanged()


# ---- 4: dictionary frames, shared and alone ------------------------------------------------------------------------------------------------------
def test_dictionary_frames_give_the_plaintexts_offsets_by_both_routes():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:4]
    plains = []
    for n in names:
        st, out = oracle_alone(pack[n], man[n]["size"] + 64, rawd)
        assert st == 0 and len(out) == man[n]["size"]
        plains.append(out)
    plain = b"".join(plains)
    d = max(range(256), key=lambda v: plain.count(bytes([v])) * (rawd.count(bytes([v])) > 50))     # a byte the dictionary is full of
    assert rawd.count(bytes([d])) > 50 and plain.count(bytes([d])) > 10
    O, tail = records.offsets(plain, d)
    z = b"".join(pack[n] for n in names)
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        s = Sources([z], [3])
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            with c.seek_index(s.ptrs, s.lens, kind="declared") as ix:
                info = ix.records(s.ptrs, s.lens, delimiter=d)[0]
                alone = c.frames_device_stats()["entries_alone"]
                assert (alone > 0) == (not shared), (shared, alone)
                assert (info.status, info.state, info.nrecords, info.flags) == (0, 1, len(O) - 1, int(tail)), (shared, info)
                got.append(ix.record_offsets(0))
                recs = [(0, 1, 2), (0, len(O) - 2, 1, STRIP)]
                want = [(0,) + records.find(O, tail, *r[1:]) for r in recs]
                a = Arena([n for _, _, n in want], [1, 2])
                res, _ = c.gather_records_indexed_device_src(ix, s.ptrs, s.lens, recs, a.ptrs, a.caps)
                assert [(r.status, r.written) for r in res] == [(0, n) for _, _, n in want]
                a.check([plain[b:b + n] for _, b, n in want])
        assert got[0] == O and got[1] == O
    finally:
        c.close()


# ---- 5: all or nothing ----------------------------------------------------------------------------------------------------------------------------
def test_a_failing_run_leaves_the_entry_without_offsets_and_its_neighbour_alone(ctx):
    text = _text_frames([30000, 50000, 20000, 45000, 8000], 0x610)
    huf, huf_status = _flip_in_huffman_stream(text[3][0])
    clean = Shard(_text_frames([900, 20, 4000], 0x630))
    good = Shard([text[0], (skippable(b"gap"), None), text[3], text[4]])
    bad = good.z[:good.C[2]] + huf + good.z[good.C[3]:]
    assert len(bad) == len(good.z)
    s = Sources([clean.z, bad, clean.z], [1, 2, 3])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        assert [i.status for i in ix.infos] == [0, 0, 0]
        infos = ix.records(s.ptrs, s.lens, run_bytes=1)
        assert (infos[1].status, infos[1].state, infos[1].nrecords) == (huf_status, 0, 0) and infos[1].row_lo <= 2 < infos[1].row_hi, infos[1]
        name = ctx.L.zgpu_status_name(huf_status).decode()
        assert "zgpu_seek_index_records_device: entry 1, run of rows [%d, %d): %s" % (infos[1].row_lo, infos[1].row_hi, name) in ctx.last_error()
        O, tail = records.offsets(clean.plain, NL)
        for e in (0, 2):
            assert infos[e].state == 1 and ix.record_offsets(e) == O
        with pytest.raises(zgpu.ZgpuError) as err:
            ix.record_offsets(1)
        assert err.value.status == zgpu.E_BAD_ARG
        _, st = ctx.record_ranges(ix, [(1, 0, 1), (0, 0, 1)])
        assert st == [zgpu.E_BAD_ARG, 0]
        # the repaired entry (the same lengths at another address): a second pass succeeds, the neighbours keep what they held
        s2 = Sources([clean.z, good.z, clean.z], [3, 1, 2])
        infos = ix.records(s2.ptrs, s2.lens, which=[0, 1, 0], run_bytes=1)
        assert [i.state for i in infos] == [1, 1, 1] and ix.record_offsets(1) == records.offsets(good.plain, NL)[0]
        assert ix.record_offsets(0) == O and ix.record_offsets(2) == O
    # a stale shard whose sizes changed: CONTENT_SIZE_MISMATCH, and earlier offsets are dropped
    a_, b_ = Shard(_text_frames([12000, 30000, 9000], 0x710)), _text_frames([11000], 0x7AA)[0]
    room = a_.cs[1] - len(b_[0])
    assert room >= 8
    stale = a_.z[:a_.C[1]] + b_[0] + skippable(bytes(room - 8)) + a_.z[a_.C[2]:]
    s = Sources([a_.z], [4])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        assert ix.records(s.ptrs, s.lens)[0].state == 1
        s2 = Sources([stale], [4])
        info = ix.records(s2.ptrs, s2.lens, run_bytes=1)[0]
        assert (info.status, info.state, info.row_lo, info.row_hi) == (zgpu.E_CONTENT_SIZE_MISMATCH, 0, 1, 2), info
        with pytest.raises(zgpu.ZgpuError):
            ix.record_offsets(0)
        assert ix.records_stats()["records_offset_bytes"] == 0


# ---- 6: export and import -------------------------------------------------------------------------------------------------------------------------
def test_offsets_exported_from_one_handle_serve_a_fresh_one(ctx):
    k = Kind("declared")
    s = Sources(k.entries, [0, 5, 0])
    recs = [(CLOSED, 3, 2), (OPEN, len(k.model[OPEN][0]) - 2, 9, STRIP), (OPEN, 10, 1, STRIP), (EMPTY, 0, 1)]
    with k.index(ctx, s) as ix, k.index(ctx, s) as fresh:
        ix.records(s.ptrs, s.lens)
        for e in (CLOSED, OPEN, EMPTY):
            fresh.set_records(e, ix.record_offsets(e), open_tail=ix.records_infos()[e].open_tail)
        infos = fresh.records_infos()
        assert [(i.status, i.state, i.delimiter, i.flags, i.nrecords) for i in infos] == [(0, zgpu.RECORDS_SET, NL, int(t), len(O) - 1) for O, t in k.model]
        assert ctx.record_ranges(fresh, recs) == ctx.record_ranges(ix, recs)
        out = []
        for x in (ix, fresh):
            ranges, _ = ctx.record_ranges(x, recs)
            a = Arena([n for _, _, n in ranges], [1, 2, 3, 4])
            res, _ = ctx.gather_records_indexed_device_src(x, s.ptrs, s.lens, recs, a.ptrs, a.caps)
            a.check([k.plains[e][b:b + n] for e, b, n in ranges])
            out.append([full_key(r) for r in res])
        assert out[0] == out[1] and all(key[0] == 0 for key in out[0])
        # what set_records refuses leaves the earlier state
        O = k.model[CLOSED][0]
        before = fresh.record_offsets(CLOSED)
        for wrong in (O[:5] + [O[4]] + O[5:], O[:-1] + [O[-1] + 1], O[:-1], [1] + O[1:], O[:3] + [O[2] - 1] + O[4:]):
            with pytest.raises(zgpu.ZgpuError) as err:
                fresh.set_records(CLOSED, wrong)
            assert err.value.status == zgpu.E_BAD_ARG
        with pytest.raises(zgpu.ZgpuError):
            fresh.set_records(EMPTY, [0], open_tail=True)                      # no record can be open
        with pytest.raises(zgpu.ZgpuError):
            fresh.set_records(7, [0])
        assert fresh.record_offsets(CLOSED) == before == O and fresh.records_infos()[CLOSED].state == zgpu.RECORDS_SET
    assert s.unchanged()


# ---- 7: arguments and states ----------------------------------------------------------------------------------------------------------------------
def test_arguments_and_states(ctx):
    sh = Shard(_text_frames([2000, 50, 700], 0x300, content_size=True))
    broken = sh.z[:-3]
    s = Sources([sh.z, sh.z, broken], [1, 2, 3])
    L = ctx.L
    O, tail = records.offsets(sh.plain, NL)
    other = zgpu.Context(0)
    try:
        with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
            assert ix.infos[2].status == zgpu.E_FRAME_INDEX
            ptrs, lens = zgpu._ptr_array(s.ptrs), zgpu._size_array(s.lens)
            assert L.zgpu_seek_index_records_device(other.h, ix.h, ptrs, lens, 3, None, NL, 0) == zgpu.E_BAD_ARG   # a handle of another context
            assert L.zgpu_seek_index_records_device(ctx.h, ix.h, ptrs, lens, 2, None, NL, 0) == zgpu.E_BAD_ARG     # n is not the entry count
            assert L.zgpu_seek_index_records_device(ctx.h, ix.h, ptrs, lens, 3, None, 256, 0) == zgpu.E_BAD_ARG    # no byte
            assert [i.state for i in ix.records_infos()] == [0, 0, 0]
            infos = ix.records(s.ptrs, [s.lens[0], s.lens[1] - 1, s.lens[2]])                                     # a wrong length
            assert [(i.status, i.state) for i in infos] == [(0, 1), (zgpu.E_BAD_ARG, 0), (zgpu.E_FRAME_INDEX, 0)]
            # ranges: an entry without records, unknown flags, an entry out of range, the refused entry's own status; none disturbs another
            recs = [(1, 0, 1), (0, 0, 1, 2), (3, 0, 1), (2, 0, 1), (0, 1, 1)]
            ranges, st = ctx.record_ranges(ix, recs)
            assert st == [zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_BAD_ARG, zgpu.E_FRAME_INDEX, 0] and ranges[4] == (0, O[1], O[2] - O[1])
            assert ranges[:4] == [(1, 0, 0), (0, 0, 0), (3, 0, 0), (2, 0, 0)]
            a = Arena([8, 8, 8, 8, O[2] - O[1]], [1, 2, 3, 4, 5])
            res, _ = ctx.gather_records_indexed_device_src(ix, s.ptrs, s.lens, recs, a.ptrs, a.caps)
            assert [(r.status, r.written) for r in res] == [(x, 0) for x in st[:4]] + [(0, O[2] - O[1])]
            a.check([None] * 4 + [sh.plain[O[1]:O[2]]])
            # a refused entry's state survives: entry 1 gets the caller's offsets, a pass with a wrong length leaves them
            ix.set_records(1, O, open_tail=tail)
            infos = ix.records(s.ptrs, [s.lens[0], s.lens[1] + 1, s.lens[2]], which=[0, 1, 0])
            assert (infos[1].status, infos[1].state, infos[1].nrecords) == (zgpu.E_BAD_ARG, zgpu.RECORDS_SET, len(O) - 1) and ix.record_offsets(1) == O
            assert infos[0].state == 1 and ix.record_offsets(0) == O
    finally:
        other.close()
    assert s.unchanged()


def test_a_changed_byte_fails_a_record_gather_under_the_flag_as_it_fails_a_byte_gather(ctx):
    """the record index is a promise about bytes: without the flag the changed bytes are delivered with status 0; with the handle's sums
    and verify_table the group fails, exactly as the gather by bytes does"""
    rng = random.Random(0x7A1E)
    raw = bytes(rng.choice(b"ab\n") for _ in range(900))
    _, zraw, praw = tabframes.build("r_raw", [("raw", raw)], differs={})
    sh = Shard(_text_frames([3000, 500], 0x410) + [(zraw, praw)] + _text_frames([800], 0x420))
    O, tail = records.offsets(sh.plain, NL)
    at = zraw.find(praw[:64])
    assert at > 0 and zraw[at:at + len(praw)] == praw
    pos, k = sh.C[2] + at + 400, sh.D[2] + 400                               # a byte of the raw block: every size stays what it was
    changed = sh.z[:pos] + bytes([sh.z[pos] ^ 0x01]) + sh.z[pos + 1:]        # ('a' <-> 'b' ... '\n' becomes 0x0B: no offset is right any more behind it)
    plain2 = sh.plain[:k] + bytes([sh.plain[k] ^ 0x01]) + sh.plain[k + 1:]
    assert oracle_alone(changed[sh.C[2]:sh.C[3]], len(praw) + 64) == (0, plain2[sh.D[2]:sh.D[3]])
    r = max(x for x in range(len(O) - 1) if O[x] <= k)                        # the record that holds the byte
    recs, other = [(0, r, 1)], [(0, 0, 1)]
    byte = [(0, O[r], O[r + 1] - O[r])]
    good, bad = Sources([sh.z], [2]), Sources([changed], [2])
    with ctx.seek_index_measured(good.ptrs, good.lens) as ix:
        ix.records(good.ptrs, good.lens)
        ix.hash(good.ptrs, good.lens)
        a = Arena([byte[0][2]], [1])
        res, _ = ctx.gather_records_indexed_device_src(ix, bad.ptrs, bad.lens, recs, a.ptrs, a.caps)
        assert (res[0].status, res[0].written) == (0, byte[0][2])
        a.check([plain2[O[r]:O[r + 1]]])                                      # status 0, the stale offsets' bytes
        b, c = Arena([byte[0][2], O[1]], [3, 1]), Arena([byte[0][2], O[1]], [3, 1])
        r1, _ = ctx.gather_records_indexed_device_src(ix, bad.ptrs, bad.lens, recs + other, b.ptrs, b.caps, verify_table=True)
        r0, _ = ctx.gather_ranges_indexed_device_src(ix, bad.ptrs, bad.lens, byte + [(0, 0, O[1])], c.ptrs, c.caps, verify_table=True)
        assert [full_key(x) for x in r1] == [full_key(x) for x in r0]
        assert [(x.status, x.written) for x in r1] == [(zgpu.E_SEEK_CHECKSUM_MISMATCH, 0), (0, O[1])]
        b.check([None, sh.plain[:O[1]]])
        d = Arena([byte[0][2]], [3])
        r2, _ = ctx.gather_records_indexed_device_src(ix, good.ptrs, good.lens, recs, d.ptrs, d.caps, verify_table=True)
        assert (r2[0].status, r2[0].written) == (0, byte[0][2])
        d.check([sh.plain[O[r]:O[r + 1]]])
    assert good.unchanged() and bad.unchanged()
