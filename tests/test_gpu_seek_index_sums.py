"""Seek index checksums on the GPU (zgpu_seek_index_hash_device, _set_sums, _read_sums, _sums_of, _export_seek_table_ex, and
ZGPU_DEVICE_VERIFY_SEEK_TABLE on entries whose handle holds sums: zg_k_idxsums; SeekIndex.hash, sums, set_sums, sums_infos,
export_seek_table(checksums=True), gather_ranges_indexed_device_src(verify_table=True)). No expectation comes from the calls under test: a
row's sum is the low 32 bits of XXH64 of the oracle's decode of that frame alone (test_gpu_seek_index_measured.Shard holds every frame's
plaintext against the oracle), records are seekidx.record on the model's prefixes, groups are tests/seekmany.py's model, delivered bytes
are slices of the oracle's plaintext, and a failing group's counts are tests/idxsums.py's. Destinations have guard bytes and odd alignments
(devmem.Arena). A successful range reports in `checksums` what it always reported — its frames that carry a Content_Checksum —; the frames
COMPARED are counted by zgpu_debug_ranges_stats [11], which every test of the handle route holds against the frames its groups decode."""
import ctypes as C
import os
import random
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import repframes
import seekidx
import tabframes
import zgpu
from devmem import ALL, Arena, Sources, oracle_alone, xxh32
from golden_io import read_manifest, read_pack
from test_gpu_gather_ranges import run_checked
from test_gpu_prefix_edges import NSEQ, _seam_frame
from test_gpu_seek_index_measured import Shard, _expect, _flip_in_huffman_stream, _text_frames
from test_gpu_seek_table import seekable
from test_walk_cpu import skippable

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: the workload generators
pytestmark = pytest.mark.gpu
MISMATCH, SIZE = zgpu.E_SEEK_CHECKSUM_MISMATCH, zgpu.E_CONTENT_SIZE_MISMATCH
TAB, DECL, MEAS, BROKEN, EMPTY, PLAIN = range(6)   # the entries of the handle


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def sums_of(sh):
    """the model: per row the low 32 bits of XXH64 of the frame's plaintext (the oracle's decode: Shard), 0 for a skippable row"""
    return [0 if p is None else xxh32(p) for _, p in sh.frames]


class Entries:
    """six entries for one handle (seek_index_measured(only_unsized=True)): a table-kind entry whose table has no checksums; a declared-kind
    shard of 65 rows, skippable frames at both ends, every frame with a Content_Checksum; a measured-kind shard of 130 rows — the 120 seam
    frames, a skippable frame, raw, RLE, no-sequence and mixed hand-built frames, five text frames —; an entry the index refuses (a broken
    chain); an entry of length 0; a small declared shard that never gets sums"""

    def __init__(self):
        rng = random.Random(0x5005)
        tf = _text_frames([4096, 100, 30000], 0x830)
        self.tabled = seekable([z for z, _ in tf], [4096, 100, 30000])
        self.tab = Shard(tf)                                         # its rows: the three frames (the table frame is not a row of a table-kind index)
        self.decl = Shard([(skippable(b"front"), None)] + _text_frames([rng.randint(1, 3000) for _ in range(63)], 0x100, checksum=True, content_size=True) +
                          [(skippable(b"back" * 5), None)])
        frames = []
        for n in NSEQ:
            for shift in range(6):
                _, z, plain = _seam_frame(n, shift)
                frames.append((z, plain))
        assert len(frames) == 120
        frames.append((skippable(b"between the families" * 3), None))
        for name, blocks in (("s_raw", [("raw", rng.randbytes(777))]), ("s_rle", [("rle", 0x41, 70001)]), ("s_noseq", [tabframes.Block(rng.randbytes(301), [])]),
                             ("s_mixed", [("raw", rng.randbytes(9)), ("rle", 7, 3), tabframes.Block(b"xyz" * 50, [])])):
            _, z, plain = tabframes.build(name, blocks, differs={})
            frames.append((z, plain))
        self.raw_row = 121
        frames += _text_frames([5000, 1, 20000, 300, 9000], 0x200)
        self.meas = Shard(frames)
        self.plain_decl = Shard(_text_frames([2000, 50, 700], 0x300, content_size=True))
        self.broken = self.plain_decl.z[:-3]
        assert (len(self.decl.cs), len(self.meas.cs)) == (65, 130) and all(d is None or d == 0 for _, d in seekidx.rows(self.meas.z)[0])
        self.all = [self.tabled, self.decl.z, self.meas.z, self.broken, b"", self.plain_decl.z]
        self.shards = {TAB: self.tab, DECL: self.decl, MEAS: self.meas, PLAIN: self.plain_decl}

    def index(self, ctx, s):
        ix = ctx.seek_index_measured(s.ptrs, s.lens, only_unsized=True)
        assert [i.kind for i in ix.infos[:3]] == [zgpu.INDEX_SEEK_TABLE, zgpu.INDEX_DECLARED, zgpu.INDEX_MEASURED] and ix.infos[BROKEN].status == zgpu.E_FRAME_INDEX
        assert [ix.infos[e].nrows for e in (TAB, DECL, MEAS, EMPTY, PLAIN)] == [3, 65, 130, 0, 3] and ix.infos[EMPTY].status == 0
        return ix


@pytest.fixture(scope="module")
def ents():
    return Entries()


def gather_both(ctx, ix, s, sh, ranges, exps_flag=None, caps=None):
    """the ranges once under the flag and once without it, both checked against the models; (results under the flag, stats under the flag)"""
    recs, grps, exps = _expect(sh, ranges)
    if caps is None:
        caps = [rg[2] + (7 if j % 2 else 0) for j, rg in enumerate(ranges)]      # (room for every range: a failing one is not TARGET_TOO_SMALL first)
    a, res, _ = run_checked(lambda p, cp: ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, p, cp, verify_table=True), s, ranges, recs,
                            exps_flag or exps, caps)
    st = ctx.gather_ranges_stats()
    if exps_flag is None:
        b, res0, _ = run_checked(lambda p, cp: ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, p, cp, hash_max=ALL), s, ranges, recs, exps, caps)
        assert [(r.status, r.written) for r in res] == [(r.status, r.written) for r in res0] and a.t.cpu().numpy().tobytes() == b.t.cpu().numpy().tobytes()
    return res, st, grps


def frames_of(sh, grps):
    return sum(sum(sh.zstd[k] for k in range(g[1], g[2] + 1)) for g in grps)


# ---- 1: the pass --------------------------------------------------------------------------------------------------------------------------------
def test_the_pass_leaves_the_models_sums(ctx, ents):
    s = Sources(ents.all, [1, 2, 3, 0, 0, 5])
    got = {}
    for run_bytes in (1, 4096, 0):
        with ents.index(ctx, s) as ix:
            before = ix.stats()
            assert ix.stats(sums=True)["sums_bytes"] == 0                       # nothing is allocated until an entry gets sums
            infos = ix.hash(s.ptrs, s.lens, run_bytes=run_bytes)
            for e, sh in ents.shards.items():
                assert ix.sums(e) == sums_of(sh), (run_bytes, e)
                assert (infos[e].status, infos[e].state, infos[e].frames, infos[e].bytes) == (0, zgpu.SUMS_HASHED, sh.nzstd, sh.D[-1]), (e, infos[e])
            assert (infos[BROKEN].status, infos[BROKEN].state) == (zgpu.E_FRAME_INDEX, 0) and (infos[EMPTY].status, infos[EMPTY].state) == (0, 1)
            assert ix.sums(EMPTY) == []
            with pytest.raises(zgpu.ZgpuError) as err:
                ix.sums(BROKEN)
            assert err.value.status == zgpu.E_BAD_ARG
            st = ix.stats(sums=True)
            assert ix.stats() == before and st["device_bytes"] == before["device_bytes"]   # (a caller that asks for 9 gets what it always got)
            assert st["sums_bytes"] == 4 * (3 + 65 + 130 + 3) and st["frames_hashed"] == sum(sh.nzstd for sh in ents.shards.values()), st
            got[run_bytes] = st
    assert s.unchanged()
    zstd_rows = sum(1 for sh in ents.shards.values() for k in range(len(sh.ds)) if sh.zstd[k] and sh.ds[k])
    assert got[1]["hash_runs"] == zstd_rows and got[1]["hash_runs"] > got[4096]["hash_runs"] > got[0]["hash_runs"] == 4, got   # (a run per zstd row; a run per entry)
    print("\nhash pass: %d frames in %d / %d / %d runs, hash kernels %d / %d / %d us" % (
        zstd_rows, got[1]["hash_runs"], got[4096]["hash_runs"], got[0]["hash_runs"], got[1]["hash_us"], got[4096]["hash_us"], got[0]["hash_us"]))


# ---- 2: export ----------------------------------------------------------------------------------------------------------------------------------
def test_export_with_checksums_round_trips_through_the_table_route(ctx, ents):
    s = Sources(ents.all, [0, 1, 2, 3, 0, 1])
    L = ctx.L
    with ents.index(ctx, s) as ix:
        ix.hash(s.ptrs, s.lens, which=[0, 1, 1, 1, 1, 0])
        tables = {e: ix.export_seek_table(e, checksums=True) for e in (DECL, MEAS)}
        for e, t in tables.items():
            sh = ents.shards[e]
            assert t == zgpu.seek_table_frame(sh.cs, sh.ds, checksums=sums_of(sh)) and len(t) == 17 + 12 * len(sh.cs)
            assert ix.export_seek_table(e) == zgpu.seek_table_frame(sh.cs, sh.ds)              # flags == 0 is the old call
        need, buf = C.c_size_t(0), C.create_string_buffer(b"\xA5" * 64, 64)
        t = tables[DECL]
        assert L.zgpu_seek_index_export_seek_table_ex(ix.h, DECL, 1, None, 0, C.byref(need)) == zgpu.E_TARGET_TOO_SMALL and need.value == len(t)
        assert L.zgpu_seek_index_export_seek_table_ex(ix.h, DECL, 1, buf, len(t) - 1, C.byref(need)) == zgpu.E_TARGET_TOO_SMALL
        assert need.value == len(t) and buf.raw == b"\xA5" * 64
        for entry, flags in ((PLAIN, 1), (TAB, 1), (DECL, 2), (DECL, 3), (BROKEN, 1)):           # unhashed entries, unknown flag bits, a refused entry
            assert L.zgpu_seek_index_export_seek_table_ex(ix.h, entry, flags, buf, 64, C.byref(need)) == zgpu.E_BAD_ARG and need.value == 0
        assert buf.raw == b"\xA5" * 64
    # the entry's bytes followed by that frame: a table-kind entry of the same rows that passes the flag by its table (zg_k_seeksums)
    for e in (DECL, MEAS):
        sh = ents.shards[e]
        s2 = Sources([sh.z + tables[e]], [3])
        with ctx.seek_index(s2.ptrs, s2.lens, kind="seek_table") as ix2:
            assert (ix2.infos[0].kind, ix2.infos[0].nrows, ix2.infos[0].plaintext) == (zgpu.INDEX_SEEK_TABLE, len(sh.cs), sh.D[-1])
            assert ix2.sums_infos[0].state == 0
            ranges = [(0, 0, sh.D[-1]), (0, sh.D[5] + 1, 3)]
            res, st, grps = gather_both(ctx, ix2, s2, sh, ranges)
            assert len(grps) == 1 and st["frames_compared"] == st["frames_decoded"] == sh.nzstd and st["compare_launches"] == 1, st
            assert all(r.checksums_unverified == 0 for r in res)
            if e == DECL:
                assert all(r.checksums == sh.nzstd for r in res)                                 # (every frame of it carries a Content_Checksum)


# ---- 3: gather under the flag, by the handle ------------------------------------------------------------------------------------------------------
def _ranges(e, sh):
    D, total = sh.D, sh.D[-1]
    first_zstd = [k for k in range(len(sh.ds)) if sh.zstd[k] and sh.ds[k] > 0]
    out = [(e, D[k], 1) for k in (first_zstd[0], 63, 64, 65) if k < len(sh.ds) and sh.ds[k]]    # groups that begin at rows 0 (or 1), 63, 64, 65
    out += [(e, D[20] + 1, D[23] - D[20] - 1), (e, D[21], 2), (e, D[22] - 1, 2)]                 # ranges that share frames
    out += [(e, total - 2, 9), (e, 7, 0), (e, total, 4)]
    if e == MEAS:
        out.append((e, D[119] - 1, D[123] - D[119] + 2))                                         # the skippable row 120 inside a group
    return out


def test_the_handle_vouches_for_declared_and_measured_entries(ctx, ents):
    s = Sources(ents.all, [1, 2, 3, 0, 0, 5])
    with ents.index(ctx, s) as ix:
        ix.hash(s.ptrs, s.lens, which=[0, 1, 1, 1, 1, 0])
        assert [i.state for i in ix.sums_infos] == [0, 1, 1, 0, 1, 0]
        for e in (DECL, MEAS):
            sh = ents.shards[e]
            for ranges in (_ranges(e, sh), [(e, 0, sh.D[-1])]):                                  # several groups; one range over every row (three steps)
                res, st, grps = gather_both(ctx, ix, s, sh, ranges)
                want = frames_of(sh, grps)
                assert (st["compare_launches"], st["frames_compared"], st["frames_decoded"], st["entries_failed_table"], st["compare_bytes_downloaded"]) == (
                    1, want, want, 0, 32 * len(grps)), (e, st)
                assert all(r.status == 0 and r.checksums_unverified == 0 for r in res), e
                if e == DECL:                                                                     # (every frame carries a Content_Checksum: per range, not only per call)
                    assert [r.checksums for r, rg in zip(res, ranges) if rg[2] and r.written] == [
                        frames_of(sh, [g]) for rg, g in zip(ranges, _group_per_range(sh, ranges)) if g is not None]
            if e == MEAS:
                assert len(grps) == 1 and (grps[0][1], grps[0][2]) == (0, 129)
        # both routes in one call: a table entry with a checksummed table beside the hashed entries is a test of its own (below); here an entry
        # of the same handle without sums still answers BAD_ARG, and a table-kind entry without handle sums answers what the table call answers
        ranges = [(PLAIN, 10, 5), (DECL, ents.decl.D[3], 4), (TAB, 4090, 20)]
        a = Arena([5, 4, 20], [1, 2, 3])
        res, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a.ptrs, a.caps, verify_table=True)
        st = ctx.gather_ranges_stats()
        b = Arena([20], [3])
        old, _ = ctx.gather_ranges_seek_table_device_src(s.ptrs[:1], s.lens[:1], [(0, 4090, 20)], b.ptrs, b.caps, verify_table=True)
        assert [r.status for r in res] == [zgpu.E_BAD_ARG, 0, MISMATCH] and old[0].status == MISMATCH            # (its table has no checksums)
        key = lambda r: (r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified)
        assert key(res[2]) == key(old[0])
        assert st["compare_launches"] == 2 and st["entries_failed_table"] == 1, st                                 # both compare kernels ran
        a.check([None, ents.decl.plain[ents.decl.D[3]:ents.decl.D[3] + 4], None])
    assert s.unchanged()


def _group_per_range(sh, ranges):
    recs, grps, _ = _expect(sh, ranges)
    out = []
    for (_, b, n), k in zip(ranges, recs):
        if not n or not k[7]:
            out.append(None)
            continue
        out.append([g for g in grps if g[1] <= k[6] <= g[2]][0])
    return out


# ---- 4: mismatch ----------------------------------------------------------------------------------------------------------------------------------
def test_a_wrong_sum_fails_exactly_the_groups_that_hold_its_row(ctx, ents):
    s = Sources(ents.all, [0, 0, 1, 0, 0, 0])
    sh, bad = ents.meas, 64
    wrong = sums_of(sh)
    wrong[bad] ^= 0x10
    D = sh.D
    ranges = [(MEAS, D[10], 5), (MEAS, D[63] + 1, D[65] - D[63]), (MEAS, D[64], 1), (MEAS, D[66], 3), (MEAS, D[62], 1), (MEAS, D[64] + 1, 2)]
    recs, grps, exps = _expect(sh, ranges, bad_rows=(bad,), bad_status=MISMATCH)
    assert [st for st, _ in exps] == [0, MISMATCH, MISMATCH, 0, 0, MISMATCH]
    with ents.index(ctx, s) as ix:
        ix.set_sums(MEAS, wrong)
        assert ix.sums_infos[MEAS].state == zgpu.SUMS_SET and ix.sums(MEAS) == wrong
        res, st, _ = gather_both(ctx, ix, s, sh, ranges, exps_flag=exps)
        assert all(r.checksum_mismatches == 1 and r.nframes == 0 for r, (x, _) in zip(res, exps) if x) and st["entries_failed_table"] == 1
        # ZGPU_E_TARGET_TOO_SMALL of one range ranks in front of its group's mismatch
        caps = [rg[2] for rg in ranges]
        caps[2] = 0
        exps2 = list(exps)
        exps2[2] = (zgpu.E_TARGET_TOO_SMALL, None)
        gather_both(ctx, ix, s, sh, ranges, exps_flag=exps2, caps=caps)
        # the right sums again: everything is served
        ix.set_sums(MEAS, sums_of(sh))
        res, st, _ = gather_both(ctx, ix, s, sh, ranges)
        assert st["entries_failed_table"] == 0 and st["frames_compared"] == st["frames_decoded"]
        with pytest.raises(zgpu.ZgpuError) as err:
            ix.set_sums(MEAS, wrong[:-1])
        assert err.value.status == zgpu.E_BAD_ARG


def _stale(ents):
    """the measured shard with one byte changed inside the raw block of a frame without a Content_Checksum: every size is what it was"""
    sh, k = ents.meas, ents.raw_row
    z, p = sh.frames[k]
    at = z.find(p[:64])
    assert at > 0 and z[at:at + len(p)] == p
    pos = sh.C[k] + at + 400
    changed = sh.z[:pos] + bytes([sh.z[pos] ^ 0x20]) + sh.z[pos + 1:]
    plain = p[:400] + bytes([p[400] ^ 0x20]) + p[401:]
    assert oracle_alone(changed[sh.C[k]:sh.C[k + 1]], len(p) + 64) == (0, plain)
    return changed, plain


def test_a_changed_byte_is_delivered_without_the_flag_and_fails_with_it(ctx, ents):
    sh, k = ents.meas, ents.raw_row
    changed, plain = _stale(ents)
    s = Sources([changed], [2])
    good = Sources([sh.z], [2])
    with ctx.seek_index_measured(good.ptrs, good.lens) as ix:
        ix.hash(good.ptrs, good.lens)
        ranges = [(0, sh.D[k] + 390, 20), (0, sh.D[2], 5)]
        a = Arena([20, 5], [1, 3])
        res, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a.ptrs, a.caps, hash_max=ALL)     # random access: a promise about sizes
        assert [(r.status, r.written) for r in res] == [(0, 20), (0, 5)]
        a.check([plain[390:410], sh.plain[sh.D[2]:sh.D[2] + 5]])
        b = Arena([20, 5], [1, 3])
        res, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, b.ptrs, b.caps, verify_table=True)
        assert (res[0].status, res[0].written, res[0].checksums, res[0].checksum_mismatches) == (MISMATCH, 0, 1, 1) and (res[1].status, res[1].written) == (0, 5)
        b.check([None, sh.plain[sh.D[2]:sh.D[2] + 5]])
    assert s.unchanged()


# ---- 5: verdicts of the pass ----------------------------------------------------------------------------------------------------------------------
def test_the_pass_sees_what_measuring_does_not(ctx):
    text = _text_frames([30000, 50000, 20000, 45000, 8000], 0x610)
    huf, huf_status = _flip_in_huffman_stream(text[3][0])
    far = [f for f in repframes.family("invalid") if f[0] == "bad_repeat_out_of_reach"][0][1]
    far_status = oracle_alone(far, 1 << 20)[0]
    ck = _text_frames([7000], 0x620, checksum=True)[0][0]
    ck = ck[:-4] + bytes(x ^ 0xFF for x in ck[-4:])
    assert huf_status and far_status and oracle_alone(ck, 1 << 20)[0] == 0            # (the reference does not enforce a Content_Checksum: this pass does)
    clean = Shard(_text_frames([900, 20, 4000], 0x630))
    for bad, status in ((huf, huf_status), (far, far_status), (ck, zgpu.E_CHECKSUM_MISMATCH)):
        row = 2
        entry = text[0][0] + skippable(b"gap") + bad + text[4][0]
        s = Sources([clean.z, entry, clean.z], [1, 2, 3])
        with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
            assert [i.status for i in ix.infos] == [0, 0, 0] and ix.infos[1].nrows == 4    # measuring indexes all three
            infos = ix.hash(s.ptrs, s.lens, run_bytes=1)
            assert (infos[1].status, infos[1].state) == (status, 0) and infos[1].row_lo <= row < infos[1].row_hi, (status, infos[1])
            assert infos[1].row_hi - infos[1].row_lo <= 2 and infos[1].row_lo >= 1          # the run holds exactly one zstd row (and the skippable one that joined)
            name = ctx.L.zgpu_status_name(status).decode()
            assert "entry 1, run of rows [%d, %d): %s" % (infos[1].row_lo, infos[1].row_hi, name) in ctx.last_error(), ctx.last_error()
            with pytest.raises(zgpu.ZgpuError) as err:
                ix.sums(1)
            assert err.value.status == zgpu.E_BAD_ARG
            for e in (0, 2):                                                                # the other entries of the same call are hashed
                assert infos[e].state == 1 and ix.sums(e) == sums_of(clean)
            # under the flag the entry without sums answers BAD_ARG, as ever
            a = Arena([4], [1])
            res, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, [(1, 3, 4)], a.ptrs, a.caps, verify_table=True)
            assert res[0].status == zgpu.E_BAD_ARG
    # a stale shard whose sizes changed: CONTENT_SIZE_MISMATCH, and earlier sums are dropped
    a_, b_ = Shard(_text_frames([12000, 30000, 9000], 0x710)), _text_frames([11000], 0x7AA)[0]
    room = a_.cs[1] - len(b_[0])
    assert room >= 8
    stale = a_.z[:a_.C[1]] + b_[0] + skippable(bytes(room - 8)) + a_.z[a_.C[2]:]
    s = Sources([a_.z], [4])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        assert ix.hash(s.ptrs, s.lens)[0].state == 1
        s2 = Sources([stale], [4])
        info = ix.hash(s2.ptrs, s2.lens, run_bytes=1)[0]
        assert (info.status, info.state, info.row_lo, info.row_hi) == (SIZE, 0, 1, 2), info
        with pytest.raises(zgpu.ZgpuError):
            ix.sums(0)


# ---- 6: alone -------------------------------------------------------------------------------------------------------------------------------------
def test_dictionary_frames_alone_get_the_same_sums_and_verdicts():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:4]
    sizes = [man[n]["size"] for n in names]
    z = b"".join(pack[n] for n in names)
    plains = []
    for n, size in zip(names, sizes):
        st, out = oracle_alone(pack[n], size + 64, rawd)
        assert st == 0 and len(out) == size
        plains.append(out)
    model = [xxh32(p) for p in plains]
    D = [0]
    for n in sizes:
        D.append(D[-1] + n)
    ranges = [(0, D[3] - 2, 4), (0, D[0], min(sizes[0], 9)), (0, D[1], 1)]
    c = zgpu.Context(0)
    try:
        c.add_dict(rawd)
        s = Sources([z], [3])
        got = []
        for shared in (1, 0):
            c.set_frames_shared_dicts(shared)
            with c.seek_index(s.ptrs, s.lens, kind="declared") as ix:
                info = ix.hash(s.ptrs, s.lens)[0]
                alone = c.frames_device_stats()["entries_alone"]
                assert (info.status, info.state, info.frames, info.bytes) == (0, 1, 4, D[-1]) and ix.sums(0) == model, (shared, info)
                assert (alone > 0) == (not shared), (shared, alone)
                out = []
                for sums in (model, model[:1] + [model[1] ^ 1] + model[2:]):
                    ix.set_sums(0, sums)
                    a = Arena([n for _, _, n in ranges], [1, 2, 3])
                    res, _ = c.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a.ptrs, a.caps, verify_table=True)
                    st = c.gather_ranges_stats()
                    out.append(([(r.status, r.written, r.checksums, r.checksum_mismatches, r.checksums_unverified) for r in res], a.t.cpu().numpy().tobytes(),
                                st["frames_compared"], st["entries_failed_table"]))
                    if not shared:
                        assert c.frames_device_stats()["entries_alone"] > 0 and st["compare_launches"] == 0     # the host's rule
                assert [x[0] for x in out[0][0]] == [0, 0, 0] and [x[0] for x in out[1][0]] == [0, 0, MISMATCH] and out[1][3] == 1
                got.append(out)
        assert got[0] == got[1]
    finally:
        c.close()


# ---- 7: arguments ---------------------------------------------------------------------------------------------------------------------------------
def test_arguments_and_states(ctx, ents):
    sh = ents.plain_decl
    s = Sources([sh.z, sh.z], [1, 2])
    L = ctx.L
    other = zgpu.Context(0)
    try:
        with ctx.seek_index(s.ptrs, s.lens, kind="declared") as ix:
            ptrs, lens = zgpu._ptr_array(s.ptrs), zgpu._size_array(s.lens)
            assert L.zgpu_seek_index_hash_device(other.h, ix.h, ptrs, lens, 2, None, 0) == zgpu.E_BAD_ARG      # a handle of another context
            assert L.zgpu_seek_index_hash_device(ctx.h, ix.h, ptrs, lens, 1, None, 0) == zgpu.E_BAD_ARG        # n is not the entry count
            assert [i.state for i in ix.sums_infos] == [0, 0]
            host = C.create_string_buffer(sh.z, len(sh.z))
            infos = ix.hash([s.ptrs[0], C.addressof(host)], s.lens)                                             # a source that is not device memory
            assert [(i.status, i.state) for i in infos] == [(0, 1), (zgpu.E_BAD_ARG, 0)]
            infos = ix.hash(s.ptrs, [s.lens[0], s.lens[1] - 1])                                                 # a wrong length
            assert [(i.status, i.state) for i in infos] == [(0, 1), (zgpu.E_BAD_ARG, 0)]
            # `which` leaves the unchosen entry's sums untouched; hashing again replaces state 2 by 1
            mine = [7, 8, 9]
            ix.set_sums(1, mine)
            ix.hash(s.ptrs, s.lens, which=[1, 0])
            assert ix.sums(1) == mine and [i.state for i in ix.sums_infos] == [1, 2]
            ix.hash(s.ptrs, s.lens, which=[0, 1])
            assert ix.sums(1) == sums_of(sh) == ix.sums(0) and [i.state for i in ix.sums_infos] == [1, 1]
            with pytest.raises(zgpu.ZgpuError) as err:
                ix.set_sums(0, [1, 2])                                                                          # another nrows
            assert err.value.status == zgpu.E_BAD_ARG
            got, n = (C.c_uint32 * 2)(5, 5), C.c_uint32(0)
            assert L.zgpu_seek_index_read_sums(ix.h, 0, got, 2, C.byref(n)) == zgpu.E_TARGET_TOO_SMALL and n.value == 3 and list(got) == [5, 5]
        ix2 = ctx.seek_index(s.ptrs, s.lens, kind="declared")
        ix2.hash(s.ptrs, s.lens)
        ix2.close()                                                                                             # destroying a hashed handle works
        assert ix2.h is None
    finally:
        other.close()
    assert s.unchanged()
