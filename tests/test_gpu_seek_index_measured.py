"""Seek indexes by measuring on the GPU (zgpu_seek_index_measure_device, zgpu_seek_index_export_seek_table; Context.seek_index_measured,
SeekIndex.export_seek_table): entries whose frames declare no size and that carry no seek table are indexed from the sums of their blocks'
sizes — zg_k_seqsize (zg_seqsize.h) in zg_k_seqpost's place, no Huffman stream, no LZ77 byte, no output — and then serve the indexed seek
and gather calls like any other index. No expectation comes from the calls under test: a row's bytes are tests/seekidx.py's model of the
header chain, its plaintext length is the oracle's decode of that frame, records are seekidx.record on those prefixes, groups are
tests/seekmany.py's model, and a gather must deliver the plaintext's slices — the same that a seek-table index of the same frames behind
a table made by zgpu.seek_table_frame delivers. Destinations have guard bytes and odd alignments (devmem.Arena)."""
import ctypes as C
import random
import struct

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import blockcheck
import dictframes
import framesuite
import seekidx
import seekmany
import seqstreams
import tabframes
import zgpu
from devmem import ALL, Arena, Sources, oracle_alone
from test_gpu_gather_ranges import Rec, run_checked
from test_gpu_prefix_edges import NSEQ, _seam_frame
from test_gpu_seek_table import seekable
from test_walk_cpu import skippable

pytestmark = pytest.mark.gpu
BAD = zgpu.E_FRAME_INDEX


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def _text_frames(sizes, seed, checksum=False, content_size=False):
    import zgdata
    plains = [zgdata.text_like(max(n, 1), seed=seed + k)[:n] for k, n in enumerate(sizes)]
    return [(zgdata.zstd_compress(p, checksum=checksum, content_size=content_size), p) for p in plains]


class Shard:
    """frames [(bytes, plaintext or None for a skippable frame)] back to back: the model of its rows — C from the header chain
    (seekidx.rows), D from the oracle's decode of every zstd frame on its own"""

    def __init__(self, frames):
        self.frames = frames
        self.z = b"".join(z for z, _ in frames)
        rw, why, _ = seekidx.rows(self.z)
        assert why == 0 and [c for c, _ in rw] == [len(z) for z, _ in frames]
        self.zstd = [p is not None for _, p in frames]
        self.ds = []
        for (z, p), (_, d) in zip(frames, rw):
            if p is None:
                assert d == 0
                self.ds.append(0)
                continue
            st, out = oracle_alone(z, len(p) + 64)
            assert st == 0 and out == p, "the oracle refuses a frame of the shard"
            self.ds.append(len(out))
        self.cs = [len(z) for z, _ in frames]
        self.C, self.D = seekmany.prefixes(self.cs, self.ds)
        self.plain = b"".join(p for _, p in frames if p is not None)
        self.nzstd = sum(self.zstd)


def parse_table(frame):
    """(csizes, dsizes) of an exported seek table frame"""
    magic, size = struct.unpack_from("<II", frame, 0)
    n, desc, seek = struct.unpack_from("<IBI", frame, len(frame) - 9)
    assert (magic, size, desc, seek, len(frame)) == (0x184D2A5E, 8 * n + 9, 0, 0x8F92EAB1, 17 + 8 * n)
    rows = [struct.unpack_from("<II", frame, 8 + 8 * k) for k in range(n)]
    return [c for c, _ in rows], [d for _, d in rows]


def check_index_of(ix, i, sh):
    """entry i of the index is the measured index of shard sh: the info, and every pair through the exported rows"""
    info = ix.infos[i]
    assert (info.status, info.why, info.kind, info.nrows, info.len, info.compressed, info.plaintext) == (
        0, 0, zgpu.INDEX_MEASURED, len(sh.cs), len(sh.z), len(sh.z), sh.D[-1]), info
    cs, ds = parse_table(ix.export_seek_table(i))
    assert cs == sh.cs
    assert ds == sh.ds, [(k, a, b) for k, (a, b) in enumerate(zip(ds, sh.ds)) if a != b][:5]


@pytest.fixture(scope="module")
def big():
    """the 120 seam frames, the extra-bit frames but the five of long plaintext (class Long: a second entry of test 1), a skippable frame, a raw-block, an RLE-block and a no-sequences frame, and two three-block
    text frames (repeat and treeless modes), the second with a checksum; no frame declares its size"""
    import zgdata
    frames, count = [], 0
    for n in NSEQ:
        for shift in range(6):
            name, z, plain = _seam_frame(n, shift)
            assert plain is not None, name
            frames.append((z, plain))
            count += 1
    assert count == 120
    small = [f for f in seqstreams.all_frames() if f[3] is not None and f[1] not in seqstreams.LARGE]
    assert len(small) >= 40
    frames += [(z, plain) for _, _, z, plain in small]
    frames.append((skippable(b"between the families" * 3), None))
    rng = random.Random(0x3EA5)
    for name, blocks in (("m_raw", [("raw", rng.randbytes(777))]), ("m_rle", [("rle", 0x41, 70001)]),
                         ("m_noseq", [tabframes.Block(rng.randbytes(301), [])]), ("m_mixed", [("raw", rng.randbytes(9)), ("rle", 7, 3), tabframes.Block(b"xyz" * 50, [])])):
        name, z, plain = tabframes.build(name, blocks, differs={})
        assert plain is not None
        frames.append((z, plain))
    text = zgdata.text_like(300 << 10, seed=0xFEED)
    for ck in (False, True):
        z = zgdata.zstd_compress(text, checksum=ck, content_size=False)
        ob = [r["type"] for r in blockcheck.oracle_blocks(z)]
        assert ob == [2, 2, 2]
        frames.append((z, text))
    sh = Shard(frames)
    assert sh.nzstd == len(frames) - 1 and len(sh.z) < 4 << 20
    assert all(d is None or d == 0 for _, d in seekidx.rows(sh.z)[0])     # no frame declares a size
    return sh


class Long:
    """the extra-bit frames whose plaintext is long (histories of 16 and 64 MiB in front of the blocks that hold the widest fields: so == 31
    and 32, LL code 35 with ML code 51 and 52) as a shard of their own, a few KiB of input: rows from the header chain, d_k the length of
    the plaintext the generator built — which tests/tabframes.py held against the oracle's decode when it built the frame. Measuring produces
    no plaintext, so these frames cost a measuring submit what any frame of their input size costs."""

    def __init__(self):
        frames = [f for f in seqstreams.all_frames() if f[3] is not None and f[1] in seqstreams.LARGE]
        assert sorted(f[1] for f in frames) == sorted(seqstreams.LARGE)
        cov = seqstreams.coverage(frames)
        assert {31, 32} <= cov["so"]["valid"], cov["so"]           # the 31- and 32-bit LL + ML fields are in THIS shard
        self.z = b"".join(f[2] for f in frames)
        rw, why, _ = seekidx.rows(self.z)
        assert why == 0 and [c for c, _ in rw] == [len(f[2]) for f in frames] and all(d is None for _, d in rw) and len(self.z) < 1 << 20
        self.cs, self.ds = [len(f[2]) for f in frames], [len(f[3]) for f in frames]
        self.C, self.D = seekmany.prefixes(self.cs, self.ds)
        self.nzstd = len(frames)
        assert max(self.ds) > 64 << 20


# ---- 1: the pairs -------------------------------------------------------------------------------------------------------------------------------
def test_pairs_are_the_chains_bytes_and_the_oracles_lengths(ctx, big):
    long = Long()
    s = Sources([big.z, long.z], [5, 2])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        check_index_of(ix, 0, big)
        check_index_of(ix, 1, long)
        st = ix.stats()
        assert (st["frames_measured"], st["rows"], st["input_bytes_to_host"], st["device_bytes"]) == (
            big.nzstd + long.nzstd, len(big.cs) + len(long.cs), 0, 16 * (len(big.cs) + 1 + len(long.cs) + 1)), st
        assert st["measure_submits"] == 1 and ix.device_bytes == st["device_bytes"]
        print("\nmeasured %d frames, %d bytes, %d plaintext bytes: phase 1 %d us, lane passes and gather %d us" % (
            big.nzstd + long.nzstd, len(big.z) + len(long.z), big.D[-1] + long.D[-1], st["measure_us"], st["kernel_us"]))
    assert s.unchanged()


# ---- 2: the records -----------------------------------------------------------------------------------------------------------------------------
def test_records_are_the_rule_on_the_measured_prefixes(ctx, big):
    s = Sources([big.z], [1])
    ranges = [(0, b, n) for b, n in seekidx.boundary_ranges(big.D)]
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        s.t.fill_(0x77)                                   # no byte of the entry is read: whatever it holds now, the records are the index's
        torch.cuda.synchronize()
        got = ctx.frames_seek_indexed_device(ix, ranges)
        st = ctx.gather_ranges_stats()
    for r, k in zip(ranges, got):
        assert k.key() == seekidx.record(big.C, big.D, len(big.z), r[1], r[2]), (r, k)
    assert (st["find_launches"], st["seek_launches"], st["prefix_launches"], st["input_bytes_to_host"], st["frames_decoded"]) == (1, 0, 0, 0, 0), st


# ---- 3: the gather ------------------------------------------------------------------------------------------------------------------------------
def _records(sh, rng, inside=40):
    """ranges that straddle every row boundary of sh, and several inside the text frames"""
    total = sh.D[-1]
    out = []
    for k in range(1, len(sh.D)):
        at = sh.D[k]
        if 3 <= at and at + 3 <= total:
            out.append((0, at - 3, 6))
    big_rows = [k for k in range(len(sh.ds)) if sh.ds[k] > 100000]
    for _ in range(inside):
        k = rng.choice(big_rows)
        b = sh.D[k] + rng.randrange(sh.ds[k] - 600)
        out.append((0, b, rng.randint(1, 500)))
    out += [(0, total - 5, 50), (0, 0, 1), (0, 7, 0), (0, total, 4)]
    return out


def _expect(sh, ranges, bad_rows=(), bad_status=0):
    """records, groups and [(status, bytes or None)]: a group that holds one of bad_rows has bad_status"""
    recs = [seekidx.record(sh.C, sh.D, len(sh.z), b, n) for _, b, n in ranges]
    grps, group_of = seekmany.groups(ranges, [Rec(k) for k in recs])
    exps = []
    for (e, b, n), g in zip(ranges, group_of):
        if g is None:
            exps.append((0, b""))
        elif any(grps[g][1] <= k <= grps[g][2] for k in bad_rows):
            exps.append((bad_status, None))
        else:
            exps.append((0, sh.plain[b:b + n]))
    return recs, grps, exps


def test_gather_serves_records_across_every_kind_of_row(ctx, big):
    rng = random.Random(0x6A7)
    ranges = _records(big, rng)
    rng.shuffle(ranges)
    assert len(ranges) >= 200
    recs, grps, exps = _expect(big, ranges)
    s = Sources([big.z], [3])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        a, res, seeks = run_checked(lambda ptrs, cp: ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, ptrs, cp, hash_max=ALL), s, ranges, recs, exps)
        st = ctx.gather_ranges_stats()
        views = [s.t[s.offs[0]:s.offs[0] + s.lens[0]]]
        outs, res_t, _ = ctx.gather_tensor_ranges(views, ranges, index=ix)
    want_frames = sum(sum(big.zstd[k] for k in range(g[1], g[2] + 1)) for g in grps)
    assert (st["groups_decoded"], st["frames_decoded"], st["find_launches"], st["input_bytes_to_host"]) == (len(grps), want_frames, 1, 0), st
    assert [t.cpu().numpy().tobytes() for t in outs] == [d for _, d in exps] and all(r.status == 0 for r in res_t)
    # the same frames behind a seek table the test writes itself: a table-kind index must serve the same
    z2 = big.z + zgpu.seek_table_frame(big.cs, big.ds)
    s2 = Sources([z2], [3])
    b = Arena(a.caps, [j % 5 for j in range(len(ranges))])
    with ctx.seek_index(s2.ptrs, s2.lens, kind="seek_table") as ix2:
        assert (ix2.infos[0].status, ix2.infos[0].nrows, ix2.infos[0].plaintext) == (0, len(big.cs), big.D[-1])
        old, old_seeks = ctx.gather_ranges_indexed_device_src(ix2, s2.ptrs, s2.lens, ranges, b.ptrs, b.caps, hash_max=ALL)
    assert [(r.status, r.written) for r in old] == [(r.status, r.written) for r in res]
    assert [k.key() for k in old_seeks] == [k.key() for k in seeks]
    assert b.t.cpu().numpy().tobytes() == a.t.cpu().numpy().tobytes()


# ---- 4: several submits -------------------------------------------------------------------------------------------------------------------------
def test_several_measuring_submits_give_the_same_pairs(big, monkeypatch):
    budget = 64 << 10
    assert max(big.cs) > budget and len(big.z) > 3 * budget     # one frame above the budget, and at least three submits
    filler = Shard(_text_frames([5000, 0, 70000], 0x440))
    with framesuite.dev_context(monkeypatch, {"ZGPU_MEASURE_SUBMIT_BYTES": str(budget)}) as c:
        s = Sources([filler.z, big.z, filler.z], [1, 2, 3])
        with c.seek_index_measured(s.ptrs, s.lens) as ix:
            check_index_of(ix, 0, filler)
            check_index_of(ix, 1, big)
            check_index_of(ix, 2, filler)
            st = ix.stats()
            want = len(big.z) // budget
            assert st["measure_submits"] >= max(3, want) and st["frames_measured"] == big.nzstd + 2 * filler.nzstd, st
        assert s.unchanged()


# ---- 5: refusals and isolation --------------------------------------------------------------------------------------------------------------------
def test_refused_entries_never_disturb_the_others(ctx):
    good = Shard(_text_frames([3000, 40000, 1, 9000], 0x510) + [(skippable(b"tail"), None)])
    rejected = [f for f in seqstreams.all_frames() if f[3] is None and seqstreams.STATUS[f[1]] in (44, 46, 47) and len(f[2]) < 1 << 20]
    by_status = {}
    for f in rejected:
        by_status.setdefault(seqstreams.STATUS[f[1]], f)
    assert len(by_status) >= 2, sorted(by_status)               # (the families hold NotEnoughBytes and ExtraBits streams, and ExtraPadding ones)
    pre = _text_frames([2000, 100], 0x520)
    host = C.create_string_buffer(good.z, len(good.z))
    dict_entry = pre[0][0] + dictframes.frame(0x4D2, dictframes.raw_block(300, last=True)) + pre[1][0]
    trunc = good.z[:good.C[2] - 7]
    why_trunc = seekidx.rows(trunc)[1]
    assert why_trunc in range(1, 9) and seekidx.rows(dict_entry)[1] == 0
    for bad in by_status.values():
        _, name, zbad, _ = bad
        status = seqstreams.STATUS[name]
        entries = [good.z, pre[0][0] + pre[1][0] + zbad + pre[0][0], trunc, dict_entry, None, b""]
        assert seekidx.rows(entries[1])[1] == 0, name      # (its chain is whole: only the measuring refuses it)
        want = [(0, 0, len(good.cs)), (BAD, zgpu.INDEX_UNMEASURED, 0), (BAD, why_trunc, 0), (BAD, zgpu.INDEX_DICT, 0), (zgpu.E_BAD_ARG, 0, 0), (0, 0, 0)]
        for order in (list(range(6)), list(range(5, -1, -1))):
            s = Sources([entries[i] or b"" for i in order], [i % 4 for i in order])
            ptrs = [C.addressof(host) if entries[i] is None else p for i, p in zip(order, s.ptrs)]
            lens = [len(good.z) if entries[i] is None else n for i, n in zip(order, s.lens)]
            with ctx.seek_index_measured(ptrs, lens) as ix:
                assert [(x.status, x.why, x.nrows) for x in ix.infos] == [want[i] for i in order], (name, order, ix.infos)
                assert all(x.kind == zgpu.INDEX_MEASURED and (x.status == 0 or (x.compressed, x.plaintext) == (0, 0)) for x in ix.infos)
                check_index_of(ix, order.index(0), good)
                err = ctx.last_error()
                assert "entry %d, frame 2: %s" % (order.index(1), zgpu.load_library().zgpu_status_name(status).decode()) in err, (err, status)
                ranges = [(e, 5, 10) for e in range(6)] + [(order.index(1), 0, 0)]
                recs = ctx.frames_seek_indexed_device(ix, ranges)
                for e in range(6):
                    st_, why_, _ = want[order[e]]
                    if st_ == zgpu.E_BAD_ARG or st_ == BAD:
                        assert recs[e].key() == (0,) * 5 + (st_, 0, 0, 0, why_, 0), (e, recs[e])
                assert recs[order.index(0)].key() == seekidx.record(good.C, good.D, len(good.z), 5, 10)
                assert recs[order.index(5)].nothing and recs[6].key() == (0,) * 11
                # a gather over the handle: the good entry is served, a refused one's range carries its status
                rr = [(order.index(0), good.D[1] - 2, 9), (order.index(1), 0, 5), (order.index(3), 0, 5)]
                a = Arena([9, 5, 5], [1, 2, 3])
                res, _ = ctx.gather_ranges_indexed_device_src(ix, ptrs, lens, rr, a.ptrs, a.caps, hash_max=ALL)
                assert [(r.status, r.written) for r in res] == [(0, 9), (BAD, 0), (BAD, 0)]
                a.check([good.plain[good.D[1] - 2:good.D[1] + 7], None, None])
            assert s.unchanged()


# ---- 6: what measuring does not see -----------------------------------------------------------------------------------------------------------------
def _flip_in_huffman_stream(z):
    """z, a frame of one block with Huffman-compressed literals in four streams, with one byte of its last literal stream changed so that
    the oracle refuses the frame; and the oracle's status. The sizes in the headers are untouched by construction."""
    assert z[4] & 0xC0 == 0 and not z[4] & 0x20 and not z[4] & 3           # no content size, a window descriptor, no dictionary id
    body = 6 + 3
    b0 = z[body]
    assert b0 & 3 == 2 and (b0 >> 2) & 3 in (1, 2, 3)                       # compressed literals, four streams
    sf = (b0 >> 2) & 3
    hl, bits = {1: (3, 10), 2: (4, 14), 3: (5, 18)}[sf]
    v = int.from_bytes(z[body:body + hl], "little") >> 4
    comp = v >> bits
    assert comp > 400
    for back in range(8, 200, 7):
        at = body + hl + comp - back                                         # inside the fourth stream, far behind the tree description and the jump table
        for x in (0xFF, 0x55, 0x01):
            cand = z[:at] + bytes([z[at] ^ x]) + z[at + 1:]
            st, _ = oracle_alone(cand, 1 << 20)
            if st in (32, 33, 34, 35):                                          # a verdict of the literal streams
                return cand, st
    raise AssertionError("no flipped byte makes the oracle refuse the literal streams")


def test_a_huffman_defect_is_indexed_and_surfaces_in_the_gather(ctx):
    frames = _text_frames([30000, 50000, 20000, 45000, 8000], 0x610)
    j = 3
    cand, status = _flip_in_huffman_stream(frames[j][0])
    clean = Shard(frames)
    flipped = clean.z[:clean.C[j]] + cand + clean.z[clean.C[j + 1]:]
    assert len(flipped) == len(clean.z) and seekidx.rows(flipped)[0] == seekidx.rows(clean.z)[0]
    s = Sources([flipped], [2])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        check_index_of(ix, 0, clean)                              # the index is built, and equals the unflipped shard's
        D = clean.D
        ranges = [(0, 10, 100), (0, D[j] - 4, 8), (0, D[j] + 500, 300), (0, D[j + 1] + 7, 70), (0, D[1] + 1, 99), (0, D[2] + 5, 10)]
        recs, grps, exps = _expect(clean, ranges, bad_rows=(j,), bad_status=status)
        # rows 2 - 3 are one group (the second range straddles them) and share frame 3's fate; rows 0, 1 and 4 are served
        assert [st for st, _ in exps] == [0, status, status, 0, 0, status] and [(g[1], g[2]) for g in grps] == [(0, 0), (1, 1), (2, 3), (4, 4)]
        run_checked(lambda ptrs, cp: ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, ptrs, cp, hash_max=ALL), s, ranges, recs, exps)


# ---- 7: a stale index -------------------------------------------------------------------------------------------------------------------------------
def test_a_stale_measured_index_is_a_size_mismatch(ctx):
    frames = _text_frames([12000, 30000, 9000, 26000], 0x710)
    a = Shard(frames)
    k = 1
    other = _text_frames([11000], 0x7AA)[0]
    room = len(frames[k][0]) - len(other[0])
    assert room >= 8
    b_frames = frames[:k] + [other, (skippable(bytes(room - 8)), None)] + frames[k + 1:]
    b = Shard(b_frames)
    assert len(b.z) == len(a.z) and b.C[k + 2] == a.C[k + 1]
    s = Sources([a.z], [6])
    with ctx.seek_index_measured(s.ptrs, s.lens) as ix:
        check_index_of(ix, 0, a)
        s.t[s.offs[0]:s.offs[0] + len(b.z)] = torch.frombuffer(bytearray(b.z), dtype=torch.uint8).to("cuda:0")   # the same tensor now holds shard B
        torch.cuda.synchronize()
        s.host = s.host[:s.offs[0]] + b.z + s.host[s.offs[0] + len(b.z):]
        D = a.D
        ranges = [(0, 5, 50), (0, D[k] + 10, 100), (0, D[k + 1] - 3, 2), (0, D[k + 1] + 3, 40), (0, D[3] + 1, 9)]
        recs, grps, exps = _expect(a, ranges, bad_rows=(k,), bad_status=zgpu.E_CONTENT_SIZE_MISMATCH)
        assert [st for st, _ in exps] == [0, zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_CONTENT_SIZE_MISMATCH, 0, 0]
        run_checked(lambda ptrs, cp: ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, ptrs, cp, hash_max=ALL), s, ranges, recs, exps)


# ---- 8: the modes -----------------------------------------------------------------------------------------------------------------------------------
def test_only_unsized_measures_what_auto_refuses_as_unsized(ctx):
    sizes = [4096, 100, 30000]
    unsized = Shard(_text_frames(sizes, 0x810))
    declared = Shard(_text_frames(sizes, 0x820, content_size=True))
    table_frames = _text_frames(sizes, 0x830)
    tabled = seekable([z for z, _ in table_frames], sizes)
    with_table = Shard(table_frames + [(tabled[sum(len(z) for z, _ in table_frames):], None)])
    assert with_table.z == tabled
    broken = unsized.z[:-3]
    s = Sources([tabled, declared.z, unsized.z, broken], [0, 1, 2, 3])
    with ctx.seek_index_measured(s.ptrs, s.lens, only_unsized=True) as ix:
        assert [(i.status, i.kind, i.nrows, i.plaintext) for i in ix.infos[:3]] == [
            (0, zgpu.INDEX_SEEK_TABLE, 3, sum(sizes)), (0, zgpu.INDEX_DECLARED, 3, sum(sizes)), (0, zgpu.INDEX_MEASURED, 3, sum(sizes))], ix.infos
        assert (ix.infos[3].status, ix.infos[3].why, ix.infos[3].kind) == (BAD, seekidx.rows(broken)[1], zgpu.INDEX_DECLARED), ix.infos[3]   # a broken chain stays the error it is
        st = ix.stats()
        assert (st["frames_measured"], st["measure_submits"], st["rows"]) == (3, 1, 9), st
        check_index_of(ix, 2, unsized)
        outs, res, _ = ctx.gather_tensor_ranges([s.t[o:o + n] for o, n in zip(s.offs, s.lens)], [(e, 4090, 20) for e in range(3)], index=ix)
        assert [r.status for r in res] == [0, 0, 0]
        assert [t.cpu().numpy().tobytes() for t in outs] == [sh.plain[4090:4110] for sh in (with_table, declared, unsized)]
    with ctx.seek_index_measured(s.ptrs[:3], s.lens[:3]) as ix:
        check_index_of(ix, 0, with_table)                         # the table frame is a row of d = 0
        check_index_of(ix, 1, declared)
        check_index_of(ix, 2, unsized)
        assert ix.stats()["frames_measured"] == 9 and ix.infos[0].nrows == 4
    assert s.unchanged()


# ---- 9: the export ----------------------------------------------------------------------------------------------------------------------------------
def test_export_round_trip(ctx):
    sizes = [5000, 0, 131073, 77]
    unsized = Shard(_text_frames(sizes, 0x910) + [(skippable(b"x" * 11), None)])
    declared = Shard([(skippable(b""), None)] + _text_frames(sizes, 0x920, content_size=True, checksum=True))
    s = Sources([unsized.z, declared.z, unsized.z[:-1]], [1, 2, 3])
    L = ctx.L
    with ctx.seek_index_measured(s.ptrs, s.lens, only_unsized=True) as ix:
        assert [i.kind for i in ix.infos[:2]] == [zgpu.INDEX_MEASURED, zgpu.INDEX_DECLARED] and ix.infos[2].status == BAD
        tables = [ix.export_seek_table(0), ix.export_seek_table(1)]
        for t, sh in zip(tables, (unsized, declared)):
            assert t == zgpu.seek_table_frame(sh.cs, sh.ds)
        # a capacity that is too small reports the size and writes nothing; an entry with a status is no entry to export
        need = C.c_size_t(0)
        buf = C.create_string_buffer(b"\xA5" * 64, 64)
        assert L.zgpu_seek_index_export_seek_table(ix.h, 0, buf, len(tables[0]) - 1, C.byref(need)) == zgpu.E_TARGET_TOO_SMALL
        assert need.value == len(tables[0]) == 17 + 8 * len(unsized.cs) and buf.raw == b"\xA5" * 64
        assert L.zgpu_seek_index_export_seek_table(ix.h, 0, None, 0, C.byref(need)) == zgpu.E_TARGET_TOO_SMALL and need.value == len(tables[0])
        for entry in (2, 3):
            assert L.zgpu_seek_index_export_seek_table(ix.h, entry, buf, 64, C.byref(need)) == zgpu.E_BAD_ARG and need.value == 0
        with pytest.raises(zgpu.ZgpuError) as err:
            ix.export_seek_table(2)
        assert err.value.status == zgpu.E_BAD_ARG
        # the entry's bytes followed by the exported frame: a seekable entry with the same rows
        seekables = [unsized.z + tables[0], declared.z + tables[1]]
        s2 = Sources(seekables, [3, 0])
        with ctx.seek_index(s2.ptrs, s2.lens, kind="seek_table") as ix2:
            for i, sh in enumerate((unsized, declared)):
                assert (ix2.infos[i].status, ix2.infos[i].kind, ix2.infos[i].nrows, ix2.infos[i].compressed, ix2.infos[i].plaintext) == (
                    0, zgpu.INDEX_SEEK_TABLE, len(sh.cs), len(sh.z), sh.D[-1])
                assert ix2.export_seek_table(i) == tables[i]                 # the same C and D, row by row
            ranges = [(e, b, n) for e, sh in enumerate((unsized, declared)) for b, n in ((0, 9), (4998, 5), (5000 + 131070, 20), (sh.D[-1] - 3, 9))]
            recs_a = ctx.frames_seek_indexed_device(ix, ranges)
            recs_b = ctx.frames_seek_indexed_device(ix2, ranges)
            assert [k.key() for k in recs_a] == [k.key() for k in recs_b]
            caps = [n for _, _, n in ranges]
            a, b = Arena(caps), Arena(caps)
            ra, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, ranges, a.ptrs, caps, hash_max=ALL)
            rb, _ = ctx.gather_ranges_indexed_device_src(ix2, s2.ptrs, s2.lens, ranges, b.ptrs, caps, hash_max=ALL)
            assert [(r.status, r.written) for r in ra] == [(r.status, r.written) for r in rb] and all(r.status == 0 for r in ra)
            assert a.t.cpu().numpy().tobytes() == b.t.cpu().numpy().tobytes()
            a.check([sh.plain[b_:b_ + n] for e, b_, n in ranges for sh in [(unsized, declared)[e]]])
    assert s.unchanged() and s2.unchanged()
