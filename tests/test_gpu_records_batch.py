"""Record batches on the GPU (zgpu_gather_records_batch_indexed_device_src, zg_k_fill; Context.gather_records_batch,
gather_records_batch_tensors). No expectation comes from the call under test: the shards are test_gpu_seek_index_records.Kind's (every frame
held against the oracle) plus one entry of lines whose lengths the test chose, the lookup is tests/records.py's, and the batch — image,
lengths, offsets, statuses — is tests/recbatch.py's, written from include/zgpu.h. Everything is compared for equality. The batch and its two
arrays lie in one devmem.Arena slot each, so the sentinel stands on every side of each; the pad bytes are not the sentinel."""
import os
import random
import struct
import sys

import numpy as np
import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import framesuite
import recbatch
import records
import tabframes
import zgpu
from devmem import Arena, Sources, full_key, oracle_alone
from test_gpu_seek_index_measured import Shard, _flip_in_huffman_stream, _text_frames
from test_gpu_seek_index_records import CLOSED, EMPTY, NL, OPEN, STRIP, Kind, _record_sets
from test_walk_cpu import skippable

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: the workload generators
pytestmark = pytest.mark.gpu
WIDTHS = (1, 17, 64, 4097)
LINES = 3                                   # the entry of chosen lines
PADS = (0x00, 0xEE)
TOO_SMALL = zgpu.E_TARGET_TOO_SMALL


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


class Data:
    """Kind("declared")'s three entries and, as entry LINES, lines of width - 1, width and width + 1 bytes (newline included) for every width"""

    def __init__(self):
        import zgdata
        self.kind = Kind("declared")
        rng = random.Random(0xBA7)
        text = b"".join(bytes(rng.choice(b"abcdefgh ") for _ in range(n - 1)) + b"\n" for w in WIDTHS for n in (w - 1, w, w + 1, 40) if n)
        self.entries = self.kind.entries + [zgdata.zstd_compress(text, checksum=False, content_size=True)]
        assert oracle_alone(self.entries[LINES], len(text) + 64) == (0, text)
        self.plains = self.kind.plains + [text]
        self.model = self.kind.model + [records.offsets(text, NL)]

    def line(self, n):
        """a record of entry LINES that is n bytes long"""
        O = self.model[LINES][0]
        return next(r for r in range(len(O) - 1) if O[r + 1] - O[r] == n)

    def rows(self, width):
        """scenario 1's rows: shorter than, equal to and one byte longer than the width, an empty range, behind the last record, a record that
        straddles a frame boundary, STRIP, the open tail, an entry out of range, the entry of length 0"""
        O, Ro = self.model[CLOSED][0], len(self.model[OPEN][0]) - 1
        straddle = _record_sets(self.kind.shards[CLOSED], O)[2]
        rows = [(LINES, self.line(width - 1), 1)] if width > 1 else []
        return rows + [(LINES, self.line(width), 1), (LINES, self.line(width + 1), 1), (CLOSED, 5, 0), (CLOSED, len(O) + 6, 1), (CLOSED,) + straddle,
                       (CLOSED, 3, 1, STRIP), (LINES, self.line(width), 1, STRIP), (OPEN, Ro - 1, 1), (9, 0, 1), (EMPTY, 0, 1)]


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def indexed(ctx, data):
    s = Sources(data.entries, [1, 2, 0, 3])
    ix = ctx.seek_index(s.ptrs, s.lens, kind="declared")
    assert [i.status for i in ix.infos] == [0] * 4
    assert [r.state for r in ix.records(s.ptrs, s.lens)] == [1] * 4
    yield s, ix
    assert s.unchanged()
    ix.close()


def _u64s(v):
    return struct.pack("<%dQ" % len(v), *v)


def batch(ctx, ix, s, recs, exp, layout, width=0, pad=0, truncate=False, shift=0, arrays=True, **opts):
    """the call into one Arena slot of exactly exp.total bytes (shifted) and one slot per array; the arena, results, statuses, lengths,
    offsets, info and record_bytes held against exp; (results, seeks, info)"""
    m = len(recs)
    a = Arena([exp.total, 8 * m, 8 * (m + 1)], [shift, 0, 8])
    res, seeks, info, rb = ctx.gather_records_batch(ix, s.ptrs, s.lens, recs, a.ptrs[0] if exp.total else 0, exp.total, layout=layout, width=width,
                                                    pad=pad, truncate=truncate, lengths_ptr=a.ptrs[1] if arrays and m else 0,
                                                    offsets_ptr=a.ptrs[2] if arrays else 0, **opts)
    print("%s width=%d m=%d: total %d, filled %d, ok %d, failed %d, truncated %d" % (layout, width, m, info.total, info.bytes_filled, info.rows_ok,
                                                                                 info.rows_failed, info.rows_truncated))
    assert [r.status for r in res] == exp.statuses
    assert [r.written for r in res] == exp.lengths
    assert rb == exp.record_bytes
    assert (info.total, info.bytes_filled, info.rows_ok, info.rows_failed, info.rows_truncated) == (exp.total, exp.filled, exp.ok, m - exp.ok, exp.truncated)
    a.check([exp.image, _u64s(exp.lengths) if arrays and m else None, _u64s(exp.offsets) if arrays else None])
    return res, seeks, info


# ---- 1: padded ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_padded_rows_equal_the_model(ctx, data, indexed, width):
    s, ix = indexed
    recs = data.rows(width)
    found = recbatch.lookup(data.model, recs)
    for shift, pad in ((0, 0x00), (5, 0xEE), (15, 0x00)):
        exp = recbatch.Batch(data.plains, found, recbatch.PADDED, width, pad)
        over = recs.index((LINES, data.line(width + 1), 1))
        assert exp.statuses[over] == TOO_SMALL and exp.lengths[over] == 0 and exp.image[over * width:(over + 1) * width] == bytes([pad]) * width
        assert exp.statuses[over - 1] == 0 and exp.lengths[over - 1] == width and exp.statuses[-2:] == [zgpu.E_BAD_ARG, 0]
        res, seeks, _ = batch(ctx, ix, s, recs, exp, "padded", width, pad, shift=shift)
        st = ctx.gather_records_stats()
        assert (st["batch_fill_launches"], st["batch_bytes_filled"], st["batch_bytes_uploaded"]) == (1, exp.filled, 8 * (2 * len(recs) + 1)), st
        assert (st["record_find_launches"], st["record_find_bytes_downloaded"]) == (1, 24 * len(recs))
    # results and seeks are the separate-destination call's on the same ranges with caps = width, key for key
    b = Arena([width] * len(recs), [j % 7 for j in range(len(recs))])
    res0, seeks0 = ctx.gather_records_indexed_device_src(ix, s.ptrs, s.lens, recs, b.ptrs, b.caps)
    assert [full_key(r) for r in res] == [full_key(r) for r in res0] and [k.key() for k in seeks] == [k.key() for k in seeks0]


# ---- 2: truncation ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_truncated_rows_equal_the_model(ctx, data, indexed, width):
    s, ix = indexed
    recs = data.rows(width)
    found = recbatch.lookup(data.model, recs)
    exp = recbatch.Batch(data.plains, found, recbatch.PADDED, width, 0xEE, truncate=True)
    assert exp.lengths == [0 if st else min(n, width) for st, _, _, n in found] and TOO_SMALL not in exp.statuses
    assert exp.truncated == sum(1 for st, _, _, n in found if not st and n > width) >= 1 and exp.record_bytes != exp.lengths
    batch(ctx, ix, s, recs, exp, "padded", width, 0xEE, truncate=True, shift=3)


def test_a_truncated_range_decodes_no_frame_behind_the_cut(ctx, data, indexed):
    s, ix = indexed
    first, count = _record_sets(data.kind.shards[CLOSED], data.model[CLOSED][0])[3]      # a range that spans several frames
    recs = [(CLOSED, first, count)]
    found = recbatch.lookup(data.model, recs)
    assert found[0][3] > 70000
    exp = recbatch.Batch(data.plains, found, recbatch.PADDED, 17, 0x00, truncate=True)
    batch(ctx, ix, s, recs, exp, "padded", 17, 0x00, truncate=True)
    cut = ctx.gather_records_stats()["frames_decoded"]
    a = Arena([17], [1])
    res, _ = ctx.gather_ranges_indexed_device_src(ix, s.ptrs, s.lens, [(CLOSED, found[0][2], 17)], a.ptrs, a.caps)
    assert res[0].status == 0 and cut == ctx.gather_records_stats()["frames_decoded"] >= 1
    whole = recbatch.Batch(data.plains, found, recbatch.PACKED)
    batch(ctx, ix, s, recs, whole, "packed")
    assert ctx.gather_records_stats()["frames_decoded"] > cut


# ---- 3: packed --------------------------------------------------------------------------------------------------------------------------------------
def test_packed_batches_equal_the_model(ctx, data, indexed):
    s, ix = indexed
    recs = data.rows(64) + [(CLOSED,) + x for x in _record_sets(data.kind.shards[CLOSED], data.model[CLOSED][0])[:4]]
    found = recbatch.lookup(data.model, recs)
    exp = recbatch.Batch(data.plains, found, recbatch.PACKED, pad=0xEE)
    assert exp.image == b"".join(data.plains[e][b:b + n] for st, e, b, n in found if not st) and exp.filled == 0
    m = len(recs)
    for shift in (0, 5, 15):
        batch(ctx, ix, s, recs, exp, "packed", pad=0xEE, shift=shift)                       # cap == total succeeds
    # the size query, and a batch one byte too small: every good row TOO_SMALL, the need in info.total, nothing written
    _, _, info, rb = ctx.gather_records_batch(ix, s.ptrs, s.lens, recs, 0, 0, layout="packed")
    assert info.total == exp.total and rb == exp.record_bytes
    a = Arena([exp.total, 8 * m, 8 * (m + 1)], [3, 0, 0])
    res, _, info, _ = ctx.gather_records_batch(ix, s.ptrs, s.lens, recs, a.ptrs[0], exp.total - 1, layout="packed", lengths_ptr=a.ptrs[1], offsets_ptr=a.ptrs[2])
    assert [r.status for r in res] == [st or TOO_SMALL for st, _, _, _ in found] and [r.written for r in res] == [0] * m
    assert (info.total, info.rows_ok, info.rows_failed, info.bytes_filled) == (exp.total, 0, m, 0)
    st = ctx.gather_records_stats()
    assert (st["batch_fill_launches"], st["batch_bytes_uploaded"], st["frames_decoded"], st["record_find_launches"]) == (0, 0, 0, 1), st
    a.check([None, None, None])
    # packed with a width and TRUNCATE
    cut = recbatch.Batch(data.plains, found, recbatch.PACKED, 17, 0x00, truncate=True)
    assert cut.truncated > 3 and cut.total < exp.total and max(cut.lengths) == 17
    batch(ctx, ix, s, recs, cut, "packed", 17, truncate=True, shift=9)
    # m == 0, with and without an offsets array
    none = recbatch.Batch(data.plains, [], recbatch.PACKED)
    assert (none.total, none.offsets) == (0, [0])
    batch(ctx, ix, s, [], none, "packed", arrays=True)
    batch(ctx, ix, s, [], none, "packed", arrays=False)
    assert ctx.gather_records_stats()["batch_fill_launches"] == 0
    batch(ctx, ix, s, [], recbatch.Batch(data.plains, [], recbatch.PADDED, 8), "padded", 8)


# ---- 4: failing rows --------------------------------------------------------------------------------------------------------------------------------
def test_rows_of_a_failing_group_are_all_pad(ctx):
    text = _text_frames([30000, 50000, 20000, 45000, 8000], 0x610)
    huf, huf_status = _flip_in_huffman_stream(text[3][0])
    clean = Shard(_text_frames([900, 20, 4000], 0x630))
    good = Shard([text[0], (skippable(b"gap"), None), text[3], text[4]])
    bad = good.z[:good.C[2]] + huf + good.z[good.C[3]:]
    assert len(bad) == len(good.z)
    plains = [clean.plain, good.plain]
    model = [records.offsets(p, NL) for p in plains]
    O = model[1][0]
    inside = [r for r in range(len(O) - 1) if good.D[2] <= O[r] and O[r + 1] <= good.D[3]]     # records that lie in the flipped frame
    before = [r for r in range(len(O) - 1) if O[r + 1] <= good.D[1]]
    recs = [(0, 1, 2), (1, inside[0], 1), (1, before[1], 1), (1, inside[-1], 1, STRIP), (0, 0, 1)]
    found = recbatch.lookup(model, recs)
    sg, sb = Sources([clean.z, good.z], [1, 2]), Sources([clean.z, bad], [2, 1])
    with ctx.seek_index_measured(sg.ptrs, sg.lens) as ix:
        assert [r.state for r in ix.records(sg.ptrs, sg.lens)] == [1, 1]
        for layout, width in ((recbatch.PADDED, max(n for _, _, _, n in found) + 5), (recbatch.PACKED, 0)):
            for pad in PADS:
                exp = recbatch.Batch(plains, found, layout, width, pad, failed={1: huf_status, 3: huf_status})
                assert exp.lengths[1] == exp.lengths[3] == 0 and exp.lengths[0] and exp.lengths[2] and exp.lengths[4]
                if layout == recbatch.PACKED:                                                # the failed rows' slots keep their place
                    assert exp.offsets[2] - exp.offsets[1] == found[1][3] > 0 and exp.filled == found[1][3] + found[3][3]
                batch(ctx, ix, sb, recs, exp, "padded" if layout == recbatch.PADDED else "packed", width, pad, shift=7)
                batch(ctx, ix, sg, recs, recbatch.Batch(plains, found, layout, width, pad), "padded" if layout == recbatch.PADDED else "packed", width, pad)
    assert sg.unchanged() and sb.unchanged()


# ---- 5: under the handle's sums ---------------------------------------------------------------------------------------------------------------------
def test_a_changed_byte_fails_its_rows_under_the_flag(ctx):
    rng = random.Random(0x7A1E)
    raw = bytes(rng.choice(b"ab\n") for _ in range(900))
    _, zraw, praw = tabframes.build("r_raw", [("raw", raw)], differs={})
    sh = Shard(_text_frames([3000, 500], 0x410) + [(zraw, praw)] + _text_frames([800], 0x420))
    O, tail = records.offsets(sh.plain, NL)
    at = zraw.find(praw[:64])
    assert at > 0 and zraw[at:at + len(praw)] == praw
    pos, k = sh.C[2] + at + 400, sh.D[2] + 400                               # a byte of the raw block: every size stays what it was
    changed = sh.z[:pos] + bytes([sh.z[pos] ^ 0x01]) + sh.z[pos + 1:]
    plain2 = sh.plain[:k] + bytes([sh.plain[k] ^ 0x01]) + sh.plain[k + 1:]
    r = max(x for x in range(len(O) - 1) if O[x] <= k)                        # the record that holds the byte
    recs = [(0, r, 1), (0, 0, 1), (0, r, 1, STRIP)]
    found = recbatch.lookup([(O, tail)], recs)
    good, bad = Sources([sh.z], [2]), Sources([changed], [2])
    with ctx.seek_index_measured(good.ptrs, good.lens) as ix:
        ix.records(good.ptrs, good.lens)
        ix.hash(good.ptrs, good.lens)
        width = max(n for _, _, _, n in found) + 3
        # without the flag the stale offsets' bytes are delivered with status 0; with it the group fails, as the byte gather refuses the same ranges
        batch(ctx, ix, bad, recs, recbatch.Batch([plain2], found, recbatch.PADDED, width, 0xEE), "padded", width, 0xEE)
        sums = zgpu.E_SEEK_CHECKSUM_MISMATCH
        for layout in (recbatch.PADDED, recbatch.PACKED):
            w = width if layout == recbatch.PADDED else 0
            exp = recbatch.Batch([sh.plain], found, layout, w, 0xEE, failed={0: sums, 2: sums})
            res, _, _ = batch(ctx, ix, bad, recs, exp, "padded" if w else "packed", w, 0xEE, shift=1, verify_table=True)
        c = Arena([n for _, _, _, n in found], [1, 2, 3])
        r0, _ = ctx.gather_ranges_indexed_device_src(ix, bad.ptrs, bad.lens, [(e, b, n) for _, e, b, n in found], c.ptrs, c.caps, verify_table=True)
        assert [x.status for x in r0] == [sums, 0, sums] == [x.status for x in res]
        batch(ctx, ix, good, recs, recbatch.Batch([sh.plain], found, recbatch.PADDED, width, 0x00), "padded", width, verify_table=True)
    assert good.unchanged() and bad.unchanged()


# ---- 6: arguments -----------------------------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_a_status_and_writes_nothing(ctx, data, indexed):
    s, ix = indexed
    recs = [(LINES, data.line(17), 1), (CLOSED, 0, 1)]
    m = len(recs)
    a = Arena([64 * m, 8 * m + 8, 8 * (m + 1) + 8], [0, 0, 0])
    host = np.zeros(4096, dtype=np.uint8)
    good = dict(dst_ptr=a.ptrs[0], cap=64 * m, layout="padded", width=64, lengths_ptr=a.ptrs[1], offsets_ptr=a.ptrs[2])
    other = zgpu.Context(0)
    try:
        def bad(c=ctx, lens=None, **change):
            kw = dict(good, **change)
            with pytest.raises(zgpu.ZgpuError) as err:
                c.gather_records_batch(ix, s.ptrs, lens or s.lens, recs, kw.pop("dst_ptr"), kw.pop("cap"), **kw)
            assert err.value.status == zgpu.E_BAD_ARG, change
        bad(c=other)                                                              # a handle of another context
        with pytest.raises(zgpu.ZgpuError):
            ctx.gather_records_batch(ix, s.ptrs[:2], s.lens[:2], recs, a.ptrs[0], 64 * m, width=64)    # n is not the entry count
        bad(pad=256)
        bad(width=0)
        bad(layout="packed", width=64)                                            # packed with a width and no TRUNCATE
        bad(lengths_ptr=a.ptrs[1] + 4)
        bad(offsets_ptr=a.ptrs[2] + 1)
        bad(dst_ptr=host.ctypes.data)                                             # host memory
        bad(dst_ptr=host.ctypes.data, cap=host.size, layout="packed", width=0)    # (the packed total is known behind the lookup; it fits)
        bad(lengths_ptr=host.ctypes.data)
        bad(offsets_ptr=host.ctypes.data)
        bad(width=1 << 63, truncate=True)                                         # m * width passes 64 bits
        bad(no_hash=True, verify=True)                                            # options the gather refuses
        L, h = ctx.L, ix.h
        info, res = zgpu.RecordBatchInfoC(), (zgpu.RangeResultC * m)()
        for change in (dict(layout=2), dict(flags=2), dict(reserved=1)):
            b = zgpu.RecordBatchC(**dict(dict(device_dst=a.ptrs[0], cap=64 * m, width=64), **change))
            assert L.zgpu_gather_records_batch_indexed_device_src(ctx.h, h, zgpu._ptr_array(s.ptrs), zgpu._size_array(s.lens), 4, ctx._record_ranges(recs), m,
                                                                  b, None, res, info) == zgpu.E_BAD_ARG, change
        a.check([None, None, None])
        assert not host.any()
        # and the same arguments, right, succeed
        exp = recbatch.Batch(data.plains, recbatch.lookup(data.model, recs), recbatch.PADDED, 64, 0)
        batch(ctx, ix, s, recs, exp, "padded", 64)
    finally:
        other.close()


# ---- 7: launch edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 2100])
def test_launch_edges(ctx, data, indexed, m):
    """2100 rows of width 32: more chunks than the 2048 waves of one launch hold, so the grid stride takes a second turn"""
    s, ix = indexed
    R = len(data.model[CLOSED][0]) - 1
    recs = [(CLOSED, (7 * j) % R, 1, STRIP) if j % 50 == 0 else (LINES, data.line(18), 1) if j % 50 == 1 else (OPEN, j, 0) for j in range(m)]
    found = recbatch.lookup(data.model, recs)
    exp = recbatch.Batch(data.plains, found, recbatch.PADDED, 32, 0xEE, truncate=True)
    chunks = sum(1 for n in exp.lengths if n < 32)                                # (a pad region of at most 32 bytes is one chunk)
    assert chunks > 2048 if m == 2100 else chunks < 2048
    batch(ctx, ix, s, recs, exp, "padded", 32, 0xEE, truncate=True, shift=m % 16)
    st = ctx.gather_records_stats()
    assert (st["batch_fill_launches"], st["batch_bytes_filled"]) == (1, exp.filled), st


# ---- 8: memory histories ----------------------------------------------------------------------------------------------------------------------------
def test_images_do_not_depend_on_what_memory_held(data, monkeypatch):
    recs = data.rows(64) + [(CLOSED,) + _record_sets(data.kind.shards[CLOSED], data.model[CLOSED][0])[3]]
    found = recbatch.lookup(data.model, recs)
    for poison in framesuite.POISONS:
        with framesuite.poisoned_context(monkeypatch, poison) as c:
            s = Sources(data.entries, [1, 2, 0, 3])
            with c.seek_index(s.ptrs, s.lens, kind="declared") as ix:
                ix.records(s.ptrs, s.lens)
                batch(c, ix, s, recs, recbatch.Batch(data.plains, found, recbatch.PADDED, 64, 0xEE), "padded", 64, 0xEE, shift=5)
                batch(c, ix, s, recs, recbatch.Batch(data.plains, found, recbatch.PACKED, pad=0x00), "packed", shift=11)
            assert s.unchanged()


# ---- 9: the tensor helper ---------------------------------------------------------------------------------------------------------------------------
def test_tensor_helper_against_numpy(ctx, data, indexed):
    s, ix = indexed
    tensors = [s.t[o:o + n] for o, n in zip(s.offs, s.lens)]
    recs = data.rows(64)
    found = recbatch.lookup(data.model, recs)
    exp = recbatch.Batch(data.plains, found, recbatch.PADDED, 64, 0xEE, truncate=True)
    rows, lengths, res = ctx.gather_records_batch_tensors(ix, tensors, recs, width=64, pad=0xEE, truncate=True)
    assert rows.shape == (len(recs), 64) and rows.dtype == torch.uint8 and lengths.dtype == torch.int64
    assert np.array_equal(rows.cpu().numpy(), np.frombuffer(exp.image, dtype=np.uint8).reshape(len(recs), 64))
    assert lengths.cpu().tolist() == exp.lengths and [r.status for r in res] == exp.statuses
    exp = recbatch.Batch(data.plains, found, recbatch.PACKED)
    flat, offsets, lengths, res = ctx.gather_records_batch_tensors(ix, tensors, recs)
    assert flat.shape == (exp.total,) and np.array_equal(flat.cpu().numpy(), np.frombuffer(exp.image, dtype=np.uint8))
    assert offsets.cpu().tolist() == exp.offsets and lengths.cpu().tolist() == exp.lengths and [r.status for r in res] == exp.statuses
    flat, offsets, lengths, res = ctx.gather_records_batch_tensors(ix, tensors, [])
    assert flat.numel() == 0 and offsets.cpu().tolist() == [0] and lengths.numel() == 0 and res == []
