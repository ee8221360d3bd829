"""The seek-many passes (zstd-rs_amd/csrc/zg_seekmany.h: locate, total, prefix, find), compiled with g++ over the SIMT emulator
(tests/emu/zg_simt.h) and run on the CPU as Engine::seekmany_pass lays them out: one lane per entry, one wave per chunk of rows, one lane per
range, the scratch sized from the located row count. tests/emu/zg_emu_seekmany.cpp is the harness, built by tests/lanesuite.py. Demanded of
every entry and every range:
  - the record equals tests/seektabs.py's model, all 64 bytes, and the one zgt::seektab_entry's wave gives for the same range;
  - no access of the entry outside [tab, len) (outside the footer, where the table is refused before its frame is located), none at all where
    every range has length 0, and no access outside the prefix scratch of 16 * (nframes + 1) bytes plus the chunk totals;
  - the prefix arrays equal Python's sums.
Entries: the whole corpus of tests/test_seektab_cpu.py (tables of 0 to 200 rows around the 64-row step, both entry sizes, every alignment mod
16, every malformed table, every single-byte edit of the framing, boundary_ranges), and tables of 1, chunk - 1, chunk, chunk + 1, 2 chunk - 1,
2 chunk + 1 and 3 chunk + 5 rows for both chunk sizes — 128, and the product's — with runs of zero-size rows at the start, at the end and
across a chunk edge, and ranges that saturate. Everything runs with both chunk sizes, and once more in a stand-alone AddressSanitizer program
(its own main, no Python in the process) in which every entry and the scratch lie in heap blocks of exactly their size."""
import ctypes as C
import os
import random
import struct
from types import SimpleNamespace as NS

import pytest

import lanesuite
import seekmany
import seektabs
import zgpu
from seektabs import U64, model
from test_seektab_cpu import cases as seektab_cases

SMALL = 128


def product_chunk():
    text = open(os.path.join(lanesuite.CSRC, "zg_seekmany.h")).read()
    return int(text.split("constexpr uint32_t kChunkRows = ")[1].split(";")[0])


def edge_ranges(ds, chunk):
    """boundary ranges at the rows around every chunk edge and step edge near it, at the zero-size runs, and ranges that saturate"""
    D = seekmany.prefixes(ds, ds)[1]
    nf, total = len(ds), D[-1]
    rows = {0, 1, nf - 1, nf - 2}
    for q in range(0, nf // chunk + 2):
        for dk in (-65, -64, -2, -1, 0, 1, 63, 64):
            rows.add(q * chunk + dk)
    out = []
    for k in sorted(r for r in rows if 0 <= r < nf):
        at = D[k]
        out += [(at, 1), (at + 1, 1), (at, D[k + 1] - at + 1)] + ([(at - 1, 2)] if at else [])
    a, b = D[min(nf - 1, chunk - 3)], D[min(nf, 2 * chunk + 2)]
    out += [(0, total), (0, U64), (total // 2, U64), (U64, 7), (U64 - 3, U64), (1, U64 - 1), (total, 1), (total + 5, 3), (5, 0), (total, 0),
            (total - 1, 1), (total - 1, 9), (a, b - a), (a + 1, max(b - a - 2, 1))]
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


def big_cases():
    """(name, entry, ranges, sizes): tables around both chunk sizes"""
    rng = random.Random(0x5EE3A27)
    out = []
    for chunk in (SMALL, product_chunk()):
        for nf in (1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk + 1, 3 * chunk + 5):
            for zeros in ("none", "start", "end", "edge"):
                if zeros != "none" and nf < chunk + 1:
                    continue
                cs = [rng.randint(0, 9) for _ in range(nf)]
                ds = [rng.randint(1, 3000) for _ in range(nf)]
                run = {"none": range(0), "start": range(0, 5), "end": range(nf - 5, nf), "edge": range(chunk - 3, chunk + 3)}[zeros]
                for k in run:
                    if k < nf:
                        ds[k] = 0
                checksums = rng.random() < 0.5
                front = bytes(sum(cs) + rng.randint(0, 15))
                e = front + zgpu.seek_table_frame(cs, ds, [rng.getrandbits(32) for _ in range(nf)] if checksums else None)
                out.append(("rows%d:chunk%d:zeros_%s" % (nf, chunk, zeros), e, edge_ranges(ds, chunk), (cs, ds)))
    return out


def _declare(L):
    vp = C.c_void_p
    L.zgemu_seekmany.argtypes = [vp, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint64]
    L.zgemu_seekmany.restype = C.c_uint32
    L.zgemu_seekmany_chunk_rows.restype = C.c_uint32
    assert L.zgemu_seekmany_chunk_rows() == product_chunk()


built = lanesuite.built_fixture("zg_emu_seekmany.cpp", "seekmany", "SEEKMANY_MAIN", declare=_declare)


@pytest.fixture(scope="module")
def expected():
    """[(name, entry, ranges, [(record, lo)], sizes or None)]: the model, computed once"""
    out = [(name, e, rg, [model(e, b, n) for b, n in rg], None) for name, e, rg in seektab_cases()]
    return out + [(name, e, rg, [model(e, b, n) for b, n in rg], sizes) for name, e, rg, sizes in big_cases()]


def run_passes(L, e, lo, rg, chunk, compare):
    """the entry at a 16-byte aligned address through the four passes; (records, counts, meta, prefix pairs)"""
    buf, at = lanesuite.aligned_copy(e)
    n = len(rg)
    nf_room = (len(e) // 8) + 2
    ranges, out = (C.c_uint64 * (2 * n))(*[x for r in rg for x in r]), (zgpu.SeekC * n)()
    counts, meta, prefix = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), (C.c_uint64 * (2 * nf_room))()
    differ = L.zgemu_seekmany(at, len(e), lo, ranges, n, chunk, 1 if compare else 0, out, counts, meta, prefix, nf_room)
    assert differ == 0, "%d records differ from zg_k_seektab's wave" % differ
    pairs = [(prefix[2 * i], prefix[2 * i + 1]) for i in range(meta[3])]
    return [zgpu.Seek(out[i]).key() for i in range(n)], list(counts), list(meta), pairs


@pytest.mark.parametrize("which", ["small", "product"])
def test_seekmany_equals_the_model_on_every_range(built, expected, which):
    L, _, _ = built
    chunk = SMALL if which == "small" else product_chunk()
    seen_why, nothing, ranges_run, multi_chunk, zero_rows = set(), 0, 0, 0, 0
    for name, e, rg, want, sizes in expected:
        live = [w for (b, n), w in zip(rg, want) if n]
        lo = min((w[1] for w in live), default=len(e))
        # (the wave of zg_k_seektab is run beside every range of the shorter tables in the small-chunk run; the model judges every record)
        recs, counts, meta, pairs = run_passes(L, e, lo, rg, chunk, compare=which == "small" and len(e) < 8192)
        for (b, n), rec, (mrec, _) in zip(rg, recs, want):
            assert rec == mrec, (name, b, n, dict(zip(seektabs.FIELDS, rec)), dict(zip(seektabs.FIELDS, mrec)))
            seen_why.add(mrec[9])
            nothing += mrec[10] == 4
            ranges_run += 1
        assert counts[1] == 0, (name, "reads outside the table frame", counts)
        assert counts[3] == 0, (name, "accesses outside the prefix scratch", counts)
        if not live or len(e) < 17:
            assert counts[0] == 0 and counts[2] == 0, (name, "nothing to read", counts)
        if sizes is not None:
            cs, ds = sizes
            Cs, Ds = seekmany.prefixes(cs, ds)
            assert meta[0] == 0 and meta[1] == len(cs) and pairs == list(zip(Cs, Ds)), (name, meta)
            multi_chunk += len(cs) > chunk
            zero_rows += 0 in ds
        elif live and meta[0] == 0:
            # the corpus of zg_k_seektab: the sums from the table's own bytes
            nf, es = meta[1], meta[2]
            tab = len(e) - (nf * es + 17)
            rows = [struct.unpack_from("<II", e, tab + 8 + k * es) for k in range(nf)]
            assert pairs == list(zip(*seekmany.prefixes([r[0] for r in rows], [r[1] for r in rows]))), name
    assert seen_why >= {0, 16, 17, 18, 19, 20}, seen_why
    assert nothing > 50 and ranges_run > 12000 and multi_chunk >= 8 and zero_rows >= 6, (nothing, ranges_run, multi_chunk, zero_rows)


def test_seekmany_pinned_examples(built):
    L, _, _ = built
    cs, ds = [10, 20, 8, 30, 5], [100, 255, 0, 100, 0]       # the third is a skippable frame, the last an empty one
    e = bytes(73) + zgpu.seek_table_frame(cs, ds)
    want = {
        (0, 1): (0, 10, 0, 100, 100, 0, 0, 1, 0, 0, 0),
        (99, 2): (0, 30, 0, 355, 355, 0, 0, 2, 0, 0, 0),
        (100, 1): (10, 30, 100, 255, 355, 0, 1, 1, 0, 0, 0),
        (355, 1): (38, 68, 355, 100, 455, 0, 3, 1, 0, 0, 0),     # the zero-size row in front is skipped: the SMALLEST k with D[k + 1] > 355
        (354, 2): (10, 68, 100, 355, 455, 0, 1, 3, 0, 0, 0),     # ... and taken inside a selection
        (0, U64): (0, 73, 0, 455, 455, 0, 0, 5, 0, 0, 0),        # no row reaches the end: last = nframes - 1
        (455, 1): (73, 73, 455, 0, 455, 0, 5, 0, 0, 0, 4),
        (5, 0): (0,) * 11,
    }
    for chunk in (SMALL, product_chunk()):
        recs, counts, meta, pairs = run_passes(L, e, 73, list(want), chunk, True)
        assert recs == list(want.values()) and counts[1] == 0 and counts[3] == 0
        assert pairs == [(0, 0), (10, 100), (30, 355), (38, 355), (68, 455), (73, 455)] and meta == [0, 5, 8, 6]
    # an empty table: one chunk without rows stores C[0] = D[0] = 0
    recs, counts, meta, pairs = run_passes(L, zgpu.seek_table_frame([], []), 0, [(0, 1)], SMALL, True)
    assert recs == [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4)] and pairs == [(0, 0)] and counts[1] == 0 and counts[3] == 0


def test_seekmany_under_address_sanitizer_stand_alone(built, expected):
    _, exe, d = built
    src, dst = d / "cases.bin", d / "records.bin"
    with open(src, "wb") as f:
        for _, e, rg, _, _ in expected:
            f.write(struct.pack("<QQ", len(e), len(rg)) + b"".join(struct.pack("<QQ", *r) for r in rg) + e)
    lanesuite.run_stand_alone(exe, [src, dst], b"seekmany_asan ok", timeout=1800)
    recs = open(dst, "rb").read()
    at = 0
    for _round in range(2):   # chunks of 128 rows, then the product's
        for name, e, rg, want, _ in expected:
            for r, (mrec, _) in zip(rg, want):
                got = zgpu.Seek(zgpu.SeekC.from_buffer_copy(recs, at)).key()
                assert got == mrec, (name, r, got, mrec)
                at += 64
    assert at == len(recs)


def test_seekmany_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = m = 1
    srcs, lens, dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * m)(), (C.c_size_t * m)()
    rg, sk, res = (zgpu.EntryRangeC * m)(), (zgpu.SeekC * m)(), (zgpu.RangeResultC * m)()
    assert C.sizeof(zgpu.EntryRangeC) == 24
    assert L.zgpu_frames_seek_table_many_device(None, srcs, lens, n, rg, m, sk) == zgpu.E_BAD_ARG          # no GPU touched
    assert L.zgpu_gather_ranges_seek_table_device_src(None, srcs, lens, n, rg, m, dsts, caps, None, res) == zgpu.E_BAD_ARG
    fake = C.create_string_buffer(4096)   # null arrays with n, m > 0: refused before the context is looked at (this one is not a context)
    for k in range(4):
        a = [srcs, lens, rg, sk]
        a[k] = None
        assert L.zgpu_frames_seek_table_many_device(fake, a[0], a[1], n, a[2], m, a[3]) == zgpu.E_BAD_ARG, k
    for k in range(6):
        a = [srcs, lens, rg, dsts, caps, res]
        a[k] = None
        assert L.zgpu_gather_ranges_seek_table_device_src(fake, a[0], a[1], n, a[2], m, a[3], a[4], None, a[5]) == zgpu.E_BAD_ARG, k
    # hash nothing with verify everything, or with the table's checksums enforced: refused in front of the first HIP call, as on the sibling
    for flags in (3, 5, 7):
        opts = zgpu.DeviceOptsC(0, flags, 0)
        assert L.zgpu_gather_ranges_seek_table_device_src(fake, srcs, lens, n, rg, m, dsts, caps, C.byref(opts), res) == zgpu.E_BAD_ARG
        assert L.zgpu_decode_ranges_seek_table_device_src(fake, srcs, lens, n, (zgpu.RangeC * n)(), dsts, caps, C.byref(opts), res) == zgpu.E_BAD_ARG
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in ("zgpu_frames_seek_table_many_device", "zgpu_gather_ranges_seek_table_device_src"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for meth in ("frames_seek_table_many_device", "gather_ranges_seek_table_device_src", "gather_tensor_ranges", "gather_ranges_stats"):
        assert hasattr(zgpu.Context, meth)
    # the appended statistics: a caller that asks for 13 gets 13, a null context nothing
    out = (C.c_uint64 * 24)(*([7] * 24))
    assert L.zgpu_debug_ranges_stats(None, out, 19) == 0 and list(out) == [7] * 24
    assert len(zgpu._STATS["Context.ranges_stats"][2]) + len(zgpu.Context.GATHER_STATS) == 19
    packed = zgpu.Context._entry_ranges([(2, 5, 7), (1, 2 ** 64 - 1, 0, 9)])
    assert [(r.entry, r.begin, r.len, r.pad) for r in packed] == [(2, 5, 7, 0), (1, 2 ** 64 - 1, 0, 9)]


S = lambda skipped, taken, status=0: NS(status=status, frames_skipped=skipped, frames_taken=taken)   # noqa: E731


def hand_written_groups():
    """[(ranges, seeks, (groups, group_of))]: what the contract's text says of each case"""
    out = []
    # rows: a [0, 2], b [2, 3] share row 2; c [4, 4] touches neither; d [3, 4] joins b and c to them: one group, transitively
    ranges = [(0, 0, 10), (0, 20, 10), (0, 40, 1)]
    seeks = [S(0, 3), S(2, 2), S(4, 1)]
    out.append((ranges, seeks, ([(0, 0, 3, [0, 1]), (0, 4, 4, [2])], [0, 0, 1])))
    out.append((ranges + [(0, 35, 6)], seeks + [S(3, 2)], ([(0, 0, 4, [0, 1, 2, 3])], [0, 0, 0, 0])))
    # order does not matter; entries never share a group; adjacent rows that share none stay apart
    ranges = [(1, 0, 5), (0, 7, 5), (0, 0, 5), (1, 9, 5)]
    seeks = [S(0, 1), S(1, 1), S(0, 1), S(0, 2)]
    out.append((ranges, seeks, ([(0, 0, 0, [2]), (0, 1, 1, [1]), (1, 0, 1, [0, 3])], [2, 1, 0, 2])))
    # no group: a length of 0, a failed record, nothing taken
    ranges = [(0, 0, 0), (0, 0, 5), (0, 99, 5), (0, 1, 1)]
    seeks = [S(0, 0), S(0, 0, zgpu.E_SEEK_TABLE), S(7, 0), S(0, 1)]
    out.append((ranges, seeks, ([(0, 0, 0, [3])], [None, None, None, 0])))
    # a range inside another one's interval
    out.append(([(0, 0, 99), (0, 50, 1)], [S(0, 9), S(4, 1)], ([(0, 0, 8, [0, 1])], [0, 0])))
    return out


def test_group_model_on_hand_written_cases():
    for ranges, seeks, want in hand_written_groups():
        assert seekmany.groups(ranges, seeks) == want


def c_groups(L, ranges, seeks, tables):
    """zgm::group_ranges (zg_seekmany.h, through tests/emu/zg_emu_seekmany.cpp) on ranges[j] = (entry, begin, len) and their records, and the
    demands that need no model: tables[entry] = (C, D), the prefix sums a record's byte and plaintext offsets are taken from — a group spans
    [C[gfirst], C[glast + 1]) and [D[gfirst], D[glast + 1]), every range that takes rows is one clip of its group's span, in the order of the
    sort, and the clip begins begin - D[gfirst] bytes into the group's plaintext. A range that takes no rows is handed offsets that would show
    in a group if it were looked at. Returns (groups, group_of) in the form of seekmany.groups."""
    m = len(ranges)
    flat, takes = [], []
    for r, s in zip(ranges, seeks):
        takes.append(bool(r[2]) and s.status == 0 and s.frames_taken > 0)
        C_, D_ = tables[r[0]]
        a, b = s.frames_skipped, s.frames_skipped + s.frames_taken
        ref = s.status == zgpu.E_BAD_ARG                      # (a refused range: told apart by its flag alone, as in front of accept_records)
        flat += [r[0], r[1], r[2], int(ref), 0 if ref else s.status, a, b - a] + ([C_[a], C_[b], D_[a], D_[b]] if takes[-1] else [1 << 62, 5, 1 << 61, 3])
    u32, u64 = C.c_uint32 * max(m, 1), C.c_uint64 * max(m, 1)
    grp, group_of, clip_of, order, first, skip, counts = (C.c_uint64 * (7 * max(m, 1)))(), u32(), u32(), u32(), (C.c_uint32 * (m + 1))(), u64(), (C.c_uint64 * 1)()
    G = L.zgemu_group_ranges((C.c_uint64 * max(len(flat), 1))(*flat), m, grp, group_of, clip_of, order, first, skip, counts)
    nclips = counts[0]
    assert nclips == sum(takes) and sorted(order[:nclips]) == [j for j in range(m) if takes[j]]
    assert first[0] == 0 and first[G] == nclips and all(first[g] < first[g + 1] for g in range(G))
    members = [[] for _ in range(G)]
    for j in range(m):
        if not takes[j]:
            continue
        g, q = group_of[j], clip_of[j]
        entry, gfirst, glast, c_lo, c_hi, d_lo, d_hi = grp[7 * g:7 * g + 7]
        C_, D_ = tables[entry]
        assert entry == ranges[j][0] and first[g] <= q < first[g + 1] and order[q] == j, (j, g, q)
        assert (c_lo, c_hi, d_lo, d_hi) == (C_[gfirst], C_[glast + 1], D_[gfirst], D_[glast + 1]), (j, g)
        assert gfirst <= seeks[j].frames_skipped and seeks[j].frames_skipped + seeks[j].frames_taken - 1 <= glast
        assert skip[q] == (ranges[j][1] - D_[gfirst]) % 2 ** 64, (j, skip[q])
        members[g].append(j)
    return [tuple(grp[7 * g:7 * g + 3]) + (members[g],) for g in range(G)], [group_of[j] if takes[j] else None for j in range(m)]


def random_ranges(rng, tables, m):
    """m ranges over the tables' entries with their records: short spans, spans that touch the one in front at one row, nested ones, duplicates,
    lengths of 0, failed records, refused ranges and records that take nothing"""
    ranges, seeks = [], []
    for _ in range(m):
        e = rng.randrange(len(tables))
        D_ = tables[e][1]
        nrows = len(D_) - 1
        kind = rng.choice(["span", "span", "span", "touch", "nested", "same", "empty", "failed", "refused", "nothing"])
        prev = [(r, s) for r, s in zip(ranges, seeks) if r[0] == e and r[2] and s.status == 0 and s.frames_taken]
        if kind in ("touch", "nested", "same") and not prev:
            kind = "span"
        if kind == "span":
            a = rng.randrange(nrows)
            b = min(nrows - 1, a + rng.choice([0, 0, 0, 1, 2, 5]))
        elif kind == "touch":       # begins at the last row of a range in front of it
            r, s = rng.choice(prev)
            a = s.frames_skipped + s.frames_taken - 1
            b = min(nrows - 1, a + rng.choice([0, 1, 3]))
        elif kind == "nested":
            r, s = rng.choice(prev)
            a = rng.randrange(s.frames_skipped, s.frames_skipped + s.frames_taken)
            b = rng.randrange(a, s.frames_skipped + s.frames_taken)
        if kind == "same":
            r, s = rng.choice(prev)
            ranges.append(r)
            seeks.append(s)
        elif kind == "empty":
            ranges.append((e, rng.randrange(D_[-1] + 9), 0))
            seeks.append(S(0, 0))
        elif kind in ("failed", "refused"):
            ranges.append((e, rng.randrange(D_[-1] + 9), rng.randint(1, 99)))
            seeks.append(S(rng.randrange(nrows), rng.randint(0, 3), zgpu.E_SEEK_TABLE if kind == "failed" else zgpu.E_BAD_ARG))
        elif kind == "nothing":
            ranges.append((e, D_[-1] + rng.randrange(9), rng.randint(1, 99)))
            seeks.append(S(nrows, 0))
        else:
            ranges.append((e, rng.randint(D_[a], D_[a + 1]), rng.randint(1, 2 * (D_[b + 1] - D_[a]) + 1)))
            seeks.append(S(a, b - a + 1))
    return ranges, seeks


def test_the_grouping_of_the_gather_calls_equals_the_model(built):
    """zgm::group_ranges is the code zg_ranges.cpp's gather_groups calls; the emulator build compiles zg_seekmany.h alone, so nothing here
    depends on zg_frames.cpp, zg_ranges.cpp or a GPU."""
    L, _, _ = built
    vp = C.c_void_p
    L.zgemu_group_ranges.argtypes = [vp, C.c_uint32] + [vp] * 7
    L.zgemu_group_ranges.restype = C.c_uint32
    flat = seekmany.prefixes([7] * 64, [100] * 64)           # the hand-written cases name rows, not bytes: any table serves
    for ranges, seeks, want in hand_written_groups():
        assert c_groups(L, ranges, seeks, [flat, flat]) == want == seekmany.groups(ranges, seeks)
    assert c_groups(L, [], [], [flat]) == ([], [])
    rng = random.Random(0x6E0095)
    tables = [seekmany.prefixes([rng.randint(0, 9) for _ in range(nrows)], [rng.choice([0, 1, 50, 3000]) for _ in range(nrows)]) for nrows in (40, 17, 1)]
    total, ngroups, shared = 0, 0, 0
    for m in (6, 20, 60, 120, 250):                          # sparse calls, where most ranges are alone, to dense ones
        ranges, seeks = random_ranges(rng, tables, m)
        got = c_groups(L, ranges, seeks, tables)
        assert got == seekmany.groups(ranges, seeks), m
        total += m
        ngroups += len(got[0])
        shared += sum(len(g[3]) > 1 for g in got[0])
    assert total > 400 and ngroups >= 30 and shared >= 15, (total, ngroups, shared)   # (the draw itself: groups of one range and of many)


def test_verdict_model_keeps_the_rank_order():
    v, small = seekmany.verdict, zgpu.E_TARGET_TOO_SMALL
    assert v() == 0
    assert v(decode=zgpu.E_CONTENT_SIZE_MISMATCH, small=True, checksum=zgpu.E_CHECKSUM_MISMATCH, table=zgpu.E_SEEK_CHECKSUM_MISMATCH) == zgpu.E_CONTENT_SIZE_MISMATCH
    assert v(small=True, checksum=zgpu.E_CHECKSUM_MISMATCH, table=zgpu.E_SEEK_CHECKSUM_MISMATCH) == small
    assert v(checksum=zgpu.E_CHECKSUM_MISMATCH, table=zgpu.E_SEEK_CHECKSUM_MISMATCH) == zgpu.E_CHECKSUM_MISMATCH
    assert v(table=zgpu.E_SEEK_CHECKSUM_MISMATCH) == zgpu.E_SEEK_CHECKSUM_MISMATCH
    assert v(small=True) == small
    assert seekmany.clipped(5, 10, 0, 8) == 3 and seekmany.clipped(5, 10, 7, 100) == 8 and seekmany.clipped(50, 10, 0, 8) == 0
    assert seekmany.prefixes([1, 2], [3, 0]) == ([0, 1, 3], [0, 3, 3])
    grps = [(0, 0, 1, [0]), (0, 3, 3, [1])]
    assert seekmany.work(grps, [True, False, True, True], [10, 0, 7, 5]) == (2, 15)
