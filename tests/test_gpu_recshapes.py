"""The record index on the GPU at its scan, lane and launch edges (zg_k_recs_count / _scan / _emit / _find, zg_records.h; records_submit in
zg_frames.cpp, records_entries / relay_records in zg_ranges.cpp), through the public calls as test_gpu_seek_index_records makes them. The shapes
are tests/recshapes.py's — the same ones tests/test_recshapes_cpu.py runs on the emulator: scans with 2, 3 and 5 chunks per thread, more than 256
and 512 frames in a submit, lanes that hold 8 and 16 delimiters at output alignments 0, 5 and 15, a run that finds nothing between runs that
do, an entry without a delimiter and one of nothing else, a pass over side buffers that still hold a larger pass's counts and prefixes, and
the find kernel in 1, 2 and 16 workgroups with a partial last one. No expectation comes from the calls under test: the plaintext is the
oracle's (test_gpu_seek_index_measured.Shard holds every frame against the oracle), an entry's offsets are tests/records.py's, delivered
bytes are slices of that plaintext, and a gather by number is held, field for field, against the gather by bytes on the model's ranges.
Everything is compared for equality. The change of records_stats() over a pass must be the shape's own submits and chunks: a shape that
the run planner cut otherwise would quietly scan at one chunk per thread. Destinations have guard bytes and odd alignments (devmem.Arena)."""
import functools
import os
import sys
import time

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import recshapes
import zgpu
from devmem import Arena, Sources, full_key
from test_gpu_seek_index_measured import Shard

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))   # zgdata: zstd_compress
pytestmark = pytest.mark.gpu
NAMES = [s.name for s in recshapes.shapes()]


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


@functools.lru_cache(None)
def _shards(name, declared):
    """one Shard per entry of the shape: every frame held against the oracle"""
    s = recshapes.lane_entries() if name == "lanes" else recshapes.by_name(name)
    shards = [Shard(s.frames(e, content_size=declared)) for e in range(len(s.entries))]
    assert [sh.plain for sh in shards] == [s.plain(e) for e in range(len(s.entries))]
    return s, shards


def _index(ctx, src, shards, kind):
    ix = ctx.seek_index_measured(src.ptrs, src.lens) if kind == "measured" else ctx.seek_index(src.ptrs, src.lens, kind="declared")
    want = zgpu.INDEX_MEASURED if kind == "measured" else zgpu.INDEX_DECLARED
    assert [(i.status, i.kind, i.plaintext) for i in ix.infos] == [(0, want, len(sh.plain)) for sh in shards], ix.infos
    return ix


def _pass_equals_the_model(ctx, name, kind="declared"):
    """index the shape, run the pass, hold offsets, infos and the stats' change against the model; the seconds the pass took"""
    s, shards = _shards(name, kind != "measured")
    src = Sources([sh.z for sh in shards], [(3 * e + 1) % 7 for e in range(len(shards))])
    with _index(ctx, src, shards, kind) as ix:
        before = ix.records_stats()
        t0 = time.perf_counter()
        infos = ix.records(src.ptrs, src.lens, delimiter=s.d, run_bytes=s.run_bytes)
        took = time.perf_counter() - t0
        after = ix.records_stats()
        for e, (O, tail) in enumerate(s.offsets()):
            got = ix.record_offsets(e)
            assert got == O, (name, kind, e, len(got), len(O), [(i, a, b) for i, (a, b) in enumerate(zip(got, O)) if a != b][:4])
            assert (infos[e].status, infos[e].state, infos[e].delimiter, infos[e].flags, infos[e].nrecords) == (
                0, zgpu.RECORDS_FOUND, s.d, int(tail), len(O) - 1), (name, kind, e, infos[e])
        want = s.submits()
        delta = {k: after[k] - before[k] for k in ("records_submits", "records_chunks")}
        assert delta == {"records_submits": len(want), "records_chunks": sum(c for c, _ in want)}, (name, kind, delta, want)
        assert after["records_held"] == sum(len(O) - 1 for O, _ in s.offsets()) and after["records_offset_bytes"] == sum(8 * len(O) for O, _ in s.offsets())
    assert src.unchanged()
    print("\n%s %s: %d chunks, %d frames, pass %.3f s, side pass %d us" % (name, kind, want[0][0], want[0][1], took, after["records_us"] - before["records_us"]))
    return took


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_leaves_the_models_offsets_at_every_shape(ctx, name):
    _pass_equals_the_model(ctx, name)


@pytest.mark.parametrize("name", ["stretch-257", "frames-257"])
def test_the_pass_over_a_measured_index(ctx, name):
    _pass_equals_the_model(ctx, name, "measured")


def test_a_smaller_pass_over_a_larger_ones_side_buffers():
    """one context of its own: the counts, prefixes and totals of stretch-1025 (1025 chunks) are what silent's 33 chunks find in the side
    buffers, those of frames-513 (513 frames' totals) what a dense shape's 6 frames find; silent-b, whose total is 0, comes last: the total
    that lies in the buffer is a larger pass's"""
    c = zgpu.Context(0)
    try:
        for name in ("stretch-1025", "silent", "frames-513", "dense-a5-dff", "dense-a15-d00", "silent-b"):
            _pass_equals_the_model(c, name)
    finally:
        c.close()


@pytest.fixture(scope="module")
def lane_index(ctx):
    """the four entries lanes(m) look records up in, indexed, with their records: (index, sources, shape)"""
    s, shards = _shards("lanes", True)
    src = Sources([sh.z for sh in shards], [2, 0, 5, 1])
    with _index(ctx, src, shards, "declared") as ix:
        infos = ix.records(src.ptrs, src.lens, delimiter=s.d, run_bytes=s.run_bytes)
        assert [(i.status, i.state, i.nrecords) for i in infos] == [(0, zgpu.RECORDS_FOUND, len(O) - 1) for O, _ in s.offsets()]
        yield ix, src, s
    assert src.unchanged()


@pytest.mark.parametrize("m", recshapes.LANES)
def test_record_ranges_equal_the_model_lane_for_lane(ctx, lane_index, m):
    ix, src, s = lane_index
    lanes, want = recshapes.lanes(m)
    ranges, statuses = ctx.record_ranges(ix, lanes)
    for j, ((rng, refused), got, st) in enumerate(zip(want, ranges, statuses)):
        assert (got, st) == (rng, zgpu.E_BAD_ARG if refused else 0), (m, j, lanes[j], got, st, rng)
    fs = ctx.gather_records_stats()
    assert (fs["record_find_launches"], fs["record_find_bytes_downloaded"]) == (1, 24 * m), fs


def test_a_thousand_record_ranges_gathered_equal_the_gather_by_bytes(ctx, lane_index):
    ix, src, s = lane_index
    m = 1000
    lanes, want = recshapes.lanes(m)
    plains = [s.plain(e) for e in range(len(s.entries))]
    exp = [None if refused else plains[e][b:b + n] for (e, b, n), refused in want]
    caps = [8 if x is None else len(x) + (5 if j % 2 else 0) for j, x in enumerate(exp)]
    shifts = [j % 7 for j in range(m)]
    t0 = time.perf_counter()
    a = Arena(caps, shifts)
    res, seeks = ctx.gather_records_indexed_device_src(ix, src.ptrs, src.lens, lanes, a.ptrs, a.caps)
    fs = ctx.gather_records_stats()
    assert (fs["record_find_launches"], fs["record_find_bytes_downloaded"]) == (1, 24 * m), fs
    assert [(r.status, r.written) for r in res] == [(zgpu.E_BAD_ARG, 0) if x is None else (0, len(x)) for x in exp]
    a.check(exp)
    ends = [(ln, x, want[j][0][1] + len(x)) for j, (ln, x) in enumerate(zip(lanes, exp)) if x and len(ln) > 3]
    stripped = [1 for ln, x, end in ends if x[-1] != s.d and plains[ln[0]][end:end + 1] == bytes([s.d])]
    assert len(stripped) > 50                                                   # a delimiter was stripped: the byte behind what was delivered
    # the gather by bytes on the model's ranges: the same results, field for field (a refused lane has no range to give)
    good = [j for j, x in enumerate(exp) if x is not None]
    b = Arena([caps[j] for j in good], [shifts[j] for j in good])
    res0, seeks0 = ctx.gather_ranges_indexed_device_src(ix, src.ptrs, src.lens, [want[j][0] for j in good], b.ptrs, b.caps)
    assert [full_key(res[j]) for j in good] == [full_key(r) for r in res0]
    assert [seeks[j].key() for j in good] == [k.key() for k in seeks0]
    b.check([exp[j] for j in good])
    print("\nlanes(1000): %d bytes by number and by bytes in %.3f s" % (sum(len(x) for x in exp if x), time.perf_counter() - t0))
