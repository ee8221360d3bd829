"""zg_k_index's lane routine (zstd-rs_amd/csrc/zg_index.h) and the host's reading of its frame records (zg_host_parse.cpp: frame_fields),
compiled with g++ and run on the CPU. For every input the lane runs twice, summary pass and emit pass, over a reader that counts every
access outside [0, len) and every access to a byte of a block body (the bodies as zgw::walk_entry's records give them), and a writer that
counts every store outside the lane's own record range (which lies between guard records). Demanded of every input:
  - bound == plaintext_bound(bytes);
  - chain_end and why are zgw::walk_entry's stop_off and why;
  - nframes, nskippable and nblocks are a count over the walk's records;
  - the frame records' bounds sum to the entry's bound, their extents tile [0, chain_end) in order, their header fields are what
    read_frame_header gives on the walk's frame records, and — on inputs parse_frames accepts — what parse_frames' FrameInfo says;
  - reads outside the entry 0, reads of a block body 0, stores outside the range 0; the emit pass says what the summary pass said.
The corpus is tests/test_walk_cpu.py's (every golden pack: decodecorpus, dictionary fixtures, fuzz artefacts, synthetic; the regress and
verdict_order frames; the seqframes families; hand-built frames; concatenations with skippable frames), every prefix of its small
inputs, and single-byte edits aimed at every frame-header and block-header byte of them. Two edges are pinned besides: an emit pass over
an input that changed since the summary pass ends in a count the host refuses and no stray store, and a frame table that is too small is
answered with the count needed. tests/emu/zg_lane_index.cpp is the harness, built by tests/lanesuite.py."""
import ctypes as C

import lanesuite
import zgpu
from test_walk_cpu import MAX_WINDOW, corpus, hand_built, skippable

SMALL = 4096   # inputs up to this long: every prefix, and every header byte edited


def _declare(L):
    u64, vp = C.c_uint64, C.c_void_p
    L.ix_check.argtypes = [vp, u64, u64]
    L.ix_check.restype = C.c_uint32
    L.ix_prefixes.argtypes = [vp, u64, u64, u64, C.POINTER(u64)]
    L.ix_prefixes.restype = C.c_uint32
    L.ix_edits.argtypes = [vp, u64, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.ix_edits.restype = C.c_uint32
    L.ix_coverage.argtypes = [C.POINTER(u64)] * 5
    L.ix_changed.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
    L.ix_changed.restype = None
    L.ix_ranges.argtypes = [C.POINTER(vp), C.POINTER(u64), C.c_uint32, C.POINTER(u64)]
    L.ix_ranges.restype = u64


lib = lanesuite.built_fixture("zg_lane_index.cpp", "index_lane", extra_sources=lanesuite.HOST_PARSE, declare=_declare)


def test_index_equals_walk_and_bound_everywhere(lib):
    where, nedits = C.c_uint64(0), C.c_uint64(0)
    total_edits = small = 0
    cases = corpus()
    assert len(cases) > 300
    packs = set(name.split(":")[0] for name, _ in cases)
    for need in ("decodecorpus.pack", "dict_tests.pack", "fuzz_artifacts.pack", "synthetic.pack", "seqframes", "hand", "concat"):
        assert need in packs, need
    for seed, (name, z) in enumerate(cases):
        buf = lanesuite.exact_buffer(z)
        assert lib.ix_check(buf, len(z), MAX_WINDOW) == 0, name
        bad = lib.ix_prefixes(buf, len(z), SMALL, MAX_WINDOW, C.byref(where))
        assert bad == 0, (name, "prefix", where.value, bad)
        every = len(z) <= SMALL
        small += every
        bad = lib.ix_edits(buf, len(z), MAX_WINDOW, 0x1DE5 + seed, 0 if every else 400, C.byref(where), C.byref(nedits))
        assert bad == 0, (name, "edit at", where.value, bad)
        assert buf.raw == z
        total_edits += nedits.value
    assert small > 100 and total_edits > 20000
    u64 = C.c_uint64
    why, fb, rf, unread, n = (u64 * 16)(), (u64 * 4)(), (u64 * 5)(), u64(0), u64(0)
    lib.ix_coverage(why, fb, rf, C.byref(unread), C.byref(n))
    assert n.value > 100000
    assert all(why[k] > 0 for k in range(9)), list(why)[:9]       # every reason a chain ends for
    assert all(x > 0 for x in fb), list(fb)                       # every entry flag seen set
    assert all(x > 0 for x in rf), list(rf)                       # every frame flag seen set
    assert unread.value > 0                                       # records of headers the chain could not read


def test_emit_pass_over_a_changed_input_is_refused_without_a_stray_store(lib):
    hb = hand_built()
    good = hb["raw_rle_blocks"]
    out = (C.c_uint64 * 6)()
    changes = [(good, good * 5),                                    # more frames than the summary pass counted
               (good * 3, good),                                    # fewer
               (good + skippable(b"abc"), skippable(b"abc") * 9),   # other kinds
               (good * 2, good + hb["bad_magic"]),                  # the same count, another end
               (b"", good * 2)]
    for then, now in changes:
        a, b = lanesuite.exact_buffer(then), lanesuite.exact_buffer(now)
        lib.ix_changed(a, len(then), b, len(now), out)
        assert out[0] == 0 and out[1] == 0, (then, now, list(out))
        assert out[2] <= out[3], list(out)
        assert out[4] == 0, list(out)                               # the host refuses the pass (ZGPU_E_INTERNAL)
    same = lanesuite.exact_buffer(good * 3)
    lib.ix_changed(same, len(good) * 3, same, len(good) * 3, out)
    assert list(out) == [0, 0, 3, 3, 1, 3]


def test_a_table_that_is_too_small_is_answered_with_the_count_needed(lib):
    hb = hand_built()
    ents = [hb["frame_skip_frame"], b"", hb["raw_rle_blocks"] * 7, hb["skip_only"], hb["frames_then_garbage"], hb["empty"]]
    want = [4, 0, 7, 2, 3, 0]          # (frames_then_garbage: two frames and the header that cannot be read)
    n = len(ents)
    bufs = [lanesuite.exact_buffer(e) for e in ents]
    ptrs = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * n)(*[len(e) for e in ents])
    first = (C.c_uint64 * (n + 1))()
    need = lib.ix_ranges(ptrs, lens, n, first)
    assert need == sum(want) and list(first) == [sum(want[:i]) for i in range(n + 1)]


def test_index_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = 1
    srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    ents = (zgpu.EntryIndexC * n)()
    first = (C.c_uint64 * (n + 1))()
    frames = (zgpu.FrameIndexC * 4)()
    need = C.c_size_t(0)
    assert C.sizeof(zgpu.EntryIndexC) == 40 and C.sizeof(zgpu.FrameIndexC) == 64
    assert L.zgpu_frames_index_device(None, srcs, lens, n, ents) == 93          # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_frames_table_device(None, srcs, lens, n, ents, first, frames, 4, C.byref(need)) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(3):
        a = [srcs, lens, ents]
        a[k] = None
        assert L.zgpu_frames_index_device(fake, a[0], a[1], n, a[2]) == 93, k
        assert L.zgpu_frames_table_device(fake, a[0], a[1], n, a[2], first, frames, 4, C.byref(need)) == 93, k
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, None, frames, 4, C.byref(need)) == 93
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, first, None, 4, C.byref(need)) == 93
    assert L.zgpu_frames_table_device(fake, srcs, lens, n, ents, first, frames, 4, None) == 93
    out = (C.c_uint64 * 4)()
    assert L.zgpu_debug_frames_index_stats(None, out, 4) == 0
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        for sym in ("zgpu_frames_index_device", "zgpu_frames_table_device", "zgpu_debug_frames_index_stats"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for m in ("frames_index_device", "frames_table_device", "frames_index_stats", "split_tensor_frames", "decode_tensors"):
        assert hasattr(zgpu.Context, m)
    # the stop reasons are public under the lanes' values
    assert [zgpu.CHAIN_END, zgpu.CHAIN_SHORT_HEADER, zgpu.CHAIN_BAD_MAGIC, zgpu.CHAIN_SKIP_PAST_END, zgpu.CHAIN_SHORT_BLOCK_HEADER,
            zgpu.CHAIN_RESERVED_BLOCK, zgpu.CHAIN_BLOCK_TOO_LARGE, zgpu.CHAIN_BODY_PAST_END, zgpu.CHAIN_SHORT_CHECKSUM] == list(range(9))
