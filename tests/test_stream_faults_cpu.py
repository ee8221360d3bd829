"""Engine errors under the io::Read surface (zstd-rs_amd/csrc/zg_stream.h), on the CPU: the table-driven stand-in for the engine
(tests/emu/zg_emu_stream.cpp) makes the nth call of one kind — prepare, launch, wait, run, commit, fetch, fetch_wait, rebase, pipe_begin,
host_alloc — return an engine error without doing its work, in every mode (block by block, runs on the caller's thread, worker thread +
ring), for slice and callback sources, with and without the hasher, for the styles of read sizes and for one read larger than the ring.
Every frame meets every mode and every source; read style and hasher on / off are a SAMPLE on top of that: they go round over the twelve
frame-by-source configurations of a mode (each style with each hasher setting at least once per mode), they are not crossed with them.

The rule (include/zgpu.h at zgpu_streaming_read): the first engine error ends the stream. Reads in front of it return
what the reference's would; the read that meets it returns it with 0 bytes, and so does every later read, without another call to the
engine or the source; every byte handed out is the frame's plaintext at its position; the calculated checksum is the XXH64 of exactly the
bytes handed out; is_finished stays false; when the failing read returns, the threads are joined, the engine has had its pipe_end and
every host allocation its host_free; freeing the stream does not hang. pipe_begin failing and host_alloc returning null are no errors: the
stream stays on the caller's thread and the caller sees nothing.

Which ordinals: each configuration runs once clean and records the calls per kind; the fault then goes to calls 1, 2, 3, the middle one,
the last but one and the last (all of them when there are six or fewer), with the codes 90, 91, 92 in turn. A fault whose ordinal is not
reached in the injected run (the worker's schedule depends on timing) must leave a run that equals the model completely; at most one case
in ten of a test may end like that."""
import ctypes as C
import os
import random
import subprocess
import threading

import pytest
import xxhash

from test_stream_cpu import Frame, K, lib, model, read_pattern, run_stream

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ["prepare", "launch", "wait", "run", "commit", "fetch", "fetch_wait", "rebase", "pipe_begin", "host_alloc"]
SILENT = ("pipe_begin", "host_alloc")
CODES = (90, 91, 92)
AFTER = [8192, 1, 0, K + 1, 3 << 20, 100, 65536, 8192]       # what a caller that does not give up asks for behind the error
FREE_LIMIT_S = 10
_READY = False
_BUF = [None, 0]                                             # one read buffer for all cases (the largest read so far)
_BYTES = {}                                                  # id(frame) -> (frame, its source, its plaintext, out[], status[]) as the stand-in takes them


def frame_args(fr):
    a = _BYTES.get(id(fr))
    if a is None or a[0] is not fr:
        a = _BYTES[id(fr)] = (fr, bytes(fr.src[:fr.src_len]), bytes(fr.plain), (C.c_uint32 * fr.nblocks)(*fr.out), (C.c_uint32 * fr.nblocks)(*fr.status))
    return a


def bounded_free(L, h):
    """the free runs on the calling (test's) thread; a watchdog thread notes when it is still running after FREE_LIMIT_S, and the test fails
    for it once the free has returned"""
    done, late = threading.Event(), []
    w = threading.Thread(target=lambda: done.wait(FREE_LIMIT_S) or late.append(1), daemon=True)
    w.start()
    L.zgemu_stream_free(h)
    done.set()
    w.join()
    assert not late, "freeing the stream took more than %d s" % FREE_LIMIT_S


def flib():
    global _READY
    L = lib()
    if not _READY:
        L.zgemu_stream_fail.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_int]
        L.zgemu_stream_stats2.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.zgemu_stream_live_allocs.restype = C.c_int64
        _READY = True
    return L


def drive(fr, reads, fault=None, read_ahead=0, pipe_after=0, first_run=0, copy_threads=2, hash_on=True, max_run_src=0, callback=False, chunk=0,
          content_size=0):
    """run_stream of test_stream_cpu with a fault set before the first read, AFTER more reads behind the first error, both stats calls, and
    a free that a watchdog bounds. -> (results per read, delivered bytes, checksum, stats, stats2)"""
    L = flib()
    _, src, plain, out, st = frame_args(fr)
    h = L.zgemu_stream_new(src, fr.src_len, plain, len(plain), out, st, bytes(fr.far), fr.nblocks, fr.window,
                           1 if fr.has_checksum else 0, fr.checksum, content_size, read_ahead, pipe_after, first_run, copy_threads,
                           1 if hash_on else 0, max_run_src, 1 if callback else 0, chunk)
    assert h
    if fault:
        L.zgemu_stream_fail(h, KINDS.index(fault[0]), fault[1], fault[2])
    res, handed = [], bytearray()
    need = max(max(reads), max(AFTER), 1)
    if _BUF[1] < need:
        _BUF[0], _BUF[1] = C.create_string_buffer(need), need
    big = _BUF[0]
    n = C.c_size_t()
    s1, s2, s_err = (C.c_uint64 * 16)(), (C.c_uint64 * 20)(), None
    try:
        todo = list(reads)
        i = 0
        while i < len(todo):
            cap = todo[i]
            i += 1
            n.value = 12345
            e = L.zgemu_stream_read(h, big, cap, C.byref(n))
            if e:
                res.append(("err", e, n.value))
                if s_err is None:
                    todo = todo[:i] + AFTER                  # the first error: a caller that goes on reading
                    s_err = (C.c_uint64 * 16)()
                    L.zgemu_stream_stats(h, s_err)           # (where the source stood when the caller learned of it)
            else:
                data = C.string_at(big, n.value)
                res.append((n.value, data))
                handed += data
        cs = L.zgemu_stream_checksum(h)
        L.zgemu_stream_stats(h, s1)
        L.zgemu_stream_stats2(h, s2)
    finally:
        bounded_free(L, h)
    assert L.zgemu_stream_live_allocs() == 0                 # every host_alloc has had its host_free
    keys = ["mode", "runs", "dropped", "be_runs", "commits", "discards", "rebases", "src_taken", "objections", "finished", "blocks", "bytes_read",
            "has_cs", "cs", "pipe_begins", "callbacks"]
    stats = dict(zip(keys, [int(x) for x in s1]))
    v = [int(x) for x in s2]
    stats2 = dict(calls=dict(zip(KINDS, v[:10])), fired=v[10], calls_after=v[11], cb_after=v[12], live=v[13], error=v[14], pipe_owed=v[15],
                  cb_after_fault=v[16], src_at_error=None if s_err is None else (int(s_err[7]), int(s_err[15])))
    return res, bytes(handed), cs, stats, stats2


def check_case(fr, reads, want, fault, kw):
    """one injected run against the rule. -> its stats, with "fired"; mode 1: the stream was with the worker thread when it ended"""
    kind, nth, code = fault
    got, handed, cs, stats, s2 = drive(fr, reads, fault=fault, **kw)
    ctx = (fault, kw, stats, s2)
    assert stats["objections"] == 0, ctx                                       # bad_src == 0
    assert frame_args(fr)[2].startswith(handed), ctx                              # everything delivered is a prefix of the plaintext
    errs = [i for i, g in enumerate(got) if g[0] == "err"]
    first = errs[0] if errs else len(got)
    for i in range(min(first, len(want))):                                      # reads in front of the first error: the model's, sizes and bytes
        assert got[i][0] == want[i][0] and got[i][1] == want[i][1], (i, reads[i], got[i][0], want[i][0], ctx)
    want_cs = xxhash.xxh64(handed if kw.get("hash_on", True) else b"").intdigest() & 0xFFFFFFFF
    assert cs == want_cs, ctx                                                   # the hash of exactly the bytes that reads returned
    assert s2["live"] == 0 or not errs, ctx
    if not s2["fired"] or kind in SILENT:
        # not reached, or one of the two failures that are no errors: the caller sees a clean stream
        assert not errs and len(got) == len(want), ctx
        assert [g[:2] for g in got] == want, ctx
        assert s2["error"] == 0 and stats["finished"] == 1, ctx
        if kind in SILENT and s2["fired"]:
            assert stats["mode"] != 1 and stats["pipe_begins"] == 0, ctx       # the stream never went to the worker thread
        return dict(stats, fired=bool(s2["fired"]))
    assert errs, ctx                                                            # the reads cover the whole frame: one of them must meet it
    assert first < len(reads), ctx
    assert len(got) == first + 1 + len(AFTER), ctx
    for g in got[first:]:
        assert g == ("err", code, 0), (g, ctx)                                  # the injected code, 0 bytes, for ever
    assert s2["error"] == code, ctx
    assert s2["calls_after"] == 0 and s2["cb_after"] == 0, ctx                  # the engine and the source are left alone
    assert s2["src_at_error"] == (stats["src_taken"], stats["callbacks"]), ctx  # (slices too: the source stands where it stood when the error was returned)
    if stats["mode"] != 1:
        assert s2["cb_after_fault"] == 0, ctx                                   # on the caller's thread nothing is taken from the source once the engine has failed (the worker meets
                                                                                # its faults while the reader may be taking a run: there what counts is what follows the failing read)
    assert stats["finished"] == 0, ctx
    assert s2["live"] == 0 and s2["pipe_owed"] == 0, ctx                        # the pipe is down when the failing read returns
    return dict(stats, fired=True)


def ordinals(c):
    if c <= 6:
        return list(range(1, c + 1))
    return sorted({1, 2, 3, (c + 1) // 2, c - 1, c})


class Sweep:
    """the faults of one test: codes in turn per kind, and the share of cases whose fault was not reached"""

    def __init__(self):
        self.turn = {k: 0 for k in KINDS}
        self.codes = {k: set() for k in KINDS}
        self.cases = self.unfired = 0

    def run(self, fr, reads, kw, kinds=KINDS):
        want, _ = model(fr, reads)
        # clean, through the existing driver and through this file's: the model's reads, and the calls per kind
        got0, handed0, cs0, st0 = run_stream(fr, reads, **kw)
        assert got0 == want and st0["objections"] == 0
        got, handed, cs, stats, s2 = drive(fr, reads, **kw)
        assert [g[:2] for g in got] == want and handed == handed0 == frame_args(fr)[2] and cs == cs0 and not s2["fired"] and s2["error"] == 0
        for kind in kinds:
            for nth in ordinals(s2["calls"][kind]):
                code = CODES[self.turn[kind] % 3]
                self.turn[kind] += 1
                self.codes[kind].add(code)
                self.cases += 1
                if not check_case(fr, reads, want, (kind, nth, code), kw)["fired"]:
                    self.unfired += 1
        return s2["calls"], stats

    def done(self, kinds_expected):
        for k in kinds_expected:
            assert self.codes[k] == set(CODES), (k, self.codes[k])              # each code at least once per kind
        assert self.unfired * 10 <= self.cases, (self.unfired, self.cases)
        print("fault cases %d, not reached %d" % (self.cases, self.unfired))


def frames():
    """about 200 small blocks; about 40 blocks, 128 KiB ones among tiny ones; each with and without a checksum"""
    out = []
    for cs in (True, False):
        out.append(("small", Frame(random.Random(71 + cs), 200, 1024, cs, small=True)))
        out.append(("mixed", Frame(random.Random(73 + cs), 40, K, cs)))
    return out


FRAMES = frames()
SOURCES = [dict(callback=False), dict(callback=True, chunk=0), dict(callback=True, chunk=1000)]
STYLES = ["small", "mixed", "big", 8192, "one"]


def pattern(rng, fr, style, ring):
    if style == "one":                                       # one read larger than the ring (read_pipe serves it piece by piece), then the end
        return [ring + (1 << 20) + 3, 8192, 1]
    return read_pattern(rng, len(fr.plain), style)


def sweep_mode(mode_kw, ring, expect_mode, kinds_expected):
    sw = Sweep()
    rng = random.Random(5)
    k = 0
    for name, fr in FRAMES:
        assert len(fr.plain) <= (6 << 20)
        for src in SOURCES:
            # the five read styles and hasher on / off go round over the twelve configurations: every pair of them occurs
            style = STYLES[k % 5]
            kw = dict(hash_on=(k // 5) % 2 == 0, **src)
            k += 1
            kw.update(mode_kw(name, fr))
            if expect_mode == 1 and style in ("mixed", "big", "one"):
                kw["content_size"] = len(fr.plain)           # (a first read that large would decode the whole frame in one run on the caller's thread: the header declares the size, the worker starts at once)
            reads = pattern(rng, fr, style, ring(fr))
            calls, stats = sw.run(fr, reads, kw)
            assert stats["mode"] == expect_mode, (name, kw, stats)
    sw.done(kinds_expected)
    return sw


def test_block_by_block_every_engine_call_can_fail():
    sweep_mode(lambda name, fr: dict(read_ahead=1), lambda fr: 8 << 20, 2, ["prepare", "launch", "wait", "run", "commit", "fetch", "fetch_wait"])


def test_runs_on_the_callers_thread_every_engine_call_can_fail():
    sweep_mode(lambda name, fr: dict(pipe_after=1 << 40, first_run=1), lambda fr: 8 << 20, 0,
               ["prepare", "launch", "wait", "run", "commit", "fetch", "fetch_wait"])


def pipe_kw(name, fr):
    # first runs of 1, 4, 16 ... blocks on the caller's thread, then the worker; callback sources: a staging buffer bounds a run
    return dict(pipe_after=(20 << 10) if name == "small" else (256 << 10), first_run=1, read_ahead=(2 << 20) + fr.window,
                max_run_src=(24 << 10) if name == "small" else (1 << 20))


def test_worker_thread_every_engine_call_can_fail():
    sw = sweep_mode(pipe_kw, lambda fr: (8 << 20) + (512 << 10), 1,
                    ["prepare", "launch", "wait", "run", "commit", "fetch", "fetch_wait", "pipe_begin", "host_alloc"])
    assert sw.cases > 300


def test_worker_thread_with_a_ring_that_wraps():
    """the ring is never smaller than 8 MiB, so the frames above do not wrap it: one frame of ~25 MiB does, three times, for a slice and a
    callback source, small reads and one read larger than the ring"""
    rng = random.Random(11)
    fr = Frame(rng, 300, K, True)
    assert (20 << 20) < len(fr.plain) < (32 << 20)
    sw = Sweep()
    kw = dict(pipe_after=256 << 10, first_run=1, read_ahead=(2 << 20) + K)
    for src, style, hash_on in ((SOURCES[0], 65536, True), (SOURCES[2], "one", True), (SOURCES[1], 1 << 20, False)):
        reads = [len(fr.plain) + 5, 8192, 1] if style == "one" else read_pattern(rng, len(fr.plain), style)
        calls, stats = sw.run(fr, reads, dict(hash_on=hash_on, max_run_src=1 << 20, content_size=len(fr.plain) if style == "one" else 0, **kw, **src), kinds=["prepare", "wait", "commit", "fetch", "fetch_wait"])
        assert stats["mode"] == 1 and calls["fetch"] > calls["commit"]          # (a run's plaintext in two pieces: the ring wrapped)
    sw.done(["prepare", "wait", "commit", "fetch", "fetch_wait"])


def test_dropped_runs_salvage_and_the_way_back_to_block_by_block_can_fail():
    """a block that sets an offset beyond the window (no error by itself: every byte arrives) makes the run it is in be dropped, its good
    prefix decoded again, the device window rebuilt (rebase) and the stream go on block by block: each of those calls can fail too"""
    sw = Sweep()
    rng = random.Random(13)
    k = 0
    for name, fr0 in FRAMES:
        fr = Frame.__new__(Frame)
        fr.__dict__.update(fr0.__dict__)
        fr.far = list(fr0.far)
        fr.far[fr.nblocks * 3 // 4] = 1
        for mode_kw in (pipe_kw(name, fr), dict(pipe_after=1 << 40, first_run=1)):
            src = SOURCES[k % 3]
            style = ["small", "mixed", "one", 8192][k % 4]
            k += 1
            kw = dict(hash_on=k % 3 != 0, **src)
            kw.update(mode_kw)
            if "read_ahead" in mode_kw and style in ("mixed", "one"):
                kw["content_size"] = len(fr.plain)
            reads = pattern(rng, fr, style, (8 << 20) + (512 << 10))
            calls, stats = sw.run(fr, reads, kw)
            assert stats["dropped"] == 1 and stats["mode"] == 2
            if "read_ahead" in mode_kw:
                assert calls["rebase"] == 1
    sw.done(["run", "commit", "fetch", "fetch_wait", "rebase"])


# ---- the four ways to wrong plaintext that reading the code showed: each is one fixed case ----------------------------------------------
def named(mode_kw, fault, style, in_pipe=False, **src):
    name, fr = FRAMES[1]                                      # the mixed frame with a checksum
    kw = dict(hash_on=True, **src)
    kw.update(mode_kw(name, fr) if callable(mode_kw) else mode_kw)
    reads = pattern(random.Random(3), fr, style, (8 << 20) + (512 << 10))
    want, _ = model(fr, reads)
    st = check_case(fr, reads, want, fault, kw)
    assert st["fired"], "the fault was not reached"
    assert (st["mode"] == 1) == in_pipe, st                  # where the stream was when it met the fault


def test_lockstep_run_failure_followed_by_a_retry():
    """run() fails after the blocks were taken from the source: a retry used to decode from behind them"""
    named(dict(read_ahead=1), ("run", 5, 90), 8192)
    named(dict(read_ahead=1), ("commit", 5, 92), 8192, callback=True, chunk=1000)


def test_inline_fetch_wait_failure_followed_by_a_retry():
    """the host buffer had been grown before the download failed: a retry used to hand out the bytes that were never written"""
    named(dict(pipe_after=1 << 40, first_run=1), ("fetch_wait", 3, 91), 8192)
    named(dict(pipe_after=1 << 40, first_run=1), ("fetch", 3, 90), "mixed", callback=True, chunk=0)


def test_pipe_commit_failure():
    """the worker's commit() fails: the runs it had taken and the queued ones used to be skipped by the block-by-block schedule behind it"""
    named(pipe_kw, ("commit", 3, 92), 8192, in_pipe=True)
    named(pipe_kw, ("commit", 4, 91), 8192, in_pipe=True, callback=True, chunk=1000)


def test_pipe_fetch_failure_behind_account():
    """the worker's fetch() fails after the run was committed and counted: its plaintext never reaches the ring"""
    named(pipe_kw, ("fetch", 3, 90), 8192, in_pipe=True)
    named(pipe_kw, ("fetch", 4, 92), 8192, in_pipe=True, callback=True, chunk=0)


# ---- threads: the same cases in a stand-alone program, under ThreadSanitizer and under AddressSanitizer ---------------------------------
@pytest.mark.parametrize("target", ["stream_faults_tsan", "stream_faults_asan"])
def test_pipe_faults_stand_alone_under_sanitizers(target, tmp_path):
    d = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", d, "-s", target, "OUT=" + str(tmp_path)])
    p = subprocess.run([str(tmp_path / target)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode()
    assert p.returncode == 0, (p.stdout.decode()[-2000:], err[-4000:])
    assert b"stream faults ok" in p.stdout
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]


def test_thread_that_cannot_be_started_and_then_a_rebase_that_fails(monkeypatch):
    """PIPE cannot start one of its threads and falls back to block by block, which rebuilds the device window (rebase): when that fails,
    the engine error surfaces in the read that started the worker, and stays"""
    name, fr = FRAMES[1]
    reads = read_pattern(random.Random(4), len(fr.plain), 8192)
    want, _ = model(fr, reads)
    for where in (1, 2):
        monkeypatch.setenv("ZGEMU_FAIL_THREAD", str(where))
        for src, code in ((SOURCES[0], 90), (SOURCES[2], 92)):
            st = check_case(fr, reads, want, ("rebase", 1, code), dict(pipe_kw(name, fr), **src))
            assert st["fired"] and st["pipe_begins"] == 1 and st["mode"] == 2, st


def test_stream_error_accessor_without_a_stream():
    """zgpu_decoder_stream_error of no decoder: 0 (with a stream behind it: tests/test_gpu_stream.py)"""
    import zgpu
    assert zgpu.load_library().zgpu_decoder_stream_error(None) == 0
