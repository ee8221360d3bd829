"""The CPU emulator's zx_* primitives (tests/emu/zg_simt.h) against the plain model of tests/zxprobe.py, one primitive per run: the source of
zg_k_zxprobe (zstd-rs_amd/csrc/zg_zxprobe.h) compiled with g++ over the emulator (tests/emu/zg_emu_zxprobe.cpp, built by tests/lanesuite.py).
tests/test_gpu_zxprobe.py runs the same cases on an MI355X: together they hold the emulator, on which some forty suites run the kernel bodies,
to the hardware. Demanded here:
  - of every case: the result words and the whole arena equal the model's, bit for bit, and the operand words are unchanged;
  - the same in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which operands, results and arena lie in
    heap blocks of exactly their sizes;
  - zgpu_debug_zx_probe and the harness refuse the same arguments, the library without a GPU and before it looks at its context;
  - outside a primitive's domain the emulator aborts with a message (a child process);
  - the cases reach what the module says they reach: every primitive, every "first j dwords in range" pattern of every width, every alignment."""
import ctypes as C
import os
import subprocess

import pytest

import lanesuite
import zgpu
import zxprobe

U32P = C.POINTER(C.c_uint32)


def _declare(L):
    L.zxp_run.argtypes = [C.c_uint32] * 5 + [U32P, U32P, C.c_char_p, C.c_char_p, C.c_uint32]


built = lanesuite.built_fixture("zg_emu_zxprobe.cpp", "zxprobe", "ZXP_MAIN", declare=_declare)


@pytest.fixture(scope="module")
def cases():
    cs = zxprobe.all_cases()
    return cs, [zxprobe.model(c) for c in cs]


def run_emulator(L, c):
    a, o = (C.c_uint32 * len(c.inp))(*c.inp), (C.c_uint32 * len(c.out0))(*c.out0)
    dst = C.create_string_buffer(len(c.arena))
    st = L.zxp_run(c.op, c.threads, c.flags, c.res_off, c.res_bytes, a, o, c.arena, dst, len(c.arena))
    return st, list(o), dst.raw, list(a)


def test_emulator_equals_the_model(built, cases):
    L = built[0]
    for c, (out, arena) in zip(*cases):
        st, got, got_arena, a = run_emulator(L, c)
        assert st == 0, c.name
        assert got == out, c.name
        assert got_arena == arena, c.name
        assert a == c.inp, c.name


def test_stand_alone_address_sanitizer(built, cases):
    _, exe, d = built
    path = os.path.join(str(d), "cases.bin")
    zxprobe.write_cases(path, *cases)
    out = lanesuite.run_stand_alone(exe, [path], b"zxprobe ok: %d cases" % len(cases[0]), 600)
    assert b"differ" not in out and b"refused" not in out


def _refusals():
    """(what is wrong, op, threads, flags, res_off, res_bytes, the words of thread 3, arena bytes): each one argument away from a call that passes"""
    O, B = zxprobe.OP, 0x80000000
    ok = ("nothing", O["Ld32"], 64, 0, 256, 16, [0, 0], 1024)
    yield ok
    for what, ch in (("63 threads", {2: 63}), ("128 threads", {2: 128}), ("1024 threads", {2: 1024}), ("an unknown primitive", {1: len(O)}),
                     ("unknown flags", {3: 2}), ("a resource 255 bytes behind the arena's start", {4: 255}),
                     ("a resource 255 bytes in front of the arena's end", {4: 1024 - 255 - 16}), ("a resource past the arena", {5: 1024}),
                     ("a resource that starts behind the arena", {4: 2048}), ("an arena below two guards", {7: 496, 4: 256, 5: 0}),
                     ("an arena of no whole 16 bytes", {7: 1028}), ("an arena above 1 MiB", {7: (1 << 20) + 16}),
                     ("a null resource with a size", {3: 1, 4: 0, 5: 16}), ("a null resource with an offset", {3: 1, 4: 256, 5: 0}),
                     ("an offset that could wrap", {6: [0, 0xFFFFFFF0]}), ("the last offset", {6: [0, 0xFFFFFFFF]}), ("ZX_OOB + 64", {6: [0, B + 64]}),
                     ("an offset that could wrap, of a lane that does nothing", {6: [1, 0xFFFFFFF0]})):
        row = list(ok)
        for k, v in ch.items():
            row[k] = v
        row[0] = what
        yield tuple(row)
    for op in ("Ld8", "Ld32", "Ld64", "Ld96", "Ld128", "St8", "St32"):
        yield ("nothing", O[op], 64, 0, 256, 16, [0, B + 12], 1024)
        yield ("nothing", O[op], 256, 0, 256, 16, [0, B + 63], 1024)
        yield ("nothing", O[op], 64, 1, 0, 0, [0, B], 512)
        yield ("an offset that could wrap", O[op], 64, 0, 256, 16, [0, 0xFFFFFFF0], 1024)
    for op in ("Gst32u", "MinGlb", "MaxGlb"):
        yield ("nothing", O[op], 64, 0, 256, 0, [0, 1020], 1024)
        yield ("an index past the arena", O[op], 64, 0, 256, 0, [0, 1021 if op == "Gst32u" else 1024], 1024)
        yield ("an index far past the arena", O[op], 64, 0, 256, 0, [0, 0xFFFFFFFC], 1024)
    yield ("nothing", O["Gst32u"], 64, 0, 256, 0, [0, 1019], 1024)
    yield ("a misaligned atomic", O["MinGlb"], 64, 0, 256, 0, [0, 1018], 1024)
    for op in ("Gst128", "Gld128"):
        yield ("nothing", O[op], 64, 0, 256, 0, [0, 1008], 1024)
        yield ("an index past the arena", O[op], 64, 0, 256, 0, [0, 1024], 1024)
        yield ("a misaligned index", O[op], 64, 0, 256, 0, [0, 1004], 1024)
        yield ("an index far past the arena", O[op], 64, 0, 256, 0, [0, 0xFFFFFFF0], 1024)
    for op in ("OrLds", "MinLds", "MinLds64", "AddLds", "CasLds"):
        yield ("nothing", O[op], 64, 0, 256, 0, [0, 63], 1024)
        yield ("a word past the LDS array", O[op], 64, 0, 256, 0, [0, 64], 1024)
    yield ("nothing", O["PubWave"], 64, 0, 256, 0, [0, 5, 63], 2048)
    yield ("a slot of another wave", O["PubWave"], 64, 0, 256, 0, [0, 5, 64], 2048)
    for op in ("PubBarrier", "PubBarrierVm", "PubFence"):
        yield ("nothing", O[op], 256, 0, 256, 0, [0, 5, 255], 2048)
        yield ("a slot past the workgroup", O[op], 256, 0, 256, 0, [0, 5, 256], 2048)
        yield ("a slot past the workgroup", O[op], 64, 0, 256, 0, [0, 5, 64], 2048)
    for op in ("PubBarrierVm", "PubFence"):
        yield ("slots past the arena", O[op], 256, 0, 256, 0, [0, 5, 0], 512)


def test_argument_rules_need_no_gpu(built):
    """what could lead outside the probe's allocations is refused by the library before any HIP call and before its context is looked at (this
    one is no context), and by the harness in the same words; what passes the rules runs on the emulator without an AddressSanitizer report
    (test_stand_alone_address_sanitizer has every case), and the library goes on to its first HIP call (no GPU here: not made)"""
    E = built[0]
    fake = C.create_string_buffer(4096)
    for dev in (False, True):
        L = zgpu.load_library(dev=dev)
        assert "zgpu_debug_zx_probe" in zgpu.EXPORTS and hasattr(L, "zgpu_debug_zx_probe")
        seen = set()
        for what, op, threads, flags, res_off, res_bytes, row, arena_bytes in _refusals():
            inp = [0] * (max(threads, 64) * zxprobe.K_IN)
            inp[3 * zxprobe.K_IN:3 * zxprobe.K_IN + len(row)] = row
            a, o = (C.c_uint32 * len(inp))(*inp), (C.c_uint32 * (max(threads, 64) * zxprobe.K_OUT))()
            src, dst = C.create_string_buffer(arena_bytes), C.create_string_buffer(arena_bytes)
            emu = E.zxp_run(op, threads, flags, res_off, res_bytes, a, o, src.raw, dst, arena_bytes)
            assert (emu != 0) == (what != "nothing"), (what, op)
            if what != "nothing":
                assert L.zgpu_debug_zx_probe(fake, op, threads, flags, res_off, res_bytes, a, o, src, dst, arena_bytes) == zgpu.E_BAD_ARG, (what, op)
            seen.add(what)
        assert len(seen) > 25
        a, o, buf = (C.c_uint32 * 512)(), (C.c_uint32 * 256)(), C.create_string_buffer(1024)
        for k in range(5):                               # a null context or array
            args = [fake, a, o, buf, buf]
            args[k] = None
            assert L.zgpu_debug_zx_probe(args[0], zxprobe.OP["Ld32"], 64, 0, 256, 16, args[1], args[2], args[3], args[4], 1024) == zgpu.E_BAD_ARG, k
    assert hasattr(zgpu.Context, "zx_probe")
    # every case of the suites passes the rules
    for c in zxprobe.all_cases():
        assert c.threads in (64, 256) and len(c.arena) % 16 == 0 and len(c.arena) >= 512, c.name
        if not c.flags:
            assert c.res_off >= 256 and c.res_off + c.res_bytes + 256 <= len(c.arena), c.name


def _abort_case(op, rows, threads=64):
    c = zxprobe.Case("outside the domain", op, threads, zxprobe._words(rows, threads))
    return c, (c.out0, c.arena)


@pytest.mark.parametrize("what,op,row,message", [
    ("mask 65", "ShflXor", lambda t: [0, t, 65], b"zx_shfl_xor with mask 65"),
    ("mask 64", "ShflXor", lambda t: [0, t, 64], b"zx_shfl_xor with mask 64"),
    ("mask 0", "ShflXor", lambda t: [0, t, 0], b"zx_shfl_xor with mask 0"),
    ("delta 65", "ShflUp", lambda t: [0, t, 65], b"zx_shfl_up by 65"),
    ("delta -1", "ShflUp", lambda t: [0, t, 0xFFFFFFFF], b"zx_shfl_up by -1"),
    ("lane 128", "Shfl", lambda t: [0, t, 128], b"zx_shfl from lane 128"),
    ("lane -1", "Lane64", lambda t: [0, t, t, 0xFFFFFFFF], b"zx_shfl from lane -1"),
])
def test_outside_its_domain_the_emulator_aborts(built, what, op, row, message):
    """a shuffle the probe does not cover ends the stand-alone program with a message, not with an answer"""
    _, exe, d = built
    path = os.path.join(str(d), "abort_%s.bin" % what.replace(" ", "_"))
    c, want = _abort_case(op, [row(t) for t in range(64)])
    zxprobe.write_cases(path, [c], [want])
    p = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"zxprobe ok" not in p.stdout
    assert b"simt: outside the tested domain: " + message in p.stderr, p.stderr[-2000:]


@pytest.mark.parametrize("what,message", [
    ("dpp-step", b"zx_scan_src with lane 5 of the wave returned"),
    ("dpp-scan", b"zx_scan_src with lane 63 of the wave returned"),
    ("dpp-shr1", b"zx_shr1 with lane 1 of the wave returned"),
    ("dpp-partial-wave", b"zx_shr1 with lane 32 of the wave returned"),
    ("ld128", b"buffer offset 0xFFFFFFF0"),
    ("ld96", b"buffer offset 0xFFFFFFF8"),
    ("ld64", b"buffer offset 0xFFFFFFFC"),
    ("ld32-unaligned", b"buffer offset 0xFFFFFFFD"),
    ("ld8", b"buffer offset 0xFFFFFFF0"),
    ("st8", b"buffer offset 0xFFFFFFFF"),
    ("st32", b"buffer offset 0xFFFFFFF0"),
])
def test_aborts_no_case_file_reaches(built, what, message):
    """a DPP primitive with a lane of its wave returned (the emulator's scheduler releases the wave's other lanes, then the call aborts) and
    a buffer offset from 0xFFFFFFF0 on: the stand-alone program calls the primitive directly, behind the argument rules"""
    p = subprocess.run([built[1], "--outside", what], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode != 0 and b"came back" not in p.stdout and b"zxprobe ok" not in p.stdout
    assert b"simt: outside the tested domain: " + message in p.stderr, p.stderr[-2000:]


def test_the_aligned_dword_above_the_limit_reads_zero(built):
    """zx_ld32 at a multiple of 4 from 0xFFFFFFEC to 0xFFFFFFFC: in the domain (zg_flat1.h's S1c goes there), out of range, 0"""
    lanesuite.run_stand_alone(built[1], ["--outside", "dword"], b"zxprobe ok: dword", 120)


def test_cases_reach_what_they_claim(cases):
    cs = cases[0]
    cov = zxprobe.coverage(cs)
    assert cov["ops"] == set(zxprobe.OP)                 # every primitive of zg_zxprobe.h
    for op, k in (("Ld32", 1), ("Ld64", 2), ("Ld96", 3), ("Ld128", 4), ("St32", 1)):
        assert cov["dwords"][op] == set(range(k + 1)), op   # the first j dwords in range, j = 0 .. k
    for op in list(zxprobe.LOADS) + list(zxprobe.STORES):
        assert cov["bases"][op] == set(range(16)), op
        assert cov["sizes"][op] == set(zxprobe.SIZES), op
    for op in zxprobe.COLLECTIVES + ("ScanSrc0", "ScanSrc5", "ScanAdd", "Shr1"):
        assert cov["threads"][op] == {64, 256}, op       # 256: no collective crosses a wave
    by = lambda op: [c for c in cs if c.opname == op]    # noqa: E731
    assert {c.a(0)[2] for c in by("ShflUp")} >= set(zxprobe.UP_DELTAS)
    assert {c.a(0)[2] for c in by("ShflXor")} == set(zxprobe.XOR_MASKS)
    idx = {c.a(t)[2] for c in by("Shfl") for t in range(c.threads)}
    assert any(i >= 64 for i in idx) and {0, 63} <= idx
    for op in ("Shfl", "ShflUp", "ShflXor", "Lane64", "Shfl63"):   # sources that have returned, read by lanes that have not
        assert any(c.a(t)[0] and not c.a(u)[0] for c in by(op) for t in range(0, c.threads, 7) for u in range(t & ~63, (t & ~63) + 64)), op
    for s in range(6):                                   # a step with fill 0 and with another fill
        fills = [{c.a(t)[2] for t in range(c.threads)} for c in by("ScanSrc%d" % s)]
        assert {0} in fills and any(0 not in f for f in fills), s
    assert any(sum(c.a(t)[1] for t in range(64)) >> 32 for c in by("ScanAdd"))   # sums that wrap
    assert {c.a(t)[3] for c in by("Alignbit") for t in range(c.threads)} >= set(range(32)) | {32, 33, 63, 255}
    halves = (0, 1, 0x7FFF, 0x8000, 0xFFFF)
    got = {(c.a(t)[1], c.a(t)[2]) for c in by("PkSub16") for t in range(c.threads)}
    assert all(((hx << 16 | lx), (hy << 16 | ly)) in got for lx in halves for ly in halves for hx in halves for hy in halves)
    assert {(c.a(t)[1] >> 16, c.a(t)[1] & 0xFFFF) for c in by("PkSign16") for t in range(c.threads)} >= {(x, y) for x in halves for y in halves}
    for op in ("Ld64", "Ld96", "Ld128", "St32"):           # only zx_ld8, zx_ld32 and zx_st8 take addresses that are no multiple of 4
        assert all((c.res_off + c.a(t)[1]) % 4 == 0 for c in by(op) for t in range(c.threads) if not c.a(t)[0] and c.a(t)[1] < zxprobe.ZX_OOB), op   # (ZX_OOB + 0 / 4 / 8 / 12: "not needed", at any base)
    for op in ("Ld8", "Ld32", "St8"):
        assert {(c.res_off + c.a(t)[1]) % 4 for c in by(op) for t in range(c.threads) if not c.a(t)[0]} == {0, 1, 2, 3}, op
    assert any(0 < c.res_bytes - c.a(t)[1] < 4 for c in by("Ld32") for t in range(c.threads))   # dwords that straddle the resource's end
    assert {c.a(t)[1] % 16 for c in by("Gst32u") for t in range(c.threads)} == set(range(16))
