"""zg_k_seektab's wave routine (zstd-rs_amd/csrc/zg_seektab.h), compiled with g++ over the SIMT emulator (tests/emu/zg_simt.h) and run on the
CPU: 64 fibers, the ballots, shuffles and prefix sums of the source as it is compiled for gfx950. tests/emu/zg_emu_seektab.cpp is the
harness, built by tests/lanesuite.py. For every entry and every range the wave runs over a reader that counts every access and every access
outside the window the model allows, and every field of its record is compared with tests/seektabs.py's model of the rule. Demanded of every
case:
  - the record equals the model's, field for field, and all 64 lanes hold the same record;
  - no access outside [tab, len) (outside the footer, where the table is refused before its frame is located);
  - no access at all for a range of length 0 and for an entry shorter than 17 bytes.
Ranges per entry (seektabs.boundary_ranges): (D_k - 1, 2), (D_k, 1), (D_k + 1, 1) at every boundary, whole, saturating, behind the end, length
0, and a range whose first and last frame lie in different steps. Entries: nframes in {0, 1, 2, 63, 64, 65, 127, 128, 129, 200} (the wave's
step is 64) with both entry sizes and zero-size entries at lanes 0 and 63 of a step and as first and last entry; the table at every
alignment mod 16; one malformed table per `why` and every single-byte edit of the 17 framing bytes of one table. The same cases run
once more in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which every entry lies in a heap block of
exactly its length, and its records are compared with the model as well."""
import ctypes as C
import random
import struct

import pytest

import lanesuite
import seektabs
import zgpu
from seektabs import U64, model

NFRAMES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def entry_of(rng, nf, checksums, zeros=False, pad=0):
    """an entry of nf frames (filler bytes: the wave never reads them) and its seek table; pad more bytes in front move the table"""
    cs = [rng.randint(0, 9) for _ in range(nf)]
    ds = [rng.randint(1, 3000) for _ in range(nf)]
    if zeros:
        for k in range(nf):
            if k % 64 in (0, 63) or k == nf - 1:
                ds[k] = 0
    front = bytes(rng.getrandbits(8) for _ in range(sum(cs) + pad))
    sums = [rng.getrandbits(32) for _ in range(nf)] if checksums else None
    return front + zgpu.seek_table_frame(cs, ds, sums), cs, ds


def cases():
    """(name, entry, ranges)"""
    rng = random.Random(0x5EE7AB)
    out = []
    for nf in NFRAMES:
        for checksums in (False, True):
            # (zero-size entries at lanes 0 and 63 of every step, first and last; the alignment entries below have none)
            e, _, ds = entry_of(rng, nf, checksums, zeros=True)
            out.append(("n%d:es%d" % (nf, 12 if checksums else 8), e, seektabs.boundary_ranges(ds)))
    # the table at every alignment mod 16 (entries lie at 16-byte aligned addresses): two steps of 8-byte entries, one of 12-byte entries
    for checksums, nf in ((False, 65), (True, 2)):
        base, _, _ = entry_of(random.Random(7), nf, checksums)
        for a in range(16):
            tablen = nf * (12 if checksums else 8) + 17
            e, _, ds = entry_of(random.Random(7), nf, checksums, pad=(a - (len(base) - tablen)) % 16)
            assert (len(e) - tablen) % 16 == a
            out.append(("align%d:es%d" % (a, 12 if checksums else 8), e, seektabs.boundary_ranges(ds)))
    return out + malformed()


def malformed():
    rng = random.Random(0xBAD7AB)
    good, cs, ds = entry_of(rng, 3, False, pad=5)
    n, tab = len(good), len(good) - (3 * 8 + 17)
    rg = [(0, 1), (ds[0], ds[1] + 1), (sum(ds), 1), (0, U64), (3, 0)]
    out = []

    def put(name, e, why):
        assert model(e, 0, U64)[0][9] == why, name
        out.append((name, bytes(e), rg))
    put("none:short", good[-16:], zgpu.SEEKTAB_NONE)
    put("none:empty", b"", zgpu.SEEKTAB_NONE)
    put("none:magic", good[:-1] + b"\x00", zgpu.SEEKTAB_NONE)
    e = bytearray(good); e[n - 5] = 0x04
    put("reserved", e, zgpu.SEEKTAB_RESERVED_BITS)
    e = bytearray(good); e[n - 9:n - 5] = struct.pack("<I", 0x8000001)
    put("too_large:count", e, zgpu.SEEKTAB_TOO_LARGE)
    put("too_large:entry", good[tab + 1:], zgpu.SEEKTAB_TOO_LARGE)
    e = bytearray(good); e[n - 9:n - 5] = struct.pack("<I", 0xFFFFFFFF); e[n - 5] = 0x80
    put("too_large:max", e, zgpu.SEEKTAB_TOO_LARGE)
    e = bytearray(good); e[tab + 4] ^= 1
    put("bad_frame:size", e, zgpu.SEEKTAB_BAD_FRAME)
    e = bytearray(good); e[tab] = 0x5F
    put("bad_frame:magic", e, zgpu.SEEKTAB_BAD_FRAME)
    put("past_table", good[5 + 1:], zgpu.SEEKTAB_PAST_TABLE)          # one byte fewer in front than the compressed sizes claim
    e = bytearray(good); e[tab + 8:tab + 12] = struct.pack("<I", 0xFFFFFFFF)
    put("past_table:huge", e, zgpu.SEEKTAB_PAST_TABLE)
    out.append(("low_descriptor_bits", good[:n - 5] + b"\x03" + good[n - 4:], rg))   # bits 1..0 are ignored
    assert model(out[-1][1], 0, 1)[0][5] == 0
    # every single-byte edit of the 17 framing bytes: a why, or a selection the model agrees with
    for pos in list(range(tab, tab + 8)) + list(range(n - 9, n)):
        for v in range(256):
            if v != good[pos]:
                out.append(("edit:%d:%d" % (pos - tab, v), good[:pos] + bytes([v]) + good[pos + 1:], rg[1:2]))
    return out


def _declare(L):
    L.zgemu_seektab.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.zgemu_seektab.restype = C.c_uint32


built = lanesuite.built_fixture("zg_emu_seektab.cpp", "seektab", "SEEKTAB_MAIN", declare=_declare)


@pytest.fixture(scope="module")
def expected():
    """[(name, entry, ranges, [(record, lo)])]: the model, computed once"""
    return [(name, e, rg, [model(e, b, n) for b, n in rg]) for name, e, rg in cases()]


def run_waves(L, e, lo, rg):
    """the entry at a 16-byte aligned address, every range through the emulated wave; [(record, reads, reads outside [lo, len))]"""
    buf, at = lanesuite.aligned_copy(e)
    n = len(rg)
    ranges, out, counts = (C.c_uint64 * (2 * n))(*[x for r in rg for x in r]), (zgpu.SeekC * n)(), (C.c_uint64 * (2 * n))()
    assert L.zgemu_seektab(at, len(e), lo, ranges, n, out, counts) == 0, "lanes of a wave disagree"
    return [(zgpu.Seek(out[i]).key(), counts[2 * i], counts[2 * i + 1]) for i in range(n)]


def test_seektab_equals_the_model_on_every_range(built, expected):
    L, _, _ = built
    seen_why, steps_apart, nothing, waves = set(), 0, 0, 0
    for name, e, rg, want in expected:
        # the window does not depend on the range, except that a range of length 0 has none: those run with the others and must not read
        lo = min(w[1] for w in want)
        got = run_waves(L, e, lo, rg)
        for (b, n), (rec, reads, bad), (mrec, mlo) in zip(rg, got, want):
            assert rec == mrec, (name, b, n, dict(zip(seektabs.FIELDS, rec)), dict(zip(seektabs.FIELDS, mrec)))
            assert bad == 0, (name, b, n, "reads outside the table frame", bad)
            if mlo == len(e):
                assert reads == 0, (name, b, n, "a range of length 0 or an entry below 17 bytes reads nothing")
            seen_why.add(mrec[9])
            steps_apart += mrec[5] == 0 and mrec[7] > 0 and mrec[6] // 64 != (mrec[6] + mrec[7] - 1) // 64
            nothing += mrec[10] == 4
            waves += 1
    assert seen_why >= {0, 16, 17, 18, 19, 20}, seen_why
    assert steps_apart > 60 and nothing > 50 and waves > 12000, (steps_apart, nothing, waves)


def test_seektab_pinned_examples(built):
    L, _, _ = built
    cs, ds = [10, 20, 8, 30, 5], [100, 255, 0, 100, 0]       # the third is a skippable frame, the last an empty one
    e = bytes(73) + zgpu.seek_table_frame(cs, ds)
    assert len(zgpu.seek_table_frame(cs, ds)) == 5 * 8 + 17 and len(zgpu.seek_table_frame(cs, ds, [1, 2, 3, 4, 5])) == 5 * 12 + 17
    tab = 73
    want = {
        (0, 1): (0, 10, 0, 100, 100, 0, 0, 1, 0, 0, 0),
        (99, 2): (0, 30, 0, 355, 355, 0, 0, 2, 0, 0, 0),
        (100, 1): (10, 30, 100, 255, 355, 0, 1, 1, 0, 0, 0),
        (355, 1): (38, 68, 355, 100, 455, 0, 3, 1, 0, 0, 0),     # the zero-size entry in front is skipped: D_2 + d_2 > 355 does not hold
        (354, 2): (10, 68, 100, 355, 455, 0, 1, 3, 0, 0, 0),     # ... and taken inside a selection
        (0, U64): (0, 73, 0, 455, 455, 0, 0, 5, 0, 0, 0),        # no entry reaches the end: last = nframes - 1
        (455, 1): (73, 73, 455, 0, 455, 0, 5, 0, 0, 0, 4),
        (5, 0): (0,) * 11,
    }
    got = run_waves(L, e, tab, list(want))
    for (rg, rec), (g, reads, bad) in zip(want.items(), got):
        assert g == rec and model(e, *rg) == (rec, len(e) if rg[1] == 0 else tab) and bad == 0, (rg, g, rec)
    # with checksums the same selection, and an entry of 12 bytes
    e12 = bytes(73) + zgpu.seek_table_frame(cs, ds, [7] * 5)
    assert run_waves(L, e12, 73, [(354, 2)])[0][0] == want[(354, 2)]


def test_seektab_under_address_sanitizer_stand_alone(built, expected):
    _, exe, d = built
    src, dst = d / "cases.bin", d / "records.bin"
    with open(src, "wb") as f:
        for _, e, rg, _ in expected:
            f.write(struct.pack("<QQ", len(e), len(rg)) + b"".join(struct.pack("<QQ", *r) for r in rg) + e)
    lanesuite.run_stand_alone(exe, [src, dst], b"seektab_asan ok", timeout=900)
    recs = open(dst, "rb").read()
    at = 0
    for name, e, rg, want in expected:
        for r, (mrec, _) in zip(rg, want):
            got = zgpu.Seek(zgpu.SeekC.from_buffer_copy(recs, at)).key()
            assert got == mrec, (name, r, got, mrec)
            at += 64
    assert at == len(recs)


def test_seek_table_argument_rules_need_no_gpu():
    L = zgpu.load_library()
    n = 1
    srcs, lens, dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_void_p * n)(), (C.c_size_t * n)()
    rg, sk, res = (zgpu.RangeC * n)(), (zgpu.SeekC * n)(), (zgpu.RangeResultC * n)()
    assert L.zgpu_frames_seek_table_device(None, srcs, lens, n, rg, sk) == 93          # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_decode_ranges_seek_table_device_src(None, srcs, lens, n, rg, dsts, caps, None, res) == 93
    fake = C.create_string_buffer(4096)   # null arrays with n > 0: refused before the context is looked at (this one is not a context)
    for k in range(4):
        a = [srcs, lens, rg, sk]
        a[k] = None
        assert L.zgpu_frames_seek_table_device(fake, *a[:2], n, *a[2:]) == 93, k
    for k in range(6):
        a = [srcs, lens, rg, dsts, caps, res]
        a[k] = None
        assert L.zgpu_decode_ranges_seek_table_device_src(fake, a[0], a[1], n, a[2], a[3], a[4], None, a[5]) == 93, k
    # flags bits 0 and 1 together (hash nothing, verify everything): refused in front of the first HIP call
    opts = zgpu.DeviceOptsC(0, 3, 0)
    assert L.zgpu_decode_ranges_seek_table_device_src(fake, srcs, lens, n, rg, dsts, caps, C.byref(opts), res) == 93
    assert zgpu.E_SEEK_TABLE == 72
    assert (zgpu.SEEKTAB_NONE, zgpu.SEEKTAB_RESERVED_BITS, zgpu.SEEKTAB_TOO_LARGE, zgpu.SEEKTAB_BAD_FRAME, zgpu.SEEKTAB_PAST_TABLE) == (16, 17, 18, 19, 20)
    for dev in (False, True):
        lib_ = zgpu.load_library(dev=dev)
        assert lib_.zgpu_status_name(72) == b"SeekTable"
        for sym in ("zgpu_frames_seek_table_device", "zgpu_decode_ranges_seek_table_device_src"):
            assert sym in zgpu.EXPORTS and hasattr(lib_, sym), sym
    for m in ("frames_seek_table_device", "decode_ranges_seek_table_device_src"):
        assert hasattr(zgpu.Context, m)
    import inspect
    assert inspect.signature(zgpu.Context.decode_tensor_ranges).parameters["seek_table"].default is False
    # a range with an anchor is refused in Python's own tensor helper as in the C call's record (the record: tests/test_gpu_seek_table.py)
    with pytest.raises(ValueError):
        zgpu.seek_table_frame([1, 2], [3])
