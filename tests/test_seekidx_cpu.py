"""A declared-kind seek index (zstd-rs_amd/csrc/zg_seekidx.h: zg_k_seekidx_rows' lane routine), compiled with g++ over the SIMT emulator
(tests/emu/zg_simt.h) and run on the CPU as zgpu_seek_index_create_device and zgpu_frames_seek_indexed_device lay the passes out: the summary
pass (zgi::index_entry<false>), the host's decision, the rows pass, the host's check, the find pass (zgm::seekmany_find).
tests/emu/zg_emu_seekidx.cpp is the harness, built by tests/lanesuite.py. Demanded of every launch:
  - the pairs of every accepted entry equal tests/seekidx.py's model (rows and prefix sums parsed from the bytes in Python);
  - reads outside [0, len) 0, reads of a block body 0, pair stores outside the lane's [pre, pre + limit] 0, pair loads outside the pairs 0;
  - every record equals the model's rule on the rows, all 64 bytes, and zgk::seek_entry's (anchor 0) in src_lo, src_hi, plain_lo, plain_seen
    and flag bit 2;
  - an entry the model refuses is refused with the model's reason, gets no lane in the rows pass and no pair is stored for it.
Entries are built by hand from zgdata.zstd_compress(content_size=True) frames, test_seek_cpu.sized_frame and test_walk_cpu.skippable. The same
launches run once more in a stand-alone AddressSanitizer program (its own main, no Python in the process) in which every entry and the pairs
lie in heap blocks of exactly their size."""
import ctypes as C
import os
import random
import struct
import sys

import pytest

import lanesuite
import seekidx
import zgpu
from seekidx import U64
from test_seek_cpu import sized_frame
from test_walk_cpu import MAGIC, block, skippable

sys.path.insert(0, os.path.join(lanesuite.ROOT, "tools"))   # zgdata: the workload generators


def eight_byte_fcs(frame):
    """the frame with its Frame_Content_Size field rewritten in the 8-byte form (the same value)"""
    d = frame[4]
    single, did, fc = (d >> 5) & 1, d & 3, d >> 6
    fl = [single, 2, 4, 8][fc]
    hs = 5 + (0 if single else 1) + [0, 1, 2, 4][did] + fl
    value = int.from_bytes(frame[hs - fl:hs], "little") + (256 if fl == 2 else 0)
    assert fl in (1, 2, 4)
    return frame[:4] + bytes([(d & 0x3F) | 0xC0]) + frame[5:hs - fl] + struct.pack("<Q", value) + frame[hs:]


def entries():
    """{name: bytes}: what the issue lists"""
    import zgdata
    rng = random.Random(0x1DE5)
    text = lambda n, k=0: zgdata.text_like(max(n, 1), seed=0x5E0 + k)[:n]   # noqa: E731
    z = lambda data, **kw: zgdata.zstd_compress(data, checksum=kw.pop("checksum", False), content_size=True, **kw)   # noqa: E731
    out = {}
    out["empty"] = b""
    out["one_frame"] = z(text(3000))
    out["fcs_zero"] = z(b"") + z(text(10)) + z(b"") + z(b"") + z(text(300, 1)) + z(b"")
    sizes = [0, 1, 255, 256, 257, 65791, 65792, 70000]
    fr = [z(text(n, n)) for n in sizes]
    flens = set()
    for f in fr:
        d = f[4]
        flens.add([(d >> 5) & 1, 2, 4, 8][d >> 6])
    assert flens == {1, 2, 4}, flens
    out["fcs_fields"] = b"".join(fr) + eight_byte_fcs(fr[-1]) + eight_byte_fcs(fr[3]) + eight_byte_fcs(fr[1])
    big = z(text(300 << 10, 3))                                                      # three compressed blocks
    raw = z(bytes(rng.getrandbits(8) for _ in range(150 << 10)))                     # raw blocks
    rle = z(bytes([7]) * (200 << 10))                                                # RLE blocks
    out["blocks"] = big + raw + rle + sized_frame(b"q" * 200)
    kinds = set()
    for part in (big, raw, rle):
        for lo, hi in seekidx.rows(part)[2]:
            kinds.add((part[lo - 3] >> 1) & 3)
    assert kinds == {0, 1, 2} and len(seekidx.rows(big)[2]) == 3
    out["checksums"] = z(text(5000, 4), checksum=True) + z(text(100, 5)) + z(b"", checksum=True) + sized_frame(b"r" * 9, checksum=True)
    out["skippable"] = (skippable(b"front" * 3) + z(text(700, 6)) + skippable(b"") + skippable(b"mid", magic=0x184D2A5F) + z(text(1, 7)) +
                        z(text(4000, 8)) + skippable(b"behind" * 9))
    fs = [z(text(n, 20 + n)) for n in (500, 0, 1200, 77)]
    out["seek_table_behind"] = b"".join(fs) + zgpu.seek_table_frame([len(f) for f in fs], [500, 0, 1200, 77])
    out["unsized_middle"] = z(text(600, 9)) + zgdata.zstd_compress(text(900, 10), checksum=False, content_size=False) + z(text(50, 11))
    good = z(text(800, 12)) + skippable(b"xy") + sized_frame(b"s" * 100)
    out["chain1"] = good + MAGIC[:3]
    out["chain2"] = good + b"\x00\x01\x02\x03\x04\x05"
    out["chain3"] = good + skippable(b"abc", length=40)
    out["chain4"] = good + sized_frame(b"t" * 10)[:8]
    out["chain5"] = good + MAGIC + bytes([0x20, 0]) + block(b"", btype=3)
    out["chain6"] = good + MAGIC + bytes([0x20, 0]) + block(b"", btype=0, size=(128 << 10) + 1)
    out["chain7"] = good + sized_frame(b"u" * 100)[:-40]
    out["chain8"] = good + sized_frame(b"v" * 10, checksum=True)[:-2]
    for k in range(1, 9):
        assert seekidx.index(out["chain%d" % k])[0] == k, k
    assert seekidx.index(out["unsized_middle"])[0] == seekidx.INDEX_UNSIZED
    return out


def launches():
    """[(name, [entry bytes], cut, [(entry, begin, rlen)])]"""
    es = entries()
    out = []

    def ranges_of(zs):
        rg = []
        for i, e in enumerate(zs):
            why, _, D = seekidx.index(e)
            rg += [(i, b, n) for b, n in (seekidx.boundary_ranges(D) if not why else [(0, 1), (5, 0), (0, U64)])]
        return rg

    for name, e in es.items():
        out.append((name, [e], -1, ranges_of([e])))
    everything = list(es.values())
    out.append(("all_in_one_launch", everything, -1, ranges_of(everything)))
    # 65 entries: the second wave has one live lane; every fifth one is refused, so the rows pass has fewer lanes than the summary pass
    small = [es["fcs_zero"], es["skippable"], es["chain7"], es["one_frame"], es["empty"]]
    many = [small[i % 5] for i in range(64)] + [es["checksums"]]
    out.append(("65_entries", many, -1, ranges_of(many)))
    sized = [es["one_frame"]] * 64 + [es["seek_table_behind"]]
    out.append(("65_accepted", sized, -1, ranges_of(sized)))
    # the input changed between the passes: a row limit one smaller than the chain yields
    for name in ("one_frame", "skippable", "fcs_fields"):
        trio = [es["fcs_zero"], es[name], es["checksums"]]
        out.append(("cut:" + name, trio, 1, ranges_of(trio)))
    return out


def _declare(L):
    vp = C.c_void_p
    L.zgemu_seekidx.argtypes = [vp, vp, C.c_uint32, C.c_int64, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp]
    L.zgemu_seekidx.restype = C.c_uint32


built = lanesuite.built_fixture("zg_emu_seekidx.cpp", "seekidx", "SEEKIDX_MAIN", declare=_declare)


@pytest.fixture(scope="module")
def cases():
    """[(name, entries, cut, ranges, [(why, C, D)], [record or None])]: the model, computed once"""
    out = []
    for name, zs, cut, rg in launches():
        idx = [seekidx.index(e) for e in zs]
        want = []
        for e, b, n in rg:
            why, Cs, Ds = idx[e]
            want.append(None if why or e == cut else seekidx.record(Cs, Ds, len(zs[e]), b, n))
        out.append((name, zs, cut, rg, idx, want))
    return out


def run_launch(L, zs, cut, rg):
    n, m = len(zs), len(rg)
    bufs = [C.create_string_buffer(e, max(len(e), 1)) for e in zs]
    ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in bufs])
    lens = (C.c_uint64 * max(n, 1))(*[len(e) for e in zs])
    ranges = (C.c_uint64 * max(3 * m, 1))(*[x for r in rg for x in r])
    out = (zgpu.SeekC * max(m, 1))()
    room = sum(len(e) // 8 + 2 for e in zs)
    counts, meta, pairs, npairs = (C.c_uint64 * 5)(), (C.c_uint64 * (8 * n))(), (C.c_uint64 * (2 * room))(), C.c_uint64(0)
    differ = L.zgemu_seekidx(ptrs, lens, n, cut, ranges, m, out, counts, meta, pairs, room, C.byref(npairs))
    assert npairs.value <= room
    return (differ, [zgpu.Seek(out[j]).key() for j in range(m)], list(counts), [list(meta[8 * i:8 * i + 8]) for i in range(n)],
            [(pairs[2 * i], pairs[2 * i + 1]) for i in range(npairs.value)])


def test_rows_pairs_and_records_equal_the_model(built, cases):
    L, _, _ = built
    seen_why, refused, nothing, ranges_run, second_wave = set(), 0, 0, 0, 0
    for name, zs, cut, rg, idx, want in cases:
        differ, recs, counts, meta, pairs = run_launch(L, zs, cut, rg)
        assert differ == 0, (name, "%d records differ from zgk::seek_entry's" % differ)
        assert counts[:4] == [0, 0, 0, 0], (name, "reads outside the entry, reads of a body, stores outside the range, loads outside the pairs", counts)
        stores = 0
        for i, ((why, Cs, Ds), mt) in enumerate(zip(idx, meta)):
            refusal, ok, nrows, pre, limit, c_end, d_end, lane_why = mt
            assert refusal == why, (name, i, mt)
            seen_why.add(why)
            if why:
                assert not ok and limit == 0, (name, i, mt)   # (no lane in the rows pass: nothing of the pairs is its own)
                refused += 1
                continue
            nr = len(Cs) - 1
            if i == cut:
                # the host expected one row fewer: rows [0, limit) are stored inside the range, the closing pair is not, the host refuses
                assert not ok and limit == nr - 1 and nrows == nr and lane_why == 0, (name, i, mt)
                assert pairs[pre:pre + limit] == list(zip(Cs, Ds))[:limit] and pairs[pre + limit] == (0xEEEEEEEEEEEEEEEE,) * 2, (name, i)
                stores += limit
                continue
            assert ok and nrows == nr == limit and (c_end, d_end) == (Cs[-1], Ds[-1]) and c_end == len(zs[i]), (name, i, mt)
            assert pairs[pre:pre + nr + 1] == list(zip(Cs, Ds)), (name, i)
            stores += nr + 1
        assert counts[4] == stores and len(pairs) == stores + sum(1 for i in range(len(zs)) if i == cut), (name, counts, stores)
        for r, rec, w in zip(rg, recs, want):
            assert rec == (w if w is not None else (0,) * 11), (name, r, rec, w)
            nothing += w is not None and w[10] == 4
            ranges_run += 1
        second_wave += len(zs) > 64
    assert seen_why >= set(range(9)) | {seekidx.INDEX_UNSIZED}, seen_why
    assert refused > 20 and nothing > 20 and ranges_run > 2000 and second_wave == 2, (refused, nothing, ranges_run, second_wave)


def test_pinned_rows(built):
    L, _, _ = built
    a, b, e = sized_frame(b"a" * 100), sized_frame(b"b" * 255, checksum=True), sized_frame(b"")
    z = skippable(b"12345") + a + e + skippable(b"") + b + e
    assert seekidx.index(z) == (0, [0, 13, 122, 131, 139, 407, 416], [0, 0, 100, 100, 100, 355, 355])
    want = {
        (0, 1): (13, 122, 0, 100, 100, 0, 1, 1, 0, 0, 0),          # the skippable frame in front is no part of the selection
        (99, 2): (13, 407, 0, 355, 355, 0, 1, 4, 0, 0, 0),         # ... the one inside it is, with the empty frame
        (100, 1): (139, 407, 100, 255, 355, 0, 4, 1, 0, 0, 0),     # the empty frame and the skippable one in front are skipped
        (0, U64): (13, 416, 0, 355, 355, 0, 1, 5, 0, 0, 0),        # no row reaches the end: last = nrows - 1
        (355, 1): (416, 416, 355, 0, 355, 0, 6, 0, 0, 0, 4),
        (7, 0): (0,) * 11,
    }
    differ, recs, counts, meta, pairs = run_launch(L, [z], -1, [(0,) + r for r in want])
    assert differ == 0 and recs == list(want.values()) and counts[:4] == [0, 0, 0, 0]
    assert pairs == list(zip(*seekidx.index(z)[1:])) and meta[0][:3] == [0, 1, 6]
    # an entry of length 0: a valid index without rows, one pair
    differ, recs, counts, meta, pairs = run_launch(L, [b""], -1, [(0, 0, 1), (0, 0, 0)])
    assert recs == [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4), (0,) * 11] and pairs == [(0, 0)] and meta[0][:3] == [0, 1, 0] and counts == [0, 0, 0, 0, 1]


def test_seekidx_under_address_sanitizer_stand_alone(built, cases):
    _, exe, d = built
    src, dst = d / "cases.bin", d / "records.bin"
    with open(src, "wb") as f:
        for _, zs, cut, rg, _, _ in cases:
            f.write(struct.pack("<QQq", len(zs), len(rg), cut) + b"".join(struct.pack("<Q", len(e)) for e in zs) +
                    b"".join(struct.pack("<QQQ", *r) for r in rg) + b"".join(zs))
    lanesuite.run_stand_alone(exe, [src, dst], b"seekidx_asan ok", timeout=1800)
    recs = open(dst, "rb").read()
    at = 0
    for name, zs, cut, rg, idx, want in cases:
        for r, w in zip(rg, want):
            got = zgpu.Seek(zgpu.SeekC.from_buffer_copy(recs, at)).key()
            assert got == (w if w is not None else (0,) * 11), (name, r, got, w)
            at += 64
        for i, (why, Cs, _) in enumerate(idx):
            ok, nrows = struct.unpack_from("<QQ", recs, at)
            assert ok == (0 if why or i == cut else 1) and (why or nrows == len(Cs) - 1), (name, i, ok, nrows)
            at += 16
    assert at == len(recs)
