"""The layout of a record batch (zstd-rs_amd/csrc/zg_records.h: plan_rows), compiled with g++ (tests/emu/zg_lane_fill.cpp), against the model in
tests/recbatch.py, which is written from include/zgpu.h's definitions: both layouts, truncation on and off, lookups with statuses (length 0)
among good ones, lengths 0, width - 1, width and width + 1, m = 0, 1 and 1000, and layouts that do not fit in 64 bits, which must be refused
and never wrap."""
import ctypes as C
import itertools
import random

import recbatch
from test_fill_cpu import built   # noqa: F401 (the fixture: one build of the harness per session)

U64 = recbatch.U64


def _rows(L, lens, layout, truncate, width):
    m = len(lens)
    a = (C.c_uint64 * max(m, 1))(*lens)
    rows, total, cut = (C.c_uint64 * max(3 * m, 1))(), C.c_uint64(77), C.c_uint32(77)
    ok = L.fl_plan_rows(a, m, layout, int(truncate), width, rows, C.byref(total), C.byref(cut))
    if not ok:
        return None
    return [tuple(rows[3 * j:3 * j + 3]) for j in range(m)], total.value, cut.value


def test_both_layouts_against_the_model(built):
    L = built[0]
    rng = random.Random(0xBA7C)
    for width in (1, 17, 64, 4097):
        edge = [0, width - 1, width, width + 1, 0, 5 * width + 3]     # (a 0 among them: a lookup that gave a status, an empty range)
        for m in (0, 1, 1000):
            for lens in ([edge[j % len(edge)] for j in range(m)], [rng.choice(edge + [rng.randrange(0, 3 * width + 2)]) for _ in range(m)]):
                for layout, truncate in itertools.product((recbatch.PADDED, recbatch.PACKED), (False, True)):
                    got, want = _rows(L, lens, layout, truncate, width), recbatch.plan(lens, layout, width, truncate)
                    assert got == want, (width, m, layout, truncate)
                    rows, total, cut = got
                    assert cut == (sum(1 for n in lens if n > width) if truncate else 0)
                    if layout == recbatch.PADDED:
                        assert total == m * width and all(r[:2] == (j * width, width) for j, r in enumerate(rows))
                    else:
                        assert total == sum(r[2] for r in rows) and all(r[1] == r[2] for r in rows)
    # packed without a width: nothing is cut, whatever the flag says
    for truncate in (False, True):
        assert _rows(L, [5, 0, 9], recbatch.PACKED, truncate, 0) == ([(0, 5, 5), (5, 0, 0), (5, 9, 9)], 14, 0)


def test_layouts_that_pass_64_bits_are_refused(built):
    L = built[0]
    big = 1 << 62
    # m * width
    assert recbatch.plan([0] * 4, recbatch.PADDED, big, False) is None and _rows(L, [0] * 4, recbatch.PADDED, False, big) is None
    assert _rows(L, [0] * 3, recbatch.PADDED, False, big) == recbatch.plan([0] * 3, recbatch.PADDED, big, False) != None   # noqa: E711
    assert _rows(L, [1, 2], recbatch.PADDED, True, U64) is None and _rows(L, [1], recbatch.PADDED, True, U64)[1] == U64
    # a packed sum
    assert recbatch.plan([big] * 4, recbatch.PACKED, 0, False) is None and _rows(L, [big] * 4, recbatch.PACKED, False, 0) is None
    assert _rows(L, [U64, 1], recbatch.PACKED, False, 0) is None and _rows(L, [U64, 0], recbatch.PACKED, False, 0)[1] == U64
    assert _rows(L, [big] * 3 + [big - 1], recbatch.PACKED, False, 0)[1] == U64
    # truncation brings a sum back into range
    assert _rows(L, [U64, U64, U64], recbatch.PACKED, True, 10) == ([(0, 10, 10), (10, 10, 10), (20, 10, 10)], 30, 3)
