"""The rule of ZGPU_DEVICE_VERIFY_SEEK_TABLE on an entry whose seek index handle holds sums, for the tests of zg_k_idxsums
(tests/test_idxsums_cpu.py, tests/test_gpu_seek_index_sums.py): a model in plain Python over pairs and sums, written from the rule's text in
include/zgpu.h (seek index checksums), not from zg_idxsums.h.

A group is rows [first, first + taken) of an entry of nrows rows; C[0 .. nrows] are the entry's compressed prefix sums, sums[0 .. nrows) its
sums. R_k = C[k] - C[first], c_k = C[k + 1] - C[k]. A decoded zstd frame (begin, clen, slot) — begin counted from the group's first byte, slot
its digest's index or None if it was not hashed — coincides with row k if begin == R_k and clen == c_k; a coinciding, hashed frame is compared:
digests[slot] & 0xFFFFFFFF against sums[k]. The record's fields, vouched() and failed_counts() are tests/seeksums.py's: one verdict."""
from seeksums import FIELDS, NO_ROW, WHY_LIST, WHY_ROWS, ZERO, failed_counts, vouched   # noqa: F401 (the tests take them from here)


def _fail(why):
    return (0, 0, 0, 0, 0, why, 0)


def model(C, sums, first, taken, frames, digests):
    """(record, pair_window, sum_window): the seven fields of the compare's record, and the rows of the entry's pairs and sums that may be
    read for it — pairs [first, first + taken], sums [first, first + taken) —, None where nothing may be read"""
    nrows = len(C) - 1
    assert len(sums) == nrows
    if taken == 0:
        return ZERO, None, None
    if first + taken > nrows:
        return _fail(WHY_ROWS), None, None
    by_begin = {b: (clen, slot) for b, clen, slot in frames}
    assert len(by_begin) == len(frames)
    coinciding = compared = differing = 0
    first_bad = NO_ROW
    windows = (first, first + taken + 1), (first, first + taken)
    for k in range(first, first + taken):
        fr = by_begin.get(C[k] - C[first])
        if fr is None or fr[0] != C[k + 1] - C[k]:
            continue
        coinciding += 1
        if fr[1] is None:
            continue
        if fr[1] >= len(digests):
            return (_fail(WHY_LIST),) + windows
        compared += 1
        if digests[fr[1]] & 0xFFFFFFFF != sums[k]:
            differing += 1
            if first_bad == NO_ROW:
                first_bad = k
    return ((taken, coinciding, compared, differing, first_bad, 0, 0),) + windows
