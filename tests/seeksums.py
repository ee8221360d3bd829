"""The rule of ZGPU_DEVICE_VERIFY_SEEK_TABLE for the tests of zg_k_seeksums (tests/test_seeksums_cpu.py, tests/test_gpu_seek_table_verify.py): a
model in plain Python, written from the rule's text in include/zgpu.h and the format's description there, not from zg_seeksums.h.

An entry's selection is table rows [first, first + taken); R_k = the compressed sizes of rows first .. k - 1. A decoded zstd frame (begin, clen,
slot) — begin counted from the selection's first byte, slot its digest's index or None if it was not hashed — coincides with row k if begin ==
R_k and clen == c_k; a coinciding, hashed frame is compared: digests[slot] & 0xFFFFFFFF against the row's Checksum."""
import struct

import seektabs
import zgpu

FIELDS = ("rows", "coinciding", "compared", "differing", "first_bad", "why", "flags")
NO_ROW = 0xFFFFFFFF
WHY_ROWS, WHY_LIST = 21, 22          # the selection leaves the table; a frame names a digest that does not exist
NO_CHECKSUMS = 1
ZERO = (0,) * 7
EMPTY_XXH32 = 0x51D8E999             # the low 32 bits of XXH64 (seed 0) of no bytes


def _fail(why):
    return (0, 0, 0, 0, 0, why, 0)


def model(entry, first, taken, frames, digests):
    """(record, windows): the seven fields of the compare's record for rows [first, first + taken) of `entry` and the decoded frames `frames`
    [(begin, clen, slot or None)], and the byte ranges [(lo, hi)] of the entry that may be read for it — the 9 footer bytes, the 8 bytes of
    the table frame's header, the taken rows; fewer where the table is refused earlier, none where nothing is taken."""
    n = len(entry)
    if taken == 0:
        return ZERO, []
    if n < 17:
        return _fail(zgpu.SEEKTAB_NONE), []
    nf, desc, magic = struct.unpack_from("<IBI", entry, n - 9)
    foot = (n - 9, n)
    if magic != seektabs.SEEK_MAGIC:
        return _fail(zgpu.SEEKTAB_NONE), [foot]
    if desc & 0x7C:
        return _fail(zgpu.SEEKTAB_RESERVED_BITS), [foot]
    es = 12 if desc & 0x80 else 8
    if nf > seektabs.MAX_FRAMES or nf * es + 17 > n:
        return _fail(zgpu.SEEKTAB_TOO_LARGE), [foot]
    tab = n - (nf * es + 17)
    head = (tab, tab + 8)
    if struct.unpack_from("<II", entry, tab) != (seektabs.SKIP_MAGIC, nf * es + 9):
        return _fail(zgpu.SEEKTAB_BAD_FRAME), [foot, head]
    if first + taken > nf:
        return _fail(WHY_ROWS), [foot, head]
    rows = (tab + 8 + first * es, tab + 8 + (first + taken) * es)
    by_begin = {b: (clen, slot) for b, clen, slot in frames}
    assert len(by_begin) == len(frames)
    at = coinciding = compared = differing = 0
    first_bad = NO_ROW
    for k in range(taken):
        c = struct.unpack_from("<I", entry, rows[0] + k * es)[0]
        fr = by_begin.get(at)
        if fr is not None and fr[0] == c:
            coinciding += 1
            if es == 12 and fr[1] is not None:
                if fr[1] >= len(digests):
                    return _fail(WHY_LIST), [foot, head, rows]
                compared += 1
                if digests[fr[1]] & 0xFFFFFFFF != struct.unpack_from("<I", entry, rows[0] + k * es + 8)[0]:
                    differing += 1
                    if first_bad == NO_ROW:
                        first_bad = first + k
        at += c
    return (taken, coinciding, compared, differing, first_bad, 0, 0 if es == 12 else NO_CHECKSUMS), [foot, head, rows]


def vouched(rec, nframes):
    """the verdict: the table vouches for all nframes decoded zstd frames (a record with a `why` is the call's error, not a verdict)"""
    d = dict(zip(FIELDS, rec))
    assert d["why"] == 0
    return not d["flags"] & NO_CHECKSUMS and d["differing"] == 0 and d["coinciding"] == nframes


def failed_counts(rec, nframes):
    """(checksums, checksum_mismatches, checksums_unverified) of an entry the flag failed: compared, differing, decoded and not compared"""
    d = dict(zip(FIELDS, rec))
    return d["compared"], d["differing"], nframes - d["compared"]
