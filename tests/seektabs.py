"""Seek tables of zstd's seekable format for the tests of zg_k_seektab (tests/test_seektab_cpu.py, tests/test_gpu_seek_table.py): a model of the
selection rule in plain Python, written from the format's description and the rule's text (include/zgpu.h), not from zg_seektab.h, and the
ranges the tests ask of an entry."""
import struct

import zgpu

SKIP_MAGIC, SEEK_MAGIC, MAX_FRAMES = 0x184D2A5E, 0x8F92EAB1, 0x8000000
U64 = 2 ** 64 - 1
FIELDS = zgpu.Seek.FIELDS   # src_lo, src_hi, plain_lo, bound, plain_seen, status, frames_skipped, frames_taken, nblocks, why, flags
ZERO = (0,) * 11


def _fail(why):
    return (0, 0, 0, 0, 0, zgpu.E_SEEK_TABLE, 0, 0, 0, why, 0)


def model(entry, begin, rlen):
    """(record, lo): the zgpu_seek fields for plaintext bytes [begin, begin + rlen) of `entry`, and the first byte of the entry the wave may
    read — the table frame's begin; the footer's where the table is refused before its frame is located; len(entry) where nothing is read."""
    n = len(entry)
    if rlen == 0 or n < 17:
        return (ZERO if rlen == 0 else _fail(zgpu.SEEKTAB_NONE)), n
    nf, desc, magic = struct.unpack_from("<IBI", entry, n - 9)
    if magic != SEEK_MAGIC:
        return _fail(zgpu.SEEKTAB_NONE), n - 9
    if desc & 0x7C:
        return _fail(zgpu.SEEKTAB_RESERVED_BITS), n - 9
    es = 12 if desc & 0x80 else 8
    if nf > MAX_FRAMES or nf * es + 17 > n:
        return _fail(zgpu.SEEKTAB_TOO_LARGE), n - 9
    tab = n - (nf * es + 17)
    if struct.unpack_from("<II", entry, tab) != (SKIP_MAGIC, nf * es + 9):
        return _fail(zgpu.SEEKTAB_BAD_FRAME), tab
    end = min(begin + rlen, U64)
    c_at = d_at = 0
    first = last = None
    for k in range(nf):
        c, d = struct.unpack_from("<II", entry, tab + 8 + k * es)
        if first is None and d_at + d > begin:
            first, c_lo, d_lo = k, c_at, d_at
        c_at, d_at = c_at + c, d_at + d
        if first is not None and d_at >= end:
            last = k
            break
    if first is None:
        rec = (c_at, c_at, d_at, 0, d_at, 0, nf, 0, 0, 0, 4)
    else:
        if last is None:
            last = nf - 1
        rec = (c_lo, c_at, d_lo, d_at - d_lo, d_at, 0, first, last - first + 1, 0, 0, 0)
    if rec[1] > tab:
        return _fail(zgpu.SEEKTAB_PAST_TABLE), tab
    return rec, tab


def boundary_ranges(dsizes):
    """(D_k - 1, 2), (D_k, 1), (D_k + 1, 1) at every boundary, the whole plaintext, a saturating range, ranges behind the end, a range of
    length 0 — and, where there are that many frames, a range whose first and last frame lie in different steps of 64 table entries."""
    out, at = [], 0
    for d in list(dsizes) + [0]:
        if at:
            out.append((at - 1, 2))
        out += [(at, 1), (at + 1, 1)]
        at += d
    total = at
    out += [(0, total), (0, U64), (total // 2, U64), (U64, 7), (total, 1), (total + 5, 3), (5, 0), (total, 0)]
    if len(dsizes) > 70:
        a, b = sum(dsizes[:10]), sum(dsizes[:len(dsizes) - 3])
        out += [(a, b - a), (a + 1, b - a + 1)]
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq
