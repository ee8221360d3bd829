"""Many ranges over few seekable entries (zgpu_frames_seek_table_many_device, zgpu_gather_ranges_seek_table_device_src): a model in plain Python
of how ranges form groups and of the order of a range's verdicts, written from the contract's text (include/zgpu.h), not from zg_ranges.cpp.
tests/test_seekmany_cpu.py checks it against hand-written cases and holds the C++ grouping (zg_seekmany.h: group_ranges) against it; tests/test_gpu_gather_ranges.py takes its expectations from it."""
import zgpu

E_TARGET_TOO_SMALL = zgpu.E_TARGET_TOO_SMALL
RANK1 = "decode"          # the group's decode or walk error, or E_CONTENT_SIZE_MISMATCH


def prefixes(csizes, dsizes):
    """(C, D): the exclusive prefix sums C[k], D[k], k = 0 .. n, of a table's compressed and decompressed sizes"""
    C, D = [0], [0]
    for c, d in zip(csizes, dsizes):
        C.append(C[-1] + c)
        D.append(D[-1] + d)
    return C, D


def groups(ranges, seeks):
    """ranges[j] = (entry, begin, len); seeks[j]: range j's record (anything with .status, .frames_skipped, .frames_taken). Only ranges of
    nonzero length with status 0 and frames_taken > 0 are in a group; ranges of one entry whose row intervals [frames_skipped, frames_skipped +
    frames_taken) share a row are in one group, transitively. Returns (groups, group_of): groups = [(entry, gfirst, glast, [j ...])] sorted by
    (entry, gfirst), members in input order; group_of[j] = the index of range j's group, or None."""
    per_entry = {}
    for j, (r, s) in enumerate(zip(ranges, seeks)):
        if r[2] and s.status == 0 and s.frames_taken > 0:
            per_entry.setdefault(r[0], []).append((s.frames_skipped, s.frames_skipped + s.frames_taken - 1, j))
    out, group_of = [], [None] * len(ranges)
    for entry in sorted(per_entry):
        cur = None
        for first, last, j in sorted(per_entry[entry]):
            if cur is None or first > cur[2]:
                cur = [entry, first, last, [j]]
                out.append(cur)
            else:
                cur[2] = max(cur[2], last)
                cur[3].append(j)
            group_of[j] = len(out) - 1
    return [(e, a, b, sorted(m)) for e, a, b, m in out], group_of


def clipped(begin, length, d_lo, d_hi):
    """what of plaintext [begin, begin + length) a group that decoded [d_lo, d_hi) of its entry delivers"""
    lo, hi = max(begin, d_lo), min(begin + length, d_hi)
    return max(hi - lo, 0)


def verdict(decode=0, small=False, checksum=0, table=0):
    """The status of a range, in the rank order of the contract: (1) its group's decode or walk error or E_CONTENT_SIZE_MISMATCH, (2)
    E_TARGET_TOO_SMALL by the range's own count against its own capacity, (3) the group's E_CHECKSUM_MISMATCH, (4) the group's
    E_SEEK_CHECKSUM_MISMATCH."""
    if decode:
        return decode
    if small:
        return E_TARGET_TOO_SMALL
    if checksum:
        return checksum
    return table


def work(grps, is_frame, dsizes):
    """(frames, bytes) a call decodes for these groups of ONE entry's table: every group once — the rows of [gfirst, glast] that are zstd
    frames (is_frame[k]) and the plaintext the table promises for them"""
    frames = sum(sum(1 for k in range(a, b + 1) if is_frame[k]) for _, a, b, _ in grps)
    nbytes = sum(sum(dsizes[a:b + 1]) for _, a, b, _ in grps)
    return frames, nbytes
