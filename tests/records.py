"""The model of the record index (include/zgpu.h: "record index"; zstd-rs_amd/csrc/zg_records.h), for the CPU suite of its kernels
(test_records_cpu, test_recshapes_cpu) and the GPU suites of its calls (test_gpu_seek_index_records, test_gpu_recshapes). Nothing here comes from the code under test: a record
offset is numpy.flatnonzero(plain == d) + 1, with O[0] = 0 in front and, for an open tail, O[R] = L behind."""
import numpy as np

CHUNK = 4096            # zgr::kChunk
STRIP = 1               # ZGPU_RECORDS_STRIP
U64 = (1 << 64) - 1


def delimiters(plain, d):
    """the positions just behind every byte of plain equal to d, as a list of ints"""
    return (np.flatnonzero(np.frombuffer(bytes(plain), dtype=np.uint8) == d) + 1).tolist()


def offsets(plain, d):
    """(O, open_tail): O[0 .. R] of plaintext `plain` under delimiter d"""
    L, found = len(plain), delimiters(plain, d)
    open_tail = L > 0 and (not found or found[-1] != L)
    return [0] + found + ([L] if open_tail else []), open_tail


def find(O, open_tail, first, count, flags=0):
    """(begin, len) of records [first, first + count) clipped to the R = len(O) - 1 the entry has"""
    R = len(O) - 1
    a, b = min(first, R), min(min(first + count, U64), R)
    if a >= b:
        return O[a], 0
    n = O[b] - O[a]
    if flags & STRIP and not (b == R and open_tail):
        n -= 1
    return O[a], n


def chunks(frames):
    """the chunk table of frames = [(out_off, size, base)]: ([(out_off, base, len, frame)], fstart)"""
    out, fstart = [], []
    for f, (off, size, base) in enumerate(frames):
        fstart.append(len(out))
        for at in range(0, size, CHUNK):
            out.append((off + at, base + at, min(CHUNK, size - at), f))
    return out, fstart + [len(out)]


def expected(buf, frames, d):
    """what the three kernels leave for frames = [(out_off, size, base)] of the output buf: (counts per chunk, prefixes, totals, staging)"""
    table, _ = chunks(frames)
    counts = [len(delimiters(buf[o:o + n], d)) for o, _, n, _ in table]
    prefix, at = [], 0
    for c in counts:
        prefix.append(at)
        at += c
    staging, ftot = [], []
    for off, size, base in frames:
        found = [base + p for p in delimiters(buf[off:off + size], d)]
        ftot.append(len(found))
        staging += found
    return counts, prefix, [at] + ftot, staging


def scan(counts, fstart):
    """what zg_k_recs_scan leaves for the chunks' counts and the frames' first chunks fstart[0 .. nframes]: (prefixes, total, frame totals),
    in plain Python integers — prefix[i] = counts[0] + ... + counts[i - 1], P(nchunks) = the total, a frame's total P(fstart[f + 1]) - P(fstart[f])"""
    prefix, at = [], 0
    for c in counts:
        prefix.append(at)
        at += int(c)
    P = prefix + [at]
    return prefix, at, [P[fstart[f + 1]] - P[fstart[f]] for f in range(len(fstart) - 1)]
