"""Seek index handles (zgpu_seek_index, zstd-rs_amd/csrc/zg_seekidx.h): a model in plain Python of an entry's rows, their prefix sums and the
record a range gets from them, written from the contract's text (include/zgpu.h) and the zstd format, not from the lane routine.
tests/test_seekidx_cpu.py holds the emulated passes to it; tests/test_gpu_seek_index.py takes its row expectations from it."""
import struct

U64 = 2 ** 64 - 1
CHAIN_SHORT_HEADER, CHAIN_BAD_MAGIC, CHAIN_SKIP_PAST_END, CHAIN_SHORT_BLOCK_HEADER = 1, 2, 3, 4
CHAIN_RESERVED_BLOCK, CHAIN_BLOCK_TOO_LARGE, CHAIN_BODY_PAST_END, CHAIN_SHORT_CHECKSUM = 5, 6, 7, 8
INDEX_UNSIZED = 32
BLOCK_MAX = 128 << 10


def rows(z):
    """(rows, why, bodies): rows = [(c_k, d_k)] of the frame records of z's header chain that the chain read to their end — a zstd frame with
    d_k = its declared Frame_Content_Size (None: it declares none), a skippable frame with d_k = 0; why = the CHAIN_* reason the chain broke
    with (the broken frame is no row), 0 if it reached the end; bodies = [(lo, hi)], the bytes of block bodies the chain passed over."""
    out, bodies, p, n = [], [], 0, len(z)
    while p < n:
        begin = p
        if n - p < 4:
            return out, CHAIN_SHORT_HEADER, bodies
        magic = struct.unpack_from("<I", z, p)[0]
        if 0x184D2A50 <= magic <= 0x184D2A5F:
            if n - p < 8:
                return out, CHAIN_SHORT_HEADER, bodies
            sl = struct.unpack_from("<I", z, p + 4)[0]
            p += 8
            if sl > n - p:
                return out, CHAIN_SKIP_PAST_END, bodies
            p += sl
            out.append((p - begin, 0))
            continue
        if magic != 0xFD2FB528:
            return out, CHAIN_BAD_MAGIC, bodies
        if n - p < 5:
            return out, CHAIN_SHORT_HEADER, bodies
        d = z[p + 4]
        single, did, fc = (d >> 5) & 1, d & 3, d >> 6
        fl = [single, 2, 4, 8][fc]
        hs = 5 + (0 if single else 1) + [0, 1, 2, 4][did] + fl
        if n - p < hs:
            return out, CHAIN_SHORT_HEADER, bodies
        fcs = None
        if fl:
            fcs = int.from_bytes(z[p + hs - fl:p + hs], "little") + (256 if fl == 2 else 0)
        p += hs
        while True:
            if n - p < 3:
                return out, CHAIN_SHORT_BLOCK_HEADER, bodies
            h = int.from_bytes(z[p:p + 3], "little")
            last, btype, size = h & 1, (h >> 1) & 3, h >> 3
            if btype == 3:
                return out, CHAIN_RESERVED_BLOCK, bodies
            if size > BLOCK_MAX:
                return out, CHAIN_BLOCK_TOO_LARGE, bodies
            content = 1 if btype == 1 else size
            if n - (p + 3) < content:
                return out, CHAIN_BODY_PAST_END, bodies
            bodies.append((p + 3, p + 3 + content))
            p += 3 + content
            if last:
                break
        if d & 4:
            if n - p < 4:
                return out, CHAIN_SHORT_CHECKSUM, bodies
            p += 4
        out.append((p - begin, fcs))
    return out, 0, bodies


def index(z):
    """(why, C, D) of the declared-kind index of entry z: why = 0 and the exclusive prefix sums C[k], D[k], k = 0 .. nrows (D saturates), or
    the refusal — the CHAIN_* reason, INDEX_UNSIZED — and None, None"""
    rw, why, _ = rows(z)
    if why:
        return why, None, None
    if any(d is None for _, d in rw):
        return INDEX_UNSIZED, None, None
    C, D = [0], [0]
    for c, d in rw:
        C.append(C[-1] + c)
        D.append(min(D[-1] + d, U64))
    return 0, C, D


def record(C, D, tab, begin, rlen):
    """the rule of zg_seektab.h on the rows: (src_lo, src_hi, plain_lo, bound, plain_seen, status, frames_skipped, frames_taken, nblocks, why, flags)"""
    if not rlen:
        return (0,) * 11
    end = min(begin + rlen, U64)
    nf = len(C) - 1
    first = next((k for k in range(nf) if D[k + 1] > begin), None)
    if first is None:
        if C[nf] > tab:
            return (0,) * 5 + (72, 0, 0, 0, 20, 0)
        return (C[nf], C[nf], D[nf], 0, D[nf], 0, nf, 0, 0, 0, 4)
    last = next((k for k in range(first, nf) if D[k + 1] >= end), nf - 1)
    if C[last + 1] > tab:
        return (0,) * 5 + (72, 0, 0, 0, 20, 0)
    return (C[first], C[last + 1], D[first], D[last + 1] - D[first], D[last + 1], 0, first, last - first + 1, 0, 0, 0)


def boundary_ranges(D):
    """every row boundary -1, +0, +1, a length of 0, ranges that saturate and ranges behind the plaintext"""
    total = D[-1]
    out = []
    for at in sorted(set(D)):
        for b in (at - 1, at, at + 1):
            if b >= 0:
                out += [(b, 1), (b, 2)]
        nxt = min((x for x in D if x > at), default=at)
        out += [(at, nxt - at), (at, nxt - at + 1)] + ([(at - 1, nxt - at + 2)] if at else [])
    out += [(0, total), (0, U64), (total // 2, U64), (U64, 7), (U64 - 3, U64), (1, U64 - 1), (total, 1), (total + 5, 3), (5, 0), (total, 0),
            (0, 0)]
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq
