"""The model of a record batch (include/zgpu.h: "record batches"), for the CPU suite of its layout function (test_recbatch_cpu) and the GPU
suite of the call (test_gpu_records_batch). Written from the header's definitions; nothing here comes from the code under test. A row is
(status, begin, len) as the lookup leaves it — tests/records.py's find, or a status the test knows —, and the batch is plain Python integers
and bytes."""
import records

PADDED, PACKED = 0, 1
U64 = (1 << 64) - 1
TOO_SMALL, BAD_ARG = 12, 93


def plan(lens, layout, width, truncate):
    """(rows, total, truncated) with rows[j] = (at, slot, want), or None where a product or a sum passes 2^64 - 1"""
    rows, at, cut = [], 0, 0
    if layout == PADDED and len(lens) * width > U64:
        return None
    for n in lens:
        want = min(n, width) if truncate and width > 0 else n
        cut += want != n
        slot = width if layout == PADDED else want
        rows.append((at, slot, want))
        at += slot
        if at > U64:
            return None
    return rows, at, cut


def lookup(models, recs):
    """recs[j] = (entry, first, count[, flags]) looked up in models[entry] = (O, open_tail) or a status (an entry the index refused, an
    entry without records); an entry out of range or unknown flags: BAD_ARG. Returns [(status, entry, begin, len)]"""
    out = []
    for r in recs:
        e, flags = r[0], r[3] if len(r) > 3 else 0
        if e >= len(models) or flags & ~records.STRIP:
            out.append((BAD_ARG, e, 0, 0))
        elif isinstance(models[e], int):
            out.append((models[e], e, 0, 0))
        else:
            O, tail = models[e]
            out.append((0, e) + records.find(O, tail, r[1], r[2], flags))
    return out


class Batch:
    """what the call must leave for the looked-up rows `found` over plaintexts plains[entry]: total, image (bytes of [0, total)), lengths,
    offsets (m + 1), record_bytes, statuses, truncated. failed: {row: status} the test knows of (a group that fails to decode, a checksum
    verdict): such a row is all pad and has length 0."""

    def __init__(self, plains, found, layout, width=0, pad=0, truncate=False, failed=None):
        failed = failed or {}
        self.record_bytes = [0 if st else n for st, _, _, n in found]
        self.rows, self.total, self.truncated = plan(self.record_bytes, layout, width, truncate)
        self.statuses, self.lengths, img = [], [], bytearray([pad]) * self.total
        for j, ((st, e, b, n), (at, slot, want)) in enumerate(zip(found, self.rows)):
            st = st or failed.get(j, 0) or (TOO_SMALL if want > slot else 0)
            self.statuses.append(st)
            self.lengths.append(0 if st else want)
            if not st:
                img[at:at + want] = plains[e][b:b + want]
        self.image = bytes(img)
        self.offsets = [at for at, _, _ in self.rows] + [self.total]
        self.ok = sum(1 for s in self.statuses if not s)
        self.filled = self.total - sum(self.lengths)
