"""What a record batch costs beside the gather into m separate destinations (LABNOTES.md "records_batch").

  python tools/dev/records_batch_rates.py --mode gather|padded|packed|torchfill [--frames 4096] [--size 65536] [--records 4096] [--calls 10]
                                          [--tree DIR] [--fill-bytes N]

The shards of seek_records_rates.py: --frames frames x --size bytes of text_like (16 distinct texts in turn) that declare their sizes, in one
torch tensor, indexed once (kind declared) with its record offsets. m = --records single records at random numbers (the same numbers in
every mode). ONE process is ONE measurement; run every invocation under a timeout of its own. Two warm-up calls, then the median of --calls
calls. Prints one JSON object.
  gather:    gather_records_indexed_device_src into m destinations back to back in one tensor, as a caller of that call lays them out. --tree
             DIR: import zgpu from DIR/zstd-rs_amd — a checkout of the parent commit with its own library.
  padded:    gather_records_batch, layout padded, at a width that holds the longest of the m records.
  packed:    gather_records_batch, layout packed, the size known from one query outside the timed calls.
  torchfill: tensor.fill_ of --fill-bytes bytes by torch (HIP events): what the fill kernel's rate is held against.
Every mode but torchfill reports the wall time of the Python method and, inside it, of the C function alone: the difference is the Python
side — where the m pointers and capacities are marshalled. padded and packed also report the fill kernel's microseconds (HIP events), the
bytes it filled and the bytes uploaded into the two arrays. The outputs are compared with the plaintext first."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    return statistics.median(xs[2:])


class TimedLib:
    """the library with one function's calls timed"""

    def __init__(self, lib, name):
        self._lib, self._name, self.ms = lib, name, []

    def __getattr__(self, k):
        f = getattr(self._lib, k)
        if k != self._name:
            return f

        def timed(*a):
            t0 = time.perf_counter()
            r = f(*a)
            self.ms.append((time.perf_counter() - t0) * 1e3)
            return r
        return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("gather", "padded", "packed", "torchfill"), required=True)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64 << 10)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--fill-bytes", type=int, default=1 << 20)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(a.tree, "zstd-rs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import numpy as np
    import torch      # noqa: F401  (before the library is loaded: one HIP runtime)
    import zgdata
    size, nf, m = a.size, a.frames, a.records
    out = {"mode": a.mode, "frames": nf, "frame_bytes": size, "tree": os.path.relpath(a.tree, ROOT)}
    if a.mode == "torchfill":
        t = torch.empty(max(a.fill_bytes, 1), dtype=torch.uint8, device="cuda:0")
        us = []
        for _ in range(2 + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.fill_(0xEE)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out.update(fill_bytes=a.fill_bytes, fill_us_median=round(med(us), 1), fill_GBps=round(a.fill_bytes / med(us) / 1e3, 2))
        print(json.dumps(out))
        return
    import zgpu
    ctx = zgpu.Context(0)
    texts = [zgdata.text_like(size, seed=0x6A00 + k) for k in range(16)]
    comp = [zgdata.zstd_compress(t, checksum=False, content_size=True) for t in texts]
    z = b"".join(comp[k % 16] for k in range(nf))
    src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ptrs, lens = [src.data_ptr()], [len(z)]
    per = [np.flatnonzero(np.frombuffer(t, dtype=np.uint8) == 10) + 1 for t in texts]
    found = np.concatenate([per[k % 16] + k * size for k in range(nf)])
    L = nf * size
    O = np.concatenate([[0], found, [L] if (not len(found) or found[-1] != L) else []]).astype(np.uint64)
    R = len(O) - 1
    ix = ctx.seek_index(ptrs, lens, kind="declared")
    assert ix.infos[0].status == 0 and ix.infos[0].plaintext == L
    ix.records(ptrs, lens)
    rng = random.Random(0x6A7E)
    nums = [rng.randrange(R) for _ in range(m)]
    ranges = [(int(O[r]), int(O[r + 1] - O[r])) for r in nums]
    caps = [n for _, n in ranges]
    recs = [(0, r, 1) for r in nums]
    plain = b"".join(texts[k % 16] for k in range(nf))
    want = [plain[b:b + n] for b, n in ranges]
    width = max(caps)
    total = {"gather": sum(caps), "packed": sum(caps), "padded": m * width}[a.mode]
    dst = torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda:0")
    arrays = torch.zeros(2 * m + 1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    fn = "zgpu_gather_records_indexed_device_src" if a.mode == "gather" else "zgpu_gather_records_batch_indexed_device_src"
    ctx.L = lib = TimedLib(ctx.L, fn)
    wall, fill_us, st = [], [], {}
    for _ in range(2 + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.mode == "gather":      # what a caller of this call does per step: m pointers and m capacities
            offs, at = [], 0
            for cp in caps:
                offs.append(at)
                at += cp
            base = dst.data_ptr()
            res, _ = ctx.gather_records_indexed_device_src(ix, ptrs, lens, recs, [base + o for o in offs], caps)
        else:
            res, _, info, _ = ctx.gather_records_batch(ix, ptrs, lens, recs, dst.data_ptr(), total, layout=a.mode, width=width if a.mode == "padded" else 0,
                                                       pad=0xEE, lengths_ptr=arrays.data_ptr(), offsets_ptr=arrays.data_ptr() + 8 * m)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert all(r.status == 0 and r.written == n for r, n in zip(res, caps))
        if a.mode != "gather":
            st = ctx.gather_records_stats()
            fill_us.append(st["batch_fill_us"])
    got = dst.cpu().numpy().tobytes()[:total]
    if a.mode == "padded":
        assert got == b"".join(w + b"\xEE" * (width - len(w)) for w in want)
    else:
        assert got == b"".join(want)
    c_ms = lib.ms
    out.update(records=m, bytes_gathered=sum(caps), batch_bytes=total, width=width if a.mode == "padded" else 0,
               wall_ms_median=round(med(wall), 3), wall_ms_min=round(min(wall[2:]), 3), c_call_ms_median=round(med(c_ms), 3),
               python_side_ms_median=round(med([w - c for w, c in zip(wall, c_ms)]), 3), frames_decoded=ctx.gather_ranges_stats()["frames_decoded"])
    if a.mode != "gather":
        f = med(fill_us)
        out.update(fill_us_median=f, bytes_filled=st["batch_bytes_filled"], bytes_uploaded=st["batch_bytes_uploaded"],
                   fill_GBps=round(st["batch_bytes_filled"] / f / 1e3, 2) if f else None)
    print(json.dumps(out))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
