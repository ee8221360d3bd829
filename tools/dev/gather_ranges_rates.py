"""What many records out of one seekable shard cost, with the gather call and with the single-range call (LABNOTES.md "gather_ranges").

  python tools/dev/gather_ranges_rates.py --mode new|old [--package DIR] [--frames 4096] [--records 4096] [--calls 10]

One shard of --frames frames x 64 KiB of text_like (16 distinct texts in turn), undeclared sizes, a seek table with checksums, in one torch
tensor. m = --records records of 1 KiB are read twice: at random offsets over the whole shard ("uniform"), and 16 per frame in m / 16 random
frames ("dense").
  new: Context.gather_ranges_seek_table_device_src — one entry, m ranges.
  old: Context.decode_ranges_seek_table_device_src with the shard's pointer repeated m times.
--package DIR: import zgpu (and load libzgpu.so) from DIR instead of this tree — the baseline is the PARENT commit's build, which has only
the old call. Two warm-up calls, then the median of --calls calls: wall time of the call, the selection kernels' time from the call's
statistics (old: zg_k_seektab; new: locate + the two prefix launches + find), frames decoded, submits. sha256 of all destinations is printed
so that the two modes can be compared before their times are.

  python tools/dev/gather_ranges_rates.py --mode new|old --table-rows 1048576

The selection alone on a table of that many rows over filler bytes, one range at the table's end: old is one zg_k_seektab wave that scans
the table to its end, new the locate pass, the prefix build and one find lane. Prints one JSON object."""
import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("new", "old"), required=True)
    ap.add_argument("--package", default=os.path.join(ROOT, "zstd-rs_amd"))
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--table-rows", type=int, default=0)
    a = ap.parse_args()
    sys.path[:0] = [a.package, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import torch      # noqa: F401  (before the library is loaded: one HIP runtime)
    import zgpu
    import zgdata
    from devmem import xxh32
    ctx = zgpu.Context(0)
    out = {"mode": a.mode, "package": os.path.relpath(a.package, ROOT)}

    def selection_us(st):
        return st["seek_us"] + st.get("prefix_us", 0) + st.get("find_us", 0)

    def stats():
        return ctx.gather_ranges_stats() if a.mode == "new" else ctx.ranges_stats()

    if a.table_rows:
        rng = random.Random(0x7AB1E)
        nf = a.table_rows
        cs, ds = [rng.randint(0, 3) for _ in range(nf)], [rng.randint(1, 65536) for _ in range(nf)]
        z = bytes(sum(cs)) + zgpu.seek_table_frame(cs, ds)
        src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        rg = (sum(ds) - 1, 1)
        us, keys = [], set()
        for _ in range(2 + a.calls):
            if a.mode == "new":
                k = ctx.frames_seek_table_many_device([src.data_ptr()], [len(z)], [(0,) + rg])[0]
            else:
                k = ctx.frames_seek_table_device([src.data_ptr()], [len(z)], [rg])[0]
            st = stats()
            us.append((selection_us(st), st["seek_us"], st.get("prefix_us", 0), st.get("find_us", 0)))
            keys.add(k.key())
        assert len(keys) == 1 and k.frames_skipped == nf - 1 and k.status == 0, keys
        med = sorted(us[2:])[len(us[2:]) // 2]
        out.update(table_rows=nf, record=list(keys)[0], selection_us=med[0], seek_or_locate_us=med[1], prefix_us=med[2], find_us=med[3])
        print(json.dumps(out))
        return

    size, nf, m = 64 << 10, a.frames, a.records
    texts = [zgdata.text_like(size, seed=0x6A00 + k) for k in range(16)]
    comp = [zgdata.zstd_compress(t, checksum=False, content_size=False) for t in texts]
    sums = [xxh32(t) for t in texts]
    z = b"".join(comp[k % 16] for k in range(nf)) + zgpu.seek_table_frame([len(comp[k % 16]) for k in range(nf)], [size] * nf,
                                                                          [sums[k % 16] for k in range(nf)])
    src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
    rng = random.Random(0x6A7E)
    rec = 1 << 10
    workloads = {
        "uniform": [(rng.randrange(nf * size - rec), rec) for _ in range(m)],
        "dense": [(f * size + rng.randrange(size - rec), rec) for f in rng.sample(range(nf), max(m // 16, 1)) for _ in range(16)][:m],
    }
    for name, rgs in workloads.items():
        n = len(rgs)
        dst = torch.zeros(n * rec, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptrs, caps = [dst.data_ptr() + j * rec for j in range(n)], [rec] * n
        wall, sel, frames, submits = [], [], 0, 0
        for _ in range(2 + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if a.mode == "new":
                res, _ = ctx.gather_ranges_seek_table_device_src([src.data_ptr()], [len(z)], [(0, b, ln) for b, ln in rgs], ptrs, caps)
            else:
                res, _ = ctx.decode_ranges_seek_table_device_src([src.data_ptr()] * n, [len(z)] * n, rgs, ptrs, caps)
            wall.append((time.perf_counter() - t0) * 1e3)
            st = stats()
            sel.append(selection_us(st))
            frames, submits = st["frames_decoded"], ctx.frames_submits()
            assert all(r.status == 0 and r.written == rec for r in res)
        got = dst.cpu().numpy().tobytes()
        want = b"".join(texts[(b // size) % 16][b % size:b % size + ln] if b % size + ln <= size else
                        (texts[(b // size) % 16] + texts[(b // size + 1) % 16])[b % size:b % size + ln] for b, ln in rgs)
        assert got == want, name
        out[name] = {"records": n, "wall_ms_median": round(statistics.median(wall[2:]), 3), "wall_ms_min": round(min(wall[2:]), 3),
                     "selection_us_median": statistics.median(sel[2:]), "frames_decoded": frames, "submits": submits,
                     "sha256": hashlib.sha256(got).hexdigest()[:16]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
