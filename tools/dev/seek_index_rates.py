"""What a seek index costs to build and what it saves per gather call (LABNOTES.md "seek_index").

  python tools/dev/seek_index_rates.py --mode build --kind declared|seek_table [--frames 4096] [--size 65536] [--calls 10]
  python tools/dev/seek_index_rates.py --mode gather --kind declared|seek_table|none|chain [--frames 4096] [--size 65536] [--records 4096]

One shard of --frames frames x --size bytes of text_like (16 distinct texts in turn) in one torch tensor: frames that declare their sizes
(declared, chain), or undeclared sizes behind a seek table (seek_table, none). ONE process is ONE measurement; run every invocation under a
timeout of its own. Two warm-up calls, then the median of --calls calls. Prints one JSON object.
  build:  Context.seek_index of that kind, built and closed per call: wall time and the build's kernel time (HIP events) from
          SeekIndex.stats(). declared: beside it the kernel time of the summary pass alone (frames_index_device: zg_k_index<false>) and of
          frames_table_device (summary + zg_k_index<true>), so that build - summary is zg_k_seekidx_rows and table - summary is
          zg_k_index<true> on the same shard. seek_table: beside it the locate + prefix time of one frames_seek_table_many_device call.
  gather: m = --records records of 1 KiB at random offsets over the whole shard, per call:
          declared / seek_table: gather_ranges_indexed_device_src on an index built once outside the loop;
          none:  gather_ranges_seek_table_device_src (the table scanned in every call);
          chain: decode_ranges_device_src with the shard's pointer repeated m times (the header chain walked from the front for every range).
          Wall time, the selection kernels' time, frames decoded; the outputs are compared with the plaintext first."""
import argparse
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    return statistics.median(xs[2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("build", "gather"), required=True)
    ap.add_argument("--kind", choices=("declared", "seek_table", "none", "chain"), required=True)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64 << 10)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "zstd-rs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import torch      # noqa: F401  (before the library is loaded: one HIP runtime)
    import zgpu
    import zgdata
    ctx = zgpu.Context(0)
    size, nf, m = a.size, a.frames, a.records
    sized = a.kind in ("declared", "chain")
    texts = [zgdata.text_like(size, seed=0x6A00 + k) for k in range(16)]
    comp = [zgdata.zstd_compress(t, checksum=False, content_size=sized) for t in texts]
    z = b"".join(comp[k % 16] for k in range(nf))
    if not sized:
        z += zgpu.seek_table_frame([len(comp[k % 16]) for k in range(nf)], [size] * nf)
    src = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    ptrs, lens = [src.data_ptr()], [len(z)]
    out = {"mode": a.mode, "kind": a.kind, "frames": nf, "frame_bytes": size, "shard_bytes": len(z)}

    if a.mode == "build":
        if a.kind not in ("declared", "seek_table"):
            ap.error("--mode build needs --kind declared or seek_table")
        wall, kus, other, other2 = [], [], [], []
        for _ in range(2 + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix = ctx.seek_index(ptrs, lens, kind=a.kind)
            wall.append((time.perf_counter() - t0) * 1e3)
            st, info = ix.stats(), ix.infos[0]
            ix.close()
            assert info.status == 0 and info.nrows == nf and info.plaintext == nf * size and st["input_bytes_to_host"] == 0, (info, st)
            kus.append(st["kernel_us"])
            if a.kind == "declared":
                ctx.frames_index_device(ptrs, lens)
                other.append(ctx.frames_index_stats()["kernel_us"])
                ctx.frames_table_device(ptrs, lens)
                other2.append(ctx.frames_index_stats()["kernel_us"])
            else:
                ctx.frames_seek_table_many_device(ptrs, lens, [(0, 0, 1)])
                g = ctx.gather_ranges_stats()
                other.append(g["seek_us"] + g["prefix_us"])
        out.update(wall_ms_median=round(med(wall), 3), build_kernel_us=med(kus), launches=st["launches"], device_bytes=st["device_bytes"],
                   bytes_downloaded=st["bytes_downloaded"])
        if a.kind == "declared":
            summary, table = med(other), med(other2)
            out.update(summary_us=summary, rows_us=med(kus) - summary, rows_ns_per_frame=round(1e3 * (med(kus) - summary) / nf, 2),
                       index_emit_us=table - summary, index_emit_ns_per_frame=round(1e3 * (table - summary) / nf, 2))
        else:
            out.update(locate_prefix_us_of_the_many_call=med(other), ns_per_row=round(1e3 * med(kus) / nf, 2))
        print(json.dumps(out))
        return

    rng = random.Random(0x6A7E)
    rec = 1 << 10
    rgs = [(rng.randrange(nf * size - rec), rec) for _ in range(m)]
    dst = torch.zeros(m * rec, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dptrs, caps = [dst.data_ptr() + j * rec for j in range(m)], [rec] * m
    many = [(0, b, ln) for b, ln in rgs]
    ix = ctx.seek_index(ptrs, lens, kind=a.kind) if a.kind in ("declared", "seek_table") else None
    wall, sel, frames = [], [], 0
    for _ in range(2 + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if ix is not None:
            res, _ = ctx.gather_ranges_indexed_device_src(ix, ptrs, lens, many, dptrs, caps)
        elif a.kind == "none":
            res, _ = ctx.gather_ranges_seek_table_device_src(ptrs, lens, many, dptrs, caps)
        else:
            res, _ = ctx.decode_ranges_device_src(ptrs * m, lens * m, rgs, dptrs, caps)
        wall.append((time.perf_counter() - t0) * 1e3)
        st = ctx.gather_ranges_stats()
        sel.append(st["seek_us"] + st.get("prefix_us", 0) + st.get("find_us", 0))
        frames = st["frames_decoded"]
        assert all(r.status == 0 and r.written == rec for r in res)
    got = dst.cpu().numpy().tobytes()
    want = b"".join((texts[(b // size) % 16] + texts[(b // size + 1) % 16])[b % size:b % size + ln] for b, ln in rgs)
    assert got == want
    out.update(records=m, wall_ms_median=round(med(wall), 3), wall_ms_min=round(min(wall[2:]), 3), selection_us_median=med(sel),
               frames_decoded=frames, submits=ctx.frames_submits(), sha256=hashlib.sha256(got).hexdigest()[:16])
    if ix is not None:
        out.update(index_device_bytes=ix.device_bytes, index_build_kernel_us=ix.stats()["kernel_us"])
        ix.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
