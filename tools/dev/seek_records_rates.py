"""What the record index costs to build and what a gather by record number costs over a gather by bytes (LABNOTES.md "seek_index_records").

  python tools/dev/seek_records_rates.py --mode pass|hash|gather|bytes|copy [--frames 4096] [--size 65536] [--records 4096] [--calls 10] [--tree DIR]

The shards of seek_index_rates.py: --frames frames x --size bytes of text_like (16 distinct texts in turn) that declare their sizes, in one
torch tensor, indexed once (kind declared). ONE process is ONE measurement; run every invocation under a timeout of its own. Two warm-up
calls, then the median of --calls calls. Prints one JSON object. --tree DIR: import zgpu from DIR/zstd-rs_amd — a checkout of the parent
commit with its own library, for the modes the parent has (hash, bytes): both passes decode everything once, so pass - hash is the side pass.
  pass:   SeekIndex.records (delimiter newline): wall time, the side kernels' microseconds (count + scan + emit, HIP events), chunks, bytes
          back; the count and emit kernels' rate = 2 x plaintext / their time (each streams the plaintext once; the scan reads 4 bytes a
          chunk). The offsets are compared with numpy.flatnonzero(plain == 10) + 1 first.
  hash:   SeekIndex.hash: wall time and the hash kernels' microseconds (zgpu_seek_index_stats [10]).
  gather: m = --records single-record gathers at random record numbers, gather_records_indexed_device_src; the lookup's microseconds and
          bytes back. The outputs are compared with the plaintext first.
  bytes:  gather_ranges_indexed_device_src on the same byte ranges (the model's).
  copy:   a device-to-device copy of the shard's plaintext size by torch (HIP events): the rate the streams are held against."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("pass", "hash", "gather", "bytes", "copy"), required=True)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64 << 10)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(a.tree, "zstd-rs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import numpy as np
    import torch      # noqa: F401  (before the library is loaded: one HIP runtime)
    import zgdata
    size, nf, m = a.size, a.frames, a.records
    out = {"mode": a.mode, "frames": nf, "frame_bytes": size, "plaintext_bytes": nf * size, "tree": os.path.relpath(a.tree, ROOT)}
    if a.mode == "copy":
        src = torch.zeros(nf * size, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        us = []
        for _ in range(2 + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        out.update(copy_us_median=round(med(us), 1), copy_GBps_read_plus_write=round(2 * nf * size / med(us) / 1e3, 1))
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
    # the model: every text's newline positions, shifted to where the text lies in the shard
    per = [np.flatnonzero(np.frombuffer(t, dtype=np.uint8) == 10) + 1 for t in texts]
    found = np.concatenate([per[k % 16] + k * size for k in range(nf)])
    L = nf * size
    O = np.concatenate([[0], found, [L] if (not len(found) or found[-1] != L) else []]).astype(np.uint64)
    R = len(O) - 1
    ix = ctx.seek_index(ptrs, lens, kind="declared")
    assert ix.infos[0].status == 0 and ix.infos[0].plaintext == L
    out.update(shard_bytes=len(z), records_in_shard=int(R))

    if a.mode in ("pass", "hash"):
        wall, kus, last = [], [], None
        for _ in range(2 + a.calls):
            before = ix.records_stats() if a.mode == "pass" else ix.stats(sums=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = (ix.records(ptrs, lens) if a.mode == "pass" else ix.hash(ptrs, lens))[0]
            wall.append((time.perf_counter() - t0) * 1e3)
            last = ix.records_stats() if a.mode == "pass" else ix.stats(sums=True)
            assert info.status == 0 and info.state == 1, info
            kus.append(last["records_us" if a.mode == "pass" else "hash_us"] - before["records_us" if a.mode == "pass" else "hash_us"])
        if a.mode == "pass":
            got = np.array(ix.record_offsets(0), dtype=np.uint64)
            assert len(got) == len(O) and (got == O).all()
            out.update(side_kernels_us_median=med(kus), count_emit_GBps=round(2 * L / med(kus) / 1e3, 1), chunks_per_call=last["records_chunks"] // (2 + a.calls),
                       submits_per_call=last["records_submits"] // (2 + a.calls), bytes_back_per_call=last["records_bytes_downloaded"] // (2 + a.calls),
                       offset_bytes=last["records_offset_bytes"])
        else:
            out.update(hash_kernels_us_median=med(kus), hash_GBps=round(L / med(kus) / 1e3, 1), submits_per_call=last["hash_submits"] // (2 + a.calls))
        out.update(wall_ms_median=round(med(wall), 3), wall_ms_min=round(min(wall[2:]), 3))
        print(json.dumps(out))
        ix.close()
        ctx.close()
        return

    rng = random.Random(0x6A7E)
    nums = [rng.randrange(R) for _ in range(m)]
    ranges = [(0, int(O[r]), int(O[r + 1] - O[r])) for r in nums]
    caps = [n for _, _, n in ranges]
    offs = [0]
    for cp in caps:
        offs.append(offs[-1] + cp)
    dst = torch.zeros(max(offs[-1], 1), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    dptrs = [dst.data_ptr() + o for o in offs[:-1]]
    recs = [(0, r, 1) for r in nums]
    if a.mode == "gather":
        ix.records(ptrs, lens)
    wall, find_us, back = [], [], 0
    for _ in range(2 + a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.mode == "gather":
            res, _ = ctx.gather_records_indexed_device_src(ix, ptrs, lens, recs, dptrs, caps)
        else:
            res, _ = ctx.gather_ranges_indexed_device_src(ix, ptrs, lens, ranges, dptrs, caps)
        wall.append((time.perf_counter() - t0) * 1e3)
        assert all(r.status == 0 and r.written == n for r, n in zip(res, caps))
        if a.mode == "gather":
            st = ctx.gather_records_stats()
            find_us.append(st["record_find_us"])
            back = st["record_find_bytes_downloaded"]
    got = dst.cpu().numpy().tobytes()[:offs[-1]]
    plain = b"".join(texts[k % 16] for k in range(nf))   # (a record may span any number of frames)
    assert got == b"".join(plain[b:b + n] for _, b, n in ranges)
    out.update(records=m, bytes_gathered=offs[-1], wall_ms_median=round(med(wall), 3), wall_ms_min=round(min(wall[2:]), 3),
               frames_decoded=ctx.gather_ranges_stats()["frames_decoded"])
    if a.mode == "gather":
        out.update(record_find_us_median=med(find_us), record_find_bytes_back=back)
    print(json.dumps(out))
    ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
