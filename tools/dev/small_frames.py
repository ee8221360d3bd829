"""Many small independent buffers, host to host: the per-entry zgpu_decode_all loop against one zgpu_decode_frames call, and the device hash.

  python tools/dev/small_frames.py [n_frames]      (default 4096 x 128 KiB)

1. the 101 decodecorpus frames as 101 entries: loop against one call;
2. n x 128 KiB zgdata.text_like frames (zgdata.zstd_compress): the loop, one call on frames WITH a Content_Checksum, one call on the same text
   compressed WITHOUT one (the call still hashes each entry's first frame for calculated_checksum: the difference is the 4-byte field only), and
   zgpu_batch_checksums on the same frames resident on the device (the hash's own cost);
3. zg_k_xxh64 on a blocks4b-like batch (65,536 single-block 128 KiB frames, bench.py's workload): zgpu_batch_checksums wall time against the
   batch's kernel pipeline;
4. where frames are hashed: one zgpu_decode_frames call on 4096 x 128 KiB, 1024 x 512 KiB, 256 x 2 MiB and 1 x 4 MiB entries with the
   library's own choice ("auto", twice) and, in the development build (ZGPU_HASH_DEVICE_MAX), every frame on the host ("host", twice) or
   every frame on the device ("device"), in that interleaved order; and the rate of one lane alone (zgpu_batch_checksums, one 4 MiB frame).
Prints one JSON object.

  python tools/dev/small_frames.py --device [workload ...]     (default: corpus101 4096x128K 1024x512K 256x2M 128x64M)

the host call (zgpu_decode_frames) against the device call (zgpu_decode_frames_device, destinations in one torch tensor) on the same entries,
in one process and in its SECOND context (the first context of a process downloads more slowly, LABNOTES round 6): best of 5 after a warm-up
each, interleaved; the device call with its default hashing and with hashing off (the difference is the device hash's share); and the scatter
kernel's own time and bytes (zgpu_debug_frames_device_stats). ZGPU_SCATTER_CHUNK (read by the development build) sets the chunk size:
`--device --dev` loads libzgpu_dev.so. Prints one JSON object.

  python tools/dev/small_frames.py --device-src [workload ...]  (default: corpus101 4096x128K 1024x512K 256x2M 128x64M 1x1024M)

compressed input that lies in device memory (one torch tensor, entries back to back): zgpu_decode_frames_device_src against the detour a
caller takes without it — download the inputs to the host (one D2H of the tensor), then zgpu_decode_frames_device — in one process and its
second context, interleaved, best of 5 after a warm-up each; the walk's and the gather's own times and the skeleton's size
(zgpu_debug_frames_device_src_stats) beside the scatter's. 1x1024M is ONE frame of 8192 blocks: the walk lane's worst case. Prints one
JSON object.

  python tools/dev/small_frames.py --index [workload ...]       (default: corpus101 4096x128K 1x1024M)

what device-resident entries hold, without a download: zgpu_frames_index_device (one zg_k_index launch, the summary pass) and
zgpu_frames_table_device (summary pass + emit pass) on the entries in one torch tensor, kernel times from zgpu_debug_frames_index_stats (HIP
events, best of 5 after a warm-up), every bound checked against zgpu_plaintext_bound of the host copy; beside them zg_k_walk's time — count and
emit pass together — from zgpu_debug_frames_device_src_stats of a decode of the same entries. Prints one JSON object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "zstd-rs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import zgpu       # noqa: E402
import zgdata     # noqa: E402
from golden_io import read_manifest, read_pack   # noqa: E402


def best(fn, n=3):
    t = None
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        t = dt if t is None else min(t, dt)
    return t


def loop(ctx, entries, caps):
    for z, c in zip(entries, caps):
        ctx.decode_all(z, c)


def device_workload(name):
    if name == "corpus101":
        pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
        names = sorted(man)
        return [pack[n] for n in names], [man[n]["size"] for n in names]
    count, size = name.split("x")
    count, size = int(count), int(size[:-1]) << (10 if size[-1] == "K" else 20)
    d = [zgdata.text_like(size, seed=0x700 + k) for k in range(min(count, 8 if size > (8 << 20) else 16))]
    c = [zgdata.zstd_compress(t) for t in d]
    return [c[k % len(c)] for k in range(count)], [size] * count


def device_main(args):
    import torch
    dev = "--dev" in args
    names = [a for a in args if not a.startswith("--")] or ["corpus101", "4096x128K", "1024x512K", "256x2M", "128x64M"]
    first = zgpu.Context(0, dev=dev)            # (the process's first context: not the one that is measured)
    first.decode_all(zgdata.zstd_compress(b"warm" * 1000), 4000)
    ctx = zgpu.Context(0, dev=dev)
    out = {"scatter_chunk_env": os.environ.get("ZGPU_SCATTER_CHUNK") if dev else None}
    for name in names:
        ent, caps = device_workload(name)
        offs, total = [], 0
        for c in caps:
            offs.append(total)
            total += (c + 255) & ~255
        buf = torch.empty(max(total, 256), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ptrs = [buf.data_ptr() + o for o in offs]
        # (address, length) entries of memory that stays alive: neither call copies the input in Python
        keep = [zgpu.C.c_char_p(z) for z in ent]
        raw = [(zgpu.C.cast(k, zgpu.C.c_void_p).value, len(z)) for k, z in zip(keep, ent)]
        host = lambda: ctx.decode_frames(raw, caps)                                        # noqa: E731
        devc = lambda: ctx.decode_frames_device(raw, ptrs, caps)                           # noqa: E731
        devn = lambda: ctx.decode_frames_device(raw, ptrs, caps, no_hash=True)             # noqa: E731
        rh, rd = host(), devc()
        assert [(x.status, x.written) for x in rh] == [(x.status, x.written) for x in rd] and all(x.status == 0 for x in rd)
        k = max(range(len(ent)), key=lambda i: caps[i])
        assert buf[offs[k]:offs[k] + rd[k].written].cpu().numpy().tobytes() == rh[k].data
        del rh
        t_host = t_dev = t_nohash = None
        for _ in range(5):                                                                 # interleaved: best of 5 each
            t_host = min(x for x in (t_host, best(host, 1)) if x is not None)
            t_dev = min(x for x in (t_dev, best(devc, 1)) if x is not None)
            t_nohash = min(x for x in (t_nohash, best(devn, 1)) if x is not None)
        devc()
        st = ctx.frames_device_stats()
        out[name] = {"entries": len(ent), "plain_MiB": sum(caps) / 2 ** 20, "host_call_ms": 1e3 * t_host, "device_call_ms": 1e3 * t_dev,
                     "device_call_no_hash_ms": 1e3 * t_nohash, "hash_share_of_device_call": max(0.0, (t_dev - t_nohash) / t_dev),
                     "speedup": t_host / t_dev, "stats": st,
                     "scatter_GBps": st["bytes_scattered"] / max(st["scatter_us"], 1) / 1e3}
        del buf
    ctx.close()
    first.close()
    print(json.dumps(out))


def device_src_main(args):
    import torch
    names = [a for a in args if not a.startswith("--")] or ["corpus101", "4096x128K", "1024x512K", "256x2M", "128x64M", "1x1024M"]
    first = zgpu.Context(0)
    first.decode_all(zgdata.zstd_compress(b"warm" * 1000), 4000)
    ctx = zgpu.Context(0)
    out = {}
    for name in names:
        ent, caps = device_workload(name)
        offs, total = [], 0
        for c in caps:
            offs.append(total)
            total += (c + 255) & ~255
        buf = torch.empty(max(total, 256), dtype=torch.uint8, device="cuda:0")
        ptrs = [buf.data_ptr() + o for o in offs]
        lens = [len(z) for z in ent]
        soffs, at = [], 0
        for n in lens:
            soffs.append(at)
            at += n
        src = torch.frombuffer(bytearray(b"".join(ent)), dtype=torch.uint8).to("cuda:0")
        pinned = torch.empty(at, dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        sptrs = [src.data_ptr() + o for o in soffs]

        def detour():
            pinned.copy_(src)                    # the caller's download (pinned: the fastest form of it)
            torch.cuda.synchronize()
            base = pinned.data_ptr()
            return ctx.decode_frames_device([(base + o, n) for o, n in zip(soffs, lens)], ptrs, caps)

        direct = lambda: ctx.decode_frames_device_src(sptrs, lens, ptrs, caps)           # noqa: E731
        ra = detour()
        want = buf.clone()
        buf.zero_()
        rb = direct()
        key = lambda r: (r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches, r.calculated_checksum, r.checksums_unverified)   # noqa: E731
        assert [key(x) for x in ra] == [key(x) for x in rb] and all(x.status == 0 for x in rb) and torch.equal(buf, want)
        del want
        t_detour = t_direct = None
        for _ in range(5):
            t_detour = min(x for x in (t_detour, best(detour, 1)) if x is not None)
            t_direct = min(x for x in (t_direct, best(direct, 1)) if x is not None)
        direct()
        out[name] = {"entries": len(ent), "plain_MiB": sum(caps) / 2 ** 20, "input_MiB": at / 2 ** 20, "download_then_device_call_ms": 1e3 * t_detour,
                     "device_src_call_ms": 1e3 * t_direct, "speedup": t_detour / t_direct, "src_stats": ctx.frames_device_src_stats(),
                     "stats": ctx.frames_device_stats()}
        st, ss = out[name]["stats"], out[name]["src_stats"]
        out[name]["scatter_GBps"] = st["bytes_scattered"] / max(st["scatter_us"], 1) / 1e3
        out[name]["gather_GBps"] = at / max(ss["gather_us"], 1) / 1e3
        del buf, src, pinned
    ctx.close()
    first.close()
    print(json.dumps(out))


def index_main(args):
    import torch
    names = [a for a in args if not a.startswith("--")] or ["corpus101", "4096x128K", "1x1024M"]
    ctx = zgpu.Context(0)
    out = {}
    for name in names:
        ent, caps = device_workload(name)
        lens = [len(z) for z in ent]
        soffs, at = [], 0
        for n in lens:
            soffs.append(at)
            at += n
        src = torch.frombuffer(bytearray(b"".join(ent)), dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        sptrs = [src.data_ptr() + o for o in soffs]
        idx = ctx.frames_index_device(sptrs, lens)
        bounds = {}
        for z, e in zip(ent, idx):
            if id(z) not in bounds:
                bounds[id(z)] = zgpu.plaintext_bound(z)
            assert e.status == 0 and e.bound == bounds[id(z)]
        summary, table = [], []
        for _ in range(5):
            ctx.frames_index_device(sptrs, lens)
            summary.append(ctx.frames_index_stats())
            _, _, frames = ctx.frames_table_device(sptrs, lens, room=sum(e.nframes + e.nskippable for e in idx) + len(ent))
            table.append(ctx.frames_index_stats())
        offs, total = [], 0
        for e in idx:
            offs.append(total)
            total += (e.bound + 255) & ~255
        buf = torch.empty(max(total, 256), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        walk = []
        for _ in range(3):
            r = ctx.decode_frames_device_src(sptrs, lens, [buf.data_ptr() + o for o in offs], [e.bound for e in idx], no_hash=True)
            assert all(x.status == 0 for x in r)
            walk.append(ctx.frames_device_src_stats())
        assert all(x.nframes == e.nframes and x.written <= e.bound for x, e in zip(r, idx))
        out[name] = {"entries": len(ent), "input_MiB": at / 2 ** 20, "frames": len(frames), "blocks": sum(e.nblocks for e in idx),
                     "summary_pass_us": min(x["kernel_us"] for x in summary), "summary": summary[-1],
                     "table_two_passes_us": min(x["kernel_us"] for x in table), "table": table[-1],
                     "zg_k_walk_two_passes_us": min(x["walk_us"] for x in walk), "walk": walk[-1]}
        del buf, src
    ctx.close()
    print(json.dumps(out))


def main():
    if "--index" in sys.argv[1:]:
        return index_main([a for a in sys.argv[1:] if a != "--index"])
    if "--device-src" in sys.argv[1:]:
        return device_src_main([a for a in sys.argv[1:] if a != "--device-src"])
    if "--device" in sys.argv[1:]:
        return device_main([a for a in sys.argv[1:] if a != "--device"])
    nf = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ctx = zgpu.Context(0)
    out = {}
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    ent, caps = [pack[n] for n in names], [man[n]["size"] for n in names]
    ctx.decode_frames(ent, caps)
    out["corpus101"] = {"loop_ms": 1e3 * best(lambda: loop(ctx, ent, caps)), "call_ms": 1e3 * best(lambda: ctx.decode_frames(ent, caps))}

    distinct = [zgdata.text_like(128 << 10, seed=0x300 + k) for k in range(64)]
    cs = [zgdata.zstd_compress(t) for t in distinct]
    ncs = [zgdata.zstd_compress(t, checksum=False) for t in distinct]
    ent = [cs[k % 64] for k in range(nf)]
    ent_n = [ncs[k % 64] for k in range(nf)]
    caps = [128 << 10] * nf
    r = ctx.decode_frames(ent, caps)                                         # (warm: pinned staging, device buffers)
    assert all(x.status == 0 and x.checksums == 1 and x.checksum_mismatches == 0 for x in r)
    assert all(x.data == distinct[k % 64] for k, x in enumerate(r))
    t_loop = 1e3 * best(lambda: loop(ctx, ent, caps), 1)
    t_cs = 1e3 * best(lambda: ctx.decode_frames(ent, caps), 5)
    ctx.decode_frames(ent_n, caps)
    t_ncs = 1e3 * best(lambda: ctx.decode_frames(ent_n, caps), 5)
    b = ctx.prepare(b"".join(ent))
    b.run()
    b.sync()
    b.checksums()
    t_hash = 1e3 * best(lambda: b.checksums(), 5)
    pipe = b.timings()["total"]
    b.close()
    out["text128k"] = {"frames": nf, "plain_MiB": nf * 128 / 1024, "loop_ms": t_loop, "call_checksum_ms": t_cs, "call_no_checksum_field_ms": t_ncs,
                       "speedup": t_loop / t_cs, "batch_checksums_ms": t_hash, "kernel_pipeline_ms": pipe,
                       "hash_share_of_call": t_hash / t_cs}

    big = zgdata.text_like(256 << 20, seed=0xE9)
    comp = [zgdata.zstd_compress(big[i:i + (128 << 10)]) for i in range(0, len(big), 128 << 10)]
    src = b"".join(comp * 32)
    del big
    b = ctx.prepare(src)
    b.run()
    b.sync()
    pipe = best(lambda: (b.run(), b.sync()), 3) * 1e3
    ms = b.timings()["total"]
    b.checksums()
    t_hash = 1e3 * best(lambda: b.checksums(), 5)
    out["blocks4b"] = {"frames": b.nframes, "plain_GiB": b.total_out / 2 ** 30, "kernel_pipeline_ms": ms, "run_sync_wall_ms": pipe,
                       "batch_checksums_ms": t_hash, "hash_share_of_pipeline": t_hash / ms}
    b.close()

    sweep = {}
    work = {}
    for name, size, count in (("4096x128K", 128 << 10, 4096), ("1024x512K", 512 << 10, 1024), ("256x2M", 2 << 20, 256), ("1x4M", 4 << 20, 1)):
        d = [zgdata.text_like(size, seed=0x700 + k) for k in range(min(count, 16))]
        c = [zgdata.zstd_compress(t) for t in d]
        work[name] = ([c[k % len(c)] for k in range(count)], [size] * count)
    for tag, h in (("auto", None), ("host", 0), ("device", 4 << 20), ("auto2", None), ("host2", 0)):
        if h is None:
            os.environ.pop("ZGPU_HASH_DEVICE_MAX", None)
        else:
            os.environ["ZGPU_HASH_DEVICE_MAX"] = str(h)
        dc = zgpu.Context(0, dev=True)
        row = {}
        for name, (ent, caps) in work.items():
            r = dc.decode_frames(ent, caps)
            assert all(x.status == 0 and x.checksum_mismatches == 0 and x.checksums == 1 for x in r)
            row[name] = 1e3 * best(lambda: dc.decode_frames(ent, caps), 5)
        sweep[tag] = row
        dc.close()
    os.environ.pop("ZGPU_HASH_DEVICE_MAX", None)
    out["hash_threshold_sweep_ms"] = sweep
    b = ctx.prepare(work["1x4M"][0][0])
    b.run()
    b.sync()
    b.checksums()
    t1 = best(lambda: b.checksums(), 5)
    out["one_lane"] = {"frame_MiB": 4, "batch_checksums_ms": 1e3 * t1, "lane_MB_per_s": (4 << 20) / t1 / 1e6}
    b.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
