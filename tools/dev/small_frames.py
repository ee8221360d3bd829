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
Prints one JSON object."""
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


def main():
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
