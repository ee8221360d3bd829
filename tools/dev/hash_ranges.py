"""The two device hash kernels side by side, and what ZGPU_DEVICE_VERIFY costs (LABNOTES.md "xxh64q").

  python tools/dev/hash_ranges.py [workload ...]      (default: 1x4M 256x2M 128x64M 4096x128K 65536x8K)

zgpu_debug_hash_ranges (Context.hash_ranges) on COUNTxSIZE ranges that lie back to back in one torch tensor of random bytes, with kernel=1
(zg_k_xxh64, one lane per range), kernel=4 (zg_k_xxh64q, four lanes per range) and kernel=0 (the launcher's choice): one warm-up call, then
the best of 3 — the kernel's own time (HIP events, zgpu_debug_hash_ranges_us) and the wall time of the call (ranges up, kernel, digests
down). per_range_MBps is a range's length over the kernel's time (every range of a workload has the same length), aggregate_GBps all bytes
over it. The digests of the two kernels are compared.

  python tools/dev/hash_ranges.py --verify [workload ...]   (default: 256x2M 128x64M)

zgpu_decode_frames_device on small_frames.py's --device workloads (text frames with Content_Checksum): hashing off (no_hash), the default
(frames up to 4 MiB hashed beside the scatter), and verify=True (every frame hashed, then the scatter), interleaved, best of 5 after a
warm-up each, in the process's second context; hash_us is the hash kernel's share (zgpu_debug_frames_device_stats [8]). Prints one JSON
object."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "zstd-rs_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tools", "dev")]
import torch      # noqa: E402  (before the library is loaded: one HIP runtime)
import zgpu       # noqa: E402


def parse(name):
    count, size = name.split("x")
    return int(count), int(size[:-1]) << (10 if size[-1] == "K" else 20)


def kernels_main(names):
    ctx = zgpu.Context(0)
    out = {}
    for name in names:
        count, size = parse(name)
        total = count * size
        buf = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        step = 256 << 20
        for at in range(0, total, step):
            buf[at:at + step].random_(0, 256)
        torch.cuda.synchronize()
        offs, lens = [k * size for k in range(count)], [size] * count
        row, digests = {}, {}
        for kernel in (1, 4, 0):
            digests[kernel] = ctx.hash_ranges(buf.data_ptr(), offs, lens, kernel=kernel)          # (warm-up)
            us, wall = [], []
            for _ in range(3):
                t0 = time.perf_counter()
                ctx.hash_ranges(buf.data_ptr(), offs, lens, kernel=kernel)
                wall.append(time.perf_counter() - t0)
                us.append(ctx.hash_ranges_us())
            k_us = max(min(us), 1)
            row["kernel%d" % kernel] = {"kernel_us": min(us), "kernel_us_runs": us, "call_wall_ms": 1e3 * min(wall),
                                        "per_range_MBps": size / k_us, "aggregate_GBps": total / k_us / 1e3}
        assert digests[1] == digests[4] == digests[0]
        row["quad_over_one_lane"] = row["kernel1"]["kernel_us"] / max(row["kernel4"]["kernel_us"], 1)
        out[name] = row
        print(json.dumps({name: row}), flush=True)
        del buf
    ctx.close()
    print(json.dumps(out))


def verify_main(names):
    import zgdata
    from small_frames import best, device_workload
    first = zgpu.Context(0)                     # (the process's first context: not the one that is measured)
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
        torch.cuda.synchronize()
        ptrs = [buf.data_ptr() + o for o in offs]
        keep = [zgpu.C.c_char_p(z) for z in ent]
        raw = [(zgpu.C.cast(k, zgpu.C.c_void_p).value, len(z)) for k, z in zip(keep, ent)]
        calls = {"no_hash": lambda: ctx.decode_frames_device(raw, ptrs, caps, no_hash=True),
                 "default": lambda: ctx.decode_frames_device(raw, ptrs, caps),
                 "verify": lambda: ctx.decode_frames_device(raw, ptrs, caps, verify=True)}
        t, stats = {}, {}
        for k, fn in calls.items():
            r = fn()                                                                               # (warm-up)
            assert all(x.status == 0 and x.checksum_mismatches == 0 for x in r)
            if k == "verify":
                assert all(x.checksums == 1 and x.checksums_unverified == 0 for x in r)
        for _ in range(5):                                                                         # interleaved: best of 5 each
            for k, fn in calls.items():
                dt = best(fn, 1)
                t[k] = dt if k not in t else min(t[k], dt)
                stats[k] = ctx.frames_device_stats(verify=True)
        out[name] = {"entries": len(ent), "plain_MiB": sum(caps) / 2 ** 20, "call_ms": {k: 1e3 * v for k, v in t.items()},
                     "verify_over_no_hash_ms": 1e3 * (t["verify"] - t["no_hash"]), "stats": stats}
        print(json.dumps({name: out[name]}), flush=True)
        del buf
    ctx.close()
    first.close()
    print(json.dumps(out))


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--verify" in args:
        verify_main([a for a in args if not a.startswith("--")] or ["256x2M", "128x64M"])
    else:
        kernels_main([a for a in args if not a.startswith("--")] or ["1x4M", "256x2M", "128x64M", "4096x128K", "65536x8K"])
