"""Dictionary entries through the three decode_frames calls: milliseconds per call with zgpu_set_frames_shared_dicts on and off.

    python tools/dev/frames_dicts.py [--entries 1024,4096] [--calls 5] [--warmup 2] [--off-entries 1024]

Workload: the 207 frames of tests/golden/dict_tests.pack (one 52 KB dictionary, plaintexts of up to 2 KB) repeated to N entries. Per call
and N: the median of --calls calls after --warmup warm-ups, the submit count, zg_k_dictfill's launches, bytes and kernel time (HIP events)
and its share of the call. The switch off is the library's behaviour without this feature (every entry alone: at least one submit each),
so it is measured on --off-entries entries only. One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch   # (before the library is loaded)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "zstd-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zgpu  # noqa: E402
from golden_io import read_manifest, read_pack  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1024,4096")
    ap.add_argument("--off-entries", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    names = sorted(n for n in man if n != "dictionary")
    c = zgpu.Context(0)
    c.add_dict(pack["dictionary"])
    for n in [int(x) for x in a.entries.split(",")]:
        entries = [pack[names[k % len(names)]] for k in range(n)]
        caps = [man[names[k % len(names)]]["size"] for k in range(n)]
        offs, at = [], 0
        for cap in caps:
            offs.append(at)
            at += (cap + 255) & ~255
        dst = torch.empty(max(at, 1), dtype=torch.uint8, device="cuda:0")
        soffs, at = [], 0
        for z in entries:
            soffs.append(at)
            at += (len(z) + 31) & ~31
        host = bytearray(at)
        for o, z in zip(soffs, entries):
            host[o:o + len(z)] = z
        src = torch.frombuffer(host, dtype=torch.uint8).to("cuda:0")
        torch.cuda.synchronize()
        dptr = [dst.data_ptr() + o for o in offs]
        sptr = [src.data_ptr() + o for o in soffs]
        lens = [len(z) for z in entries]
        calls = {
            "decode_frames": lambda: c.decode_frames(entries, caps),
            "decode_frames_device": lambda: c.decode_frames_device(entries, dptr, caps),
            "decode_frames_device_src": lambda: c.decode_frames_device_src(sptr, lens, dptr, caps),
        }
        for shared in (True, False):
            if not shared and n != a.off_entries:
                continue
            c.set_frames_shared_dicts(shared)
            for name, fn in calls.items():
                ms = []
                for k in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    res = fn()
                    t1 = time.perf_counter()
                    assert all(r.status == 0 for r in res)
                    if k >= a.warmup:
                        ms.append((t1 - t0) * 1e3)
                ds = c.frames_dict_stats()
                med = statistics.median(ms)
                print(json.dumps({"call": name, "entries": n, "shared": shared, "ms_median": round(med, 3), "ms_min": round(min(ms), 3),
                                  "ms_max": round(max(ms), 3), "submits": c.frames_submits(), "fill_launches": ds["fill_launches"],
                                  "fill_bytes": ds["bytes_replicated"], "fill_us": ds["fill_us"],
                                  "fill_share": round(ds["fill_us"] / 1e3 / med, 4) if med else 0.0, "frames_shared": ds["frames_shared"],
                                  "entries_alone": ds["entries_alone"]}), flush=True)
    c.close()


if __name__ == "__main__":
    main()
