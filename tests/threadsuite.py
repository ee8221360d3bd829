"""The library under concurrent host threads against the oracle (test helper and a program, no tests): the job lists with their
expected results, the runner, the scenarios. tests/test_gpu_threads.py runs `python tests/threadsuite.py --report PATH` once in a child
process and reads the report; tests/test_threadsuite_cpu.py pins the lists and drives the runner without a GPU.

The contract under test (include/zgpu.h, context section): distinct contexts, and everything made from them, may be used from distinct
threads at once; one context and its decoders, streams, batches and indexes are one thread's at a time; objects may change threads between
calls and may be destroyed on any thread; zgpu_release_caches is called only while no stream is in a call. No scenario ever has two threads
inside one context.

A job is Job(id, kind, inputs, expected). `expected` is computed on the main thread, before any thread starts, from the oracle alone
(oracle.FrameDecoder, test_gpu_stream.oracle_reads, devmem.oracle_alone, devmem.xxh64) — never from the library under test, and the oracle is
never called from two threads. An executor (make_executor(thread index), made inside the thread) runs a job's inputs and returns what it
got in the shape of `expected`; the runner compares. The product library only, no ZGPU_* switch."""
import collections
import json
import os
import queue
import random
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "zstd-rs_amd"))

import devmem   # (torch before the library is loaded: the process must run on one HIP runtime)
import framesuite
import oracle
from golden_io import read_manifest, read_pack
from test_exact_cpu import K
from test_gpu_stream import MODES, oracle_reads, patterns, zgpu_reads

T = 4                                   # caller threads
SEED = 0x7C3A
PIPE = 2                                # MODES[PIPE]: pipe_after=1, read_ahead=4 << 20 — the worker thread, its own engine, a pinned ring
KINDS = ("decode_all", "lockstep", "stream", "stream_abandoned", "dict", "frames", "pool", "device")
SCENARIOS = ("serial", "own_contexts", "moved", "churn", "device")
CONCURRENT = SCENARIOS[1:]
MOVED_STEPS = 9                         # every thread meets every group three times
SERIAL_DEADLINE_S = 240                 # the serial pass has no yardstick but itself: a guard against a hang
HIP_ERROR = __import__("re").compile(r"(^|[^0-9])92, expected|\('(err|init)', 92\)|HIP")   # a record that met ZGPU_E_HIP
TAIL = b"bytes of the next frame"
Job = collections.namedtuple("Job", "id kind inputs expected")


# ---- comparing ------------------------------------------------------------------------------------------------------------------------
def diff(want, got, path="result"):
    """None, or where `got` first differs from `want` (bytes by position and length, never by content)"""
    if isinstance(want, (list, tuple)) and isinstance(got, (list, tuple)):
        if len(want) != len(got):
            return "%s: %d items, expected %d" % (path, len(got), len(want))
        for i, (w, g) in enumerate(zip(want, got)):
            d = diff(w, g, "%s[%d]" % (path, i))
            if d:
                return d
        return None
    if isinstance(want, dict) and isinstance(got, dict):
        for k in want:
            if k not in got:
                return "%s: no %r" % (path, k)
            d = diff(want[k], got[k], "%s.%s" % (path, k))
            if d:
                return d
        return None
    if isinstance(want, (bytes, bytearray)) and isinstance(got, (bytes, bytearray)):
        if bytes(want) == bytes(got):
            return None
        at = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
        return "%s: bytes differ at %d (%d bytes, expected %d)" % (path, at, len(got), len(want))
    if isinstance(want, (bytes, bytearray)) or isinstance(got, (bytes, bytearray)):
        return "%s: %s, expected %s" % (path, _short(got), _short(want))
    return None if want == got else "%s: %s, expected %s" % (path, _short(got), _short(want))


def _short(v):
    return "%d bytes" % len(v) if isinstance(v, (bytes, bytearray)) else repr(v)[:120]


def leaves_of(v):
    """the error statuses in a result: every ("err" | "init", status) in it"""
    out = []
    if isinstance(v, (list, tuple)):
        if len(v) == 2 and v[0] in ("err", "init") and isinstance(v[1], int):
            return [v[1]]
        for x in v:
            out += leaves_of(x)
    elif isinstance(v, dict):
        for x in v.values():
            out += leaves_of(x)
    return out


def describe(job):
    """what the report says of a job (and what coverage() reads)"""
    i = job.inputs
    return {"id": job.id, "kind": job.kind, "name": i.get("name"), "mode": i.get("mode"), "leaves": leaves_of(job.expected),
            "plaintext": i.get("plaintext", 0)}


# ---- what both decoders are asked, in one place: the oracle's answers are `expected`, the library's are `got` ------------------------------
class Lockstep:
    """FrameDecoder.decode_blocks(UptoBlocks, 1) + collect(), call by call (framesuite.lockstep is the model), on either decoder"""

    def __init__(self, d, z):
        self.d, self.z = d, z
        self.st, self.pos, _, _ = d.init(z)
        self.fin, self.calls = False, 0
        self.most = framesuite._block_count(z, self.pos) + 2
        self.header = ("header", self.st, self.pos)

    def over(self):
        return bool(self.st or self.fin)

    def step(self):
        """one call: (status, used, finished, blocks_decoded, bytes_read_from_source, can_collect, what collect() returns); an error carries
        neither `used` nor `finished` (include/zgpu.h)"""
        d = self.d
        assert self.calls < self.most, "more calls than the frame has blocks for"
        self.st, used, self.fin = d.decode_blocks(self.z[self.pos:], oracle.STRAT_UPTO_BLOCKS, 1)
        self.calls += 1
        if not self.st:
            self.pos += used
        return (self.st, None if self.st else used, None if self.st else self.fin, d.blocks_decoded(), d.bytes_read_from_source(), d.can_collect(),
                d.collect())

    def end(self):
        d = self.d
        calc = d.get_calculated_checksum() if hasattr(d, "get_calculated_checksum") else d.calculated_checksum()
        return ("end", d.is_finished(), calc)

    def all(self):
        out = [self.header]
        while not self.over():
            out.append(self.step())
        if not self.st:
            out.append(self.end())
        return out


def decode_all_result(call):
    """("ok", bytes) or ("err", status) of a decode_all call of either side"""
    st, out = call()
    return ("err", st) if st else ("ok", out)


def _zgpu_decode_all(target, z, cap):
    import zgpu
    try:
        return 0, target.decode_all(z, cap)
    except zgpu.ZgpuError as e:
        return e.status, None


def stream_result(reads, s, end):
    """reads: [(n, bytes)], ("err" | "init", status) last. end: "full" — behind a frame that was read to its end finished, both checksums,
    blocks_decoded, bytes_read_from_source and the source position (what test_corpus_through_every_mode holds) —, "calc" — finished and the
    calculated checksum (mutated and dictionary frames) —, None (a stream that is abandoned). s: the oracle's decoder or the library's stream"""
    out = {"reads": [tuple(r) for r in reads]}
    if end is None or (reads and reads[-1][0] in ("err", "init")) or s is None:
        return out
    if isinstance(s, oracle.FrameDecoder):
        rec = (s.is_finished(), s.calculated_checksum(), s.checksum_from_data(), s.blocks_decoded(), s.bytes_read_from_source(), s.bytes_read_from_source())
    else:
        rec = (s.is_finished(), s.get_calculated_checksum(), s.get_checksum_from_data(), s.blocks_decoded(), s.bytes_read_from_source(), s.source_position())
    out["end"] = rec if end == "full" else rec[:2]
    return out


def frames_entry(z, r_or_none, cap, mutated):
    """one entry of a decode_frames call as framesuite.check_entries / check_decode_frames hold it: the status; of a good entry the bytes,
    `written`, the first frame's checksums, and of an entry that was not mutated one frame, one checksum, no mismatch"""
    if r_or_none is None:
        st, out = devmem.oracle_alone(z, cap)
        if st:
            return ("err", st)
        first = framesuite._oracle_first_frame(z) if z[:4] == devmem.MAGIC else None
        return ("ok", out, len(out), first, (1, 1, 0) if not mutated else None)
    r = r_or_none
    if r.status:
        return ("err", r.status) if r.written == 0 and r.data is None else ("err", r.status, r.written, "data behind an error")
    first = (r.checksum_from_data, r.calculated_checksum) if r.nframes and z[:4] == devmem.MAGIC else None
    return ("ok", r.data, r.written, first, (r.nframes, r.checksums, r.checksum_mismatches) if not mutated else None)


# ---- inputs: what is committed -------------------------------------------------------------------------------------------------------------
class Corpus:
    def __init__(self):
        self.pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
        self.names = sorted(man)
        self.size = {n: man[n]["size"] for n in self.names}
        self.nblocks = {}
        for n in self.names:
            st, pos, _, _ = oracle.FrameDecoder().init(self.pack[n])
            assert st == 0
            self.nblocks[n] = framesuite._block_count(self.pack[n], pos)
        dman = read_manifest("dict_tests.json")
        self.dpack = read_pack("dict_tests.pack")
        self.dict_raw = self.dpack["dictionary"]
        self.dnames = sorted(n for n in dman if n.endswith(".zst"))
        self.dsize = {n: dman[n]["size"] for n in self.dnames}

    def pick(self, rng, lo=0, hi=1 << 30, blocks=(1, 1 << 30)):
        c = [n for n in self.names if lo <= self.size[n] <= hi and blocks[0] <= self.nblocks[n] <= blocks[1]]
        return rng.choice(c)


def mutate(rng, z):
    """one to three seeded bit flips behind the magic (test_mutated_frames_fail_in_the_same_read_call)"""
    m = bytearray(z)
    for _ in range(rng.choice([1, 1, 2, 3])):
        i = rng.randrange(4, len(m))
        m[i] ^= 1 << rng.randrange(8)
    return bytes(m)


def pattern(rng, size):
    return list(patterns(rng, size))[rng.randrange(3)]


# ---- the jobs of each kind, expected included ----------------------------------------------------------------------------------------------
def decode_all_job(jid, name, z, cap, mutated=False, plaintext=0):
    return Job(jid, "decode_all", dict(name=name + ("~" if mutated else ""), z=z, cap=cap, plaintext=plaintext),
               decode_all_result(lambda: devmem.oracle_alone(z, cap)))


def lockstep_job(jid, name, z, plaintext):
    return Job(jid, "lockstep", dict(name=name, z=z, plaintext=plaintext), Lockstep(oracle.FrameDecoder(), z).all())


def stream_job(jid, name, z, pat, mode, end, plaintext, dict_raw=None, kind="stream", calls=None):
    reads = pat if calls is None else pat[:calls]
    res, o = oracle_reads(z, reads, dict_raw)
    return Job(jid, kind, dict(name=name, z=z, reads=reads, mode=mode, end=end, plaintext=plaintext, dict=dict_raw is not None),
               stream_result(res, o, end))


def abandoned_job(jid, rng, corpus):
    """a PIPE-mode stream on a frame of at least 8 blocks, closed after k reads that leave most of the frame unread: the worker is ahead"""
    name = corpus.pick(rng, lo=200 << 10, blocks=(8, 1 << 30))
    size = corpus.size[name]
    reads, total = [], 0
    for _ in range(rng.randrange(1, 5)):
        c = rng.choice([1, 4096, 8192, 20000])
        if total + c < size // 3:
            reads.append(c)
            total += c
    reads = reads or [1]
    j = stream_job(jid, name, corpus.pack[name], reads, PIPE, None, size, kind="stream_abandoned")
    assert j.expected["reads"][-1][0] not in ("err", "init", 0)
    return j


def dict_job(jid, rng, corpus, mode):
    name = rng.choice(corpus.dnames)
    z, size, raw = corpus.dpack[name], corpus.dsize[name], corpus.dict_raw
    pat = pattern(rng, size)
    res, o = oracle_reads(z, pat, raw)
    return Job(jid, "dict", dict(name=name, z=z, cap=size + 64, reads=pat, mode=mode, plaintext=2 * size),
               {"decode_all": decode_all_result(lambda: devmem.oracle_alone(z, size + 64, raw)), "stream": stream_result(res, o, "calc")})


def frames_job(jid, rng, corpus, hand):
    """about 24 entries of one decode_frames call, a third of them mutated; four of them hand-built (valid and invalid)"""
    entries = []
    for k in range(20):
        name = corpus.pick(rng, hi=40 << 10)
        z = corpus.pack[name]
        entries.append((name, mutate(rng, z), corpus.size[name] + 64, True) if k % 3 == 2 else (name, z, corpus.size[name], False))
    for name, z, plain in rng.sample(hand, 4):
        entries.append((name, z, len(plain) if plain is not None else 1 << 17, plain is None))
    rng.shuffle(entries)
    return Job(jid, "frames", dict(name="%d entries" % len(entries), names=[e[0] for e in entries], entries=[e[1] for e in entries],
                                   caps=[e[2] for e in entries], mutated=[e[3] for e in entries]),
               [frames_entry(z, None, cap, mut) for _, z, cap, mut in entries])


def pool_job(jid, rng, corpus):
    names = [corpus.pick(rng, lo=1000, hi=150 << 10) for _ in range(3)]
    z, cap = b"".join(corpus.pack[n] for n in names), sum(corpus.size[n] for n in names)
    return Job(jid, "pool", dict(name="+".join(names), z=z, cap=cap, plaintext=cap), decode_all_result(lambda: devmem.oracle_alone(z, cap)))


def hand_built():
    """frames of the hand-built generators for the decode_all and frames jobs: (name, zst, plaintext or None)"""
    import blockframes
    import seqframes
    out = list(blockframes.family("invalid")) + list(blockframes.family("neighbours")) + list(seqframes.family("short_offsets"))
    return [f for f in out if len(f[1]) <= 4096]


def own_list(t, rng, corpus, hand):
    """thread t of own_contexts: every kind but `device`, the kinds in a seeded rotation"""
    by_kind = collections.OrderedDict((k, []) for k in KINDS[:-1])
    jid = lambda kind: "own_contexts/%d/%s%d" % (t, kind, len(by_kind[kind]))
    for k in range(5):
        name = corpus.pick(rng, hi=300 << 10)
        by_kind["decode_all"].append(decode_all_job(jid("decode_all"), name, corpus.pack[name], corpus.size[name], plaintext=corpus.size[name]))
    for k in range(8):
        name = corpus.pick(rng, hi=100 << 10)
        by_kind["decode_all"].append(decode_all_job(jid("decode_all"), name, mutate(rng, corpus.pack[name]), corpus.size[name] + 64, True, corpus.size[name]))
    for name, z, plain in rng.sample([f for f in hand if f[2] is None], 2):
        by_kind["decode_all"].append(decode_all_job(jid("decode_all"), name, z, 1 << 17, True))
    for k in range(2):
        name = corpus.pick(rng, hi=450 << 10, blocks=(3, 16))
        by_kind["lockstep"].append(lockstep_job(jid("lockstep"), name, corpus.pack[name], corpus.size[name]))
    for mode in range(len(MODES)):
        blocks = (1, 64) if MODES[mode].get("read_ahead") == 1 else (1, 1 << 30)     # (block by block: a launch per block)
        name = corpus.pick(rng, lo=1000, hi=450 << 10, blocks=blocks)
        by_kind["stream"].append(stream_job(jid("stream"), name, corpus.pack[name] + TAIL, pattern(rng, corpus.size[name]), mode, "full", corpus.size[name]))
        name = corpus.pick(rng, lo=1000, hi=200 << 10, blocks=blocks)
        by_kind["stream"].append(stream_job(jid("stream"), name + "~", mutate(rng, corpus.pack[name]), pattern(rng, corpus.size[name]), mode, "calc",
                                            corpus.size[name]))
    by_kind["stream_abandoned"].append(abandoned_job(jid("stream_abandoned"), rng, corpus))
    for k in range(2):
        by_kind["dict"].append(dict_job(jid("dict"), rng, corpus, (t + k) % len(MODES)))
    by_kind["frames"].append(frames_job(jid("frames"), rng, corpus, hand))
    by_kind["pool"].append(pool_job(jid("pool"), rng, corpus))
    kinds = list(by_kind)
    rot = (2 * t + rng.randrange(2)) % len(kinds)
    return [j for k in kinds[rot:] + kinds[:rot] for j in by_kind[k]]


def moved_lists(rng, corpus):
    """three groups (a context, a FrameDecoder mid-frame, a PIPE-mode stream mid-frame) made on thread 0; at step s thread i makes the next
    calls on group (i + s) % 3: one decode_blocks + collect, one stream read, one decode_all of the group's context. Behind the last step
    the groups are destroyed mid-frame, on threads 1 and 2: never on the thread that made them"""
    groups = []
    for g in range(3):
        lname = corpus.pick(rng, hi=500 << 10, blocks=(MOVED_STEPS + 2, 64))
        sname = corpus.pick(rng, lo=200 << 10, blocks=(8, 1 << 30))
        reads = [rng.choice([1, 4096, 8192, K // 8]) for _ in range(MOVED_STEPS)]
        assert sum(reads) < corpus.size[sname] // 2
        lock = Lockstep(oracle.FrameDecoder(), corpus.pack[lname])
        steps = [lock.step() for _ in range(MOVED_STEPS)]
        assert not lock.over()
        sres, _ = oracle_reads(corpus.pack[sname], reads)
        small = []
        for s in range(MOVED_STEPS):
            n = corpus.pick(rng, hi=20 << 10)
            small.append((n, mutate(rng, corpus.pack[n]), corpus.size[n] + 64) if s % 3 == 1 else (n, corpus.pack[n], corpus.size[n]))
        groups.append(dict(lname=lname, lz=corpus.pack[lname], header=lock.header, steps=steps, sname=sname, sz=corpus.pack[sname], reads=reads,
                           sres=[tuple(r) for r in sres], small=small))
    create = Job("moved/0/create", "moved_create", dict(name="3 groups", groups=[dict(lz=g["lz"], sz=g["sz"]) for g in groups]),
                 [g["header"] for g in groups])
    lists = [[create], [], []]
    for s in range(MOVED_STEPS):
        for i in range(3):
            gi = (i + s) % 3
            g = groups[gi]
            n, z, cap = g["small"][s]
            lists[i].append(Job("moved/%d/step%d" % (i, s), "moved_step",
                                dict(name="group %d: %s, %s, %s" % (gi, g["lname"], g["sname"], n), group=gi, read=g["reads"][s], z=z, cap=cap, mode=PIPE,
                                     plaintext=cap + g["reads"][s]),
                                {"blocks": g["steps"][s], "read": g["sres"][s], "decode_all": decode_all_result(lambda: devmem.oracle_alone(z, cap))}))
    for i, gs in ((0, []), (1, [1, 0]), (2, [2])):
        lists[i].append(Job("moved/%d/close" % i, "moved_close", dict(name="groups %s" % gs, groups=gs), ["closed"] * len(gs)))
    return lists


def churn_lists(rng, corpus):
    """two rounds: threads 0 and 1 abandon PIPE-mode streams back to back while threads 2 and 3 read PIPE-mode streams to their end, so that
    the blocks and engines one thread gives back are what another takes next; between the rounds every stream is closed, the threads wait,
    and the main thread releases the caches (kind `release_caches`)"""
    lists = [[] for _ in range(T)]
    for rnd in range(2):
        for t in range(T):
            for k in range(3 if t < 2 else 2):
                jid = "churn/%d/r%d.%d" % (t, rnd, k)
                if t < 2:
                    lists[t].append(abandoned_job(jid, rng, corpus))
                else:
                    name = corpus.pick(rng, lo=100 << 10, hi=600 << 10)
                    lists[t].append(stream_job(jid, name, corpus.pack[name] + TAIL, pattern(rng, corpus.size[name]), PIPE, "full", corpus.size[name]))
            if rnd == 0:
                lists[t].append(Job("churn/%d/release" % t, "release_caches", dict(name="between the rounds"), "released"))
    return lists


def _raw_frame(payload):
    """a frame of one raw block without Content_Checksum and Frame_Content_Size: a changed byte of its payload changes no size and no verdict"""
    return devmem.MAGIC + bytes([0x00, (17 - 10) << 3]) + (1 | (len(payload) << 3)).to_bytes(3, "little") + payload, payload


def device_job(jid, rng):
    """the device-resident chain on two shards (see the executor): shard A of 12 text frames that declare their sizes and carry checksums,
    shard B of text frames that declare nothing around a raw frame; B' is B with one byte of the raw payload changed. Expectations: the
    oracle's decode of every frame (Shard), devmem.xxh32 of every row's plaintext, slices of the plaintext"""
    import zgpu
    from test_gpu_seek_index_measured import Shard, _text_frames
    seed = rng.randrange(1 << 20)
    A = Shard(_text_frames([rng.randint(1, 3000) for _ in range(12)], seed, checksum=True, content_size=True))
    fb = _text_frames([5000, 1, 20000, 300], seed + 100)
    row = 2
    fb.insert(row, _raw_frame(rng.randbytes(777)))
    B = Shard(fb)
    at = B.C[row] + 9 + 400                                        # (magic, descriptor, window byte, block header: 9 bytes in front of the payload)
    zc = B.z[:at] + bytes([B.z[at] ^ 0x20]) + B.z[at + 1:]
    pc = B.plain[:B.D[row] + 400] + bytes([B.plain[B.D[row] + 400] ^ 0x20]) + B.plain[B.D[row] + 401:]
    assert devmem.oracle_alone(zc, len(pc) + 64) == (0, pc) and pc != B.plain and len(pc) == len(B.plain)
    caps = [len(A.plain) + 13, len(pc) + 7]
    # ranges (entry, begin, len): of A anywhere, rows shared and crossed; of B' only ranges that touch the changed row, so that every group
    # of them holds it
    D = A.D
    ranges = [(0, 0, 1), (0, D[3] - 1, D[5] - D[3] + 2), (0, D[4], 7), (0, D[11], D[12] - D[11]), (0, D[7] + 1, 3),
              (1, B.D[row] + 390, 20), (1, B.D[row] - 1, 2), (1, B.D[row + 1] - 1, 5), (1, B.D[row], 777)]
    rng.shuffle(ranges)
    gcaps = [n + (7 if j % 2 else 0) for j, (_, _, n) in enumerate(ranges)]
    gplains = [A.plain[b:b + n] if e == 0 else None for e, b, n in ranges]
    expected = {
        "decode": [(0, len(A.plain), len(A.cs), len(A.cs), 0), (0, len(pc), len(B.cs), 0, 0)],
        "index": [(0, zgpu.INDEX_DECLARED, len(A.cs)), (0, zgpu.INDEX_MEASURED, len(B.cs))],
        "hash": [(0, zgpu.SUMS_HASHED, A.nzstd, A.D[-1]), (0, zgpu.SUMS_HASHED, B.nzstd, B.D[-1])],
        "sums": [[devmem.xxh32(p) for _, p in A.frames], [devmem.xxh32(p) for _, p in B.frames]],
        "gather": [(0, n) if e == 0 else (zgpu.E_SEEK_CHECKSUM_MISMATCH, 0) for e, _, n in ranges],
    }
    return Job(jid, "device", dict(name="shards %#x" % seed, good=[A.z, B.z], changed=zc, caps=caps, ranges=ranges, gcaps=gcaps,
                                   plains=[A.plain, pc], gplains=gplains, plaintext=2 * (len(A.plain) + len(pc))), expected)


def device_lists(rng, corpus):
    lists = [[device_job("device/%d/chain%d" % (t, k), rng) for k in range(2)] for t in range(T)]
    side = []
    for mode in range(len(MODES)):
        name = corpus.pick(rng, lo=50 << 10, hi=450 << 10, blocks=(1, 64))
        side.append(stream_job("device/%d/stream%d" % (T, mode), name, corpus.pack[name] + TAIL, pattern(rng, corpus.size[name]), mode, "full", corpus.size[name]))
    return lists + [side]


_BUILT = {}


def build(seed=SEED, fresh=False):
    """{scenario: one job list per thread} for the concurrent scenarios, expected included. Deterministic in `seed`"""
    if seed in _BUILT and not fresh:
        return _BUILT[seed]
    corpus, hand = Corpus(), hand_built()
    out = collections.OrderedDict()
    out["own_contexts"] = [own_list(t, random.Random(seed * 1000 + t), corpus, hand) for t in range(T)]
    out["moved"] = moved_lists(random.Random(seed * 1000 + 10), corpus)
    out["churn"] = churn_lists(random.Random(seed * 1000 + 20), corpus)
    out["device"] = device_lists(random.Random(seed * 1000 + 30), corpus)
    _BUILT[seed] = out
    return out


def serial_list(lists):
    """every job of every list for one thread: own_contexts, churn and device list after list; moved step by step, which is the order its
    barriers enforce"""
    out = []
    for sc in ("own_contexts", "churn", "device"):
        for lst in lists[sc]:
            out += lst
    m = lists["moved"]
    out.append(m[0][0])
    for s in range(MOVED_STEPS + 1):
        for i in range(3):
            out.append(m[i][s + (1 if i == 0 else 0)])
    return out


def digest(lists):
    """names, patterns and the digests of inputs and expected results: what `the same seed gives the same lists` compares"""
    def fold(v):
        if isinstance(v, (bytes, bytearray)):
            return "%d:%016x" % (len(v), devmem.xxh64(bytes(v)))
        if isinstance(v, (list, tuple)):
            return [fold(x) for x in v]
        if isinstance(v, dict):
            return {k: fold(x) for k, x in sorted(v.items())}
        return v
    return {sc: [[(j.id, j.kind, fold(j.inputs), fold(j.expected)) for j in lst] for lst in ls] for sc, ls in lists.items()}


def coverage(described):
    """described: {scenario: [[describe(job) ...] per thread]} of the concurrent scenarios (from the lists, or from a report's records). The
    floors of tests/test_gpu_threads.py are conditions on the lists: a kind or a stream mode `ran concurrently` when, in one scenario whose
    threads run at once, at least two threads have jobs of it"""
    kinds, modes = collections.Counter(), collections.Counter()
    leaves = []
    for sc, per_thread in described.items():
        seen_k, seen_m = collections.Counter(), collections.Counter()
        for jobs in per_thread:
            for k in set(j["kind"] for j in jobs):
                seen_k[k] += 1
            for m in set(j["mode"] for j in jobs if j["kind"] in ("stream", "dict", "stream_abandoned", "moved_step") and j["mode"] is not None):
                seen_m[m] += 1
            for j in jobs:
                leaves += j["leaves"]
        for k, n in seen_k.items():
            kinds[k] = max(kinds[k], n)
        for m, n in seen_m.items():
            modes[m] = max(modes[m], n)
    return {"threads_per_kind": dict(kinds), "threads_per_mode": {int(m): n for m, n in modes.items()}, "error_verdicts": len(leaves),
            "distinct_leaves": sorted(set(leaves))}


def floors(cov):
    """the coverage the issue lists, as (what, holds) pairs"""
    return [("every kind ran on at least two threads at once", all(cov["threads_per_kind"].get(k, 0) >= 2 for k in KINDS)),
            ("every stream mode ran concurrently", all(cov["threads_per_mode"].get(m, 0) >= 2 for m in range(len(MODES)))),
            ("at least 20 error verdicts", cov["error_verdicts"] >= 20),
            ("at least 4 distinct leaves", len(cov["distinct_leaves"]) >= 4)]


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def run(scenario, threads, jobs_per_thread, deadline_s, make_executor):
    """`threads` threads behind one barrier; each makes its executor through make_executor(thread index) inside the thread, runs the jobs of
    its list in order and keeps (job, ok | mismatch | exception) records of its own; the main thread joins all of them against ONE deadline.
    Returns {"scenario", "wall_s", "deadline_s", "hung": [thread ids], "threads": [{"wall_s", "done", "records": [...]}]}; a thread in `hung`
    is still running when this returns. While it waits the main thread runs the callables that executors put into
    make_executor.main_calls (a queue.Queue, optional): what only the main thread may do."""
    assert threads == len(jobs_per_thread)
    start = threading.Barrier(threads + 1)
    per = [{"wall_s": None, "done": False, "ident": None, "records": []} for _ in range(threads)]
    t_zero = [0.0]

    def body(i):
        me = per[i]
        me["ident"] = threading.get_ident()
        start.wait()
        t_in = time.monotonic()
        ex = None
        try:
            ex = make_executor(i)
            for job in jobs_per_thread[i]:
                rec = describe(job)
                rec["t0"] = round(time.monotonic() - t_zero[0], 4)
                try:
                    got = ex.run(job._replace(expected=None))
                    extra = got.pop("_extra", None) if isinstance(got, dict) else None
                    if extra is not None:
                        rec["extra"] = extra
                    d = diff(job.expected, got)
                    rec["verdict"], rec["detail"] = ("ok", None) if d is None else ("mismatch", d)
                except Exception as e:      # noqa: BLE001 (whatever a job raises is its record; the thread goes on)
                    rec["verdict"], rec["detail"] = "exception", "%s: %s" % (type(e).__name__, e)
                rec["t1"] = round(time.monotonic() - t_zero[0], 4)
                me["records"].append(rec)
        except Exception as e:              # noqa: BLE001 (the executor could not be made)
            me["records"].append({"id": "%s/%d/executor" % (scenario, i), "kind": "executor", "name": None, "mode": None, "leaves": [],
                                  "verdict": "exception", "detail": "%s: %s" % (type(e).__name__, e)})
        finally:
            try:
                if ex is not None:
                    ex.close()
            except Exception as e:          # noqa: BLE001
                me["records"].append({"id": "%s/%d/close" % (scenario, i), "kind": "executor", "name": None, "mode": None, "leaves": [],
                                      "verdict": "exception", "detail": "close: %s: %s" % (type(e).__name__, e)})
            me["wall_s"] = round(time.monotonic() - t_in, 4)
            me["done"] = True

    ths = [threading.Thread(target=body, args=(i,), name="%s-%d" % (scenario, i), daemon=True) for i in range(threads)]
    for th in ths:
        th.start()
    calls = getattr(make_executor, "main_calls", None)
    t_zero[0] = time.monotonic()
    start.wait()
    end = t_zero[0] + deadline_s
    while any(th.is_alive() for th in ths) and time.monotonic() < end:
        if calls is None:
            next(th for th in ths if th.is_alive()).join(min(0.05, max(0.0, end - time.monotonic())))
            continue
        try:
            calls.get(timeout=0.01)()
        except queue.Empty:
            pass
    hung = [i for i, th in enumerate(ths) if th.is_alive()]
    return {"scenario": scenario, "wall_s": round(time.monotonic() - t_zero[0], 4), "deadline_s": deadline_s, "hung": hung,
            "threads": [dict(p, records=list(p["records"])) for p in per]}


def failures(result):
    """[(thread, record)] of every record that is not ok"""
    return [(i, r) for i, th in enumerate(result["threads"]) for r in th["records"] if r["verdict"] != "ok"]


# ---- the executor on the GPU ---------------------------------------------------------------------------------------------------------------
class DeviceBuffers:
    """a device job's tensors, built on the main thread before the start and checked there after the join (devmem.Sources / Arena call
    torch.cuda.synchronize(), which no caller thread does)"""

    def __init__(self, job):
        i = job.inputs
        self.job = job
        self.good = devmem.Sources(i["good"], [1, 2])
        self.mine = devmem.Sources([i["good"][0], i["changed"]], [3, 1])
        self.out = devmem.Arena(i["caps"], [1, 2])
        self.gout = devmem.Arena(i["gcaps"], [(j % 5) for j in range(len(i["gcaps"]))])

    def check(self):
        """None, or what is wrong: plaintext in its slots, untouched slots, guards and gaps (Arena.check), sources unchanged"""
        i = self.job.inputs
        try:
            self.out.check(i["plains"])
            self.gout.check(i["gplains"])
            assert self.good.unchanged() and self.mine.unchanged(), "a source changed"
        except AssertionError as e:
            return "%s: %s" % (self.job.id, e)
        return None


class Shared:
    """what the executors of one scenario share: the barrier of its steps, the main thread's queue, the moved groups, the device buffers"""

    def __init__(self, scenario, parties, buffers=None, dict_raw=None):
        self.scenario, self.parties, self.buffers, self.dict_raw = scenario, parties, buffers or {}, dict_raw
        self.barrier = threading.Barrier(parties)
        self.main_calls = queue.Queue()
        self.pools = threading.Semaphore(2)          # at most two threads hold a pool at once
        self.groups, self.destroyed, self.released = [], [], []
        self.wait_s = 120

    def on_main(self, fn):
        done = threading.Event()
        self.main_calls.put(lambda: (fn(), done.set()))
        if not done.wait(self.wait_s):
            raise RuntimeError("the main thread did not answer")


class GpuExecutor:
    """one context per caller thread, made inside the thread; every object a job makes is closed before the job returns (moved groups apart)"""

    def __init__(self, shared, thread):
        import zgpu
        self.zgpu, self.shared, self.thread = zgpu, shared, thread
        assert (zgpu.STRAT_UPTO_BLOCKS, zgpu.STRAT_UPTO_BYTES) == (oracle.STRAT_UPTO_BLOCKS, oracle.STRAT_UPTO_BYTES)
        self.ctx = zgpu.Context(0)
        self.has_dict = False

    def close(self):
        self.ctx.close()

    def run(self, job):
        return getattr(self, "_" + job.kind)(job)

    def _decode_all(self, job):
        i = job.inputs
        return decode_all_result(lambda: _zgpu_decode_all(self.ctx, i["z"], i["cap"]))

    def _lockstep(self, job):
        i = job.inputs
        d = self.zgpu.FrameDecoder(self.ctx)
        try:
            return Lockstep(d, i["z"]).all()
        finally:
            d.close()

    def _stream(self, job):
        i = job.inputs
        res, s = zgpu_reads(self.ctx, i["z"], i["reads"], False, copy_threads=1, **MODES[i["mode"]])
        try:
            return stream_result(res, s, i["end"])
        finally:
            if s:
                s.close()

    _stream_abandoned = _stream                      # (end is None: close() while the worker is ahead)

    def _dict(self, job):
        i = job.inputs
        if not self.has_dict:
            self.ctx.add_dict(self.shared.dict_raw)
            self.has_dict = True
        return {"decode_all": self._decode_all(job), "stream": self._stream(job._replace(inputs=dict(i, end="calc")))}

    def _frames(self, job):
        i = job.inputs
        res = self.ctx.decode_frames(i["entries"], i["caps"])
        return [frames_entry(z, r, cap, mut) for z, r, cap, mut in zip(i["entries"], res, i["caps"], i["mutated"])]

    def _pool(self, job):
        i = job.inputs
        with self.shared.pools:
            p = self.zgpu.Pool(devices=[0])
            try:
                return decode_all_result(lambda: _zgpu_decode_all(p, i["z"], i["cap"]))
            finally:
                p.close()

    def _release_caches(self, job):
        """every stream of the round is closed; all threads wait; the main thread releases the caches; all threads wait again"""
        sh = self.shared
        if sh.barrier.wait(sh.wait_s) == 0:
            def release():
                self.zgpu.load_library().zgpu_release_caches()
                sh.released.append({"on_main_thread": threading.current_thread() is threading.main_thread(), "at": round(time.monotonic(), 3)})
            sh.on_main(release)
        sh.barrier.wait(sh.wait_s)
        return "released"

    def _device(self, job):
        """decode_frames_device_src(verify) of the thread's two shards -> seek_index -> the first hash() of the fresh handle -> sums -> gather
        under verify_table from the shards of which one was changed. Nothing here waits for the device but the calls themselves."""
        i, b, ctx = job.inputs, self.shared.buffers[job.id], self.ctx
        res = ctx.decode_frames_device_src(b.mine.ptrs, b.mine.lens, b.out.ptrs, i["caps"], verify=True)
        out = {"decode": [(r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches) for r in res]}
        extra = {"decode": [list(devmem.full_key(r)) for r in res]}
        with ctx.seek_index_measured(b.good.ptrs, b.good.lens, only_unsized=True) as ix:
            out["index"] = [(x.status, x.kind, x.nrows) for x in ix.infos]
            infos = ix.hash(b.good.ptrs, b.good.lens)
            out["hash"] = [(x.status, x.state, x.frames, x.bytes) for x in infos]
            out["sums"] = [ix.sums(0), ix.sums(1)]
            res, _ = ctx.gather_ranges_indexed_device_src(ix, b.mine.ptrs, b.mine.lens, i["ranges"], b.gout.ptrs, i["gcaps"], verify_table=True)
            out["gather"] = [(r.status, r.written) for r in res]
            extra["gather"] = [[r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified] for r in res]
        out["_extra"] = extra
        return out

    # -- moved: the groups live in Shared; a barrier in front of every step keeps every object in one call at a time
    def _moved_create(self, job):
        i, sh, out = job.inputs, self.shared, []
        for g in i["groups"]:
            ctx = self.zgpu.Context(0)
            lock = Lockstep(self.zgpu.FrameDecoder(ctx), g["lz"])
            s = self.zgpu.CStreamingDecoder(ctx, data=g["sz"], copy_threads=1, **MODES[PIPE])
            sh.groups.append({"ctx": ctx, "lock": lock, "stream": s, "made_on": threading.get_ident()})
            out.append(lock.header)
        return out

    def _moved_step(self, job):
        i, sh = job.inputs, self.shared
        sh.barrier.wait(sh.wait_s)
        g = sh.groups[i["group"]]
        out = {"blocks": g["lock"].step()}
        try:
            d = g["stream"].read(i["read"])
            out["read"] = (len(d), d)
        except self.zgpu.ZgpuError as e:
            out["read"] = ("err", e.status)
        out["decode_all"] = decode_all_result(lambda: _zgpu_decode_all(g["ctx"], i["z"], i["cap"]))
        return out

    def _moved_close(self, job):
        i, sh, out = job.inputs, self.shared, []
        sh.barrier.wait(sh.wait_s)
        for gi in i["groups"]:
            g = sh.groups[gi]
            g["stream"].close()                      # mid-frame, the worker ahead
            g["lock"].d.close()                      # mid-frame
            g["ctx"].close()
            sh.destroyed.append({"group": gi, "made_on": g["made_on"], "destroyed_on": threading.get_ident()})
            out.append("closed")
        return out


def gpu_scenario(name, lists, deadline_s, buffers=None, dict_raw=None):
    """one scenario on the GPU: (result of run(), its Shared)"""
    parties = {"moved": 3, "churn": T, "serial": 1}.get(name, 1)
    sh = Shared(name, parties, buffers, dict_raw)

    def make(i):
        return GpuExecutor(sh, i)
    make.main_calls = sh.main_calls
    res = run(name, len(lists), lists, deadline_s, make)
    for th in res["threads"]:
        th.pop("ident", None)
    return res, sh


def main(argv):
    assert len(argv) == 3 and argv[1] == "--report", "usage: python tests/threadsuite.py --report PATH"
    path = argv[2]
    import zgpu
    zgpu.load_library(dev=False)
    t_build = time.monotonic()
    lists = build()
    corpus_dict = read_pack("dict_tests.pack")["dictionary"]
    serial = serial_list(lists)
    dev_jobs = [j for lst in lists["device"] for j in lst if j.kind == "device"]
    buffers = {"serial": {j.id: DeviceBuffers(j) for j in dev_jobs}, "device": {j.id: DeviceBuffers(j) for j in dev_jobs}}
    cov = coverage({sc: [[describe(j) for j in lst] for lst in ls] for sc, ls in lists.items()})
    report = {"seed": SEED, "build_s": round(time.monotonic() - t_build, 3), "scenarios": {}, "t_serial": {}, "deadline_s": {}, "ran": [],
              "job_counts": dict(collections.Counter(j.kind for j in serial)), "coverage": cov, "hung": None, "stopped": None}

    def write():
        with open(path + ".tmp", "w") as f:
            json.dump(report, f, indent=1)
        os.replace(path + ".tmp", path)

    t_all = time.monotonic()
    for name in SCENARIOS:
        if name == "serial":
            jobs, deadline = [serial], SERIAL_DEADLINE_S
        else:
            jobs = lists[name]
            deadline = max(30.0, 20.0 * report["t_serial"][name])
        res, sh = gpu_scenario(name, jobs, deadline, buffers.get(name), corpus_dict)
        report["scenarios"][name] = res
        report["deadline_s"][name] = deadline
        report["ran"].append(name)
        if name == "serial":
            took = collections.Counter()
            for r in res["threads"][0]["records"]:
                took[r["id"].split("/")[0]] += r.get("t1", 0) - r.get("t0", 0)
            report["t_serial"] = {sc: round(took[sc], 4) for sc in CONCURRENT}
        if name in ("serial", "moved"):
            res["destroyed"] = [dict(d, off_thread=d["made_on"] != d["destroyed_on"]) for d in sh.destroyed]
        if name in ("serial", "churn"):
            res["released"] = sh.released
        if res["hung"]:
            # a thread past the deadline cannot be joined: the report, and out at once — nothing further starts on the GPU
            report["hung"] = {"scenario": name, "threads": res["hung"]}
            write()
            sys.stdout.flush()
            os._exit(3)
        if name in buffers:
            res["main_checks"] = [{"job": jid, "wrong": b.check()} for jid, b in sorted(buffers[name].items())]
        write()
        bad = failures(res)
        if any(HIP_ERROR.search(r["detail"] or "") for _, r in bad):
            report["stopped"] = "%s met a HIP error: no further scenario was started" % name
            write()
            break
    report["wall_s"] = round(time.monotonic() - t_all, 3)
    write()
    print("threadsuite: %s; t_serial %s; wall %s s" % (", ".join("%s %d failures" % (n, len(failures(report["scenarios"][n]))) for n in report["ran"]),
                                                      report["t_serial"], report["wall_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
