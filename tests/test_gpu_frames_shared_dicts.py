"""zgpu_set_frames_shared_dicts on the GPU: dictionary frames whose id is registered are decoded INSIDE the shared submits of
zgpu_decode_frames, zgpu_decode_frames_device and zgpu_decode_frames_device_src (zg_k_dictfill puts the dictionary in front of every such
frame), and every entry still gets what FrameDecoder::decode_all of that entry alone gives. Every comparison is against the oracle with the
same dictionaries registered, never against the library itself. Device destinations are slots of one torch tensor full of a sentinel with
guard regions around every slot; after a call the WHOLE arena is compared with what it must hold."""
import os
import random
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import dictframes
import oracle
import zgpu
from devmem import ALL, MAGIC, Arena, Sources, entry_key, xxh32
from golden_io import read_manifest, read_pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zstd-rs_amd"))
SKIP = (0x184D2A53).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"12345"
K = 128 << 10


class Want:
    """what the oracle says of one entry alone: status, bytes, and the checksum fields of zgpu_entry_result. pieces: the entry's frames
    and skippable frames in order (their concatenation is the entry); dicts: the raw dictionaries registered"""

    def __init__(self, pieces, cap, dicts):
        self.entry = b"".join(pieces)

        def dec():
            d = oracle.FrameDecoder()
            for raw in dicts:
                d.add_dict(raw)
            return d
        self.status, out = dec().decode_all(self.entry, cap)
        self.data = out if self.status == 0 else None
        self.key = (self.status, 0, 0, 0, 0, 0, 0)
        if self.status == 0:
            frames = [p for p in pieces if p[:4] == MAGIC]
            n = ck = bad = 0
            first = (0, 0)
            for z in frames:
                st, plain = dec().decode_all(z, 1 << 24)
                assert st == 0
                has = bool(z[4] & 4)
                stored, calc = int.from_bytes(z[-4:], "little") if has else 0, xxh32(plain)
                if n == 0:
                    first = (stored, calc)
                n += 1
                ck += has
                bad += has and stored != calc
            self.key = (0, len(out), n, ck, bad) + first


def _three_calls(c, wants, caps, shifts=None, src_shifts=None):
    """the three calls on the same entries: every result field and every destination byte as the oracle's. Returns the dict stats of each."""
    entries = [w.entry for w in wants]
    plains = [w.data for w in wants]
    stats = {}
    host = c.decode_frames(entries, caps)
    stats["host"] = (c.frames_dict_stats(), c.frames_submits(), None, None)
    for i, (r, w) in enumerate(zip(host, wants)):
        assert entry_key(r) == w.key and r.data == w.data, ("host", i, entry_key(r), w.key)
    a = Arena(caps, shifts)
    res = c.decode_frames_device(entries, a.ptrs, caps, hash_max=ALL)
    stats["device"] = (c.frames_dict_stats(), c.frames_submits(), c.frames_device_stats(), None)
    for i, (r, w) in enumerate(zip(res, wants)):
        assert entry_key(r) == w.key, ("device", i, entry_key(r), w.key)
        assert r.checksums_unverified == 0 and r.first_hashed == (1 if w.status == 0 and w.key[2] else 0), ("device", i)
    a.check(plains)
    b = Arena(caps, shifts)
    s = Sources(entries, src_shifts)
    res = c.decode_frames_device_src(s.ptrs, s.lens, b.ptrs, caps, hash_max=ALL)
    stats["device_src"] = (c.frames_dict_stats(), c.frames_submits(), c.frames_device_stats(), c.frames_device_src_stats())
    for i, (r, w) in enumerate(zip(res, wants)):
        assert entry_key(r) == w.key, ("device_src", i, entry_key(r), w.key)
    b.check(plains)
    return stats


@pytest.fixture(scope="module")
def corpus():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    names = sorted(n for n in man if n != "dictionary")
    assert len(names) == 207
    return pack["dictionary"], [pack[n] for n in names], [man[n]["size"] for n in names]


@pytest.fixture(scope="module")
def corpus_wants(corpus):
    raw, frames, sizes = corpus
    return [Want([z], n, [raw]) for z, n in zip(frames, sizes)]   # (computed once, shared, never changed)


@pytest.fixture(scope="module")
def ctx(corpus):
    c = zgpu.Context(0)
    c.add_dict(corpus[0])
    c.set_frames_shared_dicts(True)
    yield c
    c.close()


# 1, 2 ------------------------------------------------------------------------------------------------------------------------------
def test_dict_corpus_shared_then_switched_off(corpus, corpus_wants):
    raw, frames, sizes = corpus
    c = zgpu.Context(0)
    try:
        assert c.frames_shared_dicts() is False                                   # the default
        c.add_dict(raw)
        c.set_frames_shared_dicts(True)
        assert c.frames_shared_dicts() is True
        assert all(w.status == 0 for w in corpus_wants)
        caps = [n + (k % 3) * 100 for k, n in enumerate(sizes)]                   # (some slots with room to spare: their tails stay untouched)
        stats = _three_calls(c, corpus_wants, caps, shifts=[(7 * k) % 16 for k in range(207)])
        for call, (ds, submits, dev, src) in stats.items():
            assert ds["frames_shared"] == 207 and ds["entries_alone"] == 0, (call, ds)
            assert submits == 1 and ds["fill_launches"] == 2 and ds["bytes_replicated"] > 207 * len(raw) - 207 * 4096, (call, ds)
            if dev is not None:
                assert dev["entries_alone"] == 0 and dev["scatter_launches"] == 1, (call, dev)
            if src is not None:
                assert src["input_bytes_to_host"] == 0 and src["gather_launches"] == 1, src
        # the switch off on the same context: the alone path again, the same results
        c.set_frames_shared_dicts(False)
        stats = _three_calls(c, corpus_wants, caps)
        for call, (ds, submits, dev, src) in stats.items():
            assert ds == {"frames_shared": 0, "fill_launches": 0, "bytes_replicated": 0, "fill_us": 0, "entries_alone": 0}, (call, ds)
            if dev is not None:
                assert dev["entries_alone"] == 207, (call, dev)
            if src is not None:
                assert src["input_bytes_to_host"] == sum(len(z) for z in frames), src
    finally:
        c.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_mixing_and_order(ctx, corpus):
    raw, frames, sizes = corpus
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    plain_names = sorted(man)[:10]
    items = [([z], n) for z, n in zip(frames[:24], sizes[:24])]
    items += [([pack[n]], man[n]["size"]) for n in plain_names]
    items.append(([frames[30], pack[plain_names[0]], SKIP, frames[31]], sizes[30] + man[plain_names[0]]["size"] + sizes[31]))
    items.append(([], 0))                                                         # an empty entry
    items.append(([frames[40], frames[41]], sizes[40] + sizes[41] - 1))           # two dictionary frames, a byte short: TargetTooSmall
    wants = [Want(p, cap, [raw]) for p, cap in items]
    assert wants[-1].status == 12 and wants[-2].key[:3] == (0, 0, 0) and wants[-3].key[2] == 3
    for seed in (1, 2, 3):
        order = list(range(len(items)))
        random.Random(seed).shuffle(order)
        stats = _three_calls(ctx, [wants[i] for i in order], [items[i][1] for i in order], shifts=[(3 * k + seed) % 16 for k in order])
        for call, (ds, submits, dev, src) in stats.items():
            assert submits == 1 and ds["entries_alone"] == 0 and ds["frames_shared"] == 24 + 2, (call, ds)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_isolation_of_mutated_dictionary_frames(ctx, corpus):
    raw, frames, sizes = corpus
    rng = random.Random(0x150)
    picks = [k for k in range(207) if dictframes.first_block(frames[k])[0] == 2 and dictframes.first_block(frames[k])[2] is not None][:12]
    assert len(picks) == 12
    items = []
    for k in picks:
        z, n = frames[k], sizes[k]
        hdr = 5 + 4 + (2 if z[4] >> 6 == 1 else 1)                               # single-segment headers: descriptor, id, content size
        body = hdr + 3
        muts = []
        for lo, hi in ((body, body + (len(z) - body) // 3), (body + 2 * (len(z) - body) // 3, len(z) - 5)):   # literals section; sequence bitstream
            m = bytearray(z)
            for _ in range(3):
                m[rng.randrange(lo, max(hi, lo + 1))] ^= 1 << rng.randrange(8)
            muts.append(bytes(m))
        muts.append(z[:len(z) - rng.randrange(5, len(z) // 2)])                  # a truncated tail
        muts.append(z[:-1] + bytes([z[-1] ^ 0x40]))                              # a flipped stored checksum
        for m in muts:
            items += [([z], n), ([m], n), ([z], n)]                              # a good copy on either side
    wants = [Want(p, cap, [raw]) for p, cap in items]
    bad = [w for w in wants[1::3]]
    assert sum(w.status != 0 for w in bad) >= 12 and sum(w.status == 0 and w.key[4] == 1 for w in bad) >= 12   # errors, and mismatches that only count
    assert all(w.status == 0 for w in wants[0::3])
    stats = _three_calls(ctx, wants, [cap for _, cap in items], shifts=[(5 * k) % 16 for k in range(len(items))])
    for call, (ds, submits, dev, src) in stats.items():
        assert submits == 1 and ds["entries_alone"] == 0, (call, ds)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_dictionaries_and_an_unregistered_id(corpus):
    raw, frames, sizes = corpus
    did = int.from_bytes(raw[4:8], "little")
    raw2 = raw[:4] + (did + 1).to_bytes(4, "little") + raw[8:]
    c = zgpu.Context(0)
    try:
        assert c.add_dict(raw) == did and c.add_dict(raw2) == did + 1
        c.set_frames_shared_dicts(True)
        items = []
        for k in range(60):
            z = dictframes.patch_dict_id(frames[k], did + 1) if k % 3 == 1 else frames[k]
            items.append(([z], sizes[k]))
        items.insert(17, ([dictframes.patch_dict_id(frames[70], did + 2)], sizes[70]))     # a third id nobody registered
        wants = [Want(p, cap, [raw, raw2]) for p, cap in items]
        assert [w.status for w in wants] == [0] * 17 + [zgpu.E_DICT_NOT_PROVIDED] + [0] * 43
        stats = _three_calls(c, wants, [cap for _, cap in items])
        for call, (ds, submits, dev, src) in stats.items():
            assert submits == 1 and ds["frames_shared"] == 60 and ds["entries_alone"] == 1, (call, ds)   # (the unregistered id: today's path, today's answer)
    finally:
        c.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def reach_cases(corpus):
    """(names of the hand-built frames, [(pieces, cap)], wants): the dictframes cases at the edges of the reach and the corpus frames whose
    first block's tables can only come from the dictionary (tests/test_gpu_poison.py runs them under other memory histories)"""
    raw, frames, sizes = corpus
    did = int.from_bytes(raw[4:8], "little")
    # the content's length, from the oracle: the longest reach from the frame's first byte that still decodes
    f = dictframes
    lo, hi = 1, len(raw)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        st, _ = _fresh(raw).decode_all(f.frame(did, f.seq_block(mid, last=True)), 1 << 16)
        lo, hi = (mid, hi) if st == 0 else (lo, mid - 1)
    content = lo
    assert len(raw) - 2000 < content < len(raw)
    built = {
        "first_byte_of_the_content": f.frame(did, f.seq_block(content, last=True)),
        "first_byte_behind_literals": f.frame(did, f.lit_block(100), f.seq_block(content + 100, last=True)),
        "last_byte_across_into_the_frame": f.frame(did, f.lit_block(100), f.seq_block(101, last=True)),   # 1 byte of the dictionary, then 2 of the frame
        "last_byte_then_own_output": f.frame(did, f.seq_block(1, last=True)),                          # the match's own first byte repeats
        "repeat_code_1": f.frame(did, f.seq_block_value(1, last=True)),
        "repeat_code_2": f.frame(did, f.seq_block_value(2, last=True)),
        "repeat_code_3": f.frame(did, f.seq_block_value(3, last=True)),
        "repeat_codes_in_a_row": f.frame(did, f.seq_block_value(2), f.seq_block_value(3), f.seq_block_value(1, last=True)),
        "one_byte_in_front_of_the_dictionary": f.frame(did, f.seq_block(content + 1, last=True)),
        "one_byte_in_front_behind_literals": f.frame(did, f.lit_block(77), f.seq_block(content + 78, last=True)),
    }
    # first blocks whose tables can only come from the dictionary: Treeless literals; Repeat-mode LL, OF and ML
    treeless = [k for k in range(207) if f.first_block(frames[k])[1] == 3]
    repeat = [k for k in range(207) if f.first_block(frames[k])[2] is not None and f.first_block(frames[k])[2] & 0xFC == 0xFC]
    assert treeless and repeat
    items = [([z], 1 << 12) for z in built.values()]
    items += [([frames[k]], sizes[k]) for k in treeless[:4] + repeat[:4]]
    return list(built), items, [Want(p, cap, [raw]) for p, cap in items]


def test_hand_built_edges_of_the_reach(ctx, corpus):
    built, items, wants = reach_cases(corpus)
    by_name = dict(zip(built, wants))
    # (repeat code 3 with a literal length of 0 is history[0] - 1: with this dictionary's history the oracle answers 0 or ZeroOffset — it decides)
    assert all(by_name[n].status == 0 for n in built if not n.startswith("one_byte_in_front") and n != "repeat_code_3"), {n: w.status for n, w in by_name.items()}
    assert by_name["repeat_code_3"].status in (0, 51)
    assert by_name["one_byte_in_front_of_the_dictionary"].status == by_name["one_byte_in_front_behind_literals"].status == 53   # NotEnoughBytesInDictionary
    assert by_name["first_byte_of_the_content"].data[:3] != by_name["last_byte_then_own_output"].data[:3]
    for shift in (1, 15):
        stats = _three_calls(ctx, wants, [cap for _, cap in items], shifts=[shift] * len(items), src_shifts=[shift] * len(items))
        for call, (ds, submits, dev, src) in stats.items():
            assert submits == 1 and ds["entries_alone"] == 0, (call, ds)


def _fresh(raw):
    d = oracle.FrameDecoder()
    d.add_dict(raw)
    return d


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_drain_case_goes_alone(ctx, corpus):
    """more than 1 MiB of raw output in ONE dictionary frame in front of a match that starts in the dictionary: decode_all drains inside the
    frame, the device still holds the drained bytes in place, zg_k_exact refuses the frame (zg_exact.h) and its entry — that entry only — is
    decoded again alone, on the reference's schedule"""
    raw, frames, sizes = corpus
    did = int.from_bytes(raw[4:8], "little")
    f = dictframes
    z = f.frame(did, *([f.raw_block(K, i) for i in range(9)] + [f.seq_block(2 * K + 4 + 10, last=True)]))
    items = [([x], n) for x, n in zip(frames[100:110], sizes[100:110])] + [([z], 9 * K + 64)] + [([x], n) for x, n in zip(frames[110:120], sizes[110:120])]
    wants = [Want(p, cap, [raw]) for p, cap in items]
    assert all(w.status == 0 for w in wants) and len(wants[10].data) == 9 * K + 7
    stats = _three_calls(ctx, wants, [cap for _, cap in items])
    for call, (ds, submits, dev, src) in stats.items():
        assert ds["entries_alone"] == 1 and ds["frames_shared"] == 20, (call, ds)
        if dev is not None:
            assert dev["entries_alone"] == 1, (call, dev)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_many_entries_from_device_sources(ctx, corpus, corpus_wants):
    raw, frames, sizes = corpus
    n = 2048
    idx = [k % 207 for k in range(n)]
    entries, caps = [frames[k] for k in idx], [sizes[k] for k in idx]
    a = Arena(caps, shifts=[(11 * j) % 16 for j in range(n)])
    s = Sources(entries, [(5 * j) % 29 for j in range(n)])
    res = ctx.decode_frames_device_src(s.ptrs, s.lens, a.ptrs, caps, hash_max=ALL)
    ds, src = ctx.frames_dict_stats(), ctx.frames_device_src_stats()
    assert ctx.frames_submits() == 1 and ds["entries_alone"] == 0 and ds["frames_shared"] == n and src["input_bytes_to_host"] == 0, (ds, src)
    for j in range(0, n, 64):                                                     # every 64th entry against the oracle, computed here
        w = Want([entries[j]], caps[j], [raw])
        assert entry_key(res[j]) == w.key and w.data == corpus_wants[idx[j]].data, j
    for j, r in enumerate(res):
        assert entry_key(r) == corpus_wants[idx[j]].key, j
    a.check([corpus_wants[k].data for k in idx])
