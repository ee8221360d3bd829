"""zgpu_decode_frames_device (Context.decode_frames_device / decode_frames_to_tensors) on the GPU: the verdicts of zgpu_decode_frames, the
plaintext in device memory the caller owns. Destinations are slots of one torch device tensor pre-filled with a sentinel, with guard regions
around every slot; after a call the WHOLE arena is compared with what it must hold — plaintext where an entry succeeded, the sentinel
everywhere else (guards, the tail [written, cap) of a slot, every byte of a failed entry's slot)."""
import os
import random
import subprocess
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime, Context.decode_frames_to_tensors)

import zgpu
from devmem import ALL, MAGIC, SENT, Arena, entry_key, oracle_alone, xxh64
from golden_io import read_manifest, read_pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))   # zgdata: the workload generators


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def _run(c, entries, caps, shifts=None, **kw):
    a = Arena(caps, shifts)
    res = c.decode_frames_device(entries, a.ptrs, caps, **kw)
    assert len(res) == len(entries)
    return a, res


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_corpus_in_one_call(ctx):
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    assert len(names) == 101
    entries = [pack[n] for n in names]
    caps = [man[n]["size"] + (k % 3) * 100 for k, n in enumerate(names)]       # (some slots with room to spare: their tails stay untouched)
    host = ctx.decode_frames(entries, caps)
    a, res = _run(ctx, entries, caps, hash_max=ALL)
    plains = []
    for i, (z, cap, r, h) in enumerate(zip(entries, caps, res, host)):
        st, out = oracle_alone(z, cap)
        assert (st, r.status) == (0, 0), (names[i], st, r)
        assert h.data == out
        assert entry_key(r) == (h.status, len(h.data), h.nframes, h.checksums, h.checksum_mismatches, h.checksum_from_data, h.calculated_checksum), names[i]
        assert r.checksums_unverified == 0 and r.first_hashed == 1, names[i]
        plains.append(out)
    a.check(plains)
    st = ctx.frames_device_stats()
    assert st["submits"] == ctx.frames_submits() == 1 and st["scatter_launches"] == 1 and st["entries_alone"] == 0
    assert st["bytes_scattered"] == sum(len(p) for p in plains)
    assert st["frames_hashed"] == sum(r.nframes for r in res) and st["frames_not_hashed"] == 0


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_dict_corpus_takes_the_alone_path():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    raw = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")
    assert len(names) == 207
    entries = [pack[n] for n in names]
    caps = [man[n]["size"] for n in names]
    c = zgpu.Context(0)
    try:
        a, res = _run(c, entries, caps)
        assert all(r.status == zgpu.E_DICT_NOT_PROVIDED and r.written == 0 for r in res)   # (no dictionary registered: decode_all's answer)
        a.check([None] * len(entries))
        assert c.frames_device_stats()["entries_alone"] == 0
        c.add_dict(raw)
        host = c.decode_frames(entries, caps)
        a, res = _run(c, entries, caps, hash_max=ALL)
        plains = []
        for i, (z, cap, r, h) in enumerate(zip(entries, caps, res, host)):
            st, out = oracle_alone(z, cap, raw)
            assert (st, r.status, h.status) == (0, 0, 0), names[i]
            assert h.data == out and entry_key(r)[:5] == (0, len(out), h.nframes, h.checksums, h.checksum_mismatches), names[i]
            plains.append(out)
        a.check(plains)
        assert c.frames_device_stats()["entries_alone"] > 0
    finally:
        c.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _isolation_entries():
    import zgdata
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    good = [pack[n] for n in names[:12]]
    out = []
    for d in ("regress", "verdict_order"):
        for n in sorted(os.listdir(os.path.join(GOLDEN, d))):
            out.append(open(os.path.join(GOLDEN, d, n), "rb").read())
    fz = read_pack("fuzz_artifacts.pack")
    out += [fz[k] for k in sorted(fz)]
    rng = random.Random(7)
    for z in good[:6]:
        out.append(z[:rng.randrange(1, len(z))])                         # truncated
    out.append(bytes(rng.getrandbits(8) for _ in range(300)))               # garbage
    out.append(MAGIC + bytes(rng.getrandbits(8) for _ in range(200)))      # garbage behind a magic number
    out.append(b"")                                                         # empty
    out.append((0x184D2A53).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"12345")   # skippable frame only
    out.append(good[0] + good[1] + good[2])                                 # several frames
    out.append(good[3] + good[4][:len(good[4]) // 2])                       # a good frame, then a truncated one
    out.append(zgdata.zstd_compress(zgdata.text_like(300000, seed=3)))
    out += good
    caps = []
    for z in out:
        st, o = oracle_alone(z, 8 << 20)
        caps.append(len(o) if st == 0 else (1 << 20))
    caps[-1] -= 1                                                           # cap = size - 1: TargetTooSmall
    return out, caps


def test_isolation_and_order(ctx):
    entries, caps = _isolation_entries()
    verdicts = [oracle_alone(z, cap) for z, cap in zip(entries, caps)]
    assert verdicts[-1][0] == zgpu.E_TARGET_TOO_SMALL
    assert any(st not in (0, zgpu.E_TARGET_TOO_SMALL) for st, _ in verdicts) and any(st == 0 for st, _ in verdicts)
    orders = [list(range(len(entries))), list(range(len(entries)))]
    random.Random(1).shuffle(orders[1])
    for perm in orders:
        a, res = _run(ctx, [entries[i] for i in perm], [caps[i] for i in perm], shifts=[(7 * j) % 32 for j in range(len(perm))])
        for j, i in enumerate(perm):
            st, out = verdicts[i]
            assert res[j].status == st, (i, res[j], st)
            assert res[j].written == (len(out) if st == 0 else 0), i
        a.check([verdicts[i][1] if verdicts[i][0] == 0 else None for i in perm])


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def _raw_frame(payload):
    """one frame of raw blocks (single segment, a 4-byte Frame_Content_Size, a Content_Checksum): its plaintext is exactly payload"""
    z = MAGIC + bytes([0x20 | 0x80 | 0x04]) + len(payload).to_bytes(4, "little")
    cuts = list(range(0, len(payload), 128 << 10)) or [0]
    for k, o in enumerate(cuts):
        part = payload[o:o + (128 << 10)]
        z += ((1 if k == len(cuts) - 1 else 0) | (0 << 1) | (len(part) << 3)).to_bytes(3, "little") + part
    return z + (xxh64(payload) & 0xFFFFFFFF).to_bytes(4, "little")


def test_alignment_of_sources_and_destinations(ctx):
    rng = random.Random(0xA119)
    lengths = [0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 131071, 131072, 131073]
    entries, plains = [], []
    for rep in range(3):                                     # (odd lengths in front of each other: out_base takes many alignments)
        order = lengths[:]
        rng.shuffle(order)
        for n in order:
            p = rng.randbytes(n)
            z = _raw_frame(p)
            assert oracle_alone(z, n) == (0, p), n          # the hand-built frame is what the reference reads it as
            entries.append(z)
            plains.append(p)
    multi = [rng.randbytes(n) for n in (33, 0, 4097, 17, 131073, 1)]
    z = b"".join(_raw_frame(p) for p in multi)
    assert oracle_alone(z, 1 << 20) == (0, b"".join(multi))
    entries.append(z)                                        # one entry of several frames: they lie back to back in its destination
    plains.append(b"".join(multi))
    while len(entries) % 32:                                 # every destination offset 0 .. 31 is used, by entries of every kind
        p = rng.randbytes(rng.choice([15, 33, 4097]))
        entries.append(_raw_frame(p))
        plains.append(p)
    for turn in range(2):
        shifts = [(j + 13 * turn) % 32 for j in range(len(entries))]
        assert set(shifts) == set(range(32))
        caps = [len(p) + (j % 2) * 5 for j, p in enumerate(plains)]
        a, res = _run(ctx, entries, caps, shifts=shifts, hash_max=ALL)
        for j, (r, p) in enumerate(zip(res, plains)):
            assert (r.status, r.written, r.checksum_mismatches, r.checksums_unverified) == (0, len(p), 0, 0), (j, r)
        assert res[len(lengths) * 3].nframes == len(multi) and res[len(lengths) * 3].checksums == len(multi)
        a.check(plains)
        assert len(set(ptr % 32 for ptr in a.ptrs)) == 32


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def _cut(entries, S):
    """the submits zgpu_decode_frames cuts (zg_frames.cpp): by the plaintext bound and by the input bytes"""
    groups, cur, pb, ib = [], [], 0, 0
    for i, z in enumerate(entries):
        b = zgpu.plaintext_bound(z)
        if cur and (pb + b > S or ib + len(z) > S):
            groups.append(cur)
            cur, pb, ib = [], 0, 0
        cur.append(i)
        pb += b
        ib += len(z)
    if cur:
        groups.append(cur)
    return groups


def test_several_submits(ctx, monkeypatch):
    import zgdata
    rng = random.Random(5)
    texts = [zgdata.text_like(300000 + 1000 * k, seed=40 + k) for k in range(6)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    junk = [bytes(rng.getrandbits(8) for _ in range(1000)) for _ in range(3)]
    entries, plains = [], []
    for k in range(36):
        entries.append(comp[k % 6])
        plains.append(texts[k % 6])
    entries[12:12] = [MAGIC + junk[0] * 2200, MAGIC + junk[1] * 700, MAGIC + junk[2] * 700]   # input that yields nothing; the first one a submit of its own
    plains[12:12] = [None, None, None]
    caps = [len(p) if p is not None else 4096 for p in plains]
    S = 2 << 20
    a1 = Arena(caps)
    one = ctx.decode_frames_device(entries, a1.ptrs, caps)
    a1.check(plains)
    assert ctx.frames_submits() == 1
    monkeypatch.setenv("ZGPU_FRAMES_SUBMIT_BYTES", str(S))
    c = zgpu.Context(0, dev=True)
    try:
        a, res = _run(c, entries, caps)
        st = c.frames_device_stats()
    finally:
        c.close()
    groups = _cut(entries, S)
    assert len(groups) >= 4 and st["submits"] == len(groups)
    assert [entry_key(r) for r in res] == [entry_key(r) for r in one]
    assert [r.status == 0 for r in res] == [p is not None for p in plains]
    a.check(plains)
    with_success = sum(1 for g in groups if any(res[i].status == 0 for i in g))
    assert 0 < with_success < len(groups) and st["scatter_launches"] == with_success
    assert st["entries_alone"] == 0 and st["bytes_scattered"] == sum(r.written for r in res)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_wrong_pointers_become_a_status(ctx):
    import zgdata
    text = zgdata.text_like(100000, seed=21)
    z = zgdata.zstd_compress(text)
    pinned = torch.full((len(text) + 512,), SENT, dtype=torch.uint8).pin_memory()
    caps = [len(text)] * 6
    a = Arena(caps)
    ptrs = list(a.ptrs)
    ptrs[1] = 0                       # NULL with cap > 0
    ptrs[3] = pinned.data_ptr()       # pinned HOST memory: the device could write it, the contract says device memory
    ptrs[4] = 16                      # inside no allocation
    res = ctx.decode_frames_device([z] * 6, ptrs, caps)
    for i in (1, 3, 4):
        assert (res[i].status, res[i].written, res[i].nframes) == (zgpu.E_BAD_ARG, 0, 0), (i, res[i])
    for i in (0, 2, 5):
        assert (res[i].status, res[i].written) == (0, len(text)), (i, res[i])
    a.check([text, None, text, None, None, text])
    assert bytes(pinned.numpy()) == bytes([SENT]) * len(pinned)
    # a range that leaves its allocation: the slot's address with a capacity beyond the arena's end
    beyond = a.t.data_ptr() + a.t.numel() - 1000
    big = torch.cuda.get_device_properties(0).total_memory * 4
    res = ctx.decode_frames_device([z, z], [beyond, a.ptrs[0]], [big, caps[0]])
    assert res[0].status == zgpu.E_BAD_ARG and res[1].status == 0
    a.check([text, None, text, None, None, text])


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_checksums_hashed_on_the_device_or_counted(ctx):
    import seqframes
    import zgdata
    assert seqframes.libzstd() is zgdata.libzstd()
    z_small, p_small = seqframes.frame([(40, 7, 30), (500, 300, 64)], tail=900, seed=3)              # Content_Checksum on
    z_long, p_long = seqframes.frame([(60000, 1000, 3000), (20000, 50000, 9000)], tail=8000, seed=4)
    assert len(p_long) > 65536 > len(p_small)
    text = zgdata.text_like(50000, seed=8)
    z_text = zgdata.zstd_compress(text)
    z_flip = bytearray(z_text)
    z_flip[-1] ^= 0x40                                     # one byte of the stored checksum
    z_none = zgdata.zstd_compress(text, checksum=False)
    entries = [z_small, bytes(z_flip), z_long, z_none, z_text + z_long]
    plains = [p_small, text, p_long, text, text + p_long]
    caps = [len(p) for p in plains]
    low = lambda b: xxh64(b) & 0xFFFFFFFF                 # noqa: E731

    a, res = _run(ctx, entries, caps, hash_max=65536)      # z_long is longer than hash_max_bytes
    a.check(plains)
    assert [(r.status, r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed) for r in res] == [
        (0, 1, 1, 0, 0, 1), (0, 1, 1, 1, 0, 1), (0, 1, 1, 0, 1, 0), (0, 1, 0, 0, 0, 1), (0, 2, 2, 0, 1, 1)]
    assert res[0].calculated_checksum == res[0].checksum_from_data == low(p_small)
    assert res[1].calculated_checksum == low(text) != res[1].checksum_from_data
    assert res[2].calculated_checksum == 0 and res[2].checksum_from_data == low(p_long)
    assert res[3].calculated_checksum == low(text) and res[3].checksum_from_data == 0
    st = ctx.frames_device_stats()
    assert (st["frames_hashed"], st["frames_not_hashed"]) == (4, 2)

    a, res = _run(ctx, entries, caps, hash_max=1 << 20)    # raised: the long frame is verified
    a.check(plains)
    assert [(r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed) for r in res] == [
        (1, 0, 0, 1), (1, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (2, 0, 0, 1)]
    assert res[2].calculated_checksum == res[2].checksum_from_data == low(p_long)
    host = ctx.decode_frames(entries, caps)
    assert [entry_key(r) for r in res] == [(h.status, h.written, h.nframes, h.checksums, h.checksum_mismatches, h.checksum_from_data,
                                       h.calculated_checksum) for h in host]

    a, res = _run(ctx, entries, caps, no_hash=True)        # flags bit 0: nothing is hashed
    a.check(plains)
    assert [(r.status, r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed, r.calculated_checksum) for r in res] == [
        (0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 0, 0), (0, 0, 0, 0, 0, 0), (0, 2, 0, 2, 0, 0)]
    st = ctx.frames_device_stats()
    assert (st["frames_hashed"], st["frames_not_hashed"]) == (0, 6)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_scale_to_tensors(ctx):
    import zgdata
    size = 8 << 20
    texts = [zgdata.text_like(size, seed=0x800 + k) for k in range(8)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    want = [torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:0") for t in texts]
    entries = [comp[k % 8] for k in range(64)]
    tensors, res = ctx.decode_frames_to_tensors(entries)
    assert len(tensors) == len(res) == 64
    for k, (t, r) in enumerate(zip(tensors, res)):
        assert (r.status, r.written, r.nframes, r.checksums) == (0, size, 1, 1), (k, r)
        assert r.checksums_unverified == 1 and r.first_hashed == 0, k          # (8 MiB is beyond the 4 MiB default of hash_max_bytes)
        assert t.device.type == "cuda" and t.dtype == torch.uint8 and t.numel() == size and t.data_ptr() % 256 == 0
        assert torch.equal(t, want[k % 8]), k
    for k in (0, 63):
        assert oracle_alone(entries[k], size) == (0, tensors[k].cpu().numpy().tobytes())
    st = ctx.frames_device_stats()
    assert st["bytes_scattered"] == 64 * size and st["scatter_launches"] == st["submits"] >= 1
    # explicit capacities, a failing entry among them: its view is empty
    tensors, res = ctx.decode_frames_to_tensors([comp[0], comp[1][:1000], b""], caps=[size, size, 0])
    assert [r.status == 0 for r in res] == [True, False, True] and [t.numel() for t in tensors] == [size, 0, 0]
    assert torch.equal(tensors[0], want[0])


def test_import_zgpu_does_not_import_torch():
    code = "import sys; sys.path.insert(0, %r); import zgpu; zgpu.load_library(); assert 'torch' not in sys.modules" % os.path.join(ROOT, "zstd-rs_amd")
    subprocess.check_call([sys.executable, "-c", code])
