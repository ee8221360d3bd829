"""zgpu_decode_frames_device_src (Context.decode_frames_device_src / decode_tensors) on the GPU: compressed input that lies in device memory,
decoded into device memory. The reference for every case is zgpu_decode_frames_device on HOST copies of the same entries with the same
destination layout and options: the results must be equal field for field and the two arenas — plaintext, untouched tails, guard bytes,
untouched slots of failed entries — byte for byte; the source memory must be unchanged afterwards. Pointers the contract refuses are refused
by the host's check before anything is launched, so none of these cases makes a kernel touch memory it must not."""
import ctypes as C
import os
import random
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import zgpu
from devmem import ALL, MAGIC, Arena, RawDevice, RawSources, Sources, full_key, oracle_alone, xxh64
from golden_io import read_manifest, read_pack
from test_gpu_decode_frames_device import GOLDEN, _cut, _isolation_entries, _raw_frame

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


def _both(c, entries, caps, shifts=None, src_shifts=None, src=None, **kw):
    """the host-source call and the device-source call on the same entries, destination layout and options: equal results, equal arenas,
    sources untouched, the same number of submits. Returns (arena of the device-source call, its results, its stats)."""
    a = Arena(caps, shifts)
    ref = c.decode_frames_device(entries, a.ptrs, caps, **kw)
    ref_submits, ref_stats = c.frames_submits(), c.frames_device_stats()
    b = Arena(caps, shifts)
    s = src or Sources(entries, src_shifts)
    res = c.decode_frames_device_src(s.ptrs, s.lens, b.ptrs, caps, **kw)
    assert len(res) == len(entries)
    for j, (x, y) in enumerate(zip(ref, res)):
        assert full_key(x) == full_key(y), (j, full_key(x), full_key(y))
    torch.cuda.synchronize()
    assert torch.equal(a.t, b.t)
    assert s.unchanged()
    assert c.frames_submits() == ref_submits
    dst, st = c.frames_device_stats(), c.frames_device_src_stats()
    assert dst == {**ref_stats, "scatter_us": dst["scatter_us"]}       # (scatter and hash are reported for this call as for that one)
    assert st["walk_launches"] == (2 if any(s.lens) else 1)           # count and emit, once for the whole call
    return b, res, st


def _all_golden():
    pack = read_pack("decodecorpus.pack")
    out = [pack[n] for n in sorted(pack) if n.endswith(".zst")]
    fz = read_pack("fuzz_artifacts.pack")
    out += [fz[k] for k in sorted(fz)]
    for d in ("regress", "verdict_order"):
        out += [open(os.path.join(GOLDEN, d, n), "rb").read() for n in sorted(os.listdir(os.path.join(GOLDEN, d)))]
    dp = read_pack("dict_tests.pack")
    out += [dp[n] for n in sorted(dp) if n != "dictionary"][:40]
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_golden_corpus_in_one_call(ctx):
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    entries = _all_golden()
    assert len(entries) > 190
    caps = [1 << 20] * len(entries)
    names = sorted(man)
    for k, n in enumerate(names):
        assert entries[k] == pack[n]
        caps[k] = man[n]["size"] + (k % 3) * 100
    b, res, st = _both(ctx, entries, caps, hash_max=ALL)
    for k, n in enumerate(names):
        stt, out = oracle_alone(entries[k], caps[k])
        assert (stt, res[k].status, res[k].written) == (0, 0, len(out)), n
        o = b.offs[k]
        assert b.t[o:o + len(out)].cpu().numpy().tobytes() == out, n
    assert any(r.status == zgpu.E_DICT_NOT_PROVIDED for r in res) and any(r.status not in (0, zgpu.E_DICT_NOT_PROVIDED) for r in res)
    assert ctx.frames_device_stats()["entries_alone"] == 0 and st["input_bytes_to_host"] == 0
    assert st["gather_launches"] == ctx.frames_submits() == 1 and st["skeleton_bytes"] > 0


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_seqframes_set(ctx):
    import seqframes
    frames = seqframes.all_frames()
    entries = [z for _, _, z, _ in frames]
    plains = [p for _, _, _, p in frames]
    caps = [len(p) for p in plains]
    b, res, st = _both(ctx, entries, caps, src_shifts=[(5 * j) % 29 for j in range(len(entries))], hash_max=ALL)
    for (fam, name, _, p), r in zip(frames, res):
        assert (r.status, r.written, r.checksum_mismatches) == (0, len(p), 0), (fam, name, r)
    b.check(plains)
    assert st["input_bytes_to_host"] == 0


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_4096_text_frames_of_128k(ctx):
    import zgdata
    size, n = 128 << 10, 4096
    texts = [zgdata.text_like(size, seed=0x4096 + k) for k in range(8)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    entries = [comp[k % 8] for k in range(n)]
    caps = [size] * n
    b, res, st = _both(ctx, entries, caps)
    assert all((r.status, r.written, r.nframes, r.checksum_mismatches, r.checksums_unverified) == (0, size, 1, 0, 0) for r in res)
    want = [torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:0") for t in texts]
    for k in list(range(16)) + [n // 2, n - 2, n - 1]:
        assert torch.equal(b.t[b.offs[k]:b.offs[k] + size], want[k % 8]), k
    total_in = sum(len(z) for z in entries)
    print("device-src stats, 4096 x 128 KiB text:", st, "input bytes", total_in)
    assert st["input_bytes_to_host"] == 0                     # no byte of the input crossed to the host
    assert st["skeleton_bytes"] * 64 <= total_in              # the skeleton is at most 1/64 of it
    assert st["walk_launches"] == 2 and st["gather_launches"] == ctx.frames_submits()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_mix_of_failing_entries_and_permutation(ctx):
    entries, caps = _isolation_entries()          # failing, truncated, garbage, empty, skippable-only, several frames, TargetTooSmall
    assert b"" in entries
    base = None
    orders = [list(range(len(entries))), list(range(len(entries)))]
    random.Random(2).shuffle(orders[1])
    for perm in orders:
        b, res, st = _both(ctx, [entries[i] for i in perm], [caps[i] for i in perm], shifts=[(7 * j) % 32 for j in range(len(perm))],
                           src_shifts=[(3 * j) % 18 for j in range(len(perm))])
        back = [None] * len(perm)
        for j, i in enumerate(perm):
            back[i] = full_key(res[j])
        if base is None:
            base = back
        assert back == base                        # permuting the entries permutes the results
        assert st["input_bytes_to_host"] == 0
    sts = set(k[0] for k in base)
    assert 0 in sts and zgpu.E_TARGET_TOO_SMALL in sts and len(sts) > 4


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_sources_and_flush_end(ctx):
    rng = random.Random(0x5A11)
    lengths = [0, 1, 2, 3, 15, 16, 17, 31, 33, 4095, 4097, 65537, 131071]
    entries, plains = [], []
    for n in lengths + lengths[::-1] + lengths[3:] + lengths[:3]:
        p = rng.randbytes(n)
        entries.append(_raw_frame(p))          # (odd compressed lengths: 13 bytes of framing around the payload)
        plains.append(p)
    import zgdata
    text = zgdata.text_like(70001, seed=77)
    for k in range(36 - len(entries) % 36):
        entries.append(zgdata.zstd_compress(text[:70001 - 997 * k]))
        plains.append(text[:70001 - 997 * k])
    assert len(set(len(z) % 16 for z in entries)) >= 8
    for turn in range(2):
        src_shifts = [(j + 5 * turn) % 18 for j in range(len(entries))]           # offsets 0 .. 17 behind a 32-byte boundary
        assert set(src_shifts) == set(range(18))
        raw = RawSources(entries, src_shifts)
        try:
            caps = [len(p) + (j % 2) * 5 for j, p in enumerate(plains)]
            b, res, st = _both(ctx, entries, caps, shifts=[(11 * j + turn) % 32 for j in range(len(entries))], src=raw, hash_max=ALL)
            for j, (r, p) in enumerate(zip(res, plains)):
                assert (r.status, r.written, r.checksum_mismatches) == (0, len(p), 0), (j, r)
            b.check(plains)                                                       # guard bytes on both sides of every destination intact
            assert st["input_bytes_to_host"] == 0
        finally:
            raw.free()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_wrong_source_pointers_become_a_status(ctx):
    import zgdata
    text = zgdata.text_like(100000, seed=21)
    z = zgdata.zstd_compress(text)
    good = Sources([z] * 6)
    host_buf = C.create_string_buffer(z, len(z))                      # pageable host memory
    pinned = torch.frombuffer(bytearray(z), dtype=torch.uint8).pin_memory()
    raw = RawDevice(z)                                                # an allocation of exactly len(z) bytes
    try:
        ptrs, lens = list(good.ptrs), list(good.lens)
        ptrs[1] = C.addressof(host_buf)
        ptrs[2] = pinned.data_ptr()
        ptrs[3], lens[3] = raw.ptr + 100, len(z)                      # crosses the end of its allocation by 100 bytes
        ptrs[4] = 0                                                   # NULL with a length
        caps = [len(text)] * 6
        a = Arena(caps)
        res = ctx.decode_frames_device_src(ptrs, lens, a.ptrs, caps)
        for i in (1, 2, 3, 4):
            assert (res[i].status, res[i].written, res[i].nframes) == (zgpu.E_BAD_ARG, 0, 0), (i, res[i])
        for i in (0, 5):
            assert (res[i].status, res[i].written) == (0, len(text)), (i, res[i])
        a.check([text, None, None, None, None, text])
        # the same allocation, used inside its bounds: the whole of it, and a range that ends flush with it
        res = ctx.decode_frames_device_src([raw.ptr, raw.ptr + 100], [len(z), len(z) - 100], [a.ptrs[1], a.ptrs[2]], caps[:2])
        assert (res[0].status, res[0].written) == (0, len(text)) and res[1].status not in (0, zgpu.E_BAD_ARG)
        a.check([text, text, None, None, None, text])
        # a destination that is host memory, with a good source: that entry only
        res = ctx.decode_frames_device_src(good.ptrs[:2], good.lens[:2], [pinned.data_ptr(), a.ptrs[3]], [len(z), caps[3]])
        assert res[0].status == zgpu.E_BAD_ARG and (res[1].status, res[1].written) == (0, len(text))
        a.check([text, text, None, text, None, text])
        assert good.unchanged() and raw.read() == z and bytes(pinned.numpy()) == z and host_buf.raw == z
        # a length of 0: nothing is checked, nothing is read — any pointer value will do
        res = ctx.decode_frames_device_src([16, good.ptrs[0]], [0, good.lens[0]], [0, a.ptrs[4]], [0, caps[4]])
        assert (res[0].status, res[0].written, res[0].nframes) == (0, 0, 0) and res[1].status == 0
    finally:
        raw.free()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_submits_are_cut_as_for_host_sources(monkeypatch):
    import zgdata
    rng = random.Random(5)
    texts = [zgdata.text_like(300000 + 1000 * k, seed=40 + k) for k in range(6)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    junk = [bytes(rng.getrandbits(8) for _ in range(1000)) for _ in range(3)]
    entries, plains = [], []
    for k in range(36):
        entries.append(comp[k % 6])
        plains.append(texts[k % 6])
    entries[12:12] = [MAGIC + junk[0] * 2200, MAGIC + junk[1] * 700, MAGIC + junk[2] * 700]   # input that yields nothing
    plains[12:12] = [None, None, None]
    caps = [len(p) if p is not None else 4096 for p in plains]
    S = 2 << 20
    monkeypatch.setenv("ZGPU_FRAMES_SUBMIT_BYTES", str(S))
    c = zgpu.Context(0, dev=True)
    try:
        b, res, st = _both(c, entries, caps)          # (asserts that the two calls ran the same number of submits)
        groups = _cut(entries, S)
        assert len(groups) >= 4 and c.frames_submits() == len(groups)
        assert st["gather_launches"] == len(groups)   # one gather launch per submit
        assert st["walk_launches"] == 2               # the walk is done once for the whole call
        b.check(plains)
        assert [r.status == 0 for r in res] == [p is not None for p in plains]
    finally:
        c.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_dictionary_entries_take_the_alone_path():
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    rawd = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")[:60]
    plain = read_pack("decodecorpus.pack")
    pman = read_manifest("decodecorpus.json")
    pn = sorted(pman)[:5]
    entries = [pack[n] for n in names] + [plain[n] for n in pn]
    caps = [man[n]["size"] for n in names] + [pman[n]["size"] for n in pn]
    c = zgpu.Context(0)
    try:
        b, res, st = _both(c, entries, caps)
        assert all(r.status == zgpu.E_DICT_NOT_PROVIDED and r.written == 0 for r in res[:len(names)])
        assert all(r.status == 0 for r in res[len(names):])
        assert c.frames_device_stats()["entries_alone"] == 0 and st["input_bytes_to_host"] == 0
        c.add_dict(rawd)
        b, res, st = _both(c, entries, caps, hash_max=ALL)
        plains = []
        for i, (z, cap, r) in enumerate(zip(entries, caps, res)):
            stt, out = oracle_alone(z, cap, rawd)
            assert (stt, r.status, r.written) == (0, 0, len(out)), i
            plains.append(out)
        b.check(plains)
        alone = c.frames_device_stats()["entries_alone"]
        assert alone > 0
        # only the entries decoded alone crossed to the host, one download each
        assert 0 < st["input_bytes_to_host"] <= sum(len(z) for z in entries[:len(names)])
    finally:
        c.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_checksum_options(ctx):
    import seqframes
    import zgdata
    z_small, p_small = seqframes.frame([(40, 7, 30), (500, 300, 64)], tail=900, seed=3)
    z_long, p_long = seqframes.frame([(60000, 1000, 3000), (20000, 50000, 9000)], tail=8000, seed=4)
    text = zgdata.text_like(50000, seed=8)
    z_text = zgdata.zstd_compress(text)
    z_flip = bytearray(z_text)
    z_flip[-1] ^= 0x40                                     # one byte of the stored checksum
    z_none = zgdata.zstd_compress(text, checksum=False)
    entries = [z_small, bytes(z_flip), z_long, z_none, z_text + z_long]
    plains = [p_small, text, p_long, text, text + p_long]
    caps = [len(p) for p in plains]
    low = lambda b: xxh64(b) & 0xFFFFFFFF                 # noqa: E731

    b, res, _ = _both(ctx, entries, caps, hash_max=65536)  # z_long is longer than hash_max
    b.check(plains)
    assert [(r.status, r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed) for r in res] == [
        (0, 1, 1, 0, 0, 1), (0, 1, 1, 1, 0, 1), (0, 1, 1, 0, 1, 0), (0, 1, 0, 0, 0, 1), (0, 2, 2, 0, 1, 1)]
    assert res[1].calculated_checksum == low(text) != res[1].checksum_from_data
    assert res[2].calculated_checksum == 0 and res[2].checksum_from_data == low(p_long)
    b, res, _ = _both(ctx, entries, caps, hash_max=1 << 20)
    assert [(r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed) for r in res] == [
        (1, 0, 0, 1), (1, 1, 0, 1), (1, 0, 0, 1), (0, 0, 0, 1), (2, 0, 0, 1)]
    assert res[2].calculated_checksum == res[2].checksum_from_data == low(p_long)
    b, res, _ = _both(ctx, entries, caps, no_hash=True)
    b.check(plains)
    assert [(r.status, r.checksums, r.checksum_mismatches, r.checksums_unverified, r.first_hashed, r.calculated_checksum) for r in res] == [
        (0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 0, 0), (0, 1, 0, 1, 0, 0), (0, 0, 0, 0, 0, 0), (0, 2, 0, 2, 0, 0)]


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_decode_tensors_round_trip(ctx):
    import zgdata
    size = 1 << 20
    texts = [zgdata.text_like(size, seed=0x700 + k) for k in range(4)]
    comp = [zgdata.zstd_compress(t) for t in texts]
    ins = [torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0") for z in comp]
    ins.append(torch.frombuffer(bytearray(comp[0][:1000]), dtype=torch.uint8).to("cuda:0"))     # truncated: an empty view
    ins.append(torch.empty(0, dtype=torch.uint8, device="cuda:0"))
    outs, res = ctx.decode_tensors(ins, caps=[size] * 5 + [0])
    assert [r.status == 0 for r in res] == [True] * 4 + [False, True]
    assert [t.numel() for t in outs] == [size] * 4 + [0, 0]
    for t, text in zip(outs, texts):
        assert t.device.type == "cuda" and t.dtype == torch.uint8 and t.data_ptr() % 256 == 0
        assert t.cpu().numpy().tobytes() == text
    assert ctx.frames_device_src_stats()["input_bytes_to_host"] == 0
    outs2, res2 = ctx.decode_tensors(ins[:4])                                                   # capacities from the bound
    assert all(r.status == 0 for r in res2) and all(torch.equal(x, y) for x, y in zip(outs2, outs))
    with pytest.raises(ValueError):
        ctx.decode_tensors([torch.zeros(4, dtype=torch.uint8)])                                 # a host tensor
