"""zgpu_frames_index_device / zgpu_frames_table_device (Context.frames_index_device / frames_table_device / split_tensor_frames, and
decode_tensors sizing itself with them) on the GPU: what compressed entries that lie in device memory hold, answered without a byte of them
crossing to the host. The reference for the bound is zgpu_plaintext_bound of a host copy, for the frame table zgpu_batch_frame_info of a
host copy, for decoded bytes the oracle. The deterministic conditions are asserted — launches, bytes downloaded, bytes crossed —, times
are printed. Pointers the contract refuses are refused by the host's check before anything is launched, so no case here makes a kernel
touch memory it must not."""
import ctypes as C
import os
import random
import struct
import sys

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import zgpu
from devmem import MAGIC, Arena, RawDevice, RawSources, Sources, oracle_alone
from golden_io import read_manifest, read_pack
from test_gpu_decode_frames_device import _isolation_entries, _raw_frame
from test_gpu_decode_frames_device_src import _all_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KEYS = ("bound", "chain_end", "status", "nframes", "nskippable", "nblocks", "why", "flags")


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


def _key(e):
    return tuple(getattr(e, k) for k in KEYS)


def _skippable(payload, magic=0x184D2A50):
    return struct.pack("<II", magic, len(payload)) + payload


def _index(c, entries, src=None, src_shifts=None):
    """frames_index_device over the entries in device memory: the bound of every entry is the host's, the call is ONE launch that brings back
    48 bytes per entry and no byte of the input, the sources are unchanged. Returns (sources, entries' EntryIndex)."""
    import zgpu
    s = src or Sources(entries, src_shifts)
    res = c.frames_index_device(s.ptrs, s.lens)
    st = c.frames_index_stats()
    assert len(res) == len(entries)
    for j, (e, z) in enumerate(zip(res, entries)):
        assert e.status == 0 and e.bound == zgpu.plaintext_bound(z), (j, e, zgpu.plaintext_bound(z))
        assert e.chain_end <= len(z) and (e.why != zgpu.CHAIN_END or e.chain_end == len(z)), (j, e)
    assert st["launches"] == (1 if entries else 0), st
    assert st["bytes_downloaded"] == 48 * len(entries) and st["input_bytes_to_host"] == 0, st
    assert s.unchanged()
    return s, res


def _host_frames(c, z):
    """the frames of z as zgpu_batch_frame_info describes them on a host copy (z must be valid from end to end)"""
    b = c.prepare(z)
    try:
        assert b.parse_status == 0
        return [b.frame_info(f) for f in range(b.nframes)]
    finally:
        b.close()


def _mutated(rng, frames, n):
    """fixed-seed damage at the places the chain reads: single-byte edits in the first 24 bytes, truncations, garbage tails"""
    out = []
    frames = [z for z in frames if len(z) > 1]
    for k in range(n):
        z = bytearray(frames[k % len(frames)])
        how = k % 4
        if how == 0:
            z[rng.randrange(min(len(z), 24))] ^= 1 << rng.randrange(8)
        elif how == 1:
            z = z[:rng.randrange(len(z))]
        elif how == 2:
            z += bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 40)))
        else:
            z[rng.randrange(len(z))] = rng.getrandbits(8)
        out.append(bytes(z))
    return out


# 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_bound_equals_the_host_bound_on_corpus_dictionary_and_mutated_frames(ctx):
    import zgpu
    golden = _all_golden()                                   # decodecorpus, fuzz artefacts, regress, verdict_order, 40 dictionary frames
    dp = read_pack("dict_tests.pack")
    dict_frames = [dp[n] for n in sorted(dp) if n != "dictionary"]
    entries = golden + dict_frames + _mutated(random.Random(0x1DE5), golden, 600)
    assert len(entries) > 900
    _, res = _index(ctx, entries, src_shifts=[(5 * j) % 29 for j in range(len(entries))])
    whys = set(e.why for e in res)
    assert len(whys) >= 6, whys                              # most of the reasons a chain ends for
    assert all(e.any_dict for e in res[len(golden):len(golden) + len(dict_frames)])
    assert any(e.any_checksum for e in res) and any(e.all_sized for e in res) and any(e.nframes and not e.all_complete for e in res)


def test_4096_text_frames_of_128k_in_one_call(ctx):
    import zgdata
    size, n = 128 << 10, 4096
    comp = [zgdata.zstd_compress(zgdata.text_like(size, seed=0x4096 + k)) for k in range(8)]
    entries = [comp[k % 8] for k in range(n)]
    s, res = _index(ctx, entries)
    assert all((e.bound, e.nframes, e.nskippable, e.why, e.all_sized, e.any_checksum, e.all_complete) == (size, 1, 0, 0, True, True, True) for e in res)
    st = ctx.frames_index_stats()
    print("frames_index_device, 4096 x 128 KiB text:", st, "input bytes", sum(s.lens))
    ents, first, frames = ctx.frames_table_device(s.ptrs, s.lens, room=n)
    st2 = ctx.frames_index_stats()
    print("frames_table_device, 4096 x 128 KiB text:", st2)
    assert [_key(e) for e in ents] == [_key(e) for e in res] and first == list(range(n + 1)) and len(frames) == n
    assert st2["launches"] == 2 and st2["bytes_downloaded"] == 2 * 48 * n + 64 * n and st2["input_bytes_to_host"] == 0
    assert all((f.entry, f.src_begin, f.src_end, f.bound) == (k, 0, s.lens[k], size) for k, f in enumerate(frames))
    # the parent's yardstick on the same entries: zg_k_walk's count and emit passes of a decode
    a = Arena([size] * n)
    r = ctx.decode_frames_device_src(s.ptrs, s.lens, a.ptrs, [e.bound for e in res], no_hash=True)
    assert all(x.status == 0 and x.written == size for x in r)
    print("decode_frames_device_src of the same entries:", ctx.frames_device_src_stats())


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_frame_table_equals_the_host_parse(ctx):
    import zgdata
    import zgpu
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    texts = [zgdata.text_like(50000 + 7000 * k, seed=0x7AB + k) for k in range(5)]
    multi = [
        b"".join(pack[n] for n in names[:12]),
        b"".join(zgdata.zstd_compress(t, checksum=k % 2 == 0, content_size=k % 3 != 0) for k, t in enumerate(texts)),
        _raw_frame(b"x" * 300000) + pack[names[20]] + _raw_frame(b"") + zgdata.zstd_compress(texts[0], window_log=17),
        pack[names[30]],
    ]
    s = Sources(multi, [3, 0, 17, 9])
    ents, first, frames = ctx.frames_table_device(s.ptrs, s.lens, room=1)       # (sized by the second call)
    assert first[0] == 0 and first[-1] == len(frames) and len(ents) == len(multi)
    for i, z in enumerate(multi):
        want = _host_frames(ctx, z)
        got = frames[first[i]:first[i + 1]]
        assert len(got) == len(want) == ents[i].nframes and ents[i].nskippable == 0 and ents[i].why == zgpu.CHAIN_END
        assert sum(f.bound for f in got) == ents[i].bound == zgpu.plaintext_bound(z)
        for f, w in zip(got, want):
            assert (f.entry, f.src_begin, f.src_end, f.window_size, f.frame_content_size, f.nblocks, f.has_checksum) == \
                   (i, w.src_begin, w.src_end, w.window_size, w.frame_content_size, w.nblocks, bool(w.has_checksum)), (i, f, w.src_begin)
            assert f.header_status == 0 and f.complete and not f.skippable and f.skip_magic == 0 and f.dict_id == 0
        assert sum(f.nblocks for f in got) == ents[i].nblocks
    assert s.unchanged()
    # skippable frames between the frames, a dictionary frame, and an entry whose chain ends at a header it cannot read
    dp = read_pack("dict_tests.pack")
    dz = dp[sorted(n for n in dp if n != "dictionary")[0]]
    mixed = [_skippable(b"hello") + pack[names[0]] + _skippable(b"", 0x184D2A5F) + pack[names[1]] + _skippable(b"xyz"),
             dz + pack[names[2]],
             pack[names[3]] + pack[names[4]] + b"\x00\x01\x02\x03\x04\x05"]
    s = Sources(mixed, [1, 2, 3])
    ents, first, frames = ctx.frames_table_device(s.ptrs, s.lens)
    assert [(e.nframes, e.nskippable, e.why) for e in ents] == [(2, 3, 0), (2, 0, 0), (2, 0, zgpu.CHAIN_BAD_MAGIC)]
    assert [first[i + 1] - first[i] for i in range(3)] == [5, 2, 3]
    for i, z in enumerate(mixed):
        got = frames[first[i]:first[i + 1]]
        assert got[0].src_begin == 0 and got[-1].src_end == ents[i].chain_end and all(a.src_end == b.src_begin for a, b in zip(got, got[1:]))
        assert sum(f.bound for f in got) == ents[i].bound == zgpu.plaintext_bound(z)
    g = frames[first[0]:first[1]]
    assert [f.skippable for f in g] == [True, False, True, False, True] and [f.header_status for f in g] == [zgpu.E_SKIP_FRAME, 0] * 2 + [zgpu.E_SKIP_FRAME]
    assert [f.skip_magic for f in g] == [0x184D2A50, 0, 0x184D2A5F, 0, 0x184D2A50] and g[0].src_end == 13
    g = frames[first[1]:first[2]]
    assert g[0].dict_id != 0 and g[1].dict_id == 0 and ents[1].any_dict
    g = frames[first[2]:first[3]]
    assert g[2].header_status == 2 and g[2].src_begin == g[2].src_end == len(mixed[2]) - 6 and g[2].bound == 0      # ZGPU_E_BAD_MAGIC
    # a table with too little room: the count needed, entries and frame_first filled, one launch
    n = len(mixed)
    srcs, lens = (C.c_void_p * n)(*s.ptrs), (C.c_size_t * n)(*s.lens)
    ec, fc, few, need = (zgpu.EntryIndexC * n)(), (C.c_uint64 * (n + 1))(), (zgpu.FrameIndexC * 4)(), C.c_size_t(0)
    assert ctx.L.zgpu_frames_table_device(ctx.h, srcs, lens, n, ec, fc, few, 4, C.byref(need)) == zgpu.E_TARGET_TOO_SMALL
    assert need.value == 10 and list(fc) == first and [_key(zgpu.EntryIndex(ec[i])) for i in range(n)] == [_key(e) for e in ents]
    assert ctx.frames_index_stats()["launches"] == 1


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_sources_at_odd_alignments_and_flush_with_the_allocation(ctx):
    import zgdata
    rng = random.Random(0x5A11)
    lengths = [0, 1, 2, 3, 15, 16, 17, 31, 33, 4095, 4097, 65537, 131071]
    entries = [_raw_frame(rng.randbytes(n)) for n in lengths + lengths[::-1]]
    text = zgdata.text_like(70001, seed=77)
    entries += [zgdata.zstd_compress(text[:70001 - 997 * k]) for k in range(10)]
    for turn in range(2):
        shifts = [(j + 5 * turn) % 18 for j in range(len(entries))]
        raw = RawSources(entries, shifts)                                     # the last entry ends flush with the hipMalloc'ed block
        try:
            _, res = _index(ctx, entries, src=raw)
            assert all(e.why == 0 and e.nframes == 1 and e.all_complete for e in res)
            # truncated to end flush: every cut of the last entry's tail, as a source that ends with the allocation
            last, z = raw.ptrs[-1], entries[-1]
            cuts = list(range(1, 24)) + [len(z) - k for k in range(1, 8)]
            import zgpu
            res = ctx.frames_index_device([last + len(z) - n for n in cuts], cuts)
            for n, e in zip(cuts, res):
                assert e.status == 0 and e.bound == zgpu.plaintext_bound(z[len(z) - n:]), (n, e)
        finally:
            raw.free()


def test_zero_length_entries_wrong_pointers_and_permutation(ctx):
    import zgdata
    import zgpu
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
        for call in (ctx.frames_index_device, lambda p, n: ctx.frames_table_device(p, n)[0]):
            res = call(ptrs, lens)
            for i in (1, 2, 3, 4):
                assert _key(res[i]) == (0, 0, zgpu.E_BAD_ARG, 0, 0, 0, 0, 0), (i, res[i])
            for i in (0, 5):
                assert (res[i].status, res[i].bound, res[i].nframes) == (0, len(text), 1), (i, res[i])
        ents, first, frames = ctx.frames_table_device(ptrs, lens)
        assert first == [0, 1, 1, 1, 1, 1, 2] and [f.entry for f in frames] == [0, 5]
        # the same allocation inside its bounds: the whole of it, and a range that ends flush with it
        res = ctx.frames_index_device([raw.ptr, raw.ptr + 100], [len(z), len(z) - 100])
        assert res[0].status == 0 and res[0].bound == len(text) and res[1].status == 0 and res[1].bound == zgpu.plaintext_bound(z[100:])
        # a length of 0: nothing is checked, nothing is read — any pointer value will do
        res = ctx.frames_index_device([16, good.ptrs[0], 0], [0, good.lens[0], 0])
        assert _key(res[0]) == _key(res[2]) == (0,) * 8 and res[1].bound == len(text)
        assert ctx.frames_index_device([], []) == [] and ctx.frames_index_stats()["launches"] == 0
        assert good.unchanged() and raw.read() == z and host_buf.raw == z
    finally:
        raw.free()
    # permuting the entries permutes the results
    entries, _ = _isolation_entries()          # failing, truncated, garbage, empty, skippable-only, several frames
    assert b"" in entries
    base = [_key(e) for e in _index(ctx, entries)[1]]
    perm = list(range(len(entries)))
    random.Random(2).shuffle(perm)
    s = Sources([entries[i] for i in perm], [(3 * j) % 18 for j in range(len(perm))])
    ents, first, frames = ctx.frames_table_device(s.ptrs, s.lens)
    assert [_key(ents[perm.index(i)]) for i in range(len(entries))] == base
    s0 = Sources(entries)
    _, first0, frames0 = ctx.frames_table_device(s0.ptrs, s0.lens)
    tab = lambda fr, fi, j: [(f.src_begin, f.src_end, f.bound, f.nblocks, f.flags, f.header_status) for f in fr[fi[j]:fi[j + 1]]]   # noqa: E731
    assert all(tab(frames, first, perm.index(i)) == tab(frames0, first0, i) for i in range(len(entries)))
    assert len(set(k[6] for k in base)) >= 3


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_decode_tensors_sizes_itself_without_a_download(ctx):
    import zgdata
    size = 1 << 20
    texts = [zgdata.text_like(size - 1000 * k, seed=0x700 + k) for k in range(4)]
    comp = [zgdata.zstd_compress(t, content_size=k != 2) for k, t in enumerate(texts)]
    multi = comp[1] + _skippable(b"between") + comp[3]
    ins = [torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0") for z in comp + [multi]]
    ins.append(torch.empty(0, dtype=torch.uint8, device="cuda:0"))
    outs, res = ctx.decode_tensors(ins)                                     # caps=None: the capacities come from frames_index_device
    st = ctx.frames_index_stats()
    assert (st["launches"], st["bytes_downloaded"], st["input_bytes_to_host"]) == (1, 48 * len(ins), 0), st
    assert ctx.frames_device_src_stats()["input_bytes_to_host"] == 0
    idx = ctx.frames_index_device([t.data_ptr() if t.numel() else 0 for t in ins], [t.numel() for t in ins])
    for z, t, r, e in zip(comp + [multi, b""], outs, res, idx):
        st, ref = oracle_alone(z, 4 << 20)
        assert (st, r.status, r.written) == (0, 0, len(ref)) and t.cpu().numpy().tobytes() == ref
        assert r.nframes == e.nframes and r.written <= e.bound                # the index agrees with the decode
    assert outs[4].cpu().numpy().tobytes() == texts[1] + texts[3]
    with pytest.raises(ValueError):
        ctx.split_tensor_frames(torch.zeros(4, dtype=torch.uint8))              # a host tensor


def test_split_tensor_frames_of_64_concatenated_frames(ctx):
    import zgdata
    rng = random.Random(64)
    plains = [zgdata.text_like(rng.randrange(1000, 200000), seed=0x640 + k) for k in range(64)]
    frames = [zgdata.zstd_compress(p, checksum=k % 3 != 0) for k, p in enumerate(plains)]
    parts = []
    for k, z in enumerate(frames):
        parts.append(z)
        if k % 9 == 4:
            parts.append(_skippable(bytes(k)))                                # skippable frames are left out of the views
    shard = torch.frombuffer(bytearray(b"".join(parts)), dtype=torch.uint8).to("cuda:0")
    views = ctx.split_tensor_frames(shard)
    assert ctx.frames_index_stats()["input_bytes_to_host"] == 0
    assert [v.numel() for v in views] == [len(z) for z in frames]
    assert all(v.data_ptr() >= shard.data_ptr() and v.data_ptr() + v.numel() <= shard.data_ptr() + shard.numel() for v in views)
    outs, res = ctx.decode_tensors(views)                                     # 64 entries, each its own tensor
    whole, wres = ctx.decode_tensors([shard])                                 # one entry into one destination
    assert wres[0].status == 0 and wres[0].nframes == 64 and all(r.status == 0 and r.nframes == 1 for r in res)
    assert ctx.frames_device_src_stats()["input_bytes_to_host"] == 0
    assert torch.equal(torch.cat(outs), whole[0])
    assert whole[0].cpu().numpy().tobytes() == b"".join(plains)
    for v, p, t in zip(views, plains, outs):
        assert t.numel() == len(p)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_long_frame_of_more_than_2048_blocks(ctx):
    import zgpu
    rng = random.Random(2048)
    nblocks = 2600
    z = bytearray(MAGIC + bytes([0x00, 0x58]))                               # no content size, a window descriptor, no checksum
    total = 0
    for k in range(nblocks):
        last = 1 if k == nblocks - 1 else 0
        if k % 3 == 1:                                                        # RLE: one byte of body, Block_Size of output
            n = rng.randrange(1, 128 << 10)
            z += struct.pack("<I", (n << 3) | (1 << 1) | last)[:3] + bytes([k & 255])
        else:                                                                 # raw
            n = rng.randrange(0, 3000)
            z += struct.pack("<I", (n << 3) | last)[:3] + rng.randbytes(n)
        total += n
    z = bytes(z)
    assert zgpu.plaintext_bound(z) == total
    s, res = _index(ctx, [z, z[:len(z) // 2]], src_shifts=[7, 0])
    print("frames_index_device, one frame of %d blocks (%d bytes):" % (nblocks, len(z)), ctx.frames_index_stats())
    host = _host_frames(ctx, z)
    assert len(host) == 1 and host[0].nblocks == nblocks
    assert (res[0].bound, res[0].nblocks, res[0].nframes, res[0].why, res[0].chain_end) == (total, nblocks, 1, 0, len(z))
    assert res[1].nblocks < nblocks and res[1].why != 0 and not res[1].all_complete
    ents, first, frames = ctx.frames_table_device(s.ptrs, s.lens)
    assert (frames[0].nblocks, frames[0].bound, frames[0].src_end, frames[0].window_size) == (nblocks, total, len(z), host[0].window_size)
    st, ref = oracle_alone(z, total)
    t = torch.frombuffer(bytearray(z), dtype=torch.uint8).to("cuda:0")
    outs, r = ctx.decode_tensors([t])
    assert (st, r[0].status, r[0].written) == (0, 0, total) and outs[0].cpu().numpy().tobytes() == ref
