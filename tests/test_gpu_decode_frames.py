"""zgpu_decode_frames (Context.decode_frames) and zgpu_batch_checksums on the GPU: every entry of a call gets what FrameDecoder::decode_all of
that entry ALONE gives — the oracle's verdict and bytes, and zgpu_decode_all's — whatever the other entries hold or their order; the content
checksums come from the device (zg_k_xxh64) for short frames and from the host for long ones."""
import os
import random
import sys

import pytest

from devmem import MAGIC, oracle_alone, xxh64
from framesuite import check_entries
from golden_io import read_manifest, read_pack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))   # zgdata: the workload generators


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


def _key(r):
    return (r.status, r.data, r.nframes, r.checksums, r.checksum_mismatches, r.checksum_from_data, r.calculated_checksum)


def test_corpus_in_one_call(ctx):
    import zgpu
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    entries = [pack[n] for n in names]
    caps = [man[n]["size"] for n in names]
    res = ctx.decode_frames(entries, caps)
    check_entries(ctx, entries, caps, res)
    for n, r in zip(names, res):
        assert r.status == 0 and r.nframes >= 1, n
        assert r.checksum_mismatches == 0, n
    # the default capacity (a bound from the headers) gives the same
    res2 = ctx.decode_frames(entries)
    assert [_key(r) for r in res2] == [_key(r) for r in res]
    assert zgpu.plaintext_bound(entries[0]) >= caps[0]


def test_dict_corpus_in_one_call():
    import zgpu
    pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
    raw = pack["dictionary"]
    names = sorted(n for n in man if n != "dictionary")
    entries = [pack[n] for n in names]
    caps = [man[n]["size"] for n in names]
    c = zgpu.Context(0)
    try:
        before = c.decode_frames(entries[:3], caps[:3])
        assert all(r.status == zgpu.E_DICT_NOT_PROVIDED for r in before)   # (no dictionary registered: decode_all's answer)
        c.add_dict(raw)
        res = c.decode_frames(entries, caps)
        check_entries(c, entries, caps, res, dict_raw=raw)
        assert all(r.status == 0 for r in res)
    finally:
        c.close()


def _isolation_entries():
    import zgdata
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    good = [pack[n] for n in names[:12]]
    out = []
    for n in sorted(os.listdir(os.path.join(GOLDEN, "regress"))):
        out.append(open(os.path.join(GOLDEN, "regress", n), "rb").read())
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
    text = zgdata.text_like(300000, seed=3)
    out.append(zgdata.zstd_compress(text))
    out += good
    caps = []
    for z in out:
        st, o = oracle_alone(z, 8 << 20)
        caps.append(len(o) if st == 0 else (8 << 20))
    caps[-1] -= 1                                                           # one byte short: TargetTooSmall
    return out, caps


def test_isolation_and_order(ctx):
    import zgpu
    entries, caps = _isolation_entries()
    res = ctx.decode_frames(entries, caps)
    check_entries(ctx, entries, caps, res)
    assert res[-1].status == zgpu.E_TARGET_TOO_SMALL
    assert any(r.status not in (0, zgpu.E_TARGET_TOO_SMALL) for r in res)
    for seed in (1, 2):
        perm = list(range(len(entries)))
        random.Random(seed).shuffle(perm)
        rp = ctx.decode_frames([entries[i] for i in perm], [caps[i] for i in perm])
        for j, i in enumerate(perm):
            assert _key(rp[j]) == _key(res[i]), (seed, i)


def _raw_frame(payload, checksum=True):
    """one frame of one raw block (single segment, FCS of 2 bytes): its payload is copied as it is, and nothing but the checksum covers it"""
    fhd = 0x20 | (0x40) | (0x04 if checksum else 0)
    h = MAGIC + bytes([fhd]) + (len(payload) - 256).to_bytes(2, "little")
    bh = (1 | (0 << 1) | (len(payload) << 3)).to_bytes(3, "little")
    z = h + bh + payload
    if checksum:
        z += (xxh64(payload) & 0xFFFFFFFF).to_bytes(4, "little")
    return z


def test_checksums_reported_not_enforced(ctx):
    import zgdata
    text = zgdata.text_like(200000, seed=11)
    z = zgdata.zstd_compress(text)                       # with the checksum
    zc = bytearray(z)
    zc[-2] ^= 0x5A                                       # one byte of the stored checksum
    payload = bytes(range(256)) * 8
    zr = _raw_frame(payload)
    zr_bad = bytearray(zr)
    zr_bad[20] ^= 0x01                                   # inside the raw block's payload: the decoder cannot see it
    plain_bad = payload[:10] + bytes([payload[10] ^ 1]) + payload[11:]   # (7 bytes of frame header + 3 of block header in front)
    zn = zgdata.zstd_compress(text, checksum=False)
    entries = [z, bytes(zc), zr, bytes(zr_bad), zn, z + zr]
    caps = [len(text), len(text), len(payload), len(payload), len(text), len(text) + len(payload)]
    res = ctx.decode_frames(entries, caps)
    check_entries(ctx, entries, caps, res)
    r = res[0]
    assert (r.status, r.nframes, r.checksums, r.checksum_mismatches) == (0, 1, 1, 0)
    assert r.calculated_checksum == r.checksum_from_data == xxh64(text) & 0xFFFFFFFF
    r = res[1]
    assert (r.status, r.checksums, r.checksum_mismatches) == (0, 1, 1) and r.data == text
    r = res[2]
    assert (r.status, r.checksums, r.checksum_mismatches) == (0, 1, 0)
    r = res[3]
    assert (r.status, r.checksums, r.checksum_mismatches) == (0, 1, 1)
    assert r.data == plain_bad and r.calculated_checksum == xxh64(plain_bad) & 0xFFFFFFFF
    r = res[4]
    assert (r.status, r.nframes, r.checksums, r.checksum_mismatches, r.checksum_from_data) == (0, 1, 0, 0, 0)
    assert r.calculated_checksum == xxh64(text) & 0xFFFFFFFF
    r = res[5]
    assert (r.status, r.nframes, r.checksums, r.checksum_mismatches) == (0, 2, 2, 0)


def _small_frames():
    import zgdata
    distinct = [zgdata.text_like(128 << 10, seed=100 + k) for k in range(32)]
    comp = [zgdata.zstd_compress(t) for t in distinct]
    plains = [distinct[k % 32] for k in range(4096)]
    entries = [comp[k % 32] for k in range(4096)]
    for n in (0, 1, 31, 32, 33, (4 << 20) + 1, 6 << 20):              # (6 MiB: longer than the device-hash threshold)
        t = zgdata.text_like(n, seed=n + 5) if n else b""
        plains.append(t)
        entries.append(zgdata.zstd_compress(t))
    return entries, plains


def _check_small(ctx, entries, plains):
    res = ctx.decode_frames(entries, [len(p) for p in plains])
    for i, (r, p) in enumerate(zip(res, plains)):
        assert r.status == 0 and r.data == p, i
        assert (r.nframes, r.checksums, r.checksum_mismatches) == (1, 1, 0), i
        assert r.calculated_checksum == r.checksum_from_data == xxh64(p) & 0xFFFFFFFF, i
    caps = [len(p) for p in plains]
    for i in list(range(0, 4096, 509)) + list(range(4096, len(entries))):
        check_entries(ctx, [entries[i]], [caps[i]], [res[i]])


def test_many_small_frames(ctx, monkeypatch):
    import zgpu
    entries, plains = _small_frames()
    _check_small(ctx, entries, plains)
    assert ctx.frames_submits() == 2          # 4096 x 128 KiB fill the first submit (512 MiB), the rest goes in a second one
    # the development build with submits of 8 MiB: several submits, the long entries alone; every frame hashed on the host
    monkeypatch.setenv("ZGPU_FRAMES_SUBMIT_BYTES", str(8 << 20))
    monkeypatch.setenv("ZGPU_HASH_DEVICE_MAX", "0")
    c = zgpu.Context(0, dev=True)
    try:
        _check_small(c, entries, plains)
        assert c.frames_submits() >= 66       # 64 of the 128 KiB entries, the (4 MiB + 1) one and the 6 MiB one
    finally:
        c.close()
    # ... and every frame, the 6 MiB one included, hashed on the device
    monkeypatch.setenv("ZGPU_HASH_DEVICE_MAX", str(64 << 20))
    c = zgpu.Context(0, dev=True)
    try:
        _check_small(c, entries, plains)
    finally:
        c.close()


def test_input_bytes_bound_the_submits(monkeypatch):
    """entries that yield no plaintext (skippable frames, garbage) still count against a submit by their input bytes"""
    import zgpu
    skip = (0x184D2A50).to_bytes(4, "little") + (1 << 20).to_bytes(4, "little") + bytes(1 << 20)
    junk = bytes(range(256)) * 4096
    entries = [skip, junk] * 8
    monkeypatch.setenv("ZGPU_FRAMES_SUBMIT_BYTES", str(4 << 20))
    c = zgpu.Context(0, dev=True)
    try:
        res = c.decode_frames(entries, [0] * len(entries))
        assert c.frames_submits() >= 4
        check_entries(c, entries, [0] * len(entries), res)
    finally:
        c.close()


def test_batch_checksums(ctx):
    import zgdata
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = sorted(man)
    bad = open(os.path.join(GOLDEN, "regress", "exec_error_behind_good_blocks.zst"), "rb").read()
    parts = [pack[names[k]] for k in range(0, 40, 3)] + [bad, zgdata.zstd_compress(zgdata.text_like(3 << 20, seed=9)),
                                                        zgdata.zstd_compress(b""), zgdata.zstd_compress(b"x" * 33)]
    b = ctx.prepare(b"".join(parts))
    b.run()
    b.sync()
    assert b.nframes == len(parts)
    cs = b.checksums()
    failed = 0
    for f in range(b.nframes):
        fi = b.frame_info(f)
        failed += fi.status != 0
        assert cs[f] == xxh64(b.read(fi.out_base, fi.out_size)), f
    assert failed == 1
    b.close()
