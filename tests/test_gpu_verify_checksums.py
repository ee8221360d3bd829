"""ZGPU_DEVICE_VERIFY (decode_frames_device / decode_frames_device_src with verify=True) on the GPU: a Content_Checksum that does not match
becomes the entry's verdict, ZGPU_E_CHECKSUM_MISMATCH, and no byte of that entry's destination is written.

Frames are built here from raw blocks (magic, a single-segment header with Content_Checksum and a 1-, 2- or 4-byte Frame_Content_Size, raw
blocks of at most 128 KiB, the low 32 bits of the oracle's XXH64 of the plaintext), so no compressor is needed and every expected checksum
is the oracle's. Destinations are the arena of test_gpu_decode_frames_device.py: a sentinel fill, guards around every slot, and the whole
arena compared afterwards."""
import os
import random

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

import zgpu
from devmem import MAGIC, Arena, full_key, oracle_alone, xxh32
from golden_io import read_pack

pytestmark = pytest.mark.gpu
BLOCK = 128 << 10
LENS = [0, 1, 31, 32, 33, 255, 256, 257, BLOCK + 1, 5 << 20]     # (the 5 MiB frame lies above the 4 MiB default of hash_max_bytes)
BIG = len(LENS) - 1


def make_frame(plain, checksum=True, dict_id=None):
    """one frame of raw blocks; returns (bytes, offset of the first block's body)"""
    n = len(plain)
    desc = 0x20 | (0x04 if checksum else 0) | (3 if dict_id is not None else 0)
    if n < 256:
        fcs = bytes([n])
    elif n < 65536 + 256:
        desc |= 1 << 6
        fcs = (n - 256).to_bytes(2, "little")
    else:
        desc |= 2 << 6
        fcs = n.to_bytes(4, "little")
    z = bytearray(MAGIC + bytes([desc]) + (dict_id.to_bytes(4, "little") if dict_id is not None else b"") + fcs)
    body0 = len(z) + 3
    at = 0
    while True:
        k = min(BLOCK, n - at)
        last = at + k == n
        z += ((k << 3) | (1 if last else 0)).to_bytes(3, "little") + plain[at:at + k]
        at += k
        if last:
            break
    if checksum:
        z += xxh32(plain).to_bytes(4, "little")
    return bytes(z), body0


def flip_checksum(z):
    return z[:-1] + bytes([z[-1] ^ 0x10])


def flip_payload(z, body0, k=0):
    """byte k of the PLAINTEXT flipped where it lies in the frame (a 3-byte block header stands in front of every 128 KiB of it)"""
    at = body0 + k + 3 * (k // BLOCK)
    return z[:at] + bytes([z[at] ^ 0x01]) + z[at + 1:]


def _arena(caps):
    return Arena(caps, shifts=[i % 5 for i in range(len(caps))])                  # (destinations at any alignment)


def _run(c, entries, caps, **kw):
    a = _arena(caps)
    res = c.decode_frames_device(entries, a.ptrs, caps, **kw)
    assert len(res) == len(entries)
    return a, res


@pytest.fixture(scope="module")
def ctx():
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def good():
    """(plaintexts, frames, offsets of the first block bodies) of LENS"""
    rng = random.Random(0xC5)
    plains = [rng.randbytes(n) for n in LENS]
    built = [make_frame(p) for p in plains]
    return plains, [z for z, _ in built], [b for _, b in built]


@pytest.fixture(scope="module")
def good_run(ctx, good):
    """the all-good call with verify, checked once: what every other test compares its untouched entries with"""
    plains, frames, _ = good
    caps = [len(p) + 7 for p in plains]
    a, res = _run(ctx, frames, caps, verify=True)
    for z, p, cap, r in zip(frames, plains, caps, res):
        st, out = oracle_alone(z, cap)
        assert (st, out) == (0, p)
        assert (r.status, r.written, r.nframes, r.checksums, r.checksum_mismatches) == (0, len(p), 1, 1, 0), (len(p), full_key(r))
        assert r.checksums_unverified == 0 and r.first_hashed == 1, len(p)
        assert r.checksum_from_data == r.calculated_checksum == xxh32(p)
    a.check(plains)
    st = ctx.frames_device_stats(verify=True)
    assert st["entries_failed_verify"] == 0 and st["frames_hashed"] == len(LENS) and st["frames_not_hashed"] == 0
    assert st["scatter_launches"] == 1 and st["entries_alone"] == 0
    return caps, [full_key(r) for r in res]


def test_all_good_with_verify(good_run):
    caps, res = good_run
    assert len(res) == len(LENS) and all(r[0] == 0 for r in res)


def _two_bad(good):
    plains, frames, body0 = good
    entries, a_bad, b_bad = list(frames), 7, 8
    entries[a_bad] = flip_checksum(frames[a_bad])                               # the stored checksum, one bit
    entries[b_bad] = flip_payload(frames[b_bad], body0[b_bad], 70000)           # a payload byte inside a raw block
    wrong = bytearray(plains[b_bad])
    wrong[70000] ^= 0x01
    return entries, a_bad, b_bad, bytes(wrong)


def test_mismatch_fails_the_entry_and_writes_nothing(ctx, good, good_run):
    """fails on the parent commit: status 0 where ZGPU_E_CHECKSUM_MISMATCH is due"""
    plains, _, _ = good
    caps, ref = good_run
    entries, a_bad, b_bad, wrong = _two_bad(good)
    a, res = _run(ctx, entries, caps, verify=True)
    for i, r in enumerate(res):
        if i in (a_bad, b_bad):
            assert full_key(r) == (zgpu.E_CHECKSUM_MISMATCH, 0, 0, 1, 1, 0, 0, 0, 0), (i, full_key(r))
        else:
            assert full_key(r) == ref[i], i
    a.check([None if i in (a_bad, b_bad) else p for i, p in enumerate(plains)])
    st = ctx.frames_device_stats(verify=True)
    assert st["entries_failed_verify"] == 2 and st["frames_hashed"] == len(LENS)
    assert st["bytes_scattered"] == sum(len(p) for i, p in enumerate(plains) if i not in (a_bad, b_bad))
    # without verify: today's behaviour — the mismatch is counted, the bytes are written
    a, res = _run(ctx, entries, caps)
    for i, r in enumerate(res):
        bad = i in (a_bad, b_bad)
        assert (r.status, r.written, r.checksums, r.checksum_mismatches) == (0, len(plains[i]), 1, 1 if bad else 0), (i, full_key(r))
        assert r.checksums_unverified == (1 if i == BIG else 0)                  # (the 5 MiB frame: above the default limit, not hashed)
    a.check([wrong if i == b_bad else p for i, p in enumerate(plains)])
    assert ctx.frames_device_stats(verify=True)["entries_failed_verify"] == 0


def test_isolation_and_entry_order(ctx, good, good_run):
    plains, frames, _ = good
    caps, ref = good_run
    three = frames[3] + flip_checksum(frames[6]) + frames[4]                     # 32, 256 (bad), 33 bytes
    small = [0, 1, 2, 5, 7]
    entries = [frames[i] for i in small] + [three]
    ecaps = [caps[i] for i in small] + [400]
    want = [ref[i] for i in small] + [(zgpu.E_CHECKSUM_MISMATCH, 0, 0, 3, 1, 0, 0, 0, 0)]
    wplain = [plains[i] for i in small] + [None]
    for perm in ([0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 5, 0, 4, 1, 3]):
        a, res = _run(ctx, [entries[k] for k in perm], [ecaps[k] for k in perm], verify=True)
        assert [full_key(r) for r in res] == [want[k] for k in perm], perm
        a.check([wplain[k] for k in perm])
        assert ctx.frames_device_stats(verify=True)["entries_failed_verify"] == 1


def test_precedence(ctx, good, good_run):
    plains, frames, body0 = good
    no_sum, _ = make_frame(plains[5], checksum=False)                              # passes: nothing to compare with
    broken = flip_payload(frames[8], body0[8], 5)[:-10]                           # corrupted AND its last block cut short: the decode error stays
    too_small = flip_checksum(frames[6])                                          # corrupted, and the destination does not hold it
    entries, caps = [no_sum, broken, too_small, frames[2]], [len(plains[5]), len(plains[8]), len(plains[6]) - 1, len(plains[2])]
    a0, plain_res = _run(ctx, entries, caps)
    a, res = _run(ctx, entries, caps, verify=True)
    assert [full_key(r) for r in res] == [full_key(r) for r in plain_res]
    st_broken, _ = oracle_alone(broken, caps[1])
    assert st_broken not in (0, zgpu.E_CHECKSUM_MISMATCH) and res[1].status == st_broken
    assert res[2].status == zgpu.E_TARGET_TOO_SMALL
    assert (res[0].status, res[0].written, res[0].checksums, res[0].first_hashed) == (0, len(plains[5]), 0, 1)
    assert res[3].status == 0
    for x in (a0, a):
        x.check([plains[5], None, None, plains[2]])
    assert ctx.frames_device_stats(verify=True)["entries_failed_verify"] == 0


def test_hash_max_still_bounds_what_is_hashed(ctx, good, good_run):
    plains, frames, body0 = good
    big_bad = flip_payload(frames[BIG], body0[BIG], 3 << 20)
    wrong = bytearray(plains[BIG])
    wrong[3 << 20] ^= 0x01
    entries, caps = [big_bad, flip_checksum(frames[7]), frames[4]], [len(plains[BIG]), len(plains[7]), len(plains[4])]
    a, res = _run(ctx, entries, caps, verify=True, hash_max=1 << 20)
    assert (res[0].status, res[0].written, res[0].checksums, res[0].checksums_unverified, res[0].checksum_mismatches) == (0, len(wrong), 1, 1, 0)
    assert res[1].status == zgpu.E_CHECKSUM_MISMATCH and res[2].status == 0
    a.check([bytes(wrong), None, plains[4]])
    # with no limit the same frame is caught
    a, res = _run(ctx, entries, caps, verify=True)
    assert [r.status for r in res] == [zgpu.E_CHECKSUM_MISMATCH, zgpu.E_CHECKSUM_MISMATCH, 0]
    a.check([None, None, plains[4]])


def test_verify_with_no_hash_is_bad_arg(ctx, good):
    plains, frames, _ = good
    caps = [len(plains[2]), len(plains[6])]
    a = _arena(caps)
    with pytest.raises(zgpu.ZgpuError) as e:
        ctx.decode_frames_device([frames[2], frames[6]], a.ptrs, caps, verify=True, no_hash=True)
    assert e.value.status == zgpu.E_BAD_ARG
    src = torch.frombuffer(bytearray(frames[2]), dtype=torch.uint8).to("cuda:0")
    with pytest.raises(zgpu.ZgpuError) as e:
        ctx.decode_frames_device_src([src.data_ptr()], [src.numel()], a.ptrs[:1], caps[:1], verify=True, no_hash=True)
    assert e.value.status == zgpu.E_BAD_ARG
    a.check([None, None])


def test_device_sources_give_the_same(ctx, good, good_run):
    plains, frames, body0 = good
    caps, _ = good_run
    entries, a_bad, b_bad, _ = _two_bad(good)
    entries = entries + [flip_payload(frames[8], body0[8], 5)[:-10], frames[3] + flip_checksum(frames[6]) + frames[4]]
    caps = caps + [len(plains[8]), 400]
    a, ref = _run(ctx, entries, caps, verify=True)
    ref_stats = ctx.frames_device_stats(verify=True)
    blob = bytearray()
    offs = []
    for z in entries:
        blob += b"\x00" * ((-len(blob)) % 8 + 3)                                  # (sources at odd addresses)
        offs.append(len(blob))
        blob += z
    src = torch.frombuffer(blob, dtype=torch.uint8).to("cuda:0")
    keep = src.clone()
    b = _arena(caps)
    res = ctx.decode_frames_device_src([src.data_ptr() + o for o in offs], [len(z) for z in entries], b.ptrs, caps, verify=True)
    assert [full_key(r) for r in res] == [full_key(r) for r in ref]
    torch.cuda.synchronize()
    assert torch.equal(a.t, b.t) and torch.equal(src, keep)
    st = ctx.frames_device_stats(verify=True)
    assert st["entries_failed_verify"] == ref_stats["entries_failed_verify"] == 3
    assert [r.status for r in res].count(zgpu.E_CHECKSUM_MISMATCH) == 3


def test_dictionary_frame_alone_and_in_the_shared_submit(good):
    raw = read_pack("dict_tests.pack")["dictionary"]
    plains, frames, _ = good
    c = zgpu.Context(0)
    try:
        did = c.add_dict(raw)
        plain = plains[7]
        z, _ = make_frame(plain, dict_id=did)
        assert oracle_alone(z, len(plain), raw) == (0, plain)
        entries, caps = [flip_checksum(z), frames[4], z], [len(plain), len(plains[4]), len(plain)]
        for shared in (False, True):
            c.set_frames_shared_dicts(shared)
            a, res = _run(c, entries, caps)                                       # without verify: as today
            assert [(r.status, r.written, r.checksum_mismatches) for r in res] == [(0, len(plain), 1), (0, len(plains[4]), 0), (0, len(plain), 0)]
            a.check([plain, plains[4], plain])
            assert (c.frames_device_stats()["entries_alone"] > 0) == (not shared)
            assert (c.frames_dict_stats()["frames_shared"] > 0) == shared
            a, res = _run(c, entries, caps, verify=True)
            assert full_key(res[0]) == (zgpu.E_CHECKSUM_MISMATCH, 0, 0, 1, 1, 0, 0, 0, 0), (shared, full_key(res[0]))
            assert [(r.status, r.written, r.checksum_mismatches) for r in res[1:]] == [(0, len(plains[4]), 0), (0, len(plain), 0)]
            a.check([None, plains[4], plain])
            assert c.frames_device_stats(verify=True)["entries_failed_verify"] == 1
    finally:
        c.close()


def test_status_name():
    assert zgpu.load_library().zgpu_status_name(zgpu.E_CHECKSUM_MISMATCH) == b"ChecksumMismatch"
    assert zgpu.E_CHECKSUM_MISMATCH == 70
    assert "ChecksumMismatch" in str(zgpu.ZgpuError(zgpu.E_CHECKSUM_MISMATCH))
