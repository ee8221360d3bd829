"""The lane routine of zg_k_xxh64 (zstd-rs_amd/csrc/zg_xxh64_dev.h), compiled with g++ (tests/emu/zg_lane_xxh64.cpp,
built by tests/lanesuite.py), against the oracle's XXH64; and zgpu_decode_frames'
argument check, which needs no GPU."""
import ctypes as C
import random

import lanesuite


def _lane(tmp_path):
    L, _ = lanesuite.build(tmp_path, "zg_lane_xxh64.cpp", "xxh64_lane")
    L.lane_xxh64.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.lane_xxh64.restype = C.c_uint64
    return L


def _oracle():
    import oracle
    return oracle.lib()


def test_lane_xxh64_matches_oracle(tmp_path):
    L, O = _lane(tmp_path), _oracle()
    rng = random.Random(0x5EED)
    buf = bytes(rng.getrandbits(8) for _ in range((1 << 20) + 64))
    cbuf = C.create_string_buffer(buf, len(buf))
    base = C.addressof(cbuf)

    def check(off, n, seed=0):
        want = O.zor_xxh64(buf[off:off + n], n, seed)
        got = L.lane_xxh64(base + off, n, seed)
        assert got == want, (off, n, seed, hex(got), hex(want))

    for n in range(0, 301):                       # short inputs, every tail shape, 1 .. 9 stripes
        check(0, n)
    for off in range(1, 17):                      # unaligned starts
        for n in (0, 1, 7, 8, 31, 32, 33, 63, 64, 65, 100, 255, 4096 + 13):
            check(off, n)
    for _ in range(40):                           # random lengths up to 1 MiB at random offsets
        n = rng.randrange(0, 1 << 20)
        check(rng.randrange(0, 64), n)
    check(0, 1 << 20)
    check(3, 1000, seed=12345)                    # (any seed: the frames use 0)


def test_decode_frames_null_ctx_is_bad_arg():
    import zgpu
    L = zgpu.load_library()
    n = 1
    srcs, lens = (C.c_void_p * n)(), (C.c_size_t * n)()
    dsts, caps = (C.c_void_p * n)(), (C.c_size_t * n)()
    res = (zgpu.EntryResultC * n)()
    assert L.zgpu_decode_frames(None, srcs, lens, n, dsts, caps, res) == 93       # ZGPU_E_BAD_ARG, no GPU touched
    assert L.zgpu_batch_checksums(None, None, 0) == 93


def test_plaintext_bound_walks_headers():
    """zgpu_plaintext_bound (the C walk zgpu_decode_frames cuts its submits by, also Context.decode_frames' default capacity)"""
    import zgpu
    L = zgpu.load_library()
    bound = lambda b: L.zgpu_plaintext_bound(b, len(b))           # noqa: E731
    assert zgpu.plaintext_bound is not None and zgpu.plaintext_bound(b"abc") == bound(b"abc")
    # one frame: single segment, FCS 5, one raw last block of 5 bytes, no checksum
    raw = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 5]) + (1 | (0 << 1) | (5 << 3)).to_bytes(3, "little") + b"hello"
    assert bound(raw) == 5
    skip = (0x184D2A50).to_bytes(4, "little") + (3).to_bytes(4, "little") + b"abc"
    assert bound(skip + raw + raw) == 10
    assert bound(raw[:7]) == 0                                          # a block header that is not all there
    assert bound(b"") == 0 and bound(skip) == 0 and bound(b"\x00" * 40) == 0
    # no content size, a window descriptor, one compressed block of 10 bytes (+ checksum): 128 KiB
    comp = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x04, 0x58]) + (1 | (2 << 1) | (10 << 3)).to_bytes(3, "little") + bytes(10) + bytes(4)
    assert bound(comp) == 128 << 10
    assert bound(comp + raw) == (128 << 10) + 5
    # a declared content size smaller than what the blocks can give lowers the bound
    small = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x20, 3]) + (1 | (2 << 1) | (10 << 3)).to_bytes(3, "little") + bytes(10)
    assert bound(small) == 3
    # the walk stops at the first frame it cannot finish, keeping what it found
    assert bound(raw + comp[:12]) == 5 + (128 << 10)
    assert bound(raw + b"garbage" + raw) == 5
