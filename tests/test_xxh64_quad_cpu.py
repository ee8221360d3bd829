"""The quad routine of zg_k_xxh64q (zstd-rs_amd/csrc/zg_xxh64_dev.h: xxh64q_acc, xxh64q_finish), compiled with g++ (tests/emu/zg_lane_xxh64_quad.cpp,
built by tests/lanesuite.py), against the oracle's XXH64.

The harness plays one quad: lane l = 0 .. 3 computes its accumulator over the whole stripes (the lanes exchange nothing before the gather, so
running them one after the other is what four lanes in lockstep compute), the gather is four plain variables, and lane 0's finish does the
merge, the tail and the avalanche. The length and offset lists are shared with tests/test_gpu_xxh64_quad.py (quad_cases)."""
import ctypes as C
import random

import lanesuite

DATA_BYTES = (1 << 20) + 64


def quad_data():
    rng = random.Random(0x5EED)
    return rng.randbytes(DATA_BYTES)


def quad_cases(R):
    """(offset, length) of every range the issue lists, for a loop unrolled by R stripes; all inside DATA_BYTES"""
    cases = [(0, n) for n in range(0, 301)]                                         # every short length, every tail shape
    for k in (1, 2, 3):                                                               # one, two, three rounds: the loop's two exits and its body
        cases += [(0, 32 * R * k - 1), (0, 32 * R * k), (0, 32 * R * k + 1), (0, 32 * R * k + 31)]
    cases += [(0, 32 * R - 1), (0, 32 * R), (0, 32 * R + 1), (0, 64 * R - 1), (0, 64 * R + 31)]
    for off in range(1, 17):                                                          # unaligned starts
        cases += [(off, n) for n in (0, 1, 31, 32, 33, 63, 64, 65, 4096 + 13)]
    rng = random.Random(0xC0FFEE)
    for _ in range(40):                                                               # random lengths below 1 MiB at random offsets
        cases.append((rng.randrange(0, 64), rng.randrange(0, 1 << 20)))
    cases.append((64, 1 << 20))                                                       # ends at the data's last byte
    return cases


def _quad(tmp_path):
    L, _ = lanesuite.build(tmp_path, "zg_lane_xxh64_quad.cpp", "xxh64_quad")
    L.quad_xxh64.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.quad_xxh64.restype = C.c_uint64
    L.quad_round.restype = C.c_uint32
    return L


def test_quad_xxh64_matches_oracle(tmp_path):
    import oracle
    L, O = _quad(tmp_path), oracle.lib()
    buf = quad_data()
    cbuf = C.create_string_buffer(buf, len(buf))
    base = C.addressof(cbuf)
    R = L.quad_round()
    assert R >= 1

    def check(off, n, seed=0):
        assert off + n <= len(buf)
        want = O.zor_xxh64(buf[off:off + n], n, seed)
        got = L.quad_xxh64(base + off, n, seed)
        assert got == want, (off, n, seed, hex(got), hex(want))

    for off, n in quad_cases(R):
        check(off, n)
    for off, n in ((3, 1000), (0, 31), (5, 32 * R * 3 + 77)):                         # (any seed: the frames use 0)
        check(off, n, seed=12345)
