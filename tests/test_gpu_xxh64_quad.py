"""zg_k_xxh64q (four lanes per range) and zg_k_xxh64 (one lane per range) on the GPU through zgpu_debug_hash_ranges (Context.hash_ranges):
both kernels against the oracle's XXH64 on ranges of one device tensor of 1 MiB + 64 random bytes. The expected digests come from the oracle
only, once per module. No range leaves the tensor, and the two refused calls are refused on the host, before any launch."""
import random

import pytest
import torch   # (before the library is loaded: the process must run on one HIP runtime)

from test_xxh64_quad_cpu import DATA_BYTES, quad_cases, quad_data

pytestmark = pytest.mark.gpu
R = 16                                             # zgx::kQuadRound (test_round_constant reads it from the header)


@pytest.fixture(scope="module")
def ctx():
    import zgpu
    c = zgpu.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """(the bytes, their device tensor, a memo of the oracle's digests)"""
    import oracle
    host = quad_data()
    t = torch.frombuffer(bytearray(host), dtype=torch.uint8).to("cuda:0")
    torch.cuda.synchronize()
    assert t.numel() == DATA_BYTES
    memo, O = {}, oracle.lib()

    def want(off, n):
        if (off, n) not in memo:
            memo[(off, n)] = O.zor_xxh64(host[off:off + n], n, 0)
        return memo[(off, n)]
    return host, t, want


def _check(ctx, data, cases, kernels=(4, 0, 1)):
    _, t, want = data
    offs, lens = [o for o, _ in cases], [n for _, n in cases]
    assert all(o + n <= DATA_BYTES for o, n in cases)
    exp = [want(o, n) for o, n in cases]
    for k in kernels:
        got = ctx.hash_ranges(t.data_ptr(), offs, lens, kernel=k)
        bad = [(i, cases[i], hex(got[i]), hex(exp[i])) for i in range(len(cases)) if got[i] != exp[i]]
        assert not bad, (k, len(bad), bad[:5])


def test_round_constant():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "zstd-rs_amd", "csrc", "zg_xxh64_dev.h")).read()
    assert int(re.search(r"kQuadRound = (\d+);", hdr).group(1)) == R


def test_lengths_and_offsets_of_the_cpu_test(ctx, data):
    """every length 0 .. 300, the round boundaries, offsets 1 .. 16, 40 random lengths: in one call per kernel, and one range at a time for
    the lengths around the stripe and round boundaries (a lone range is a wave with one live quad)"""
    cases = quad_cases(R)
    _check(ctx, data, cases)
    for c in [(0, 0), (0, 31), (0, 32), (3, 33), (0, 32 * R - 1), (0, 32 * R), (5, 64 * R + 31), (1, 96 * R + 7)]:
        _check(ctx, data, [c], kernels=(4, 1))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 1000])
def test_range_counts_mixed_lengths(ctx, data, n):
    """short ranges (< 32 bytes: lane 0 alone) between long ones, so that the longest-first permutation moves every digest, the launch's last
    wave is partly filled, and digests[i] must still be range i's"""
    rng = random.Random(1000 + n)
    cases = []
    for i in range(n):
        kind = i % 4
        ln = (rng.randrange(0, 32) if kind == 1 else rng.randrange(32, 32 * R) if kind == 2 else
              rng.randrange(32 * R, 40000) if kind == 3 else rng.randrange(40000, 200000))
        if n > 100 and kind == 0:
            ln = rng.randrange(32 * R * 2, 20000)          # (1000 ranges: keep the call short)
        cases.append((rng.randrange(0, DATA_BYTES - ln + 1), ln))
    _check(ctx, data, cases)


def test_range_ends_at_the_tensors_last_byte(ctx, data):
    cases = [(DATA_BYTES - n, n) for n in (1, 31, 32, 33, 32 * R, 32 * R + 1, 64 * R + 31, 4096 + 13, DATA_BYTES)]
    _check(ctx, data, cases)
    for c in cases[:-1]:
        _check(ctx, data, [c], kernels=(4, 1))


def test_bad_pointers_are_refused_before_any_launch(ctx, data):
    import ctypes as C
    import zgpu
    host, t, _ = data
    hb = C.create_string_buffer(host[:4096], 4096)
    for kernel in (0, 1, 4):
        with pytest.raises(zgpu.ZgpuError) as e:                       # a host pointer
            ctx.hash_ranges(C.addressof(hb), [0], [4096], kernel=kernel)
        assert e.value.status == zgpu.E_BAD_ARG
        with pytest.raises(zgpu.ZgpuError) as e:                       # a range that leads past the allocation (by far: no neighbour holds it)
            ctx.hash_ranges(t.data_ptr(), [0, 64], [32, 1 << 40], kernel=kernel)
        assert e.value.status == zgpu.E_BAD_ARG
    with pytest.raises(zgpu.ZgpuError) as e:                           # a kernel that does not exist
        ctx.hash_ranges(t.data_ptr(), [0], [32], kernel=2)
    assert e.value.status == zgpu.E_BAD_ARG
    _check(ctx, data, [(0, 4096)])                                     # (the context is as good as before)
