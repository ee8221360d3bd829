"""The zx_* primitives as zg_kernels.hip defines them for gfx950, one primitive and one workgroup per launch (zg_k_zxprobe through
zgpu_debug_zx_probe, Context.zx_probe), against the plain model of tests/zxprobe.py: the cases tests/test_zxprobe_cpu.py runs on the CPU
emulator, on libzgpu.so and on libzgpu_dev.so. Result words and the whole arena equal the model's bit for bit; the operand words and the
arena that went up are unchanged. Every case passes the host's argument rules (tests/test_zxprobe_cpu.py), so no launch can touch a byte
outside its own three allocations: the resource has 256 bytes of arena on either side, no buffer offset can wrap, every index is checked.
Where the hardware disagrees with the model, the hardware is right: the model and the emulator change (DESIGN.md "The emulator as a tested
model")."""
import pytest
import torch   # noqa: F401  (before the library is loaded: the process must run on one HIP runtime)

import zxprobe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    cs = zxprobe.all_cases()
    return cs, [zxprobe.model(c) for c in cs]


def run_cases(ctx, cases, wants):
    """[(case name, what differs)] over all cases"""
    bad = []
    for c, (out, arena) in zip(cases, wants):
        got, got_arena, a = ctx.zx_probe(c.op, c.threads, c.flags, c.res_off, c.res_bytes, c.inp, c.out0, c.arena)
        if got != out:
            t = next(i for i in range(len(out)) if got[i] != out[i])
            bad.append((c.name, "result word %d of thread %d: 0x%08X, the model 0x%08X; operands %s" % (
                t % zxprobe.K_OUT, t // zxprobe.K_OUT, got[t], out[t], ["0x%X" % w for w in c.a(t // zxprobe.K_OUT)[:4]])))
        if got_arena != arena:
            i = next(i for i in range(len(arena)) if got_arena[i] != arena[i])
            bad.append((c.name, "arena byte %d (resource at %d, %d bytes): 0x%02X, the model 0x%02X" % (i, c.res_off, c.res_bytes, got_arena[i], arena[i])))
        assert a == c.inp, c.name
    return bad


@pytest.mark.parametrize("dev", [False, True], ids=["libzgpu", "libzgpu_dev"])
def test_hardware_equals_the_model(cases, dev):
    import zgpu
    ctx = zgpu.Context(0, dev=dev)
    try:
        bad = run_cases(ctx, *cases)
    finally:
        ctx.close()
    assert not bad, (len(bad), bad[:12])


def test_a_refused_call_launches_nothing():
    """the rules of tests/test_zxprobe_cpu.py hold with a real context too: an offset that could wrap is a status"""
    import zgpu
    ctx = zgpu.Context(0)
    try:
        c = next(c for c in zxprobe.all_cases() if c.opname == "Ld128" and not c.flags)
        inp = list(c.inp)
        inp[1] = 0xFFFFFFF0
        with pytest.raises(zgpu.ZgpuError) as e:
            ctx.zx_probe(c.op, c.threads, c.flags, c.res_off, c.res_bytes, inp, c.out0, c.arena)
        assert e.value.status == zgpu.E_BAD_ARG
    finally:
        ctx.close()
