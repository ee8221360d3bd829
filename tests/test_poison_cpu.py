"""The CPU harness under other memory histories (tests/emu/zg_emu_fill.h). What no stage of a submit has written holds one fixed value per
site in the harness (0xAA in the output, 0xEEEEEEEE in the flatten scratch, 0x55 / 0xEE in the literals, 0xDEADBEEF / 0xFFFF in the table
slots, zeros in the record arrays and pads), so every routine run here has been checked against exactly one history. zgemu_set_fill
replaces all of them by one byte. Every frame of every hand-built family goes through framesuite.check_on_harness — plaintext, the
oracle's per-block records, zg_exact.h's verdict — under each fill, and what the harness leaves (the walk's status, every frame's size,
status, failing block and good blocks' bytes) must be the same as under the sites' own values. The SOURCE of the kernels that
run on those arenas — both flatten bodies with the sweep model and zg_k_sparse's body (zg_flat1.h, zg_flat4.h, zg_inorder.h), zg_k_huf's
body in both placements (zg_huf.h), zg_k_lz's body (zg_inorder.h) and zg_k_seqsize's (zg_seqsize.h) — runs under each fill on the frames
the SIMT emulator gets through in well under a second each (SMALL_*); the bytes and verdicts must be the generators' and the oracle's.
tests/test_gpu_poison.py asks the same of the GPU build through ZGPU_POISON."""
import contextlib
import ctypes as C

import pytest

import blockframes
import emu
import framesuite
import hufstreams
import latelits
import repframes
import seqframes
import seqstreams
import sweepframes
import tabframes
import test_flat1_cpu
import test_huf_cpu
import test_hufstreams_cpu
import test_seqsize_cpu

FILLS = (0xA5, 0xFF)                       # beside every site's own value (None)
# generator -> (status table, oblocks(name) for check_on_harness)
GENS = {
    "tabframes": (tabframes, tabframes.STATUS, None),
    "hufstreams": (hufstreams, hufstreams.STATUS, None),
    "seqstreams": (seqstreams, seqstreams.STATUS, lambda name: (lambda z: seqstreams.oracle_blocks(name, z))),
    "repframes": (repframes, repframes.STATUS, None),
    "blockframes": (blockframes, blockframes.STATUS, None),
    "seqframes": (seqframes, None, None),
    "sweepframes": (sweepframes, {}, None),
    "latelits": (latelits, latelits.STATUS, None),
}
built = test_seqsize_cpu.built                  # (the fixture that builds tests/emu/zg_emu_seqsize.cpp)
SMALL_BLOCKS, SMALL_BYTES, SMALL_SEQS = 6, 40000, 600     # a frame the emulator's fibers get through in well under a second


@contextlib.contextmanager
def fill(v):
    """the harness's fill is v (None: every site's own value) inside the block, and what it was behind it"""
    L = emu.lib()
    was = L.zgemu_set_fill(-1 if v is None else v)
    try:
        yield
    finally:
        L.zgemu_set_fill(was)


def test_the_fill_reaches_the_harness():
    """the self-test of the switch: the flatten scratch of a frame with a direct unit only is never written, and reads back as the fill"""
    name, z, plain = next(f for f in seqframes.family("seq_counts") if [u[3] for u in emu.Plan(f[1]).units] == [2])   # (one direct unit)
    seen = []
    for v in (None,) + FILLS:
        with fill(v):
            st, got, og, units = test_flat1_cpu.run_flatten(z, 0, 0)
        assert st == 0 and got == plain and [u[3] for u in units] == [2], (name, units)
        assert len(set(og.tolist())) == 1
        seen.append(int(og[0]))
    assert seen == [0xEEEEEEEE] + [0x01010101 * v for v in FILLS]


def snapshot(e):
    """what the harness left of one entry (e: the batch check_on_harness decoded): the walk's status, every frame's (size, status, failing
    block, bytes)"""
    L = test_huf_cpu._lib()
    assert e.nframes <= 1
    frames = []
    for f in range(e.nframes):
        _, size, st, bad = e.frame(f)
        data = e.frame_bytes(f)[0]
        if st and bad < e.nblocks:      # (a frame that fails in execution keeps the size of all its blocks here: its good blocks' bytes)
            data = data[:L.zgemu_block_out_base(e.h, bad)]
        frames.append((size, st, bad, data))
    return e.parse_status, frames          # (zg_exact.h's verdict: check_on_harness asserts it against the oracle's under every fill)


@pytest.mark.parametrize("gen", sorted(GENS))
def test_every_family_under_every_fill(gen):
    mod, status, ob = GENS[gen]
    frames = mod.all_frames()
    ran = 0
    for _, name, z, plain in frames:
        check = lambda: snapshot(framesuite.check_on_harness(name, z, plain, status, *((ob(name),) if ob else ())))
        want = snapshot(emu.EmuBatch(z, max_window=1 << 31))       # (the sites' own values: the generator's own CPU suite runs check_on_harness there)
        for v in FILLS:
            with fill(v):
                got = check()
            assert got == want, (name, "fill 0x%02X against the sites' own values" % v)
        ran += 1
    assert ran == len(mod.all_frames())


def _small(z, plain):
    if plain is None or len(plain) > SMALL_BYTES:
        return False
    p = emu.Plan(z)
    return p.nblocks <= SMALL_BLOCKS and sum(p.nseq) <= SMALL_SEQS


@pytest.mark.parametrize("gen", sorted(GENS))
def test_kernel_sources_under_every_fill(gen):
    """the small valid frames of the generator: both flatten bodies (one block per unit, so that every frame of two blocks has a pointer-mode
    unit; the plan's own units as well), zg_k_huf's body with the literals in the arena and straight in the output, zg_k_lz's body"""
    mod = GENS[gen][0]
    small = [f for f in mod.valid_frames() if _small(f[2], f[3])]
    assert small, gen
    for _, name, z, plain in small:
        for v in (None,) + FILLS:
            with fill(v):
                for ub in (0, 1):
                    st, got, _, _ = test_flat1_cpu.run_flatten(z, ub, 0)
                    assert st == 0 and got == plain, (name, "flatten", ub, v)
                for direct in (False, True):
                    if gen == "hufstreams":       # (its unevenly split streams end with the true counts and a count mismatch: its own check)
                        test_hufstreams_cpu._kernel_source(name, z, plain, direct)
                    else:
                        test_huf_cpu.check_against_model(z, direct)      # (every Huffman-coded block: the serial model's literals and counts)
                e = emu.EmuBatch(z, max_window=1 << 31)
                out, verdicts = e.inorder_lz()
                assert out == plain and verdicts[0][0] == 0, (name, "zg_k_lz", v, verdicts)


def test_seqsize_source_under_every_fill(built):
    """zg_k_seqsize's source (tests/test_seqsize_cpu.py) on seqstreams' valid frames: the sums and the status are the oracle's whatever the
    input's pads, the slots of the FSE arena behind a table's last entry, the state records behind nseq and the workgroup's LDS hold"""
    built.sz_set_fill.argtypes = [C.c_int]
    frames = [f for f in seqstreams.valid_frames() if len(f[2]) < 20000]
    assert len(frames) >= 20
    try:
        for v in FILLS:
            built.sz_set_fill(v)
            for _, name, z, plain in frames:
                test_seqsize_cpu.check_valid(built, name, z, seqstreams.oracle_blocks(name, z), (0, 3))
    finally:
        built.sz_set_fill(-1)

