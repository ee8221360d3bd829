"""No result may depend on device memory its submit never wrote. Every arena of the engine is grow-only, so a submit starts on what
earlier submits left, and every other suite here runs the same frames in the same order on long-lived contexts: one memory history.
Here the development build fills every byte the design does not define when a submit starts (ZGPU_POISON, zg_engine.h: Poison) with
0x00, 0xA5 and 0xFF, a fresh context per value, and every hand-built family runs under each: framesuite.submit with the oracle's
per-block records, submit_verdicts of every invalid frame among valid ones in shared submits (_verdict_submits), check_decode_frames,
sweepframes' plan / scratch / sweep-mode check, the block-by-block decoder with k = 1 and 4 on the multi-block families, the
streaming decoder in its four modes. Every frame alone gives (status, failing block, out_size, bytes): the oracle's, and identical
across the three values; the message names the frame and the two values. The device-resident surfaces — decode_frames_device and
_device_src, decode_ranges_device_src, the seek-table call with verify_table, gather_ranges, the seek index calls (create, measure,
hash, indexed gathers) — and the dictframes cases in the shared-dictionary submits each run one scenario of their own test file
under the three values in one test. test_the_fill_reaches_memory shows that the switch does something.
The product library has no switch: test_product_build_after_a_dirtying_submit gives it another history the way a caller would, a
large submit in front of every family, the families in reverse and in forward order on one context."""
import hashlib

import pytest
import torch   # noqa: F401  (before the library is loaded: the process must run on one HIP runtime)

import blockframes
import framesuite
import hufstreams
import latelits
import repframes
import seqframes
import seqstreams
import sweepframes
import tabframes
from framesuite import POISONS, poisoned_context

pytestmark = pytest.mark.gpu

# generator -> (module, STATUS for check_decode_frames, oblocks or None: blockcheck.oracle_blocks)
GENS = {
    "tabframes": (tabframes, tabframes.STATUS, None),
    "hufstreams": (hufstreams, hufstreams.STATUS, None),
    "seqstreams": (seqstreams, seqstreams.STATUS, seqstreams.oracle_blocks),
    "repframes": (repframes, repframes.STATUS, None),
    "blockframes": (blockframes, blockframes.STATUS, None),
    "seqframes": (seqframes, {}, None),
    "sweepframes": (sweepframes, {}, None),
    "latelits": (latelits, latelits.STATUS, None),
}
ORDER = list(GENS)
_ALONE = {}      # (generator, poison) -> {frame name: (status, failing block, out_size, sha256 of the bytes)}
_ORACLE = {}     # generator -> {frame name: the same from the oracle}
_VERDICT = {}    # generator -> {name of an invalid frame: (status, failing block, bytes of the good blocks)} from the oracle
_OBLOCKS = {}


def _key(v):
    return v[0], v[1], v[2], hashlib.sha256(v[3]).hexdigest()


def _judged(key):
    """a key as it is held against the oracle's: a frame that did not fail has no failing block (the oracle counts its blocks there)"""
    return key if key[0] else (key[0], None) + key[2:]


def _oracle(gen):
    if gen not in _ORACLE:
        _ORACLE[gen], _VERDICT[gen] = {}, {}
        for _, name, z, plain in GENS[gen][0].all_frames():
            st, bad, good = framesuite.oracle_verdict(z)
            assert (st == 0) == (plain is not None), name
            _ORACLE[gen][name] = _key((st, bad, len(good), good))
            if plain is None:
                _VERDICT[gen][name] = (st, bad, good)
    return _ORACLE[gen]


def _oblocks(gen):
    import blockcheck
    mod, _, ob = GENS[gen]
    if ob is not None:
        return ob
    if gen not in _OBLOCKS:
        _OBLOCKS[gen] = {name: blockcheck.oracle_blocks(z) for _, name, z, _ in mod.valid_frames()}
    return _OBLOCKS[gen]


def _frames(mod):
    """(valid, invalid) frames of a generator"""
    every = mod.all_frames()
    return [f for f in every if f[3] is not None], [f for f in every if f[3] is None]


def _submits(gen, valid):
    """the valid frames as the generator's own test_submit cuts them"""
    if gen == "seqstreams":
        large = [f for f in valid if f[1] in seqstreams.LARGE]
        return [large, [f for f in valid if f[1] not in seqstreams.LARGE]]
    return [valid]


def _alone(c, mod):
    """{name: (status, failing block, out_size, sha256 of the bytes, the walk's status)} of every frame of a generator as a submit of its own"""
    out = {}
    for _, name, z, _ in mod.all_frames():
        v = framesuite.frame_alone(c, z)
        out[name] = _key(v) + (v[4],)
    return out


def _verdict_submits(c, gen, valid, invalid, alone):
    """framesuite.submit_verdicts of every invalid frame of a generator among valid ones: status, failing block, out_size and the good
    blocks' bytes of a frame whose arenas have neighbours. repframes and latelits bring their own tables and their own mix. For the other
    generators the three come from the oracle block by block (framesuite.oracle_verdict). A frame in which the host's walk finds the
    error ends its submit, prepare parses nothing behind it; alone[name][4], the walk's status of the frame alone, says which these are
    (it only sorts the frames, every expectation is the oracle's). All the others share one submit, an invalid frame behind every second
    valid one; each of those closes a submit of its own, behind two valid frames and an invalid one between them, and the walk's
    status there is the oracle's status of that frame"""
    if not invalid:
        return
    if gen == "repframes":
        from test_gpu_repframes import _mixed
        return framesuite.submit_verdicts(c, _mixed(valid, invalid), repframes.STATUS, repframes.GOOD, lambda n: repframes.META[n]["bad_block"])
    if gen == "latelits":
        from test_gpu_latelits import _mixed
        frames, ps = _mixed(valid, invalid)
        return framesuite.submit_verdicts(c, frames, latelits.STATUS, latelits.GOOD, lambda n: latelits.META[n]["bad_block"], parse_status=ps)
    _oracle(gen)
    v = _VERDICT[gen]
    status, good = {n: x[0] for n, x in v.items()}, {n: x[2] for n, x in v.items()}
    small = [f for f in valid if gen != "seqstreams" or f[1] not in seqstreams.LARGE]
    dev = [f for f in invalid if alone[f[1]][4] == 0]
    host = [f for f in invalid if alone[f[1]][4] != 0]
    assert dev and len(small) >= 2, (gen, len(dev), len(small))
    every = 2 if len(small) >= 2 * len(dev) else 1            # (seqstreams has about as many invalid frames as small valid ones)
    framesuite.submit_verdicts(c, framesuite.interleave(small, dev, every), status, good, lambda n: v[n][1])
    for i, f in enumerate(host):
        front = [small[(2 * i) % len(small)], dev[i % len(dev)], small[(2 * i + 1) % len(small)]]
        framesuite.submit_verdicts(c, front + [f], status, good, lambda n: v[n][1], parse_status=status[f[1]])


def _family_run(c, gen):
    """everything one generator runs on one context; {name: key} of every frame alone"""
    mod, status, _ = GENS[gen]
    valid, invalid = _frames(mod)
    for frames in _submits(gen, valid):
        framesuite.submit(c, frames, _oblocks(gen))
    if gen == "sweepframes":
        from test_gpu_sweepframes import check_submit
        for sname, (mode, frames) in sweepframes.submits().items():
            check_submit(c, sname, frames, mode)
    # every frame alone: what most generators have no table of (failing block, out_size, the good blocks' bytes) comes from the oracle
    alone = _alone(c, mod)
    _verdict_submits(c, gen, valid, invalid, alone)
    if gen == "repframes":
        from test_gpu_repframes import _mixed
        big = [f for f in valid if repframes.META[f[1]]["nblocks"] >= 1000]
        framesuite.check_decode_frames(c, _mixed(valid, invalid) + big, status)
    else:
        framesuite.check_decode_frames(c, framesuite.interleave(valid, invalid, 2) if invalid else valid, status)
    return {name: v[:4] for name, v in alone.items()}


def _against_the_oracle(gen, poison, got):
    want = _oracle(gen)
    assert len(got) == len(GENS[gen][0].all_frames()) == len(want)
    wrong = [(name, got[name][:3], want[name][:3]) for name in want if _judged(got[name]) != _judged(want[name])]
    assert not wrong, ("poison 0x%02X against the oracle: (frame, got, oracle)" % poison, len(wrong), wrong[:10])


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "0x%02X" % p)
@pytest.mark.parametrize("gen", ORDER)
def test_family_under_poison(gen, poison, monkeypatch):
    with poisoned_context(monkeypatch, poison) as c:
        got = _family_run(c, gen)
        assert c.tuning()["poisoned_bytes"] > 0
    _against_the_oracle(gen, poison, got)
    _ALONE[gen, poison] = got


@pytest.mark.parametrize("gen", ORDER)
def test_identical_across_poisons(gen, monkeypatch):
    """(status, failing block, out_size, bytes) of every frame alone under the three values. test_family_under_poison has left them
    where it ran in this process; a value it has not run (this test selected alone, or tests spread over processes) runs here, every
    frame alone on a fresh context"""
    runs = []
    for p in POISONS:
        if (gen, p) not in _ALONE:
            with poisoned_context(monkeypatch, p) as c:
                _ALONE[gen, p] = {name: v[:4] for name, v in _alone(c, GENS[gen][0]).items()}
            _against_the_oracle(gen, p, _ALONE[gen, p])
        runs.append((p, _ALONE[gen, p]))
    (p0, first) = runs[0]
    for p, other in runs[1:]:
        assert len(other) == len(first) == len(GENS[gen][0].all_frames())
        for name in first:
            assert first[name] == other[name], "frame %s differs between poison 0x%02X and 0x%02X: %r / %r" % (name, p0, p, first[name][:3], other[name][:3])


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "0x%02X" % p)
@pytest.mark.parametrize("k", [1, 4])
def test_block_by_block_under_poison(k, poison, monkeypatch):
    """carried tables, offset history and the window rebuilt call by call: sweepframes' tails_heads and beyond_window, repframes' and
    seqstreams' frames that carry tables across blocks (the ones their own suites step through)"""
    from test_gpu_repframes import STEP_FRAMES
    with poisoned_context(monkeypatch, poison) as c:
        for fam in ("tails_heads", "beyond_window"):
            for name, z, plain in sweepframes.family(fam):
                st, out, _ = framesuite.lockstep(c, name, z, k=k, header=(0, 6))
                assert name == "bw_w1" or (st == 0 and out == plain), (name, st)
        for _, name, z, plain in repframes.valid_frames():
            if name in STEP_FRAMES[2:] or repframes.META[name]["nblocks"] in range(2, 12):
                st, out, _ = framesuite.lockstep(c, name, z, k=k)
                assert st == 0 and out == plain, (name, k, st)
        for name, z, plain in seqstreams.family("workgroup_mixes"):
            if plain is not None and len(plain) < 1 << 22:
                st, out, _ = framesuite.lockstep(c, name, z, k=k)
                assert st == 0 and out == plain, (name, k, st)


@pytest.mark.parametrize("poison", POISONS, ids=lambda p: "0x%02X" % p)
def test_streaming_modes_under_poison(poison, monkeypatch):
    """the streaming decoder's four MODES (tests/test_gpu_stream.py) on two small corpus frames and on the frame whose offset reaches
    beyond the window: a dropped run, rebase and the block-by-block schedule, every read() against the oracle's"""
    import random
    from golden_io import read_manifest, read_pack
    from test_gpu_stream import MODES, K, frame, lit_block, oracle_reads, patterns, raw_block, same, seq_block, zgpu_reads
    pack, man = read_pack("decodecorpus.pack"), read_manifest("decodecorpus.json")
    names = [n for n in sorted(man) if 0 < man[n]["size"] <= 1 << 20][:2]
    assert len(names) == 2
    far = frame(*([raw_block(K, i) for i in range(12)] + [seq_block(6 * K)] + [raw_block(K, 40 + i) for i in range(6)] + [lit_block(100, last=True)]))
    rng = random.Random(61)
    cases = [(n, pack[n], list(patterns(rng, man[n]["size"]))[0]) for n in names] + [("far", far, [8192] * 400), ("far", far, [20 * K] * 3)]
    with poisoned_context(monkeypatch, poison) as c:
        for name, z, pat in cases:
            want, o = oracle_reads(z, pat)
            for kw in MODES:
                for callback in (False, True):
                    got, s = zgpu_reads(c, z, pat, callback, **kw)
                    same(want, got, (name, kw, callback, poison))
                    s.close()


# ---- the device-resident surfaces and the shared-dictionary submits: one small scenario of each surface's own test file, through the helpers that
# file exports, which hold every status, `written`, record and destination byte (guards included) against the models and the oracle. A scenario
# returns what it got, in parts, and test_device_resident_surface_under_every_poison requires every part identical under the three values.
_BUILT = {}      # inputs of the scenarios that cost something to build, made once


def _once(name, make):
    if name not in _BUILT:
        _BUILT[name] = make()
    return _BUILT[name]


def _bytes_of(arena):
    return arena.t.cpu().numpy().tobytes()


def _decode_frames_device(c):
    """decode_frames_device and decode_frames_device_src (tests/test_gpu_blockframes.py's scenario): both calls agree; status, written,
    checksum fields and bytes are the plaintext's"""
    from devmem import full_key, xxh32
    from test_gpu_decode_frames_device_src import _both
    frames = [f for f in blockframes.valid_frames() if f[0] in ("neighbours", "sources", "lit_alignment")]
    entries, plains = [z for _, _, z, _ in frames], [p for _, _, _, p in frames]
    caps = [len(p) + (j % 2) * 5 for j, p in enumerate(plains)]
    arena, res, _ = _both(c, entries, caps, shifts=[(7 * j) % 32 for j in range(len(entries))], src_shifts=[(3 * j) % 18 for j in range(len(entries))])
    for (_, name, z, plain), r in zip(frames, res):
        assert (r.status, r.written, r.nframes, r.checksum_mismatches) == (0, len(plain), 1, 0), (name, r)
        if z[4] & 4 and r.first_hashed:
            assert r.checksum_from_data == r.calculated_checksum == xxh32(plain), (name, r)
    arena.check(plains)
    return [full_key(r) for r in res], _bytes_of(arena)


def _decode_ranges(c):
    """decode_ranges_device_src (tests/test_gpu_decode_ranges.py: six text frames, a reserved block type, a truncated entry, ranges inside a
    frame, across a boundary and behind the plaintext), every frame hashed: run_and_check, and the checksum fields from the oracle's
    decode of the frames the model says are taken"""
    from devmem import ALL, full_key, xxh32
    from test_gpu_decode_ranges import _decode, _edit, _six_frames, chain, run_and_check, select
    z, plains = _six_frames()
    fr = chain(z)
    off = [sum(len(p) for p in plains[:k]) for k in range(7)]
    mid = (off[3] + 100, 5000)
    head1 = _edit(z, fr[1].block_at, lambda x: x | 6)
    trunc = z[:len(z) - 100]
    entries = [z, head1, trunc, trunc, z, z, z]
    rgs = [mid, mid, (off[5] + 7, 100), (off[0] + 7, 100), (off[3] - 1, 2), (off[6] + 5, 9), (off[1] - 3, len(plains[1]) + 6)]
    a, res, seeks, exps = run_and_check(c, None, rgs, entries=entries, hash_max=ALL)
    assert [r.status == 0 for r in res] == [True, False, False, True, True, True, True]
    for i, (e, rg, r, (st, d)) in enumerate(zip(entries, rgs, res, exps)):
        if st == 0 and d:
            taken = select(e, *rg)[4]
            first = _decode(e[taken[0].begin:taken[0].end])[1]
            assert all(f.desc & 4 for f in taken)
            assert (r.nframes, r.checksums, r.checksum_mismatches, r.checksums_unverified) == (len(taken), len(taken), 0, 0), (i, r)
            assert r.checksum_from_data == r.calculated_checksum == xxh32(first), (i, r)
    return [full_key(r) for r in res], [k.key() for k in seeks], _bytes_of(a)


def _seek_table_verified(c):
    """the seek-table call with verify_table=True (tests/test_gpu_seek_table_verify.py): its ranks scenario (too small, a false size, a false
    Content_Checksum, a reserved block, a false row) with a table that vouches beside them, and selections of 65 rows, a good one and
    one whose last row is false"""
    import zgpu
    from devmem import full_key, xxh32
    from test_gpu_decode_ranges import _edit
    from test_gpu_seek_table_verify import BAD, _edge, checked_frame, payload, run, table
    plains = [payload(k, 20) for k in range(6)]
    frames = [checked_frame(p) for p in plains]
    rg = (25, 70)                                                   # frames 1 .. 4
    good, flipped = table(frames, plains), table(frames, plains, flip=(2,))
    ends = [sum(len(f) for f in frames[:k + 1]) for k in range(6)]
    false_size = table(frames, plains, flip=(2,), lie=lambda cs, ds: ds.__setitem__(3, ds[3] + 1))
    bad_content = _edit(flipped, ends[3] - 1, lambda x: x ^ 0x40)
    reserved = _edit(flipped, ends[0] + 6, lambda x: x | 6)
    a, res, exps = run(c, [flipped, false_size, bad_content, reserved, flipped, good], [rg] * 6, caps=[69, 70, 70, 70, 70, 75], verify=True)
    assert [r.status for r in res] == [zgpu.E_TARGET_TOO_SMALL, zgpu.E_CONTENT_SIZE_MISMATCH, zgpu.E_CHECKSUM_MISMATCH, zgpu.E_RESERVED_BLOCK, BAD, 0]
    assert (res[4].checksums, res[4].checksum_mismatches) == (4, 1)
    assert (res[5].written, res[5].nframes, res[5].checksums, res[5].checksum_mismatches, res[5].checksums_unverified) == (70, 4, 4, 0, 0), res[5]
    assert res[5].checksum_from_data == res[5].calculated_checksum == xxh32(plains[1]), res[5]
    edges = [_edge(65, 1), _edge(65, 2, flip=(64,))]
    a2, res2, _ = run(c, [e[0] for e in edges], [e[2] for e in edges], shifts=[e[1] for e in edges])
    assert [r.status for r in res2] == [0, BAD]
    return [full_key(r) for r in res], _bytes_of(a), [full_key(r) for r in res2], _bytes_of(a2)


def _gather_ranges(c):
    """gather_ranges (tests/test_gpu_gather_ranges.py): many ranges that share frames, every frame with a Content_Checksum and hashed; then
    verify_table on a table whose row 5 is false"""
    import zgpu
    from devmem import ALL, full_key, xxh32
    from test_gpu_gather_ranges import _eight_frames, run_gather
    from test_gpu_seek_table import seekable
    size = 4096
    frames, plains = _once("eight_checked", lambda: _eight_frames(checksum=True))
    z = seekable(frames, [size] * 8)
    ranges = [(0, 2 * size + 61 * k, 60) for k in range(16)] + [(0, 5 * size - 10, 20), (0, 5 * size - 3, 6), (0, 7 * size - 1, 2), (0, 8 * size, 3)]
    a, res, seeks, exps, grps, group_of = run_gather(c, [z], ranges, hash_max=ALL)
    assert [(g[1], g[2]) for g in grps] == [(2, 2), (4, 5), (6, 7)] and all(r.status == 0 for r in res)
    for j, r in enumerate(res):
        if group_of[j] is not None:
            _, first, last, _ = grps[group_of[j]]
            assert (r.checksums, r.checksum_mismatches, r.checksums_unverified) == (last - first + 1, 0, 0), (j, r)
            assert r.checksum_from_data == r.calculated_checksum == xxh32(plains[first]), (j, r)
    frames2, plains2 = _once("eight_2000", lambda: _eight_frames(size=2000))
    bad = zgpu.E_SEEK_CHECKSUM_MISMATCH
    z2 = seekable(frames2, [2000] * 8, checksums=[xxh32(p) ^ (0x100 if k == 5 else 0) for k, p in enumerate(plains2)])
    ranges2 = [(0, 5 * 2000 + 5, 10), (0, 5 * 2000 - 1, 2), (0, 4 * 2000 + 7, 3), (0, 6 * 2000, 2000), (0, 100, 3000), (0, 5 * 2000 + 800, 10)]
    a2, res2, seeks2, _, _, _ = run_gather(c, [z2], ranges2, caps=[10, 2, 3, 2000, 3000, 9], group_status=lambda e, a, b: bad if a <= 5 <= b else 0, verify_table=True)
    assert [r.status for r in res2] == [bad, bad, bad, 0, 0, zgpu.E_TARGET_TOO_SMALL]
    assert (res2[0].nframes, res2[0].checksums, res2[0].checksum_mismatches, res2[0].checksums_unverified) == (0, 2, 1, 0)
    return ([full_key(r) for r in res], [k.key() for k in seeks], _bytes_of(a), [full_key(r) for r in res2], [k.key() for k in seeks2], _bytes_of(a2))


def _seek_index(c):
    """seek_index_create (a declared-kind handle over eight sized frames between skippable ones) and an indexed gather; then
    seek_index_measured, the hash pass and gathers under verify_table on tests/test_gpu_seek_index_sums.py's entries: the sums are the
    model's, the handle vouches for the declared and the measured entry"""
    import zgpu
    from devmem import ALL, Sources, full_key
    from test_gpu_seek_index import _eight_declared, run_indexed, with_skippables
    from test_gpu_seek_index_sums import DECL, MEAS, Entries, _ranges, gather_both, sums_of
    size = 4096
    sized, plains = _once("eight_declared", lambda: _eight_declared(checksum=True))
    whole = b"".join(plains)
    za = with_skippables(sized)
    sa = Sources([za], [5])
    ranges = [(0, 2 * size + 61 * k, 60) for k in range(8)] + [(0, 5 * size - 10, 20), (0, 7 * size - 1, 2), (0, 8 * size - 1, 5), (0, 0, 0), (0, size, 1)]
    with c.seek_index(sa.ptrs, sa.lens, kind="declared") as ix:
        info = ix.infos[0]
        assert (info.status, info.kind, info.nrows, info.len, info.compressed, info.plaintext) == (0, zgpu.INDEX_DECLARED, 11, len(za), len(za), 8 * size)
        a, res, seeks, exps, grps = run_indexed(c, ix, sa, [za], ranges, hash_max=ALL)
    assert all(r.status == 0 and r.checksum_mismatches == 0 for r in res) and [d for _, d in exps] == [whole[b:b + n] for _, b, n in ranges]
    out = [[full_key(r) for r in res], [k.key() for k in seeks], _bytes_of(a)]
    ents = _once("index_entries", Entries)
    s = Sources(ents.all, [1, 2, 3, 0, 0, 5])
    with ents.index(c, s) as ix:
        ix.hash(s.ptrs, s.lens, which=[0, 1, 1, 1, 1, 0])
        assert [i.state for i in ix.sums_infos] == [0, 1, 1, 0, 1, 0]
        for e in (DECL, MEAS):
            sh = ents.shards[e]
            assert ix.sums(e) == sums_of(sh), e
            out.append(ix.sums(e))
            for rgs in (_ranges(e, sh), [(e, 0, sh.D[-1])]):
                res, st, grps = gather_both(c, ix, s, sh, rgs)
                assert all(r.status == 0 and r.checksums_unverified == 0 and r.checksum_mismatches == 0 for r in res), e
                assert st["entries_failed_table"] == 0 and st["frames_compared"] == st["frames_decoded"] > 0, (e, st)
                out.append([full_key(r) for r in res])
    assert s.unchanged()
    return out


def _shared_dicts(c):
    """the dictframes cases through zgpu_set_frames_shared_dicts (tests/test_gpu_frames_shared_dicts.py: the hand-built frames at the edges
    of the reach, and corpus frames whose first block takes its tables from the dictionary) in the three decode_frames calls: every
    result field and destination byte is the oracle's with the dictionary registered, and no entry leaves the shared submit"""
    from devmem import entry_key
    from golden_io import read_manifest, read_pack
    from test_gpu_frames_shared_dicts import _three_calls, reach_cases

    def corpus():
        pack, man = read_pack("dict_tests.pack"), read_manifest("dict_tests.json")
        names = sorted(n for n in man if n != "dictionary")
        return pack["dictionary"], [pack[n] for n in names], [man[n]["size"] for n in names]
    raw, _, _ = cp = _once("dict_corpus", corpus)
    built, items, wants = _once("reach_cases", lambda: reach_cases(cp))
    assert len(built) == 10 and len(items) == 18
    c.add_dict(raw)
    c.set_frames_shared_dicts(True)
    caps, n = [cap for _, cap in items], len(items)
    stats = _three_calls(c, wants, caps, shifts=[1] * n, src_shifts=[15] * n)
    for call, (ds, submits, dev, src) in stats.items():
        assert submits == 1 and ds["entries_alone"] == 0 and ds["frames_shared"] > 0 and ds["fill_launches"] > 0, (call, ds)
    res = c.decode_frames([w.entry for w in wants], caps)
    return [entry_key(r) for r in res], [r.data for r in res]


SURFACES = {
    "decode_frames_device": _decode_frames_device,
    "decode_ranges_device_src": _decode_ranges,
    "seek_table_verify_table": _seek_table_verified,
    "gather_ranges": _gather_ranges,
    "seek_index": _seek_index,
    "shared_dicts": _shared_dicts,
}


@pytest.mark.parametrize("surface", list(SURFACES))
def test_device_resident_surface_under_every_poison(surface, monkeypatch):
    """one scenario per surface on a fresh context per value: against the models and the oracle inside the scenario, and every part of
    what it returns (result keys with the checksum fields, seek records, sums, the destinations' bytes) identical across the values"""
    runs = []
    for p in POISONS:
        with poisoned_context(monkeypatch, p) as c:
            runs.append((p, SURFACES[surface](c)))
            assert c.tuning()["poisoned_bytes"] > 0
    p0, first = runs[0]
    for p, other in runs[1:]:
        assert len(other) == len(first)
        for part, (x, y) in enumerate(zip(first, other)):
            assert x == y, "%s: part %d of the results differs between poison 0x%02X and 0x%02X" % (surface, part, p0, p)


def test_the_fill_reaches_memory(monkeypatch):
    """the hook itself: a submit fills more than nothing and at least the capacity of its scratch buffers; and the flatten scratch of a
    frame whose only unit is direct — Batch.scratch_words, words no kernel of the submit writes — reads back as the value, under two"""
    import emu
    name, z, plain = next(f for f in seqframes.family("seq_counts") if [u[3] for u in emu.Plan(f[1]).units] == [2])
    for poison in (0xA5, 0x3C):
        with poisoned_context(monkeypatch, poison) as c:
            b = c.prepare(z)
            try:
                b.run()
                b.sync()
                assert b.frame_bytes(0) == plain
                t = c.tuning()
                assert t["poisoned_bytes"] > 0 and t["scratch_cap_bytes"] > 0 and t["poisoned_bytes"] >= t["scratch_cap_bytes"], t
                words = b.scratch_words(0, len(plain))
                assert (words == 0x01010101 * poison).all(), (poison, hex(int(words[0])))
            finally:
                b.close()
    monkeypatch.delenv("ZGPU_POISON")
    with framesuite.dev_context(monkeypatch, {}) as c:       # the switch unset: nothing is filled
        assert c.tuning()["poison"] == -1
        assert framesuite.frame_alone(c, z)[3] == plain and c.tuning()["poisoned_bytes"] == 0


def test_product_build_after_a_dirtying_submit():
    """libzgpu.so, no switch, one fresh context: a submit that leaves every arena larger and fuller than any family needs (all valid seqframes
    and sweepframes frames, 4 MiB of text, a frame of 0xFF bytes with Huffman literals), the families in reverse order, the dirtying
    submit again, the families in forward order: framesuite.submit with the oracle's records, every invalid frame alone and among valid
    ones in shared submits (_verdict_submits). Every result is the oracle's"""
    import zgdata
    import zgpu
    dirty = [f[1:] for f in seqframes.valid_frames() + sweepframes.valid_frames()]
    text = zgdata.text_like(4 << 20, seed=4)
    dirty.append(("text_4m", zgdata.zstd_compress(text), text))
    ff = next(f for f in blockframes.family("lit_sizes") if f[0].startswith("lit_sizes_lit_huf"))
    ones = bytes([0xFF]) * (1 << 17) + bytes(range(256)) * 4
    dirty.append(("ff_huf", zgdata.zstd_compress(ones), ones))
    dirty.append(ff)
    c = zgpu.Context(0)
    try:
        for order in (ORDER[::-1], ORDER):
            framesuite.submit(c, dirty)
            for gen in order:
                mod, status, _ = GENS[gen]
                valid, invalid = _frames(mod)
                for frames in _submits(gen, valid):
                    framesuite.submit(c, frames, _oblocks(gen))
                want, alone = _oracle(gen), {}
                for _, name, z, _ in invalid:
                    v = framesuite.frame_alone(c, z)
                    alone[name] = _key(v) + (v[4],)
                wrong = [name for name, v in alone.items() if _judged(v[:4]) != _judged(want[name])]
                assert not wrong, (gen, wrong[:10])
                _verdict_submits(c, gen, valid, invalid, alone)     # ... and among valid frames in one submit
    finally:
        c.close()
