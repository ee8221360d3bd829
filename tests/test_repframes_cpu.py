"""Frames built from chosen repeat codes (tests/repframes.py) through the CPU harness, and the map algebra of the symbolic offset
history on the host. The harness decodes with a serial history (zg_hist_step, block after block), so the frames pin themselves,
the serial lane logic and zg_exact.h's use of zg_sym_resolve here; ZgHistMap / zg_map_apply / zg_map_compose (zg_dev.h), which
only the kernels' scans call, are proven by test_map_algebra: every bracketing of compose over random code strings must resolve
to what zg_hist_step gives serially, and that to RFC 8878's rule in plain Python. The scans themselves (zg_k_seqpost, zg_k_scan)
run on the same frames in tests/test_gpu_repframes.py.

zg_exact.h on the SIMT emulator takes 3.5 ms per block: the valid frames of more than 1025 blocks (scan_8191 .. scan_16385) go
through the harness's decode and blockcheck only, without e.exact()."""
import random
import re

import pytest

import blockcheck
import emu
import framesuite
import repframes
from repframes import META, STATUS

FAMS = sorted(repframes.FAMILIES)
OFF_HUGE = int(re.search(r"#define ZG_OFF_HUGE (0x[0-9A-Fa-f]+)u", open(repframes._CSRC + "/zg_dev.h").read()).group(1), 16)
KMAX = 0x3FFFFFFF


@pytest.mark.parametrize("fam", FAMS)
def test_family_matches_plaintext_and_oracle(fam):
    """frame bytes == plaintext; per block the sequences and the history at its start == the oracle's == the Python model's; an
    invalid frame gets the oracle's status, and what the harness produced in front of the failing block is the model's"""
    for name, z, plain in repframes.family(fam):
        m = META[name]
        if plain is None:
            framesuite.check_on_harness(name, z, None, STATUS)
            e = emu.EmuBatch(z, max_window=1 << 31)
            out, st = e.frame_bytes(0)
            assert st and e.frame(0)[3] == m["bad_block"], (name, st, e.frame(0))      # (the verdict is zg_exact.h's, above: the harness's serial executor only stops there)
            assert out[:len(repframes.GOOD[name])] == repframes.GOOD[name], name
            continue
        e = emu.EmuBatch(z, max_window=1 << 31)
        assert e.parse_status == 0 and e.nframes == 1, name
        out, st = e.frame_bytes(0)
        assert st == 0 and out == plain, name
        ob = blockcheck.oracle_blocks(z)
        assert e.nblocks == len(ob) == m["nblocks"], name
        assert [r["hist_after"] for r in ob] == m["hist_at"][1:] + [m["hist_end"]], (name, "the model's history differs from the oracle's")
        blockcheck.check_frame(e, 0, ob, name)
        if m["nblocks"] <= repframes.SCAN_LIMITS[1] + 1:
            ex = e.exact(drain_rule=1)
            assert ex[0][0] == 0, (name, ex)


def test_coverage():
    """what the families reach, from the Python model, with no frame skipped: every (index mod S, repeat code) pair; a sequence that
    repeats what the one, two and three in front of it put into slot 0 across a thread, a wave and a pass boundary; k up to
    PASS + 1 on every tag at a block end; block maps of 0 .. 3 symbolic slots and all six permutations; the scan's sizes; a
    history-dependent first sequence in every block at and next to the scan's edges; the invalid frames' places and statuses"""
    frames = repframes.all_frames()
    cov = repframes.coverage(frames)
    print("\ncoverage:", {k: (sorted(v) if isinstance(v, set) else v) for k, v in cov.items()})
    S, PASS, CHUNK = repframes.S, repframes.PASS, repframes.CHUNK
    assert cov["valid"] + cov["invalid"] == len(frames) and cov["valid"] >= 130 and cov["invalid"] >= 17
    assert cov["pairs"] == {(i, c) for i in range(S) for c in (1, 2, 3, 4)}
    assert cov["deps"] >= {(kind, d) for kind in ("thread", "wave", "pass") for d in (1, 2, 3)}
    assert all(cov["max_k"][t] >= PASS + 1 for t in (1, 2, 3)), cov["max_k"]
    assert all(cov["run_k"][t] >= set(repframes.CHAIN) for t in (1, 2, 3)), cov["run_k"]     # a block map with "slot t minus n" for every run length n (tag 1: in slot 0)
    assert cov["shapes"] == {0, 1, 2, 3} and len(cov["permutations"]) == 6
    assert cov["nblocks"] == set(repframes.NBLOCKS) and max(cov["nblocks"]) > 2 * CHUNK
    assert cov["edges_missing"] == [] and cov["edges_open"] > 3 * (2 * CHUNK // repframes.SCAN_I)
    assert cov["bad_blocks"] >= set(repframes.BAD_AT) | {0}
    assert cov["statuses"] == {51, 53}                   # ZG_EXE_ZERO_OFFSET, ZG_EXE_OFFSET_TOO_BIG: whatever the oracle said (tabframes.STATUS)
    for fam in ("perm_blocks", "dec_chains", "mixed_maps", "initial_history"):
        assert cov["of_modes"][fam] - {"pre"}, fam      # a variant with an RLE or FSE offset table in every family
    assert not repframes.LIBZSTD_DIFFERS


def _ref(h, ll, ov):
    """RFC 8878 3.1.1.5 with the reference's saturating "minus one" (an offset of 0 is refused later, by the executor)"""
    d, h = repframes.step(h, ll, ov)
    if d < 0:
        d, h = 0, [0] + h[1:]
    return d, h


HISTS = ([1, 4, 8], [1, 1, 1], [5, 5, 5], [2, 1, 3], [3, 2, 1], [1, 2, 2], [OFF_HUGE, 4, 8], [7, OFF_HUGE, OFF_HUGE - 1], [OFF_HUGE] * 3)


def test_map_algebra():
    """24000 seeded strings of (LL zero or not, offset_value) over initial histories that include 1 / 4 / 8, equal slots, values near
    1 and ZG_OFF_HUGE: zg_hist_step on concrete slots equals the RFC rule after every sequence, and the per-sequence maps composed
    as a left fold, a right fold and random trees (leaves of one sequence, and of up to 8 stepped directly, as a thread of
    zg_k_seqpost does) resolve with zg_sym_resolve to the same history and the same actual offset, for every prefix"""
    rng = random.Random(20261)
    total = 0
    for it in range(24000):
        hist = list(HISTS[it % len(HISTS)]) if it % 3 else [rng.choice((1, 2, 3, rng.randint(1, 40), rng.randint(1, KMAX))) for _ in range(3)]
        n = rng.choice((1, 2, 3, 5, 8, 9, 13, 17, 24, 33))
        mode = it % 4                                    # 0: repeat codes only, 1: mostly "minus one", else mixed with new offsets
        codes = []
        for _ in range(n):
            ll = rng.choice((0, 0, 1, 2))
            r = rng.random()
            if mode == 0 or r < 0.7:
                ov = 3 if mode == 1 and rng.random() < 0.8 else rng.randint(1, 3)
                ll = 0 if mode == 1 and ov == 3 and rng.random() < 0.9 else ll
            else:
                ov = 3 + rng.choice((1, 1, 2, 3, rng.randint(1, 60), rng.randint(1, KMAX - 4), OFF_HUGE))
            codes.append((ll, ov))
        serial, fail, which = emu.map_fold(codes, hist, seed=it, ntrees=4)
        assert fail == 0, (it, hist, codes, "prefix %d, bracketing %d" % (fail - 1, which))
        h = list(hist)
        for i, (ll, ov) in enumerate(codes):
            d, h = _ref(h, ll, ov)
            assert serial[i] == (d, h[0], h[1], h[2]), (it, i, hist, codes, serial[i], d, h)
        total += n
    assert total >= 200000


def _model(m, hist):
    """the history behind a map given as [(tag, k)], as integers of any size"""
    return [max((v if t == 0 else hist[t - 1] - v), 0) for t, v in m]


def _words(m):
    return [(t << 30) | v for t, v in m]


def test_map_saturation():
    """k saturates at 0x3FFFFFFF in zg_map_apply: no history value is larger, so a saturated slot resolves to 0 like the true sum.
    Maps with k around the limit composed in both bracketings against integer arithmetic"""
    rng = random.Random(7)
    ks = (0, 1, 2, KMAX - 1, KMAX, KMAX // 2, KMAX // 2 + 1)

    def rand_map():
        return [(t, rng.choice(ks + (rng.randint(0, KMAX),))) if t else (0, rng.choice((0, 1, 5, KMAX, rng.randint(0, KMAX)))) for t in (rng.randint(0, 3) for _ in range(3))]

    def comp_model(a, b):                                # apply a, then b, on exact integers; constants clamp at 0 as they are made
        out = []
        for t, v in b:
            if t == 0:
                out.append((0, v))
            else:
                ta, va = a[t - 1]
                out.append((0, max(va - v, 0)) if ta == 0 else (ta, va + v))
        return out

    sat = 0
    for it in range(6000):
        a, b, c = rand_map(), rand_map(), rand_map()
        hist = [rng.choice((1, 4, 8, KMAX, rng.randint(1, KMAX))) for _ in range(3)]
        ab, bc = emu.map_compose(_words(a), _words(b)), emu.map_compose(_words(b), _words(c))
        want_ab = _model(comp_model(a, b), hist)
        assert [emu.sym_resolve(w, hist) for w in ab] == want_ab, (a, b, hist)
        want = _model(comp_model(comp_model(a, b), c), hist)
        left, right = emu.map_compose(ab, _words(c)), emu.map_compose(_words(a), bc)
        assert [emu.sym_resolve(w, hist) for w in left] == want == [emu.sym_resolve(w, hist) for w in right], (a, b, c, hist)
        sat += any(w >> 30 and (w & KMAX) == KMAX and t and ta and va + v > KMAX for w, (t, v), (ta, va) in zip(ab, b, (a[t - 1] if t else (0, 0) for t, _ in b)))
    assert sat >= 500                                    # the saturating branch was taken
    assert emu.map_compose([(1 << 30) | KMAX, 2 << 30, 3 << 30], [(1 << 30) | 1, (1 << 30) | KMAX, 2 << 30]) == [(1 << 30) | KMAX, (1 << 30) | KMAX, 2 << 30]
