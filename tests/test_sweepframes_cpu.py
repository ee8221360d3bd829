"""Frames built at the edges of zg_k_sweep (tests/sweepframes.py) without a GPU: that they are what they are meant to be. The CPU
harness has no sweep (a plain serial model resolves the scratch, tests/emu/zg_emu_flat.cpp), so what is proven here is the aim:
every frame decodes to its plaintext on the harness and agrees block by block with the oracle; the harness's plan (the same
BatchBuilder::finish, flat_slots 256) cuts every frame and submit into the units the generator laid out; and from
lz_model.expected_scratch on that plan the group keys, shifts, unit sizes, head sizes and aimed matches are the ones the families
name. tests/test_gpu_sweepframes.py runs the kernel on the same frames and fails if the GPU's plan is another one."""
import numpy as np
import pytest

import framesuite
import lz_model
import sweepframes as S
import test_flat1_cpu

BATCH = S.BATCH


@pytest.fixture(scope="module")
def covs():
    """sweepframes.coverage of every submit, and of the big frame alone, each computed once"""
    out = {name: S.coverage(frames) for name, (_, frames) in S.submits().items()}
    out["head_groups_big"] = S.coverage([S.head_groups_big()])
    return out


@pytest.mark.parametrize("fam", list(S.FAMILIES))
def test_family_matches_plaintext_and_oracle(fam):
    for name, z, plain in S.family(fam):
        framesuite.check_on_harness(name, z, plain, {})


def test_big_frame_matches_plaintext_and_oracle():
    framesuite.check_on_harness(*S.head_groups_big(), {})


@pytest.mark.parametrize("fam", S.SMALL_FAMILIES)
def test_flatten_scratch(fam):
    """zg_flat1.h on the emulator with the product's plan (unit_blocks 0): the scratch words of every pointer-mode unit are the
    model's, so a scratch error cannot pass as a sweep error on the GPU. groups_far has 1 MiB of Raw blocks and one unit: the
    emulator's time goes to other frames"""
    n = sum(test_flat1_cpu.check_scratch(z, 0, 0) for name, z, _ in S.family(fam) if name != "groups_far")
    assert n >= len(S.family(fam))


def _split_expected(frames):
    """the model of zg_launch_sweep's choice and of Batch::sync's repeat: 1 if the submit has more than one step and window_max / batch
    + 2 batches + 65536 bytes stay below the bytes of a unit of the plan's blocks, 2 if an offset then exceeds its frame's window"""
    _, plan = S.plan_of(frames)
    ub = max(S.UB, max(u[2] for u in plan.units))
    wmax = max(S.LAYOUT[n]["window"] if n in S.LAYOUT else 1 << 17 for n, _, _ in frames)
    split = len(plan.steps) > 1 and (wmax // BATCH + 2) * BATCH + 65536 < ub * 131072
    if not split:
        return 0
    beyond = any(d > S.LAYOUT[n]["window"] for n, _, _ in frames if n in S.LAYOUT for _, _, d in S.LAYOUT[n]["aims"])
    return 2 if beyond else 1


def test_plans(covs):
    """every frame and submit: the plan's units are the generator's (four blocks each; the first unit direct while the frame has at
    most direct_max_units units, every unit with a sequence behind it pointer-mode, the units of Raw blocks without a step), no
    frame is sparse but mx_sparse, and the expected sweep_mode() follows from zg_launch_sweep's condition"""
    c = S.constants()
    assert (BATCH, S.UB, c["sparse_max"], c["sparse_per_block"], c["direct_max_units"], c["group"], c["events"]) == (2048, 4, 2048, 4, 32, 16, 80)
    subs = dict(S.submits())
    subs["head_groups_big"] = (1, [S.head_groups_big()])
    for sname, (mode, frames) in subs.items():
        cov = covs[sname]
        assert _split_expected(frames) == mode, sname
        assert cov["sparse"] == [n for n, _, _ in frames if n == "mx_sparse"], sname
        for name, z, plain in frames:
            if name not in S.LAYOUT:
                continue
            fc = cov["frames"][name]
            lay = S.LAYOUT[name]["units"]
            assert [(a, b - a) for a, b in zip(fc["bounds"], fc["bounds"][1:])] == [(s, n) for s, n, _ in lay], (sname, name)
            direct = 2 if len(lay) <= c["direct_max_units"] else 0
            assert [u[1:] for u in fc["units"]] == [(S.UB, {"first": direct, "ptr": 0, "noseq": 1}[k]) for _, _, k in lay], (sname, name)
    print("\nsteps per submit:", {k: v["steps"] for k, v in covs.items()})


def test_coverage(covs):
    """what the families reach, asserted exactly"""
    show = lambda d: {k: sorted(v) for k, v in d.items()}   # noqa: E731
    g = covs["groups"]
    print("\ngroups: keys per lowb", {r: len(v) for r, v in g["keys"].items()}, sorted(g["keys"][0]))
    print("impossible (a run of one or two match bytes between literals, Match_Length >= 3):", sorted(S.IMPOSSIBLE))
    print("shifts per load:", show(g["shifts"]), "small e:", sorted(v for v in g["e"] if v <= 5), "groups_far e_max:", covs["groups_far"]["e_max"])
    for r in range(4):
        assert g["keys"][r] == S.KEYS, (r, sorted(S.KEYS - g["keys"][r]), sorted(g["keys"][r] - S.KEYS))
    for load in "ABCD":
        assert g["shifts"][load] == {0, 1, 2, 3}, load
    assert {0, 1, 2, 3, 4, 5} <= g["e"]
    assert covs["groups_far"]["e_max"] > 1 << 20
    for name, cov in covs.items():                       # no frame anywhere holds a key called impossible
        for r in range(4):
            assert not cov["keys"][r] & S.IMPOSSIBLE, name

    u = covs["unit_ends"]
    print("unit_ends: sizes", sorted(u["sizes"]), "byte tails", sorted(u["tail_sizes"]))
    behind = {37, 40}                                    # the units behind: 37 bytes, and 3 more where they copy the last three
    assert u["sizes"] == {n for n in S.SMALL_SIZES if n >= 3} | set(S.BIG_SIZES) | behind
    assert u["tail_sizes"] == {1, 2, 3}
    seen = set()
    for name, fc in u["frames"].items():
        n, end = int(name.split("_")[1]), name.split("_")[2]
        sizes = [b - a for a, b in zip(fc["bounds"], fc["bounds"][1:])]
        assert sizes[1] == n and sizes[-1] == n and len(sizes) == 4, name      # in the middle, and the frame's last unit
        assert [x[2] for x in fc["units"]] == ([2, 0, 0, 0] if n >= 3 else [2, 1, 0, 1]), name
        seen.add((n, end))
        e = fc["e"]
        for at in (fc["bounds"][2], fc["bounds"][4]):    # the unit's last byte
            if end == "lit" or n < 3:
                assert e[at - 1] == 0, name
            elif end == "front":
                assert e[at - 1] > n - 1, name
            else:
                assert 0 < e[at - 1] <= n - 1 and e[at - 1 - e[at - 1]] == 0, name
        if n >= 3:                                       # the unit behind starts at the end of this one and copies its last three bytes
            assert list(e[fc["bounds"][2]:fc["bounds"][2] + 3]) == [3, 3, 3], name
    assert seen == {(n, end) for n in S.SMALL_SIZES + S.BIG_SIZES for end in S.ENDS if S.end_fits(n, end)}
    assert {n for n, _ in seen} == set(S.SMALL_SIZES + S.BIG_SIZES)

    t = covs["tails_heads"]
    print("tails_heads: sizes", sorted(t["sizes"]), "(s - W, head)", sorted(t["s_minus_w"]))
    assert t["sizes"] == {w + d for w in (1024, 2048) for d in S.HEAD_EDGES}
    assert t["s_minus_w"] == {(d, S.head_of(2048 + d, 2048)) for d in S.HEAD_EDGES}
    assert [h for _, h in sorted(t["s_minus_w"])] == [0, 0, 0, 0, 1, 1, 1, 2, 2]
    for name, fc in t["frames"].items():                 # the unit of 1 byte and the unit of Raw blocks: no step
        assert [x[2] for x in fc["units"]].count(1) == 2 and fc["bounds"][6] - fc["bounds"][5] == 1, name

    h = dict(covs["head_groups"]["pointer_units"])
    big = covs["head_groups_big"]
    print("head_groups: pointer-mode units", h, big["pointer_units"], "steps of the big frame", big["steps"])
    c = S.constants()
    assert sorted(h.values()) == list(S.HEAD_GROUP_UNITS) == [c["group"] - 1, c["group"], c["group"] + 1, c["group"] + 2, 2 * c["group"] + 1]
    assert covs["head_groups"]["steps"] == max(S.HEAD_GROUP_UNITS)
    assert big["pointer_units"] == {"hg_big": S.big_units()} and big["steps"] == S.big_units() > (c["events"] - 2) * c["group"]
    for cov in (covs["head_groups"], big):
        assert {hd for _, hd in cov["s_minus_w"]} >= {1}

    m = covs["mixed_counts"]["pointer_units"]
    print("mixed_counts: pointer-mode units", m, "sparse", covs["mixed_counts"]["sparse"])
    assert m == {"mx_p1": 1, "mx_p2": 2, "mx_sparse": 0, "mx_p3": 3, "mx_one_block": 0, "mx_p9": 9}
    assert covs["mixed_counts"]["steps"] == 9
    for name in ("mixed_windows", "mixed_windows_1m"):
        assert {hd for d, hd in covs[name]["s_minus_w"] if d > 0} == {1, 2}, name      # (mx_w20: far below its declared window)


def _where(fc, lay, pos, w):
    """(index of the unit that holds output position pos, "head" or "tail" by the model head = (size - W) // batch; the first unit and
    the units without a step are final before any step runs: "final")"""
    b = fc["bounds"]
    i = max(k for k in range(len(b) - 1) if b[k] <= pos)
    if lay[i][2] != "ptr":
        return i, "final"
    return i, "head" if pos - b[i] < S.head_of(b[i + 1] - b[i], w) * BATCH else "tail"


def test_aimed_matches(covs):
    """every match a family aims lies where it says and its source lands where it says, from the oracle's sequences and the model of
    sd.head: the W and W - 1 matches of tails_heads start at a unit's first byte, last head byte, first tail byte, or end at its
    last byte, and read a tail byte (or a byte that is final before the sweep), through the units of 1 and W - 1 bytes and the unit of
    Raw blocks into the unit in front of those; bw_w reads the first tail byte and bw_w1 the last head byte of the unit in front,
    both from the first byte of a head; the unit written by hand of groups reaches the last byte in front of it and the frame's
    first byte, groups_far more than 2^20 bytes back"""
    seen, through = set(), 0
    for sname in ("groups", "groups_far", "tails_heads", "head_groups", "beyond_window"):
        for name, fc in covs[sname]["frames"].items():
            info = S.LAYOUT[name]
            lay, w, e, b = info["units"], info["window"], fc["e"], fc["bounds"]
            parent, _ = lz_model.frame_parents(dict((n, z) for n, z, _ in S.submits()[sname][1])[name])
            assert info["aims"], name
            for what, pos, dist in info["aims"]:
                # the match copies from pos - dist; what the sweep reads for it is pos - e: the same place, or further back where that
                # byte is itself a match byte of the unit (e(x) = dist + e(x - dist))
                assert parent[pos] == pos - dist and e[pos] >= dist, (name, what, pos)
                ui, part = _where(fc, lay, pos, w)
                src = pos - int(e[pos])
                si, spart = _where(fc, lay, src, w)
                assert e[pos] == dist or pos - dist >= b[ui], (name, what, pos)
                rel, hd = pos - b[ui], S.head_of(b[ui + 1] - b[ui], w) * BATCH
                srel, shd = src - b[si], S.head_of(b[si + 1] - b[si], w) * BATCH
                if si == ui:                             # a fresh literal of the unit itself
                    assert e[src] == 0, (name, what)
                    spart = "final"
                assert si <= ui and src >= b[ui] - w - (what == "beyond"), (name, what)
                seen.add((sname, what, dist - w if sname != "groups" and sname != "groups_far" else 0, part, spart))
                if what == "first":
                    assert rel == 0, name
                elif what == "last":
                    assert rel + 3 == b[ui + 1] - b[ui] and part == "tail", name
                elif what == "last_head":
                    assert hd and rel == hd - 1 and part == "head", name
                elif what == "first_tail":
                    assert hd and rel == hd and part == "tail", name
                elif what == "in_front":
                    assert pos - dist == b[ui] - 1, name
                elif what == "first_byte":
                    assert pos - dist == 0, name
                elif what == "far":
                    assert dist > 1 << 20, name
                elif what == "exact":
                    assert (rel, part, srel, spart) == (0, "head", shd, "tail") and shd, name
                elif what == "beyond":
                    assert (rel, part, srel, spart) == (0, "head", shd - 1, "head") and shd and dist == w + 1, name
                if what != "beyond":
                    assert dist <= w and spart in ("tail", "final"), (name, what, spart)
                through += si < ui - 1 and what == "first"
    print("\naimed matches (submit, what, distance - W, where it lies, where its source lies):", sorted(seen))
    for dw in (0, -1):
        for what, part in (("first", "head"), ("first", "tail"), ("last", "tail"), ("last_head", "head"), ("first_tail", "tail")):
            assert ("tails_heads", what, dw, part, "tail") in seen, (what, dw, part)
    assert ("head_groups", "first", 0, "head", "tail") in seen
    assert ("beyond_window", "beyond", 1, "head", "head") in seen and ("beyond_window", "exact", 0, "head", "tail") in seen
    # behind the unit of 1 byte and the unit of Raw blocks in each of the 8 frames, behind the unit of W - 1 bytes where the distance is W
    assert through >= 8 * 2 + 4


def test_relays(covs):
    """every match byte of a relay frame takes its value from the last W bytes in front of its unit, and fresh literals are few: less
    than a tenth of any unit"""
    for sname in ("tails_heads", "head_groups", "beyond_window", "head_groups_big"):
        for name, fc in covs[sname]["frames"].items():
            lay, w, e, b = S.LAYOUT[name]["units"], 1024 if name.startswith(("hg_", "bw_")) else S.LAYOUT[name]["window"], fc["e"], fc["bounds"]
            for i, (s, n, kind) in enumerate(lay):
                if kind != "ptr":
                    continue
                ee = e[s:s + n].astype(np.int64)
                x = np.arange(n)
                m = ee != 0
                far = m & (ee - x > w + (name == "bw_w1"))
                assert not far.any(), (name, i)
                assert (~m).sum() * 10 < n, (name, i, int((~m).sum()))
