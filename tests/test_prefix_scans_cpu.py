"""The wave scan the kernels do on DPP (zx_scan_src / zx_scan_takes / zx_scan_incl_add / zx_shr1 and zg_map_scan_incl in
zg_kernels.hip: zg_k_seqpost, zg_k_scan), as a host model: four shifts inside the rows of 16 lanes (row_shr:1/2/4/8), then lane 15
of rows 0 and 2 to all of rows 1 and 3 (row_bcast:15, row mask 0xA), then lane 31 to all of rows 2 and 3 (row_bcast:31, row mask
0xC); a lane whose step has no source lane, or whose row the mask leaves out, keeps `old` (bound_ctrl off), which the kernels set
to the operation's identity. The model is the DPP rule itself, lane by lane; the row boundaries are where such a scan goes wrong,
so all the weight is put on lanes 15, 16, 31, 32, 47, 48 and 63 in turn. The sum is compared with a plain prefix sum mod 2^32, the
composition of history maps (zg_map_compose of zg_dev.h through the CPU harness: it does not commute) with a left fold. The kernels
themselves meet the same seams in tests/test_gpu_prefix_edges.py."""
import random
import re

import emu
import repframes

M32 = 0xFFFFFFFF
STEPS = 6
EDGE_LANES = (15, 16, 31, 32, 47, 48, 63)
IDENT = [1 << 30, 2 << 30, 3 << 30]


def dpp(v, ctrl, row_mask, old):
    """v_mov_b32_dpp with bank mask 0xF and bound_ctrl off, for the controls the scan uses: what each of the 64 lanes holds
    afterwards, given v per lane and `old` per lane in the destination"""
    out = list(old)
    for lane in range(64):
        row, l = divmod(lane, 16)
        if not (row_mask >> row) & 1:
            continue
        if 0x111 <= ctrl <= 0x11F:                      # row_shr:n — inside the row only
            src = lane - (ctrl - 0x110) if l >= ctrl - 0x110 else None
        elif ctrl == 0x142:                             # row_bcast:15 — lane 15 of each row to the next row
            src = 16 * row - 1 if row else None
        elif ctrl == 0x143:                             # row_bcast:31 — lane 31 to rows 2 and 3
            src = 31 if row >= 2 else None
        elif ctrl == 0x138:                             # wave_shr:1
            src = lane - 1 if lane else None
        else:
            raise ValueError(hex(ctrl))
        if src is not None:
            out[lane] = v[src]
    return out


def _kernel_steps():
    """(ctrl, row mask) of the six steps and the lane rule of zx_scan_takes, as zg_kernels.hip states them"""
    src = open(repframes._CSRC + "/zg_kernels.hip").read()
    m = re.search(r"constexpr int ctrl = S < 4 \? (0x[0-9A-Fa-f]+) \+ \(1 << S\) : S == 4 \? (0x[0-9A-Fa-f]+) : (0x[0-9A-Fa-f]+), "
                  r"rows = S == 4 \? (0x[0-9A-Fa-f]+) : S == 5 \? (0x[0-9A-Fa-f]+) : (0x[0-9A-Fa-f]+);", src)
    assert m, "zx_scan_src has another form: tests/test_prefix_scans_cpu.py reads it"
    base, c4, c5, r4, r5, rall = (int(x, 16) for x in m.groups())
    assert "return S < 4 ? (lane & 15u) >= (1u << S) : (lane & (S == 4 ? 16u : 32u)) != 0u;" in src, "zx_scan_takes has another form"
    assert "__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xF, 0xF, false)" in src, "zx_shr1 has another form"
    return [(base + (1 << s), rall) for s in range(4)] + [(c4, r4), (c5, r5)]


KSTEPS = _kernel_steps()


def takes(step, lane):
    """zx_scan_takes<step>(lane)"""
    return (lane & 15) >= (1 << step) if step < 4 else (lane & (16 if step == 4 else 32)) != 0


def scan_src(v, step, fill):
    """zx_scan_src<step>(v, fill) on all lanes"""
    ctrl, rows = KSTEPS[step]
    return dpp(v, ctrl, rows, [fill] * 64)


def scan_add(v):
    """zx_scan_incl_add"""
    v = list(v)
    for s in range(STEPS):
        src = scan_src(v, s, 0)
        v = [(a + b) & M32 for a, b in zip(v, src)]
    return v


def scan_maps(maps):
    """zg_map_scan_incl: per component a move with the identity's word as fill, the composition where the lane takes one"""
    maps = [list(m) for m in maps]
    for s in range(STEPS):
        src = [scan_src([m[k] for m in maps], s, IDENT[k]) for k in range(3)]
        maps = [emu.map_compose([src[0][l], src[1][l], src[2][l]], maps[l]) if takes(s, l) else maps[l] for l in range(64)]
    return maps


def test_steps_are_the_scan_controls():
    """row_shr:1/2/4/8 under every row, row_bcast:15 under rows 1 and 3, row_bcast:31 under rows 2 and 3; zx_scan_takes names exactly
    the lanes a step gives a source lane to, and the lane it reads holds the run right below the lane's own"""
    assert KSTEPS == [(0x111, 0xF), (0x112, 0xF), (0x114, 0xF), (0x118, 0xF), (0x142, 0xA), (0x143, 0xC)]
    lo = list(range(64))                                # lane l holds the run [lo[l], l]
    for s in range(STEPS):
        got = scan_src(list(range(64)), s, -1)
        assert [g != -1 for g in got] == [takes(s, l) for l in range(64)], s
        for l in range(64):
            if takes(s, l):
                assert got[l] == lo[l] - 1, (s, l)      # the source lane is the top of the run that ends right below this lane's
        lo = [lo[got[l]] if takes(s, l) else lo[l] for l in range(64)]
    assert lo == [0] * 64


def test_sum_scan_random_and_row_edges():
    rng = random.Random(1)
    cases = [[rng.randrange(1 << 32) for _ in range(64)] for _ in range(300)]
    cases += [[rng.randrange(4) for _ in range(64)] for _ in range(100)]
    cases += [[1] * 64, [M32] * 64, [0] * 64, list(range(64))]
    for lane in EDGE_LANES + (0, 1, 14, 17, 30, 33, 62):
        for w in (1, 0x80000000, M32, 12345):
            cases.append([w if l == lane else 0 for l in range(64)])          # all the weight in one lane
            cases.append([0 if l == lane else w for l in range(64)])          # ... and in every other one
    for a in EDGE_LANES:
        for b in EDGE_LANES:
            cases.append([(7 if l == a else 0) + (1 << 20 if l == b else 0) for l in range(64)])
    for v in cases:
        want, acc = [], 0
        for x in v:
            acc = (acc + x) & M32
            want.append(acc)
        assert scan_add(v) == want, v


def test_shift_by_one():
    """zx_shr1: wave_shr:1 crosses the rows; lane 0 keeps the fill"""
    v = [100 + l for l in range(64)]
    assert dpp(v, 0x138, 0xF, [7] * 64) == [7] + v[:63]


# maps that do not commute: swaps, rotations, a new offset, "slot 0 minus one" (the effect of a sequence on the history)
def _elementary(rng):
    kind = rng.randrange(6)
    if kind == 0:
        return [2 << 30, 1 << 30, 3 << 30]              # repeat code 2: slots 0 and 1 swap
    if kind == 1:
        return [3 << 30, 1 << 30, 2 << 30]              # repeat code 3
    if kind == 2:
        return [rng.randint(1, 1 << 20), 1 << 30, 2 << 30]      # a new offset
    if kind == 3:
        return [(1 << 30) | 1, 1 << 30, 2 << 30]        # slot 0 minus one
    if kind == 4:
        return [(1 << 30) | rng.randint(2, 3000), 1 << 30, 2 << 30]
    return list(IDENT)


def _lane_map(rng, n):
    m = list(IDENT)
    for _ in range(n):
        m = emu.map_compose(m, _elementary(rng))
    return m


def _left_fold(maps):
    out, acc = [], list(IDENT)
    for m in maps:
        acc = emu.map_compose(acc, m)
        out.append(acc)
    return out


def test_map_scan_random_and_row_edges():
    """the composition scan against a left fold: random maps in every lane; the identity everywhere but on one or two of the lanes
    next to a row boundary; symbolic maps only (no constant ever hides the order); the resolved histories agree as well"""
    rng = random.Random(2)
    cases = [[_lane_map(rng, rng.randint(0, 8)) for _ in range(64)] for _ in range(60)]
    sym = lambda: rng.choice(([2 << 30, 1 << 30, 3 << 30], [3 << 30, 1 << 30, 2 << 30], [(1 << 30) | 1, 1 << 30, 2 << 30]))
    cases += [[sym() for _ in range(64)] for _ in range(40)]
    for a in EDGE_LANES:
        cases.append([_lane_map(rng, 5) if l == a else list(IDENT) for l in range(64)])
        for b in EDGE_LANES:
            if a < b:                                    # two maps that do not commute on either side of (or across) a boundary
                cases.append([[3 << 30, 1 << 30, 2 << 30] if l == a else [77, 1 << 30, 2 << 30] if l == b else list(IDENT) for l in range(64)])
                cases.append([[77, 1 << 30, 2 << 30] if l == a else [3 << 30, 1 << 30, 2 << 30] if l == b else list(IDENT) for l in range(64)])
    differ = 0
    for maps in cases:
        want = _left_fold(maps)
        assert scan_maps(maps) == want
        hist = [rng.randint(4000, 1 << 20) for _ in range(3)]
        assert [[emu.sym_resolve(w, hist) for w in m] for m in scan_maps(maps)] == [[emu.sym_resolve(w, hist) for w in m] for m in want]
        differ += _left_fold(maps[::-1])[-1] != want[-1]
    assert differ >= len(cases) // 2                    # the order mattered in most cases
    # the exclusive map of a lane: the inclusive one of the lane below, the identity in lane 0
    incl = scan_maps(cases[0])
    ex = list(zip(*[dpp([m[k] for m in incl], 0x138, 0xF, [IDENT[k]] * 64) for k in range(3)]))
    assert [list(e) for e in ex] == [list(IDENT)] + incl[:63]
