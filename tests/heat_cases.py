"""Seeded cases for the heat-map stage, shared by tests/test_heat_oracle.py (which shows through the oracle alone
that together they reach every branch) and tests/test_gpu_heat.py (which holds the device to the oracle on each).

A case is dict(name, streams, hw, kw, cap, ops).  An op is one call:
    ("update", rows[tick][stream])      ("drain",)      ("flush", stream or None)      ("reset", stream)
    ("import", stream, layer_mask, values [n, GH, GW])      ("decay", stream or None, layer_mask, shift)
Each shape is the smallest that can break: frames of 48 x 64 and 37 x 61 (partial last cells), at most 12 ticks a call, max_tracks 4."""
import numpy as np

import heat_oracle as HO

EMPTY = np.zeros((0, 6), np.int32)


def rows_array(rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def person(x, y, tid, cls=0, w=6, h=10):
    """A box whose foot anchor is pixel (x, y): fx = 2 x, fy = 2 y."""
    return [x - w // 2, y - h, x + w // 2, y, tid, cls]


def oracles_for(case):
    return [HO.HeatOracle(case["hw"], stream=s, **case["kw"]) for s in range(case["streams"])]


def run_op(oracles, op, cap):
    """One op through the oracles -> the packed outputs of an update / drain / flush, or None."""
    kind = op[0]
    if kind == "update":
        return HO.run_bank(oracles, op[1], cap)
    if kind == "drain":
        return HO.run_bank(oracles, [], cap)
    if kind == "flush":
        return HO.flush_bank(oracles, cap, op[1])
    if kind == "reset":
        oracles[op[1]].reset()
    elif kind == "import":
        oracles[op[1]].import_layers(op[2], op[3])
    elif kind == "decay":
        for s, o in enumerate(oracles):
            if op[1] is None or op[1] == s:
                o.decay(op[2], op[3])
    else:
        raise ValueError(kind)
    return None


# ---------------------------------------------------------------------------------------------------- the planted walk
WALK = ((20, 20), (26, 20), (31, 25), (31, 31), (26, 36), (20, 36), (15, 31), (15, 25), (20, 20), (20, 20), None, (21, 20))
"""Foot positions of id 1, tick by tick: E, SE, S, SW, W, NW, N, NE (back into the first cell), still, a tick away (within forget_after), then a
step of one pixel = 2 doubled pixels, below min_move = 4."""


def walk_case(hw=(48, 64), cell=8, anchor=HO.FOOT, name="walk"):
    H, W = hw
    ticks = []
    for t, p in enumerate(WALK):
        rows = []
        if p is not None:
            rows.append(person(p[0], p[1], 1))
        rows.append([10, H - 12, 16, H, 2, 1])                               # feet at y2 = H: below the picture, clamped into the last row
        rows.append([-30, 5, -1, 25, 3, 0])                                  # x2 < 0: outside, never counted
        rows.append([W, 5, W + 9, 25, 4, 0])                                 # x1 >= W: outside, never counted
        if t % 3 == 0:
            rows.append([-30, 8, 5, 30, 5, 0])                               # overlaps the left edge: x1 + x2 < 0 is clamped to 0
        if t % 4 == 1:
            rows.append([W - 3, 8, W + 40, 30, 6, 0])                        # overlaps the right edge
        if t == 5:
            rows.append(person(40, 40, 1, cls=1))                            # id 1 again in the same frame: only the first counts
        if t == 6:
            rows.append([4, -30, 12, 5, 7, 0])                               # mostly above the picture (the centre anchor is clamped to row 0)
        if t == 7:
            rows.append([5, 5, 4, 9, 8, 0])                                  # x2 < x1: not valid
            rows.append([5, 5, 9, (1 << 20) + 1, 9, 0])                      # a coordinate past 2^20: not valid
        ticks.append([rows_array(rows)])
    kw = dict(cell=cell, max_tracks=8, forget_after=2, anchor=anchor, min_move=4)
    return dict(name=f"{name}-{H}x{W}-c{cell}-a{anchor}", streams=1, hw=hw, kw=kw, cap=16,
                ops=[("update", ticks[:5]), ("update", ticks[5:]), ("update", [[EMPTY]] * 4), ("flush", None)])


# ---------------------------------------------------------------------------------------------------- seeded crowds
def crowd_case(seed, hw, cell, streams, ids, ticks=12, cap=1, forget_after=1, anchor=HO.FOOT, split=(5, 1), extra_ops=True):
    """Random walkers; stream s holds ids[s] of them over max_tracks = 4 slots, so a stream with five stops with ERR_CAPACITY.  Walkers
    come and go (expiry, slots taken again, finals waiting when cap = 1); boxes reach over every edge."""
    rng = np.random.default_rng(seed)
    H, W = hw
    pos = [[(int(rng.integers(0, W)), int(rng.integers(4, H + 4))) for _ in range(n)] for n in ids]
    rows = []
    for t in range(ticks):
        tick = []
        for s in range(streams):
            fr = []
            for j in range(ids[s]):
                x, y = pos[s][j]
                x, y = x + int(rng.integers(-6, 7)), y + int(rng.integers(-6, 7))
                if rng.random() < 0.2:
                    x, y = pos[s][j]                                         # stands still
                pos[s][j] = (int(np.clip(x, -4, W + 4)), int(np.clip(y, 2, H + 6)))
                away = j >= 1 and (t + 2 * j + s) % 5 in (2, 3) and ids[s] <= 4
                late = ids[s] > 4 and j == 4 and t < 3                       # the fifth id arrives at tick 3
                if not away and not late:
                    fr.append(person(pos[s][j][0], pos[s][j][1], 100 * s + j, cls=j % 2, w=int(rng.integers(2, 12)), h=int(rng.integers(4, 20))))
            tick.append(rows_array(fr))
        rows.append(tick)
    kw = dict(cell=cell, max_tracks=4, forget_after=forget_after, anchor=anchor, min_move=4)
    a, b = split
    ops = [("update", rows[:a]), ("update", rows[a:a + b])]
    if extra_ops:
        ops += [("reset", 0), ("update", rows[a + b:a + b + 2]), ("flush", streams - 1), ("decay", None, 0b10, 1), ("update", rows[a + b + 2:]),
                ("drain",), ("decay", 0, 0xFFD, 31), ("flush", None), ("drain",)]
    else:
        ops += [("update", rows[a + b:]), ("flush", None), ("drain",)]
    return dict(name=f"crowd{seed}-{H}x{W}-c{cell}-S{streams}", streams=streams, hw=hw, kw=kw, cap=cap, ops=ops)


def contention_case():
    """One frame of 512 rows whose feet share one cell: +512 to DWELL, VISITS and STARTS of it in one tick.  Then the same ids step east."""
    hw = (48, 64)
    first = rows_array([person(34 + i % 3, 20 + i % 5, i) for i in range(512)])
    second = rows_array([person(37 + i % 3, 20 + i % 5, i) for i in range(512)])
    kw = dict(cell=16, max_tracks=512, forget_after=1, anchor=HO.FOOT, min_move=4)
    return dict(name="contention", streams=1, hw=hw, kw=kw, cap=512, ops=[("update", [[first], [second]]), ("update", [[EMPTY]] * 3), ("flush", None)])


def saturation_case():
    """2^30 - 3 planted in one cell of every layer; five walkers land there, stay, step, and end: every layer stops at 2^30."""
    hw, cell = (37, 61), 8
    o = HO.HeatOracle(hw, cell=cell)
    planted = np.zeros((12, o.GH, o.GW), np.int32)
    planted[:, 2, 3] = HO.SAT - 3
    planted[HO.DWELL, 0, 0] = 5
    a = rows_array([person(26 + i % 2, 18 + i % 3, 10 + i) for i in range(5)])               # cell (2, 3): x 24..31, y 16..23
    far = rows_array([person(5, 5, 10 + i) for i in range(5)])                              # away to cell (0, 0) ...
    back = rows_array([person(30, 19, 10 + i) for i in range(5)])                           # ... and back from the west-north-west: one octant
    kw = dict(cell=cell, max_tracks=8, forget_after=1, anchor=HO.FOOT, min_move=4)
    ops = [("import", 0, 0xFFF, planted), ("update", [[a], [a], [far], [back]]), ("flush", None)]
    return dict(name="saturation", streams=1, hw=hw, kw=kw, cap=16, ops=ops)


def seeded_cases():
    return [walk_case((48, 64), 8), walk_case((37, 61), 16), walk_case((37, 61), 8, anchor=HO.CENTRE), walk_case((64, 96), 4), walk_case((64, 96), 32),
            crowd_case(1, (48, 64), 16, 3, (3, 4, 5)), crowd_case(2, (37, 61), 8, 3, (4, 5, 2), cap=2, forget_after=2),
            crowd_case(3, (37, 61), 16, 1, (4,), cap=16, anchor=HO.CENTRE), contention_case(), saturation_case()]


# ---------------------------------------------------------------------------------------------------- layers to render
def blob_layers(hw, cell, seed, peak=1000):
    """[12, GH, GW]: a few hot cells and a long tail, so that both scales and the floor have something to decide."""
    o = HO.HeatOracle(hw, cell=cell)
    rng = np.random.default_rng(seed)
    lay = np.zeros((12, o.GH, o.GW), np.int32)
    for l in range(12):
        v = rng.integers(0, 6, (o.GH, o.GW))
        v[rng.random((o.GH, o.GW)) < 0.5] = 0
        v[rng.integers(0, o.GH), rng.integers(0, o.GW)] = peak
        v[o.GH - 1, o.GW - 1] = peak // 3                                    # the partial last cell
        lay[l] = v
    return lay
