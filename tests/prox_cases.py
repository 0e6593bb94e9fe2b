"""Seeded cases for the proximity stage, shared by tests/test_prox_oracle.py (which shows through the oracle alone
that together they reach every branch) and tests/test_gpu_prox.py (which holds the device to the oracle on each).

A case is dict(name, streams, hw, kw, cap, cap_pairs, ops).  An op is one call:
    ("update", rows[tick][stream])      ("drain",)      ("flush", stream or None)      ("reset", stream)
    ("option", key, value)              ("ground", stream or None, H[9], shift)
Frames are 48 x 64 (none is read); each shape is the smallest that can break."""
import numpy as np

import prox_oracle as PO

EMPTY = np.zeros((0, 6), np.int32)
HW = (48, 64)


def rows_array(rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def person(x, y, tid, h=20, cls=0):
    """A box whose foot anchor is pixel (x, y): fx = 2 x, fy = 2 y, hc = h."""
    return [x - 3, y - h, x + 3, y, tid, cls]


def anchored(fx, fy, tid, h=3):
    """A box with the anchor (fx, fy) in doubled pixels (fy even)."""
    return [fx // 2, fy // 2 - h, fx - fx // 2, fy // 2, tid, 0]


def oracles_for(case):
    return [PO.ProxOracle(case["hw"], stream=s, **case["kw"]) for s in range(case["streams"])]


def run_op(oracles, op, cap, cap_pairs):
    """One op through the oracles -> the packed outputs of an update / drain / flush, or None."""
    kind = op[0]
    if kind == "update":
        return PO.run_bank(oracles, op[1], cap, cap_pairs)
    if kind == "drain":
        return PO.run_bank(oracles, [], cap, 0)
    if kind == "flush":
        return PO.flush_bank(oracles, cap, op[1])
    if kind == "reset":
        oracles[op[1]].reset()
    elif kind == "option":
        for o in oracles:
            o.option(op[1], op[2])
    elif kind == "ground":
        for s, o in enumerate(oracles):
            if op[1] is None or op[1] == s:
                o.set_ground(op[2], op[3])
    else:
        raise ValueError(kind)
    return None


# ---------------------------------------------------------------------------------------------------- the planted pair
def pair_case():
    """A (id 1) stands still, B (id 2) stands 6 pixels away: they LINK at the third tick and not before.  B misses a tick (the pair is
    frozen), comes back a pixel further (dt = 2), walks away: UNLINK at the second far tick.  B leaves for good; D (id 4) takes B's slot
    while A is still there and inherits nothing: A and D link three ticks later.  C (id 3) runs along the bottom."""
    ticks = []
    for t in range(14):
        rows = [person(20, 30, 1)]
        if t <= 2:
            rows.append(person(26, 30, 2))
        elif t == 4:
            rows.append(person(27, 30, 2))
        elif t in (5, 6):
            rows.append(person(45, 30, 2))
        if t >= 9:
            rows.append(person(25, 31, 4))
        rows.append(person(4 + 2 * t, 46, 3))
        if t == 1:
            rows.append(person(50, 20, 1, cls=1))                            # id 1 again in the same frame: only the first counts
        if t == 7:
            rows.append([5, 5, 4, 9, 8, 0])                                  # x2 < x1: not valid
            rows.append([70, 5, 80, 25, 9, 0])                               # x1 >= W: outside, never counted
        ticks.append([rows_array(rows)])
    kw = dict(max_tracks=8, forget_after=2, metric=PO.BODY, near=700, link_ticks=3, unlink_ticks=2, speed_shift=1, still_speed=5, run_speed=70)
    return dict(name="pair", streams=1, hw=HW, kw=kw, cap=4, cap_pairs=4,
                ops=[("update", ticks[:5]), ("update", ticks[5:12]), ("update", ticks[12:]), ("update", [[EMPTY]] * 4), ("flush", None)])


# ---------------------------------------------------------------------------------------------------- the ground plane
GROUND_H, GROUND_SHIFT = (1024, 0, 0, 0, 1024, 0, 0, -1, 40), 14
"""den = 80 - fy: rows with their feet at y >= 40 lie at or above the horizon (den <= 0); just below it the numerators, shifted by 14, go
beyond 2^24."""


def ground_case():
    ticks = []
    for t in range(8):
        rows = [person(10 + t, 10, 1), person(14 + t, 10, 2), person(30, 12 + t, 3), person(20, 40, 4), person(22, 44, 5), person(40, 39, 6),
                person(50, 5, 7), person(52 - t, 5 + t, 8)]
        ticks.append([rows_array(rows), rows_array(rows[::-1][:5 + t % 3])])
    kw = dict(max_tracks=16, forget_after=3, metric=PO.GROUND, near=1 << 19, link_ticks=2, unlink_ticks=2, speed_shift=2, still_speed=1 << 10,
              run_speed=1 << 19)
    ident = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    return dict(name="ground", streams=2, hw=HW, kw=kw, cap=16, cap_pairs=8,
                ops=[("ground", None, GROUND_H, GROUND_SHIFT), ("update", ticks[:3]), ("ground", 1, ident, 0), ("option", "near", 12),
                     ("update", ticks[3:6]), ("option", "metric", PO.BODY), ("option", "near", 900), ("update", ticks[6:]), ("flush", None)])


# ---------------------------------------------------------------------------------------------------- seeded crowds
def crowd_case(seed, streams, ids, ticks=12, cap=1, cap_pairs=2, split=(5, 1), max_tracks=4, extra_ops=True, **kw_over):
    """Random walkers in a small room, so that pairs form and break; stream s holds ids[s] of them over max_tracks slots, so a stream with
    more stops with ERR_CAPACITY.  Walkers come and go (expiry, slots taken again, finals waiting when cap = 1)."""
    rng = np.random.default_rng(seed)
    H, W = HW
    pos = [[(int(rng.integers(10, 40)), int(rng.integers(20, 44))) for _ in range(n)] for n in ids]
    rows = []
    for t in range(ticks):
        tick = []
        for s in range(streams):
            fr = []
            for j in range(ids[s]):
                x, y = pos[s][j]
                if rng.random() >= 0.3:
                    x, y = x + int(rng.integers(-3, 4)), y + int(rng.integers(-3, 4))
                pos[s][j] = (int(np.clip(x, -4, W + 4)), int(np.clip(y, 2, H + 6)))
                away = j >= 1 and (t + 2 * j + s) % 7 in (2, 3) and ids[s] <= max_tracks
                late = ids[s] > max_tracks and j == ids[s] - 1 and t < 3     # the last id arrives at tick 3
                if not away and not late:
                    fr.append(person(pos[s][j][0], pos[s][j][1], 100 * s + j, h=int(rng.integers(14, 26)), cls=j % 2))
            if fr and rng.random() < 0.5:
                fr = [fr[i] for i in rng.permutation(len(fr))]               # the row order changes: a pair's owner changes
            tick.append(rows_array(fr))
        rows.append(tick)
    kw = dict(max_tracks=max_tracks, forget_after=1, metric=PO.BODY, near=900, height_ratio_q8=320, link_ticks=2, unlink_ticks=2, speed_shift=2,
              still_speed=20, run_speed=120)
    kw.update(kw_over)
    a, b = split
    ops = [("update", rows[:a]), ("update", rows[a:a + b])]
    if extra_ops:
        ops += [("reset", 0), ("update", rows[a + b:a + b + 2]), ("flush", streams - 1), ("update", rows[a + b + 2:]), ("drain",), ("flush", None), ("drain",)]
    else:
        ops += [("update", rows[a + b:]), ("flush", None), ("drain",)]
    return dict(name=f"crowd{seed}-S{streams}", streams=streams, hw=HW, kw=kw, cap=cap, cap_pairs=cap_pairs, ops=ops)


# ---------------------------------------------------------------------------------------------------- frame sizes
DOUBLED = (2, 0, 0, 0, 2, 0, 0, 0, 1)
"""The ground map whose unit is the doubled pixel: gx = fx, gy = fy (the identity's unit is the pixel: its denominator is 2 H8 = 2)."""


def lattice_rows(n, seed, step=4, shuffle=True):
    """n rows on a lattice of `step` doubled pixels, ids 1000 + k, in shuffled row order."""
    rng = np.random.default_rng(seed)
    rows = [anchored(2 + step * (k % 30), 8 + step * (k // 30), 1000 + k) for k in range(n)]
    if shuffle and n:
        rows = [rows[i] for i in rng.permutation(n)]
    return rows_array(rows)


def sizes_case():
    """Frames of 0, 1, 2, 63, 64, 65 and 512 rows (the last three across a mask word's edge) on a lattice whose 4-neighbours are near;
    link_ticks 2, so the second frame of a size links them."""
    kw = dict(max_tracks=512, forget_after=1, metric=PO.GROUND, near=4, link_ticks=2, unlink_ticks=1, speed_shift=0, still_speed=0, run_speed=3)
    ticks = []
    for k, n in enumerate((0, 1, 2, 63, 64, 65, 512)):
        ticks += [[lattice_rows(n, k)], [lattice_rows(n, 100 + k)]]
    return dict(name="sizes", streams=1, hw=HW, kw=kw, cap=512, cap_pairs=16, ops=[("ground", None, DOUBLED, 0), ("update", ticks[:7]), ("update", ticks[7:]), ("flush", None)])


def path_rows(n=512, run=60):
    """n anchors along a comb: runs of `run` points two doubled pixels apart, joined at alternating ends by three points: consecutive
    points are exactly 2 apart, all others more.  [(fx, fy)] in path order."""
    pts, fy, k = [], 0, 0
    while len(pts) < n:
        xs = range(0, 2 * run, 2) if k % 2 == 0 else range(2 * run - 2, -2, -2)
        pts += [(x, fy) for x in xs]
        end = pts[-1][0]
        pts += [(end, fy + 2), (end, fy + 4), (end, fy + 6)]
        fy, k = fy + 8, k + 1
    return pts[:n]


def path_case():
    """A path graph of 512 rows in shuffled row order: one component, the worst case of label propagation, for the near graph and (link_ticks
    1) for the linked graph.  Then the path is cut in the middle (one row missing)."""
    pts = path_rows()
    rng = np.random.default_rng(55)
    order = rng.permutation(len(pts))
    full = rows_array([anchored(pts[i][0], pts[i][1], 1 + int(i)) for i in order])
    cut = rows_array([anchored(pts[i][0], pts[i][1], 1 + int(i)) for i in order if i != 256])
    kw = dict(max_tracks=512, forget_after=1, metric=PO.GROUND, near=2, link_ticks=1, unlink_ticks=1, speed_shift=0, still_speed=0, run_speed=1)
    return dict(name="path", streams=1, hw=HW, kw=kw, cap=0, cap_pairs=600, ops=[("ground", None, DOUBLED, 0), ("update", [[full], [cut]])])


def cliques_case():
    """Two cliques of four joined by one edge: one party of eight; the second clique steps away, the edge unlinks after two far ticks:
    two parties of four."""
    A = [(10, 10), (12, 10), (10, 12), (12, 12)]
    B = [(16, 10), (18, 10), (17, 12), (19, 12)]
    def frame(shift):
        return rows_array([anchored(x, y, 1 + i) for i, (x, y) in enumerate(A)] + [anchored(x + shift, y, 11 + i) for i, (x, y) in enumerate(B)])
    kw = dict(max_tracks=8, forget_after=1, metric=PO.GROUND, near=4, link_ticks=2, unlink_ticks=2, speed_shift=1, still_speed=0, run_speed=2)
    ticks = [[frame(0)], [frame(0)], [frame(0)], [frame(2)], [frame(2)], [frame(2)]]
    return dict(name="cliques", streams=1, hw=HW, kw=kw, cap=8, cap_pairs=32, ops=[("ground", None, DOUBLED, 0), ("update", ticks[:2]), ("update", ticks[2:]), ("flush", None)])


def truncation_case():
    """Six people in one spot with link_ticks 1: fifteen LINK events in the first tick, cap_pairs 4: the list is cut, the count is true."""
    fr = rows_array([person(20 + i % 3, 30 + i // 3, 1 + i) for i in range(6)])
    kw = dict(max_tracks=8, forget_after=1, metric=PO.BODY, near=700, link_ticks=1, unlink_ticks=1)
    return dict(name="truncation", streams=1, hw=HW, kw=kw, cap=2, cap_pairs=4, ops=[("update", [[fr], [fr], [EMPTY], [EMPTY]]), ("drain",), ("drain",)])


def long_case(ticks=32770):
    """Two people who stay together for more than 32767 ticks: `on` stops there."""
    fr = rows_array([person(20, 30, 1), person(24, 30, 2)])
    kw = dict(max_tracks=2, forget_after=1, metric=PO.BODY, near=700, link_ticks=2, unlink_ticks=2)
    return dict(name="long", streams=1, hw=HW, kw=kw, cap=2, cap_pairs=1, ops=[("update", [[fr]] * ticks)])


def seeded_cases(long=True):
    cases = [pair_case(), ground_case(), crowd_case(1, 3, (3, 4, 5)), crowd_case(2, 3, (4, 5, 2), cap=2, forget_after=2, cap_pairs=0),
             crowd_case(3, 1, (4,), cap=16, cap_pairs=64), sizes_case(), path_case(), cliques_case(), truncation_case()]
    return cases + [long_case()] if long else cases
