"""tests/zones_oracle.py -- the specification of the zone / line counting stage -- against answers computed by
hand, the inside rule against an independent exact method, boundary points pinned as literals, and the seeded scenes of
tests/test_gpu_zones.py shown to be non-vacuous through the oracle alone."""
from fractions import Fraction

import numpy as np
import pytest

import zones_cases as ZC
import zones_oracle as ZO

E, X, LOST, CR = ZO.ENTER, ZO.EXIT, ZO.LOST, ZO.CROSS


def run(o, frames):
    return [o.step(r) for r in frames]


def test_square_walker_in_along_an_edge_out_and_lost():
    """A 10 x 10 square, one walker (id 7, cls 2), forget_after = 2.  By hand: f0 outside; f1 (5, 5) inside -> ENTER; f2 (5, 0) on the
    bottom edge, which the rule puts inside -> nothing; f3 (10, 5) on the right edge, outside -> EXIT, dwell 3 - 1 = 2; f4 (5, 5) ->
    ENTER; f5..f6 empty; f7: 7 - 4 > 2 -> LOST, dwell 4 + 1 - 4 = 1, anchor and cls as last seen."""
    o = ZO.ZonesOracle([ZC.SQUARE], [], forget_after=2)
    path = [(-5, 5), (5, 5), (5, 0), (10, 5), (5, 5)]
    got = run(o, [ZC.rows_at([p], ids=[7], cls=2) for p in path] + [np.zeros((0, 6), np.int32)] * 3)
    want_ev = [[], [(E, 0, 7, 2, 1, 0, 10, 10)], [], [(X, 0, 7, 2, 3, 2, 20, 10)], [(E, 0, 7, 2, 4, 0, 10, 10)], [], [], [(LOST, 0, 7, 2, 7, 1, 10, 10)]]
    assert [g[0] for g in got] == want_ev
    assert [g[1] for g in got] == [[0], [1], [1], [0], [1], [0], [0], [0]]
    zi, zo, lp, ln = o.counters()
    assert zi.tolist() == [2] and zo.tolist() == [2] and lp.size == 0 and ln.size == 0
    assert all(t is None for t in o.slots) and o.frame == 8


def test_centre_anchor():
    o = ZO.ZonesOracle([ZC.SQUARE], [], anchor="centre")
    ev, occ = o.step(np.array([[2, 1, 5, 8, 1, 0]], np.int32))               # centre (3.5, 4.5): doubled (7, 9)
    assert ev == [(E, 0, 1, 0, 0, 0, 7, 9)] and occ == [1]
    o = ZO.ZonesOracle([ZC.SQUARE], [], anchor="bottom")
    ev, occ = o.step(np.array([[2, 1, 5, 18, 1, 0]], np.int32))              # bottom centre (3.5, 18): outside
    assert ev == [] and occ == [0]


LINE = ((0, 0), (10, 0))                                                     # cross(B - A, p - A) = 10 * p.y: the + side is y >= 0


def crossing(p0, p1):
    o = ZO.ZonesOracle([], [LINE])
    o.step(ZC.rows_at([p0]))
    ev, _ = o.step(ZC.rows_at([p1]))
    assert all(e[0] == CR and e[1] == 0 for e in ev) and len(ev) <= 1
    return ev[0][5] if ev else 0


def test_line_crossing_and_recrossing_signs():
    o = ZO.ZonesOracle([], [LINE])
    evs = [o.step(ZC.rows_at([p]))[0] for p in [(5, -5), (5, 5), (5, -5), (5, 5)]]
    assert evs == [[], [(CR, 0, 1, 0, 1, 1, 10, 10)], [(CR, 0, 1, 0, 2, -1, 10, -10)], [(CR, 0, 1, 0, 3, 1, 10, 10)]]
    assert o.counters()[2].tolist() == [2] and o.counters()[3].tolist() == [1]


def test_line_touched_at_an_endpoint():
    """By hand (ta, tb of the spec): a move up through A crosses, up through B does not; down through B crosses, down through A does not.
    Half-open: a chain of segments sharing an endpoint counts a track through the joint once per direction."""
    assert crossing((0, -5), (0, 5)) == 1
    assert crossing((10, -5), (10, 5)) == 0
    assert crossing((10, 5), (10, -5)) == -1
    assert crossing((0, 5), (0, -5)) == 0
    assert crossing((11, -5), (11, 5)) == 0 and crossing((-1, -5), (-1, 5)) == 0     # past the ends


def test_track_stopping_on_the_line_counts_once():
    o = ZO.ZonesOracle([], [LINE])
    evs = [o.step(ZC.rows_at([p]))[0] for p in [(5, -5), (5, 0), (5, 5), (5, 0), (5, -5)]]
    assert [[e[5] for e in ev] for ev in evs] == [[], [1], [], [], [-1]]     # y = 0 is the + side


def test_collinear_and_zero_moves_do_not_cross():
    assert crossing((2, 0), (8, 0)) == 0
    assert crossing((-5, 0), (15, 0)) == 0
    assert crossing((15, 0), (-5, 0)) == 0
    assert crossing((5, 5), (5, 5)) == 0
    assert crossing((5, 0), (5, 0)) == 0


def test_first_sighting_has_no_line_test_and_a_gap_keeps_the_last_anchor():
    o = ZO.ZonesOracle([], [LINE], forget_after=3)
    empty = np.zeros((0, 6), np.int32)
    assert o.step(ZC.rows_at([(5, -5)]))[0] == []
    for _ in range(2):
        o.step(empty)
    assert [e[5] for e in o.step(ZC.rows_at([(5, 5)]))[0]] == [1]            # frame 3: 3 - 0 is not > 3, the track still crosses
    for _ in range(3):
        o.step(empty)
    assert o.step(ZC.rows_at([(5, -5)]))[0] == []                            # frame 7: 7 - 3 > 3, forgotten: a first sighting again


def test_duplicates_ignored_rows_and_slot_order():
    o = ZO.ZonesOracle([ZC.SQUARE], [], max_tracks=3, forget_after=1)
    far = 1 << 20
    rows = np.array([ZC.box(5, 5) + [4, 0], ZC.box(50, 50) + [4, 1], [far + 1, 0, far + 1, 5, 9, 0], ZC.box(5, 6) + [9, 0], ZC.box(5, 7) + [2, 0]], np.int32)
    ev, occ = o.step(rows)
    assert [(e[0], e[2]) for e in ev] == [(E, 4), (E, 9), (E, 2)] and occ == [3]   # the ignored row does not claim id 9
    assert [t["id"] for t in o.slots] == [4, 9, 2]
    assert o.step(ZC.rows_at([(5, 5)], ids=[9])) == ([], [1])                # frame 1: 1 - 0 is not > 1, nobody expires
    ev, occ = o.step(ZC.rows_at([(5, 5)], ids=[9]))                          # frame 2: 4 and 2 expire in slot order, 9 stays in slot 1
    assert [(e[0], e[2], e[5]) for e in ev] == [(LOST, 4, 1), (LOST, 2, 1)] and occ == [1]
    ev, _ = o.step(ZC.rows_at([(5, 5), (5, 5), (5, 5)], ids=[9, 30, 31]))
    assert [t["id"] for t in o.slots] == [30, 9, 31]                         # the lowest free slot first
    assert o.step(ZC.rows_at([(5, 5)] * 4, ids=[9, 30, 31, 32]))[0] == [] and o.status == ZO.ERR_CAPACITY
    assert o.step(ZC.rows_at([(5, 5)], ids=[9])) == ([], [0]) and o.frame == 4       # stopped: nothing until reset
    o.reset()
    assert o.status == 0 and o.counters()[0].tolist() == [0] and [e[0] for e in o.step(ZC.rows_at([(5, 5)]))[0]] == [E]


def test_expiring_slots_make_room_in_the_same_frame():
    o = ZO.ZonesOracle([ZC.SQUARE], [], max_tracks=2, forget_after=0)
    o.step(ZC.rows_at([(5, 5), (5, 5)], ids=[1, 2]))
    ev, _ = o.step(ZC.rows_at([(5, 5), (5, 5)], ids=[3, 4]))
    assert [(e[0], e[2]) for e in ev] == [(LOST, 1), (LOST, 2), (E, 3), (E, 4)] and o.status == 0


# ---- the inside rule against the winding number in exact rationals
def winding_inside(poly, px, py):
    wn = 0
    for i in range(len(poly)):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % len(poly)]
        if ay == by:
            continue
        x = Fraction(ax) + Fraction(py - ay) * Fraction(bx - ax, by - ay)   # where the edge's line meets the ray's height
        if ay <= py < by and x > px:
            wn += 1
        elif by <= py < ay and x > px:
            wn -= 1
    return wn != 0


def on_boundary(poly, px, py):
    for i in range(len(poly)):
        (ax, ay), (bx, by) = poly[i], poly[(i + 1) % len(poly)]
        if (bx - ax) * (py - ay) == (px - ax) * (by - ay) and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return True
    return False


def random_concave(rng, n):
    """A simple polygon: vertices at increasing angles around a centre with random radii (star-shaped, so it never crosses itself)."""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    rad = rng.uniform(15, 100, n)
    pts = [(int(round(100 + r * np.cos(a))), int(round(100 + r * np.sin(a)))) for a, r in zip(ang, rad)]
    return pts if len(set(pts)) == n else random_concave(rng, n)


@pytest.mark.parametrize("seed", range(6))
def test_inside_rule_equals_the_winding_number_off_the_boundary(seed):
    rng = np.random.default_rng(seed)
    poly = random_concave(rng, int(rng.integers(3, 33)))
    if seed % 2:
        poly = poly[::-1]                                                    # either winding
    poly2 = [(2 * x, 2 * y) for x, y in poly]
    n_in = n = 0
    for px, py in rng.integers(-10, 420, (400, 2)):                          # doubled coordinates: odd ones are half pixels
        px, py = int(px), int(py)
        if on_boundary(poly2, px, py):
            continue
        got = ZO.inside(poly2, px, py)
        assert got == winding_inside(poly2, px, py), (poly, px, py)
        n_in += got
        n += 1
    assert n > 300 and 20 < n_in < n - 20


def test_boundary_points_are_pinned():
    """Worked by hand from the rule.  Counter-clockwise square (0,0) (10,0) (10,10) (0,10): of its boundary only the open bottom edge is
    inside; the same square clockwise takes its left and right edges (open at the top) and the bottom edge with both corners."""
    ccw = [(2 * x, 2 * y) for x, y in ZC.SQUARE]
    cw = ccw[::-1]
    pts = {"left": (0, 10), "right": (20, 10), "bottom": (10, 0), "top": (10, 20), "v00": (0, 0), "v10": (20, 0), "v11": (20, 20), "v01": (0, 20)}
    assert {k: ZO.inside(ccw, *p) for k, p in pts.items()} == dict(left=False, right=False, bottom=True, top=False, v00=False, v10=False, v11=False, v01=False)
    assert {k: ZO.inside(cw, *p) for k, p in pts.items()} == dict(left=True, right=True, bottom=True, top=False, v00=True, v10=True, v11=False, v01=False)
    tri = [(0, 0), (20, 0), (0, 20)]                                          # slanted edge x + y = 20
    assert ZO.inside(tri, 10, 10) is False and ZO.inside(tri, 9, 10) is True and ZO.inside(tri, 11, 10) is False
    assert ZO.inside(tri[::-1], 10, 10) is True


def test_int64_is_needed():
    """Vertices and anchors near +-2^20: doubled differences reach 2^22 and the edge products 2^44."""
    m = 1 << 20
    poly = [(-m, -m), (m, -m + 1), (m, m), (-m, m - 1)]
    o = ZO.ZonesOracle([poly], [((-m, -m), (m, m))])
    # by hand: the bottom edge rises one pixel over 2^21, at x = m - 1 it is 1 / 2^21 below y = -m + 1; the top edge likewise
    pts = [(m - 1, -m + 1), (m - 1, -m), (-m + 1, m - 1), (-m + 1, m), (0, 0)]
    masks = [o.step(np.array([[x - 1, y, x + 1, y, 1, 0]], np.int32))[1][0] for x, y in pts]
    assert masks == [1, 0, 1, 0, 1]
    assert (4 * m) * (4 * m - 2) > 1 << 43                                   # an edge product of the first point


# ---- the seeded scenes of the GPU tests, through the oracle alone
def test_bank_scenes_produce_every_kind_of_event():
    for streams, frames, seed in ((3, 20, 1), (256, 1, 2)):
        geo, fr = ZC.bank_scene(streams, frames + (streams == 256), seed=seed)
        out = ZO.run_bank(ZC.oracles_for(geo, forget_after=3), fr, 64)
        assert out[0].max() <= 64 and out[0].sum() > 0 and out[2].sum() > 0
        if streams == 3:
            assert ZC.kinds_seen(out[1]) == ZC.ALL_KINDS
            assert all(len({len(r) for r in f}) > 1 for f in fr) and any(len(r) != len(np.unique(r[:, 4])) for f in fr for r in f)
