"""tests/heat_oracle.py (the specification of the heat-map stage) against independent statements of its rules, on
the CPU: the octant rule against exact fractions, the Q8 logarithm against math.log2, the bilinear level against a Fraction evaluation,
the colour ramp's anchors, and the seeded cases of tests/heat_cases.py reaching every branch."""
import math
from fractions import Fraction

import numpy as np
import pytest

import heat_cases as HC
import heat_oracle as HO


def test_octant_against_exact_fractions():
    """tan 22.5 degrees = sqrt(2) - 1 is irrational; the rule's 5 / 12 is the boundary.  Every (dx, dy) in -40..40, both boundary lines
    (12 |dy| = 5 |dx| and 12 |dx| = 5 |dy|, which belong to the diagonals) included."""
    t = Fraction(5, 12)
    on_lines = 0
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            if dx == 0 and dy == 0:
                continue
            ax, ay = abs(dx), abs(dy)
            if ax and Fraction(ay, ax) < t:
                want = 0 if dx > 0 else 4
            elif ay and Fraction(ax, ay) < t:
                want = 2 if dy > 0 else 6
            else:
                assert dx != 0 and dy != 0                                   # a zero component never reaches the diagonal branch
                want = {(1, 1): 1, (-1, 1): 3, (-1, -1): 5, (1, -1): 7}[(dx > 0) - (dx < 0), (dy > 0) - (dy < 0)]
                on_lines += 12 * ay == 5 * ax or 12 * ax == 5 * ay
            assert HO.octant(dx, dy) == want, (dx, dy)
            # clockwise from east with y down: the octant holds the step's angle
            ang = math.degrees(math.atan2(dy, dx)) % 360
            assert min(abs(ang - 45 * want), 360 - abs(ang - 45 * want)) <= 22.7, (dx, dy, want, ang)
    assert on_lines == 4 * 3 * 2                                             # (12, 5), (24, 10), (36, 15) and their mirrors, on both lines


def test_log_q8_against_log2():
    vs = {0, 1, 2, 3, HO.SAT}
    for b in range(1, 31):
        vs |= {(1 << b) - 2, (1 << b) - 1, 1 << b}
    vs |= {int(v) for v in np.random.default_rng(49).integers(0, HO.SAT, 4000)}
    vs = sorted(v for v in vs if 0 <= v <= HO.SAT)
    last = -1
    for v in vs:
        n, u = v + 1, HO.log_q8(v)
        b = math.floor(math.log2(n))
        # u is floor(log2) plus a LINEAR mantissa cut to 8 bits: within 1 / 256 of b + (n / 2^b - 1) everywhere ...
        assert 0 <= b + n / 2 ** b - 1 - u / 256 < 1 / 256, (v, u)
        # ... and so within 1 / 256 of log2 itself wherever the mantissa is below 2^-8 or a whole 1 - 2^-8: at every power of two, and at
        # every power of two +- 1 from 2^9 on.  Between them a linear mantissa trails log2 by up to 0.0861 (at m = 0.4427): that is the
        # rule's choice, and what a colour scale needs of it is that it is monotone.
        if n & (n - 1) == 0 or (b >= 9 and ((n - 1) & (n - 2) == 0 or (n + 1) & n == 0)):
            assert abs(math.log2(n) - u / 256) <= 1 / 256, (v, u)
        assert -1 / 256 < math.log2(n) - u / 256 < 0.0861 + 1 / 256, (v, u)
        assert u >= last, v
        last = u
    for b in range(0, 31):                                                   # exact at every power of two
        assert HO.log_q8((1 << b) - 1) == b << 8
    assert HO.log_q8(HO.SAT) == 30 << 8 and HO.log_q8(0) == 0
    assert all(HO.log_q8(v + 1) >= HO.log_q8(v) for v in range(0, 70000))
    for scale in (HO.LINEAR, HO.LOG):
        assert HO.level(0, 7, scale) == 0 and HO.level(7, 7, scale) == HO.Q_MAX and HO.level(HO.SAT, HO.SAT, scale) == HO.Q_MAX
        assert HO.level(1, 1, scale) == HO.Q_MAX


@pytest.mark.parametrize("cell", [4, 8, 16, 32])
def test_bilinear_against_fractions(cell):
    H, W = 37, 61
    GH, GW = -(-H // cell), -(-W // cell)
    q = np.random.default_rng(cell).integers(0, HO.Q_MAX + 1, (GH, GW))
    q[0, 0], q[-1, -1] = HO.Q_MAX, HO.Q_MAX
    got = HO.bilinear(q, H, W, cell)
    assert got.shape == (H, W) and got.min() >= 0 and got.max() <= 255
    for y in range(H):
        for x in range(W):
            # the pixel's centre in units of cells, from the centre of cell 0; neighbours clamped to the grid
            u, v = Fraction(2 * x + 1 - cell, 2 * cell), Fraction(2 * y + 1 - cell, 2 * cell)
            i, j = math.floor(u), math.floor(v)
            a, b = u - i, v - j
            g = lambda r, c: int(q[min(max(r, 0), GH - 1), min(max(c, 0), GW - 1)])      # noqa: E731
            val = (g(j, i) * (1 - a) + g(j, i + 1) * a) * (1 - b) + (g(j + 1, i) * (1 - a) + g(j + 1, i + 1) * a) * b
            assert got[y, x] == math.floor(val / 256 + Fraction(1, 2)), (cell, y, x)
    flat = HO.bilinear(np.full((GH, GW), HO.Q_MAX), H, W, cell)
    assert (flat == 255).all()


def test_lut_anchors_and_monotone_segments():
    lut = HO.default_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    for L, rgb in HO.LUT_ANCHORS:
        assert lut[L].tolist() == list(rgb)[::-1], L                         # stored BGR
    for (a, p), (b, q) in zip(HO.LUT_ANCHORS, HO.LUT_ANCHORS[1:]):
        for c in range(3):
            d = np.diff(lut[a:b + 1, 2 - c].astype(int))
            assert (d >= 0).all() if q[c] >= p[c] else (d <= 0).all(), (a, c)
            assert abs(d).max() <= -(-abs(q[c] - p[c]) // (b - a)), (a, c)


def test_seeded_cases_reach_every_branch():
    log = {}
    for case in HC.seeded_cases():
        oracles = HC.oracles_for(case)
        for op in case["ops"]:
            HC.run_op(oracles, op, case["cap"])
        for o in oracles:
            for k, v in o.log.items():
                log[k] = [a + b for a, b in zip(log.get(k, [0] * 8), v)] if isinstance(v, list) else log.get(k, 0) + v
    for k in ("new", "same_cell", "new_cell", "moved", "still", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom", "duplicate", "expired",
              "flushed", "capacity_stop", "pending_over_cap", "saturated"):
        assert log[k] > 0, (k, log)
    assert all(n > 0 for n in log["octants"]), log["octants"]


def test_planted_walk_is_what_it_says():
    case = HC.walk_case()
    (o,) = HC.oracles_for(case)
    tags = []
    for t in range(len(HC.WALK)):
        rows = (case["ops"][0][1] + case["ops"][1][1])[t][0]
        tags.append(o.step(rows, [], 16)[0])                                 # (row 0 is id 1's, except at the tick it is away)
    octs = [int(t[3]) for t in tags[1:9]]
    assert octs == [0, 1, 2, 3, 4, 5, 6, 7]
    assert tags[9].tolist() == [2 * o.GW + 2, 2, 0, -1]                      # still, second tick in the cell it re-entered
    assert tags[11].tolist() == [2 * o.GW + 2, 3, 2, -1]                     # a tick away, then one pixel: below min_move
    assert o.layers[HO.VISITS, 2, 2] == 2 and o.layers[HO.STARTS, 2, 2] == 1     # entered twice, started once
    assert o.layers[HO.DWELL, o.GH - 1, 1] == 12                            # the feet below the picture stand in the last row
    assert o.layers[HO.ENDS, 2, 2] == 0 and o.layers[HO.ENDS, o.GH - 1, 1] == 0      # ids 1 and 2 have not left the table
    assert o.layers[HO.ENDS].sum() > 0                                       # the edge boxes that come every third tick have, by expiry


def test_ends_follow_the_drain_and_import_checks_its_range():
    o = HO.HeatOracle((48, 64), cell=8, max_tracks=4, forget_after=0)
    a = HC.rows_array([HC.person(10, 10, 1), HC.person(30, 30, 2)])
    out, pend, st, _ = o.update([a, HC.EMPTY], 1)
    assert len(out) == 1 and pend == 1 and st == 0 and o.layers[HO.ENDS].sum() == 1
    out, pend, _, _ = o.update([], 1)
    assert len(out) == 1 and pend == 0 and o.layers[HO.ENDS].sum() == 2 and o.layers[HO.ENDS, 3, 3] == 1
    with pytest.raises(ValueError):
        o.import_layers(1, np.full((1, o.GH, o.GW), HO.SAT + 1))
    with pytest.raises(ValueError):
        o.import_layers(1, np.full((1, o.GH, o.GW), -1))
    o.import_layers(0b101, np.full((2, o.GH, o.GW), 9))
    assert (o.layers[0] == 9).all() and (o.layers[2] == 9).all() and o.layers[1].max() == 1
    o.decay(0b100, 1)
    assert (o.layers[2] == 4).all() and (o.layers[0] == 9).all()
    o.decay(0xFFF, 31)
    assert not o.layers.any()
