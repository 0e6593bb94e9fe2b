"""tests/render_oracle.py, the specification of the redaction / annotation stage, held to a per-pixel pure-Python
restatement of the issue's rules on frames of at most 24 x 40, with the corner cases pinned: mosaic rounding, kind-3 ties, polygon
boundary pixels under both windings, and equality with oracle/overlay_oracle.py where only kinds 0 to 2 are drawn."""
import numpy as np
import pytest

import render_oracle as RO
import zones_oracle as ZO
from conftest import pkg
from oracle.overlay_oracle import FONT, paint

H, W = 24, 40


def frame(seed=0, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def prim_hit(p, text, x, y):
    kind, x0, y0, x1, y1, _, toff, tls = p
    if kind == 1:
        return x0 <= x <= x1 and y0 <= y <= y1
    if kind == 0:
        return (x0 - 1 <= x <= x1 + 1 and y0 - 1 <= y <= y1 + 1) and not (x0 < x < x1 and y0 < y < y1)
    if kind == 2:
        s, ln = tls >> 16, tls & 0xFFFF
        dx, dy = x - x0, y - y0
        if not (0 <= dy < 7 * s and 0 <= dx < 6 * s * ln):
            return False
        ci, gx, gy = dx // (6 * s), dx % (6 * s) // s, dy // s
        ch = int(text[toff + ci])
        return gx < 5 and 32 <= ch <= 126 and bool(int(FONT[ch - 32, gx]) >> gy & 1)
    ax, ay, bx, by, t = x0, y0, x1, y1, toff
    dx, dy = bx - ax, by - ay
    if abs(dx) >= abs(dy) and dx != 0:
        return min(ax, bx) <= x <= max(ax, bx) and 2 * abs(dx * (y - ay) - dy * (x - ax)) <= t * abs(dx)
    if abs(dy) > abs(dx):
        return min(ay, by) <= y <= max(ay, by) and 2 * abs(dy * (x - ax) - dx * (y - ay)) <= t * abs(dy)
    return False


def per_pixel(fr, rect_list, prims, text, polys, style, cell, fill_color, mask_color):
    """The issue's rules, a pixel at a time, first rule first."""
    h, w = fr.shape[:2]
    out = fr.copy()
    prims = np.asarray(prims, np.int64).reshape(-1, 8).tolist()
    for y in range(h):
        for x in range(w):
            hit = [p for p in prims if prim_hit(p, text, x, y)]
            if hit:
                out[y, x] = RO.bgr(hit[-1][5])
            elif any(ZO.inside([(2 * int(px), 2 * int(py)) for px, py in poly], 2 * x, 2 * y) for poly in polys):
                out[y, x] = RO.bgr(mask_color)
            elif any(x0 <= x <= x1 and y0 <= y <= y1 for x0, y0, x1, y1 in rect_list):
                if style == "fill":
                    out[y, x] = RO.bgr(fill_color)
                else:
                    cx, cy = x // cell * cell, y // cell * cell
                    blk = fr[cy:min(cy + cell, h), cx:min(cx + cell, w)].reshape(-1, 3).astype(int)
                    n = len(blk)
                    out[y, x] = [(int(blk[:, c].sum()) + n // 2) // n for c in range(3)]
    return out


def some_prims():
    V = pkg("visualization")
    pl = V.PrimList()
    pl.fill(3, 2, 12, 9, (1, 2, 3))
    pl.outline(8, 5, 30, 20, (4, 5, 6))
    pl.put_text(2, 8, "a}", 2, (7, 8, 9))
    pl.segment(0, 23, 39, 1, 3, (10, 11, 12))
    pl.segment(35, -3, 31, 30, 2, (13, 14, 15))
    pl.fill(10, 10, 14, 12, (16, 17, 18))
    pl.put_text(-4, 17, "Q", 1, (19, 20, 21))
    return pl.arrays()


@pytest.mark.parametrize("style,cell", [("mosaic", 4), ("mosaic", 8), ("mosaic", 16), ("mosaic", 32), ("fill", 16)])
def test_oracle_equals_the_per_pixel_rules(style, cell):
    fr = frame(1)
    prims, text = some_prims()
    rect_list = [(-3, -2, 6, 5), (20, 10, 45, 30), (22, 12, 25, 14), (15, 3, 15, 3), (50, 0, 60, 5)]
    polys = [[(5, 12), (30, 14), (18, 18), (28, 26), (-4, 22)], [(33, 2), (38, 2), (38, 7), (33, 7)]]
    kw = dict(style=style, cell=cell, fill_color=0x112233, mask_color=0x445566)
    for r, p, m in ((rect_list, prims, polys), (rect_list, [], []), ([], prims, []), ([], [], polys), ([], [], [])):
        got = RO.render_frame(fr, r, p, text, m, **kw)
        assert np.array_equal(got, per_pixel(fr, r, p, text, m, **kw))
    assert np.array_equal(RO.render_frame(fr), fr)


def test_mosaic_rounding_pins():
    fr = np.zeros((6, 9, 3), np.uint8)
    fr[0:4, 0:4, 0] = 10
    fr[0, 0:2, 0] = 11                                   # sum 162 over 16: mean 10.125 -> 10
    fr[0:4, 4:8, 1] = 7
    fr[0:2, 4:8, 1] = 8                                  # sum 120 over 16: mean 7.5 -> 8 (a half rounds up)
    fr[0:4, 8, 2] = [1, 2, 2, 2]                         # clipped to 1 x 4: n = 4, sum 7, mean 1.75 -> 2
    fr[4:6, 0:4, 2] = 3
    fr[4, 0, 2] = 7                                      # clipped to 4 x 2: n = 8, sum 28, mean 3.5 -> 4
    fr[4:6, 8, 0] = [200, 255]                           # the corner cell, 1 x 2: n = 2, sum 455 -> 228
    out = RO.render_frame(fr, [(0, 0, 100, 100)], style="mosaic", cell=4)
    assert out[1, 1, 0] == 10 and out[3, 6, 1] == 8 and (out[0:4, 8, 2] == 2).all() and (out[4:6, 0:4, 2] == 4).all() and (out[4:6, 8, 0] == 228).all()
    # only redacted pixels change; the cell mean uses ORIGINAL pixels whatever else is drawn or redacted in the cell
    out = RO.render_frame(fr, [(1, 1, 1, 1)], prims=[(1, 0, 0, 0, 0, 0xFFFFFF, 0, 0)], style="mosaic", cell=4)
    assert out[1, 1, 0] == 10 and tuple(out[0, 0]) == (255, 255, 255) and np.array_equal(out[2:], fr[2:]) and out[0, 1, 0] == 11
    # the grid is anchored at the origin: a box that moves by a pixel shows the same values where both cover
    a = RO.render_frame(frame(3), [(5, 5, 20, 15)], cell=8)
    b = RO.render_frame(frame(3), [(6, 5, 21, 15)], cell=8)
    assert np.array_equal(a[5:16, 6:21], b[5:16, 6:21])
    # overlapping boxes and their order cannot matter
    assert np.array_equal(RO.render_frame(frame(3), [(5, 5, 20, 15), (10, 2, 30, 9)], cell=8), RO.render_frame(frame(3), [(10, 2, 30, 9), (5, 5, 20, 15)], cell=8))


def test_segments_in_all_octants_and_ties():
    c = (20, 12)
    ends = [(34, 12), (32, 6), (26, 0), (20, 1), (14, 0), (8, 6), (6, 12), (8, 18), (14, 23), (20, 22), (26, 23), (32, 18),    # axes + octants
            (30, 2), (10, 2), (10, 22), (30, 22)]                                                                           # the diagonals
    for t in range(1, 9):
        for e in ends:
            m = RO.segment_mask(H, W, c[0], c[1], e[0], e[1], t)
            ref = np.array([[prim_hit((3, c[0], c[1], e[0], e[1], 0, t, 0), b"", x, y) for x in range(W)] for y in range(H)])
            assert np.array_equal(m, ref) and m[c[1], c[0]] and m[e[1], e[0]], (t, e)
            assert np.array_equal(m, RO.segment_mask(H, W, e[0], e[1], c[0], c[1], t)), "a segment does not depend on its direction"
            dx, dy = abs(e[0] - c[0]), abs(e[1] - c[1])
            if dx >= dy:                                   # square ends on the major axis
                assert not m[:, :min(c[0], e[0])].any() and not m[:, max(c[0], e[0]) + 1:].any()
            else:
                assert not m[:min(c[1], e[1])].any() and not m[max(c[1], e[1]) + 1:].any()
        assert not RO.segment_mask(H, W, 7, 7, 7, 7, t).any()        # A == B draws nothing
    # ties: the band is closed.  t = 1 on a 1 : 2 slope lights both neighbours where the line passes half way between two rows
    m = RO.segment_mask(H, W, 0, 0, 8, 4, 1)
    assert [int(m[:, x].sum()) for x in range(9)] == [1, 2, 1, 2, 1, 2, 1, 2, 1] and m[0, 1] and m[1, 1]
    # axis-parallel: odd t lights t rows, even t lights t + 1
    assert [int(RO.segment_mask(H, W, 2, 10, 9, 10, t)[:, 5].sum()) for t in range(1, 9)] == [1, 3, 3, 5, 5, 7, 7, 9]
    assert [int(RO.segment_mask(H, W, 10, 2, 10, 9, t)[5].sum()) for t in range(1, 9)] == [1, 3, 3, 5, 5, 7, 7, 9]
    # |dx| == |dy| is x-major
    m = RO.segment_mask(H, W, 2, 2, 6, 6, 1)
    assert int(m.sum()) == 5 and all(m[k, k] for k in range(2, 7))


def test_polygon_boundary_pixels_under_both_windings():
    """The rule is tests/zones_oracle.py's: rows are half-open (top row in, bottom row out) under either winding; a pixel exactly ON a
    non-horizontal edge counts that edge as crossed iff the edge runs towards smaller y, so with the vertices clockwise on the screen (y
    down) the pixels on left and right edges are outside, and with the opposite order both are inside."""
    sq = [(4, 3), (10, 3), (10, 8), (4, 8)]                # clockwise on the screen
    for poly, xs in ((sq, (5, 10)), (sq[2:] + sq[:2], (5, 10)), (sq[::-1], (4, 11))):
        exp = np.zeros((H, W), bool)
        exp[3:8, xs[0]:xs[1]] = True
        assert np.array_equal(RO.polygon_mask(H, W, poly), exp)
    tri = [(2, 2), (12, 2), (2, 12)]                       # clockwise; the hypotenuse is x + y = 14
    exp = np.array([[2 < x and 2 <= y < 12 and x + y < 14 for x in range(W)] for y in range(H)])
    assert np.array_equal(RO.polygon_mask(H, W, tri), exp)
    exp = np.array([[2 <= x and 2 <= y < 12 and x + y <= 14 for x in range(W)] for y in range(H)])
    assert np.array_equal(RO.polygon_mask(H, W, tri[::-1]), exp)
    conc = [(5, 12), (30, 14), (18, 18), (28, 26), (-4, 22)]
    bow = [(2, 2), (20, 16), (20, 2), (2, 16)]             # self-crossing: even-odd
    for poly in (conc, conc[::-1], bow, bow[::-1]):
        m = RO.polygon_mask(H, W, poly)
        ref = np.array([[ZO.inside([(2 * px, 2 * py) for px, py in poly], 2 * x, 2 * y) for x in range(W)] for y in range(H)])
        assert np.array_equal(m, ref) and m.any()
    assert RO.polygon_mask(H, W, bow)[9, 5] and RO.polygon_mask(H, W, bow)[9, 17] and not RO.polygon_mask(H, W, bow)[4, 11]


def test_paint_equivalence_for_kinds_0_to_2():
    V = pkg("visualization")
    pl = V.PrimList()
    V.track_prims(pl, [(5, 12, 30, 22, 3, "person", 0.5), (-3, 4, 12, 30, 4, "car")])
    V.info_prims(pl, ["ab", "c"])
    prims, text = pl.arrays()
    fr = frame(5)
    assert np.array_equal(RO.render_frame(fr, prims=prims, text=text), paint(fr.copy(), prims, text))
    out = RO.render(np.stack([fr, frame(6)]), prim_lists=[(prims, text), None])
    assert np.array_equal(out[0], paint(fr.copy(), prims, text)) and np.array_equal(out[1], frame(6))


def test_rows_to_rectangles():
    m = 1 << 20
    rows = [(10, 20, 30, 60, 1, 0), (5, 5, 4, 9, 2, 0), (5, 5, 9, 4, 3, 0), (7, 7, 7, 7, 4, 1), (-2 * m, -2 * m, 2 * m, 2 * m, 5, 2),
            (1, 2, 3, 4, 6, 64), (1, 2, 3, 4, 7, -1), (1, 2, 3, 4, 8, 63)]
    assert RO.rects(rows, "off").shape == (0, 4)
    box = RO.rects(rows, "box", pad=3).tolist()
    assert box == [[7, 17, 33, 63], [4, 4, 10, 10], [-m - 3, -m - 3, m + 3, m + 3], [-2, -1, 6, 7], [-2, -1, 6, 7], [-2, -1, 6, 7]]
    head = RO.rects(rows, "head", pad=1, head_q8=64).tolist()
    assert head[0] == [9, 19, 31, 30] and head[1] == [6, 6, 8, 7] and head[2] == [-m - 1, -m - 1, m + 1, -m + (2 * m * 64 >> 8)]
    assert RO.rects(rows, "head", head_q8=256).tolist()[0] == [10, 20, 30, 60] and RO.rects(rows, "head", head_q8=1).tolist()[0] == [10, 20, 30, 20]
    sel = RO.rects(rows, "box", classes={1, 63}).tolist()
    assert sel == [[7, 7, 7, 7], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]           # class 1, then cls 64 and -1 (fail safe), then class 63
    assert RO.rects(rows, "box", classes=set()).tolist() == [[1, 2, 3, 4], [1, 2, 3, 4]]
