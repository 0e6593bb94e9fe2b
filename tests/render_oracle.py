"""The executable specification of the redaction / annotation stage (aic_render_*), in NumPy integers.  The
device is held to it bit for bit (tests/test_gpu_render.py).

A frame is uint8 [H, W, 3] BGR.  The final value of a pixel is the first rule that applies; everything "original" is read from the
frame as handed in, never from a partly rendered one:
  (a) annotation primitives: the colour of the LAST primitive of the frame's list that covers the pixel.  Kinds 0, 1, 2 are
      oracle/overlay_oracle.py's (outline ring of thickness 2, inclusive filled rectangle, 5x7 text).  Kind 3 = (3, ax, ay, bx, by,
      color, t, 0) is a segment A->B of thickness t in 1..8: with dx = bx - ax, dy = by - ay,
        |dx| >= |dy| and dx != 0:  hit iff min(ax, bx) <= x <= max(ax, bx) and 2 * |dx * (y - ay) - dy * (x - ax)| <= t * |dx|
        |dy| > |dx|:               hit iff min(ay, by) <= y <= max(ay, by) and 2 * |dy * (x - ax) - dx * (y - ay)| <= t * |dy|
        A == B:                    nothing.
      Consequences that the tests pin: the ends are cut square on the major axis (no caps); the band is CLOSED, so a pixel whose centre
      lies exactly t / 2 from the line is lit on both sides -- an odd t on a line through half-integer minor positions lights t + 1
      pixels in that column (t = 1 on a 1 : 2 slope lights two pixels every other column), an even t on an axis-parallel line lights
      t + 1.
  (b) static masks: (x, y) is inside one of the camera's polygons -> mask_color.  Inside = the even-odd rule with half-open edges of
      tests/zones_oracle.py on the integer point: an edge A->B counts iff (ay > y) != (by > y) and the point lies strictly on the side
      of the edge that a ray towards +x crosses, d = (bx - ax)(y - ay) - (x - ax)(by - ay), (d > 0) == (by > ay).  Consequences: rows are
      half-open under either winding (a polygon's top row is inside, its bottom row outside; horizontal edges never count); a pixel
      exactly ON a non-horizontal edge counts that edge iff the edge runs towards smaller y, so the boundary columns depend on the
      winding: vertices clockwise on the screen (y down) leave the pixels on left and right edges outside (an axis-aligned polygon
      with corners (x0, y0), (x1, y1) masks x0 < x < x1, y0 <= y < y1), the opposite order takes both in (x0 <= x <= x1).
  (c) redaction: the pixel lies in the union of the frame's rectangles (inclusive corners, clipped to the frame).  style "fill" ->
      fill_color; style "mosaic" with cell c in {4, 8, 16, 32} -> per channel the mean of the ORIGINAL pixels of cell (x // c, y // c),
      grid anchored at the frame's origin, over the n pixels the cell has inside the frame: (sum + n // 2) // n.
  (d) unchanged.

Rows [n, 6] int32 = x1 y1 x2 y2 id cls give the rectangles (rects()): coordinates saturated to +-2^20 first, then a row with x2 < x1
or y2 < y1 is dropped; "box" = (x1 - pad, y1 - pad, x2 + pad, y2 + pad), "head" = the same x range and y from y1 - pad to
y1 + (((y2 - y1) * head_q8) >> 8); classes None = every row, else rows whose cls is in the set or outside 0..63; "off" = none."""
import numpy as np

from oracle.overlay_oracle import paint

COORD_MAX = 1 << 20
CELLS = (4, 8, 16, 32)


def rects(rows, redact="box", pad=0, head_q8=64, classes=None):
    """-> int64 [m, 4] = x0 y0 x1 y1 inclusive, in row order."""
    assert redact in ("off", "box", "head") and 1 <= head_q8 <= 256 and pad >= 0
    out = []
    if redact != "off":
        for r in np.asarray(rows, np.int64).reshape(-1, 6).tolist():
            x1, y1, x2, y2 = (min(max(v, -COORD_MAX), COORD_MAX) for v in r[:4])
            cls = r[5]
            if x2 < x1 or y2 < y1:
                continue
            if classes is not None and 0 <= cls <= 63 and cls not in classes:
                continue
            out.append((x1 - pad, y1 - pad, x2 + pad, y2 + pad if redact == "box" else y1 + (((y2 - y1) * head_q8) >> 8)))
    return np.array(out, np.int64).reshape(-1, 4)


def _window(h, w, x0, y0, x1, y1):
    """The part of the frame inside the inclusive box, as (ys, xs, slices): the masks below are evaluated there and are False elsewhere."""
    x0, y0, x1, y1 = max(int(x0), 0), max(int(y0), 0), min(int(x1), w - 1), min(int(y1), h - 1)
    if x1 < x0 or y1 < y0:
        return None
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    return ys, xs, (slice(y0, y1 + 1), slice(x0, x1 + 1))


def segment_mask(h, w, ax, ay, bx, by, t):
    out = np.zeros((h, w), bool)
    win = _window(h, w, min(ax, bx) - t, min(ay, by) - t, max(ax, bx) + t, max(ay, by) + t)      # |offset| <= t / 2 on the minor axis
    dx, dy = int(bx) - int(ax), int(by) - int(ay)
    if win is None or (dx == 0 and dy == 0):
        return out
    ys, xs, where = win
    if abs(dx) >= abs(dy):
        out[where] = (xs >= min(ax, bx)) & (xs <= max(ax, bx)) & (2 * np.abs(dx * (ys - ay) - dy * (xs - ax)) <= t * abs(dx))
    else:
        out[where] = (ys >= min(ay, by)) & (ys <= max(ay, by)) & (2 * np.abs(dy * (xs - ax) - dx * (ys - ay)) <= t * abs(dy))
    return out


def polygon_mask(h, w, poly):
    out = np.zeros((h, w), bool)
    pts = [(int(x), int(y)) for x, y in np.asarray(poly).reshape(-1, 2).tolist()]
    win = _window(h, w, min(p[0] for p in pts), min(p[1] for p in pts), max(p[0] for p in pts), max(p[1] for p in pts))   # nothing is inside beyond it
    if win is None:
        return out
    ys, xs, where = win
    odd = np.zeros(ys.shape, bool)
    for i, (ax, ay) in enumerate(pts):
        bx, by = pts[(i + 1) % len(pts)]
        d = (bx - ax) * (ys - ay) - (xs - ax) * (by - ay)
        odd ^= ((ay > ys) != (by > ys)) & ((d > 0) == (by > ay))
    out[where] = odd
    return out


def mosaic(frame, cell, red=None):
    """Every pixel (of the cells that hold a pixel of `red`, when given) replaced by its cell's rounded mean."""
    h, w = frame.shape[:2]
    out = frame.copy()
    for y0 in range(0, h, cell):
        for x0 in range(0, w, cell):
            if red is not None and not red[y0:y0 + cell, x0:x0 + cell].any():
                continue
            blk = frame[y0:y0 + cell, x0:x0 + cell].astype(np.int64)
            n = blk.shape[0] * blk.shape[1]
            out[y0:y0 + cell, x0:x0 + cell] = (blk.sum((0, 1)) + n // 2) // n
    return out


def bgr(color):
    return (color & 255, (color >> 8) & 255, (color >> 16) & 255)


def render_frame(frame, rect_list=(), prims=(), text=(), polys=(), style="mosaic", cell=16, fill_color=0, mask_color=0):
    """One frame -> a new array.  rect_list [m, 4] (from rects()), prims [n, 8] with `text` their buffer, polys the camera's masks."""
    assert style in ("fill", "mosaic") and cell in CELLS
    orig = np.ascontiguousarray(frame, np.uint8)
    h, w = orig.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    out = orig.copy()
    # (c) first, then (b), then (a) painted over them: the first rule that applies wins
    red = np.zeros((h, w), bool)
    for x0, y0, x1, y1 in np.asarray(rect_list, np.int64).reshape(-1, 4).tolist():
        red |= (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
    if red.any():
        out[red] = mosaic(orig, cell, red)[red] if style == "mosaic" else bgr(fill_color)
    inside = np.zeros((h, w), bool)
    for poly in polys:
        inside |= polygon_mask(h, w, poly)
    out[inside] = bgr(mask_color)
    prims = np.asarray(prims, np.int64).reshape(-1, 8)
    i = 0
    while i < len(prims):                                   # runs of kinds 0..2 go through the overlay oracle, kind 3 is painted here
        if prims[i, 0] == 3:
            _, ax, ay, bx, by, color, t, _ = prims[i].tolist()
            assert 1 <= t <= 8
            out[segment_mask(h, w, ax, ay, bx, by, t)] = bgr(color)
            i += 1
        else:
            j = i
            while j < len(prims) and prims[j, 0] != 3:
                j += 1
            paint(out, prims[i:j], text)
            i = j
    return out


def render(frames, rows=None, counts=None, prim_lists=None, cameras=None, masks=None, n_cameras=1, redact="off", style="mosaic", cell=16,
           fill_color=0, pad=0, head_q8=64, classes=None, mask_color=0):
    """The whole call: frames [F, H, W, 3] -> a new array.  rows flat [n, 6] with counts [F]; prim_lists = one (prims, text) per frame or
    None; masks = {camera: [polygon, ...]}; cameras defaults to f % n_cameras."""
    frames = np.asarray(frames, np.uint8)
    F = len(frames)
    out = np.empty_like(frames)
    rows = np.zeros((0, 6), np.int64) if rows is None else np.asarray(rows, np.int64).reshape(-1, 6)
    counts = [0] * F if counts is None else [int(c) for c in counts]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    for f in range(F):
        cam = f % n_cameras if cameras is None else int(cameras[f])
        prims, text = prim_lists[f] if prim_lists is not None and prim_lists[f] is not None else (np.zeros((0, 8), np.int64), b"")
        out[f] = render_frame(frames[f], rects(rows[off[f]:off[f + 1]], redact, pad, head_q8, classes), prims, text,
                              (masks or {}).get(cam, ()), style, cell, fill_color, mask_color)
    return out
