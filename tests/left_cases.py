"""Planted scenes for the left-objects stage, shared by tests/test_left_oracle.py (the oracle alone, no GPU) and
tests/test_gpu_left.py (the device against the oracle).  A case is dict(name, hw, cell, max_objects, options, frames [ticks, S, H, W, 3]
u8, rows = None or [tick][stream] -> int32 [n, 6], plus whatever the scene planted).  A uniform cell colour (v, v, v) has gray level v
exactly: the exact scenes are painted cell by cell with scene_cases.paint."""
import numpy as np

import left_oracle as LO
from scene_cases import paint, rows_for

NO_ROWS = np.zeros((0, 6), np.int32)


def case(name, hw, cell, frames, options=None, rows=None, max_objects=32, **planted):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim == 4:
        frames = frames[:, None]
    assert frames.shape[2:] == (hw[0], hw[1], 3), frames.shape
    return dict(name=name, hw=tuple(hw), cell=cell, max_objects=max_objects, options=dict(options or {}), frames=frames, rows=rows, **planted)


def oracles_for(cs):
    return [LO.LeftOracle(cs["hw"], cs["cell"], cs["max_objects"], **cs["options"]) for _ in range(cs["frames"].shape[1])]


# ---- a bag on a noisy gradient: 240 x 320, c = 8, default options ------------------------------------------------------------------------
BAG_HW, BAG_AT, BAG_STEP, BAG_LEVEL = (24, 32), (120, 96), 3, 230             # block height x width, x y at rest, px per tick while sliding


def gradient(ticks, sigma=6, seed=1):
    """float [ticks, 240, 320, 3]: the smooth gradient of scene_cases.noise_mover plus Gaussian noise, one frame at a time."""
    rng = np.random.default_rng(seed)
    h, w = 240, 320
    base = 60 + (np.arange(w)[None, :] * 100) // w + (np.arange(h)[:, None] * 40) // h
    for _ in range(ticks):
        yield base[:, :, None] + rng.normal(0.0, sigma, (h, w, 3))


def bag_x(t, slide_from, rest_from):
    return BAG_AT[0] - BAG_STEP * max(rest_from - t, 0) if t >= slide_from else None


def bag(ticks=300, slide_from=30, rest_from=60, taken_at=260, row=None, options=None, name="a bag"):
    """A 24 x 32 px block of level 230 slides in at 3 px per tick from `slide_from`, rests cell-aligned at x 120, y 96 from `rest_from`
    and is taken away at `taken_at`.  row = (id, first tick, last tick + 1, on_rest): a tracker row of that id over the block's own
    box in those ticks."""
    frames = np.zeros((ticks, 240, 320, 3), np.uint8)
    rows = [[NO_ROWS] for _ in range(ticks)]
    for t, f in enumerate(gradient(ticks)):
        x = bag_x(t, slide_from, rest_from)
        if x is not None and t < taken_at:
            f[BAG_AT[1]:BAG_AT[1] + BAG_HW[0], x:x + BAG_HW[1]] = BAG_LEVEL
            if row is not None and row[1] <= t < row[2]:
                rows[t] = [np.array([[x, BAG_AT[1], x + BAG_HW[1] - 1, BAG_AT[1] + BAG_HW[0] - 1, row[0], 0]], np.int32)]
        frames[t] = np.clip(np.rint(f), 0, 255)
    box = [BAG_AT[0], BAG_AT[1], BAG_AT[0] + BAG_HW[1], BAG_AT[1] + BAG_HW[0]]
    return case(name, (240, 320), 8, frames, options, rows if row is not None else None, box=box, rest_from=rest_from, taken_at=taken_at)


def mirror(ticks=170):
    """The block is there from tick 0 and taken at tick 60."""
    return bag(ticks, slide_from=0, rest_from=0, taken_at=60, name="the mirror")


def owner_carried(owner_window=None):
    """A row of id 12 covers the block while it slides in and leaves at tick 70."""
    opts = {} if owner_window is None else dict(owner_window=owner_window)
    return bag(200, row=(12, 30, 70), options=opts, name=f"owner carried, window {owner_window}")


def owner_standing():
    """A row of id 5 stands on the resting block for 400 ticks."""
    return bag(560, taken_at=10 ** 6, row=(5, 60, 460), name="owner standing")


# ---- exact scenes: painted cell by cell ---------------------------------------------------------------------------------------------------
EXACT = dict(warmup=1, min_ticks=1, fast_shift=1)


def painted(name, cells, c=4, options=None, rows=None, hw=None, **planted):
    cells = np.asarray(cells)
    hw = hw or (cells.shape[1] * c, cells.shape[2] * c)
    return case(name, hw, c, [paint(x, c, hw) for x in cells], dict(EXACT, **(options or {})), rows, **planted)


def df_edge(history=24):
    """Cell (1, 1) falls from 150 to 100: its fast settles at 25600 exactly (a floor shift of a negative gap reaches it).  Cell (1, 3)
    rises from 50 to 100: its fast stops at 25599.  Both then show 110 for one tick: df = 2560 = thresh << 8 is stable, 2561 is not."""
    g = np.full((history + 2, 3, 5), 100, np.uint8)
    g[0, 1, 1], g[0, 1, 3] = 150, 50
    g[history + 1, 1, 1] = g[history + 1, 1, 3] = 110
    return painted("df edge", g, test_tick=history + 1)


def ds_edge(history=24):
    """Cells (1, 1) and (1, 3) start at 100; at tick 1 the second shows 101 and its slow learns 1 (25601).  From tick 2 both show 90 under a
    row that covers the grid (slow and still stay, fast settles at 23040); at the last tick the row is gone: ds = 2560 = thresh << 8 does
    not differ, 2561 does."""
    g = np.full((history + 3, 3, 5), 100, np.uint8)
    g[1, 1, 3] = 101
    g[2:, 1, 1] = g[2:, 1, 3] = 90
    T = len(g)
    cover = np.array([[0, 0, 19, 11, 3, 0]], np.int32)
    rows = [[cover if 2 <= t < T - 1 else NO_ROWS] for t in range(T)]
    return painted("ds edge", g, options=dict(pad_cells=0), rows=rows, test_tick=T - 1)


def jump(ticks=40, options=None, name="a 100-level jump"):
    """Cells (1, 1) and (1, 2) of a 3 x 5 grid jump from 100 to 200 at tick 3 and stay."""
    g = np.full((ticks, 3, 5), 100, np.uint8)
    g[3:, 1, 1:3] = 200
    return painted(name, g, options=options, jump_at=3)


def absorb():
    return jump(30, dict(absorb_ticks=8, alarm_hold=2, gone_ticks=1), "absorb")


def no_decay(decay=0):
    """The jump settles, then from tick 16 the two cells flicker between 200 and 120: unstable on every tick."""
    g = np.full((30, 3, 5), 100, np.uint8)
    g[3:, 1, 1:3] = 200
    g[16::2, 1, 1:3] = 120
    return painted(f"decay {decay}", g, options=dict(decay=decay), flicker_from=16)


# ---- components: a pattern of cells jumps from 100 to 200 and every one becomes a candidate at the same tick --------------------------------
def pattern(name, mask, c=4, options=None, max_objects=32, after=7, hw=None):
    mask = np.asarray(mask, bool)
    g = np.full((2 + after,) + mask.shape, 100, np.uint8)
    g[2:, mask] = 200
    cs = painted(name, g, c, options, hw=hw, mask=mask)
    cs["max_objects"] = max_objects
    return cs


def spiral(n=17):
    """A square spiral, one cell wide, walls one cell apart: one blob whose smallest index is far from its far end."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    for _ in range(n * n):
        ny, nx = y + dy, x + dx
        ahead = 0 <= ny < n and 0 <= nx < n and not m[ny, nx]
        ny2, nx2 = ny + dy, nx + dx
        blocked = ahead and 0 <= ny2 < n and 0 <= nx2 < n and m[ny2, nx2]
        if not ahead or blocked:
            dy, dx = dx, -dy                                                 # turn right
            ny, nx = y + dy, x + dx
            ny2, nx2 = ny + dy, nx + dx
            if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx] or (0 <= ny2 < n and 0 <= nx2 < n and m[ny2, nx2]):
                break
        y, x = ny, nx
        m[y, x] = True
    return m


def comb(h=9, w=17):
    """Teeth hanging from a bar in the LAST row: every tooth's own least label has to travel down and along the bar."""
    m = np.zeros((h, w), bool)
    m[-1, :] = True
    m[:, ::2] = True
    return m


def isolated(h, w):
    m = np.zeros((h, w), bool)
    m[::2, ::2] = True
    return m


def component_cases(c=4):
    corner = np.zeros((4, 5), bool)
    corner[1, 1] = corner[2, 2] = True
    apart = np.zeros((4, 5), bool)
    apart[1, 1] = apart[1, 3] = True
    sizes = np.zeros((5, 13), bool)                                          # blobs of 2, 3 and 4 cells
    sizes[1, 1:3] = sizes[1, 5:8] = sizes[1, 9:13] = True
    one = dict(min_cells=1)
    return [pattern(f"corner c{c}", corner, c, one), pattern(f"apart c{c}", apart, c, one), pattern(f"spiral c{c}", spiral(), c),
            pattern(f"comb c{c}", comb(), c), pattern(f"70 isolated c{c}", isolated(14, 20), c, one, max_objects=64),
            pattern(f"40 on 32 c{c}", isolated(10, 16), c, one), pattern(f"sizes 3..3 c{c}", sizes, c, dict(min_cells=3, max_cells=3)),
            pattern(f"sizes 2..4 c{c}", sizes, c, dict(min_cells=2, max_cells=4)), split_merge(c)]


def split_merge(c=4):
    """A bar of 5 cells (slot 0); its middle cell goes back (two blobs: the left one keeps slot 0 by label order, the right one opens
    slot 1); the middle cell changes again (one blob meeting both slots with 2 cells each: the lowest slot takes it, slot 1 ends)."""
    g = np.full((40, 3, 7), 100, np.uint8)
    g[2:, 1, 1:6] = 200
    g[12:22, 1, 3] = 100
    return painted(f"split and merge c{c}", g, c, dict(decay=64, gone_ticks=2, alarm_hold=3), phases=(12, 22))


# ---- seeded cases for the device ------------------------------------------------------------------------------------------------------------
def small_rows(rng, hw, n):
    """scene_cases.rows_for with every box a quarter as wide and high (a coordinate past the limit stays), ids 1..n."""
    r = rows_for(rng, hw, n)
    keep = r[:, 3] <= 1 << 20
    r[keep, 2] = r[keep, 0] + (r[keep, 2] - r[keep, 0]) // 4
    r[keep, 3] = r[keep, 1] + (r[keep, 3] - r[keep, 1]) // 4
    return r


def seeded(name, hw, cell, streams=1, ticks=40, seed=0, options=None, max_objects=32):
    """Per stream a random cell texture with per-pixel noise of +-2 levels; blocks of a few cells appear at random ticks, rest for a random
    while and go; rows_for rows (some valid, some not) with small ids wander over the frame.  Options short enough for every path of a
    tick inside 40 ticks."""
    rng = np.random.default_rng(seed)
    h, w = hw
    hc, wc = h // cell, w // cell
    frames = np.zeros((ticks, streams, h, w, 3), np.uint8)
    for s in range(streams):
        tex = np.repeat(np.repeat(rng.integers(60, 140, (hc + 1, wc + 1)), cell, axis=0), cell, axis=1)[:h, :w].astype(np.int64)
        blocks = []
        for _ in range(6):
            bh, bw = int(rng.integers(1, max(hc // 2, 1) + 1)) * cell, int(rng.integers(1, max(wc // 2, 1) + 1)) * cell
            y, x = int(rng.integers(0, hc)) * cell, int(rng.integers(0, wc)) * cell
            t0 = int(rng.integers(2, ticks // 2))
            blocks.append((y, x, bh, bw, t0, t0 + int(rng.integers(4, ticks)), int(rng.integers(180, 256))))
        for t in range(ticks):
            f = tex[:, :, None] + rng.integers(-2, 3, (h, w, 3))
            for y, x, bh, bw, t0, t1, level in blocks:
                if t0 <= t < t1:
                    f[y:y + bh, x:x + bw] = level
            frames[t, s] = np.clip(f, 0, 255)
    rows = [[small_rows(rng, hw, int(rng.integers(0, 4))) for s in range(streams)] for t in range(ticks)]
    opts = dict(warmup=2, min_ticks=3, absorb_ticks=14, fast_shift=1, slow_shift=4, decay=1, alarm_hold=2, gone_ticks=2, owner_window=10, min_cells=1)
    opts.update(options or {})
    return case(name, hw, cell, frames, opts, rows, max_objects)
