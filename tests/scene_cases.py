"""Planted scenes for the scene-watch stage, shared by tests/test_scene_oracle.py (the oracle alone, no GPU) and
tests/test_gpu_scene.py (the device against the oracle).  A case is dict(name, hw, cell, options, frames [ticks, S, H, W, 3] u8,
rows = None or [tick][stream] -> int32 [n, 6], plus whatever the scene planted).  A uniform cell colour (v, v, v) has gray level v
exactly (29 + 150 + 77 = 256): the exact scenes are painted cell by cell."""
import numpy as np

import scene_oracle as SO


def paint(cells, c, hw=None):
    """u8 [H, W, 3] whose cell (y, x) is uniformly cells[y, x]; hw may add remainder rows / columns (filled with 7)."""
    cells = np.asarray(cells, np.uint8)
    img = np.repeat(np.repeat(cells, c, axis=0), c, axis=1)
    h, w = hw or img.shape
    out = np.full((h, w), 7, np.uint8)
    out[:img.shape[0], :img.shape[1]] = img
    return np.repeat(out[:, :, None], 3, axis=2)


def case(name, hw, cell, frames, options=None, rows=None, **planted):
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim == 4:
        frames = frames[:, None]
    assert frames.shape[2:] == (hw[0], hw[1], 3), frames.shape
    return dict(name=name, hw=tuple(hw), cell=cell, options=dict(options or {}), frames=frames, rows=rows, **planted)


def oracles_for(cs):
    return [SO.SceneOracle(cs["hw"], cs["cell"], **cs["options"]) for _ in range(cs["frames"].shape[1])]


# ---- noise and a mover: 240 x 320, c = 8, default options --------------------------------------------------------------------------
MOVER_FROM, MOVER_HW, MOVER_STEP, MOVER_AT = 60, (32, 64), 3, (20, 100)      # first tick, block height x width, px per tick, x y at MOVER_FROM


def mover_box(t):
    """x0 y0 x1 y1 (exclusive) of the moving block at tick t >= MOVER_FROM."""
    x, y = MOVER_AT[0] + MOVER_STEP * (t - MOVER_FROM), MOVER_AT[1]
    return x, y, x + MOVER_HW[1], y + MOVER_HW[0]


def noise_mover(sigma, ticks=100, seed=0):
    """A smooth gradient plus Gaussian noise of `sigma` gray levels, independent per pixel and channel; from tick 60 a 32 x 64 block
    of level 230 moves right by 3 px per tick."""
    rng = np.random.default_rng(seed)
    h, w = 240, 320
    base = 60 + (np.arange(w)[None, :] * 100) // w + (np.arange(h)[:, None] * 40) // h
    frames = np.zeros((ticks, h, w, 3), np.uint8)
    for t in range(ticks):
        f = base[:, :, None] + rng.normal(0.0, sigma, (h, w, 3))
        if t >= MOVER_FROM:
            x0, y0, x1, y1 = mover_box(t)
            f[y0:y1, x0:x1] = 230
        frames[t] = np.clip(np.rint(f), 0, 255)
    return case(f"noise sigma {sigma} + mover", (h, w), 8, frames, sigma=sigma)


# ---- exact scenes ---------------------------------------------------------------------------------------------------------------------
def threshold_edge():
    """learn_shift 8, dev_init 0, warmup 2.  Tick 1 puts cell (1, 1) at 99: bg 25600 -> 25599.  Tick 2 shows 106 in (1, 1) and in (1, 3):
    d = 1537 = thr + 1 in the first, d = 1536 = thr in the second."""
    g = np.full((3, 3, 5), 100, np.uint8)
    g[1, 1, 1] = 99
    g[2, 1, 1] = g[2, 1, 3] = 106
    return case("threshold edge", (12, 20), 4, [paint(x, 4) for x in g], dict(learn_shift=8, dev_init_q8=0, warmup=2, min_neighbours=1))


def floor_shift(ticks=80):
    g = np.full((ticks, 3, 3), 100, np.uint8)
    g[3:] = 50
    return case("floor shift", (12, 12), 4, [paint(x, 4) for x in g], dict(learn_shift=2, slow_extra=0, warmup=1))


def cleanup(min_neighbours=3):
    """Tick 3: an isolated cell at (3, 4) and three in a row at the corner, (0, 0) (0, 1) (0, 2), jump from 100 to 200."""
    g = np.full((4, 6, 8), 100, np.uint8)
    g[3, 3, 4] = g[3, 0, 0] = g[3, 0, 1] = g[3, 0, 2] = 200
    return case(f"clean-up, {min_neighbours} neighbours", (24, 32), 4, [paint(x, 4) for x in g], dict(warmup=2, min_neighbours=min_neighbours))


ALARM_OPTIONS = dict(hold=3, learn_shift=2, slow_extra=1, warmup=4)


def texture(seed=3, grid=(12, 16)):
    return np.random.default_rng(seed).integers(30, 221, grid).astype(np.uint8)


def flicker(cells, t):
    """The texture with one cell toggling by one level per tick, so that no two consecutive frames are equal."""
    out = cells.copy()
    out[0, 0] += t & 1
    return out


def alarm_scene(kind, ticks=None):
    """96 x 128 at c = 8, a random cell texture (levels 30..220).  From tick 10: `dark` = lights off until tick 20; `defocus` = a flat frame
    of the texture's mean for 100 ticks; `frozen` = the frame of tick 9 repeated until tick 20; `scene` = the texture rolled by 40 px."""
    tex = texture()
    ticks = ticks or dict(dark=30, defocus=112, frozen=30, scene=80)[kind]
    cells = []
    for t in range(ticks):
        c = flicker(tex, t)
        if kind == "dark" and 10 <= t < 20:
            c = c >> 5
        if kind == "defocus" and 10 <= t < 110:
            c = np.full_like(tex, int(tex.mean())) + (t & 1)
        if kind == "frozen" and 10 <= t < 20:
            c = flicker(tex, 9)
        if kind == "scene" and t >= 10:
            c = np.roll(c, 5, axis=1)
        cells.append(c)
    return case(f"alarm {kind}", (96, 128), 8, [paint(c, 8) for c in cells], ALARM_OPTIONS, kind=kind)


GATE_HOLD, GATE_BUSY = 5, ((6, 12), (30, 33))                                 # ticks [a, b) in which a 3 x 3 block of cells jumps about


def gate_scene(ticks=40):
    """64 x 96 at c = 8 (8 x 12 cells), level 100; in the busy ticks a 3 x 3 block of level 200 sits at a fresh place every tick."""
    places = [(0, 0), (0, 4), (0, 8), (4, 0), (4, 4), (4, 8), (2, 2), (2, 6), (5, 9)]
    cells, k = [], 0
    for t in range(ticks):
        c = np.full((8, 12), 100, np.uint8)
        c[7, 11] += t & 1
        if any(a <= t < b for a, b in GATE_BUSY):
            y, x = places[k % len(places)]
            c[y:y + 3, x:x + 3] = 200
            k += 1
        cells.append(c)
    return case("gate", (64, 96), 8, [paint(c, 8) for c in cells], dict(warmup=4, gate_hold=GATE_HOLD, gate_cells=4))


# ---- seeded cases for the device: every path of a tick inside 40 ticks ---------------------------------------------------------------------
def rows_for(rng, hw, n):
    """n rows: most inside the frame, some hanging over it, some invalid."""
    h, w = hw
    out = np.zeros((n, 6), np.int32)
    for i in range(n):
        x1, y1 = int(rng.integers(-w // 2, w)), int(rng.integers(-h // 2, h))
        x2, y2 = x1 + int(rng.integers(0, w)), y1 + int(rng.integers(0, h))
        kind = rng.integers(0, 12)
        if kind == 0:
            x2 = x1 - 1                                                      # inverted
        elif kind == 1:
            y2 = (1 << 20) + 1                                               # a coordinate past the limit
        elif kind == 2:
            x1, x2 = w + 5, w + 50                                           # beside the frame
        elif kind == 3:
            x1, y1, x2, y2 = -5, -5, w + 5, h + 5                            # all of it
        elif kind == 4:
            x2, y2 = x1, y1                                                  # one pixel
        out[i] = x1, y1, x2, y2, i + 1, 0
    return out


def seeded(name, hw, cell, streams=1, ticks=40, seed=0, with_rows=True, options=None):
    """Per stream a random cell texture with per-pixel noise of +-3 levels, a block about a third of the frame at a fresh place every tick
    from tick 6, lights off in ticks 12..16, the frame of tick 21 repeated in ticks 22..26, the texture rolled from tick 30."""
    rng = np.random.default_rng(seed)
    h, w = hw
    hc, wc = h // cell, w // cell
    frames = np.zeros((ticks, streams, h, w, 3), np.uint8)
    rows = [] if with_rows else None
    for s in range(streams):
        tex = np.repeat(np.repeat(rng.integers(40, 201, (hc + 1, wc + 1)), cell, axis=0), cell, axis=1)[:h, :w].astype(np.int64)
        for t in range(ticks):
            f = np.roll(tex, 3 * cell, axis=1) if t >= 30 else tex
            f = f[:, :, None] + rng.integers(-3, 4, (h, w, 3))
            if t >= 6:
                bh, bw = max(h // 3, 1), max(w // 3, 1)
                y, x = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
                f[y:y + bh, x:x + bw] = 255 - f[y:y + bh, x:x + bw]
            if 12 <= t < 17:
                f = f >> 5
            frames[t, s] = np.clip(f, 0, 255)
            if 22 <= t < 27:
                frames[t, s] = frames[21, s]
    if with_rows:
        rows = [[rows_for(rng, hw, int(rng.integers(0, 6))) for s in range(streams)] for t in range(ticks)]
    opts = dict(warmup=4, hold=3, learn_shift=2, slow_extra=1, gate_hold=2)
    opts.update(options or {})
    return case(name, hw, cell, frames, opts, rows)
