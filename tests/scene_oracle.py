"""Scene watch: the executable specification, in NumPy.  One SceneOracle is one camera; the device
(ai-camera_amd/scene.py, csrc/kernels_scene.hip) is held to it with np.array_equal -- records, masks, row_motion and the exported state.

Integer arithmetic only (int64 here; every value fits int32 except the sums the text names); every shift is NumPy's >> on signed
integers, a floor shift.

Readings this file decides where the text leaves a gap:
  * tick 0 of a stream (age == 0) computes mean_luma and sharp like any other, and its record carries them; ref_q8 starts at sharp << 8.
  * DEFOCUS is judged against ref_q8 as it stood BEFORE the tick's reference update; the record's ref_q8 is the value AFTER it.
  * `alarms`, `edges` and `active` of a record are the values after steps 6 and 7 of their own tick.
  * FROZEN compares with the previous tick's gray; warmup >= 1, so a ready tick always has one.
  * quiet counts from create / reset on, also while not ready (n_moving is 0 there); `active` is forced while not ready, so a stream
    that never moved goes idle on its first ready tick with quiet > gate_hold.
  * a row_motion box is clipped to the pixels the grid covers, [0, Wc c - 1] x [0, Hc c - 1]; the remainder columns belong to no cell.
  * export of a stream that has seen no tick (or was just reset) is all zeros.
"""
import numpy as np

KINDS = ("dark", "bright", "defocus", "scene", "frozen")
DARK, BRIGHT, DEFOCUS, SCENE, FROZEN = (1 << i for i in range(5))
SAT = 1 << 30
COORD_MAX = 1 << 20
RECORD_FIELDS = ("frame", "ready", "active", "n_moving", "n_raw", "x0", "y0", "x1", "y1", "mean_luma", "sharp", "ref_q8", "n_changed", "cond",
                 "alarms", "edges")
# name: (default, lowest, highest)
OPTIONS = dict(thresh=(6, 0, 255), noise_k_q4=(64, 0, 4096), warmup=(16, 1, 1 << 20), big_thresh=(24, 0, 255), learn_shift=(4, 1, 12),
               slow_extra=(3, 0, 8), dev_init_q8=(512, 0, 65280), min_neighbours=(3, 1, 9), dark_luma=(16, 0, 256), bright_luma=(240, 0, 255),
               min_ref_q8=(512, 0, 1 << 20), defocus_q8=(96, 0, 256), scene_q16=(39322, 0, 65536), ref_shift=(6, 1, 12), hold=(25, 1, 1 << 20),
               gate_cells=(4, 1, 1 << 24), gate_hold=(30, 0, 1 << 20))


def gray(bgr, c):
    """int64 [H // c, W // c] in 0..255: (sum over the c x c cell of 29 B + 150 G + 77 R) >> (8 + 2 log2 c)."""
    assert c in (4, 8, 16)
    bgr = np.asarray(bgr)
    hc, wc = bgr.shape[0] // c, bgr.shape[1] // c
    v = bgr[:hc * c, :wc * c].astype(np.int64)
    y = (29 * v[..., 0] + 150 * v[..., 1] + 77 * v[..., 2]).reshape(hc, c, wc, c).sum(axis=(1, 3))
    return y >> (8 + 2 * (c.bit_length() - 1))


def count3x3(m):
    """Per cell, the set cells of its 3 x 3 neighbourhood (itself included), outside the grid counting 0."""
    p = np.pad(m.astype(np.int64), 1)
    h, w = m.shape
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))


def sharpness(g):
    hc, wc = g.shape
    if hc < 3 or wc < 3:
        return 0
    lap = np.abs(4 * g[1:-1, 1:-1] - g[:-2, 1:-1] - g[2:, 1:-1] - g[1:-1, :-2] - g[1:-1, 2:])
    return int(lap.sum()) // ((hc - 2) * (wc - 2))


def row_motion(rows, clean, c):
    """int32 [n]: per row 256 * moving // covered over the cells its box touches, -1 for an invalid or empty one."""
    rows = np.asarray(rows, np.int64).reshape(-1, 6)
    hc, wc = clean.shape
    out = np.full(len(rows), -1, np.int32)
    for i, (x1, y1, x2, y2) in enumerate(rows[:, :4]):
        if max(abs(int(v)) for v in (x1, y1, x2, y2)) > COORD_MAX or x2 < x1 or y2 < y1:
            continue
        X0, Y0, X1, Y1 = max(x1, 0), max(y1, 0), min(x2, wc * c - 1), min(y2, hc * c - 1)
        if X1 < X0 or Y1 < Y0:
            continue
        box = clean[Y0 // c:Y1 // c + 1, X0 // c:X1 // c + 1]
        out[i] = 256 * int(box.sum()) // box.size
    return out


class SceneOracle:
    def __init__(self, frame_hw, cell=8, **options):
        self.h, self.w, self.c = int(frame_hw[0]), int(frame_hw[1]), int(cell)
        self.hc, self.wc = self.h // self.c, self.w // self.c
        assert self.c in (4, 8, 16) and self.hc >= 1 and self.wc >= 1
        self.o = {k: v[0] for k, v in OPTIONS.items()}
        for k, v in options.items():
            self.set_option(k, v)
        self.reset()

    def set_option(self, key, value):
        _, lo, hi = OPTIONS[key]
        assert lo <= value <= hi, (key, value)
        o = dict(self.o, **{key: int(value)})
        assert o["learn_shift"] + o["slow_extra"] <= 14
        self.o = o

    def reset(self):
        z = np.zeros((self.hc, self.wc), np.int64)
        self.bg, self.dev, self.prev = z.copy(), z.copy(), z.copy()
        self.age = self.quiet = self.ref_q8 = self.alarm = 0
        self.on, self.off = [0] * 5, [0] * 5

    def export(self):
        """bg, dev, prev int32 [Hc, Wc]; scalars int32 [16] = age, quiet, ref_q8, alarms, on[5], off[5], 0, 0."""
        sc = np.array([self.age, self.quiet, self.ref_q8, self.alarm] + self.on + self.off + [0, 0], np.int32)
        return self.bg.astype(np.int32), self.dev.astype(np.int32), self.prev.astype(np.int32), sc

    def tick(self, frame_bgr, rows=None):
        """One frame [H, W, 3] u8 BGR -> (record int32 [16], mask u8 [Hc, Wc] (bit 0 clean, bit 1 raw), row_motion int32 [n])."""
        o, c = self.o, self.c
        g = gray(frame_bgr, c)
        g256 = 256 * g
        sharp = sharpness(g)
        ready = self.age >= o["warmup"]
        # 1, 2: the model
        if self.age == 0:
            self.bg = g256.copy()
            self.dev = np.full_like(g, o["dev_init_q8"])
            raw = changed = np.zeros(g.shape, bool)
            self.ref_q8 = sharp << 8
        else:
            d = np.abs(g256 - self.bg)
            thr = np.maximum(o["thresh"] << 8, (self.dev * o["noise_k_q4"]) >> 4)
            raw = (d > thr) & ready
            changed = (d > (o["big_thresh"] << 8)) & ready
            a = o["learn_shift"] + o["slow_extra"] * raw
            self.bg = self.bg + ((g256 - self.bg) >> a)
            self.dev = self.dev + ((d - self.dev) >> a)
        # 3: clean-up
        clean = raw & (count3x3(raw) >= o["min_neighbours"])
        # 4: statistics
        n_raw, n_moving, n_changed = int(raw.sum()), int(clean.sum()), int(changed.sum())
        if n_moving:
            ys, xs = np.nonzero(clean)
            box = [int(xs.min()) * c, int(ys.min()) * c, (int(xs.max()) + 1) * c, (int(ys.max()) + 1) * c]
        else:
            box = [-1, -1, -1, -1]
        mean_luma = int(g.sum()) // (self.hc * self.wc)
        # 5: conditions
        cond = 0
        if ready:
            cond |= DARK * (mean_luma < o["dark_luma"])
            cond |= BRIGHT * (mean_luma > o["bright_luma"])
            cond |= DEFOCUS * (self.ref_q8 >= o["min_ref_q8"] and (sharp << 16) < self.ref_q8 * o["defocus_q8"])
            cond |= SCENE * (n_changed * 65536 > o["scene_q16"] * self.hc * self.wc)
            cond |= FROZEN * bool((g == self.prev).all())
        if not ready or not cond & DEFOCUS:
            self.ref_q8 += ((sharp << 8) - self.ref_q8) >> o["ref_shift"]
        # 6: alarms
        edges = 0
        for k in range(5):
            if cond >> k & 1:
                self.on[k], self.off[k] = min(self.on[k] + 1, SAT), 0
            else:
                self.off[k], self.on[k] = min(self.off[k] + 1, SAT), 0
            if not self.alarm >> k & 1 and self.on[k] >= o["hold"]:
                self.alarm |= 1 << k
                edges |= 1 << k
            elif self.alarm >> k & 1 and self.off[k] >= o["hold"]:
                self.alarm &= ~(1 << k)
                edges |= 1 << (8 + k)
        # 7: gate
        self.quiet = 0 if n_moving >= o["gate_cells"] else min(self.quiet + 1, SAT)
        active = (not ready) or self.quiet <= o["gate_hold"]
        rec = np.array([self.age, ready, active, n_moving, n_raw] + box + [mean_luma, sharp, self.ref_q8, n_changed, cond, self.alarm, edges],
                       np.int32)
        # 8
        self.prev = g.copy()
        self.age = min(self.age + 1, SAT)
        mask = (clean.astype(np.uint8) | (raw.astype(np.uint8) << 1))
        rm = row_motion(rows, clean, c) if rows is not None else np.zeros(0, np.int32)
        return rec, mask, rm


def run(oracles, frames, rows=None):
    """frames [ticks, S, H, W, 3]; rows[tick][stream] -> (records [ticks, S, 16], masks [ticks, S, Hc, Wc], row_motion flat in
    tick-major order)."""
    T, S = frames.shape[:2]
    recs = np.zeros((T, S, 16), np.int32)
    masks = np.zeros((T, S, oracles[0].hc, oracles[0].wc), np.uint8)
    rm = []
    for t in range(T):
        for s in range(S):
            recs[t, s], masks[t, s], m = oracles[s].tick(frames[t, s], None if rows is None else rows[t][s])
            rm.append(m)
    return recs, masks, np.concatenate(rm) if rm else np.zeros(0, np.int32)
