"""Pixels, frames and seeded scenes shared by tests/test_colours_oracle.py (are they non-vacuous?), tests/test_colours_host.py (the
host's pixel rule) and tests/test_gpu_colours.py (does the device agree?).  A case is dict(name, hw, streams, kw, cap, calls): kw = the
stage's parameters, calls = [(frames [ticks, S, H, W, 3] uint8, rows[tick][stream] = [n, 6] int32)] -- one entry per update call."""
import functools

import numpy as np

import colours_oracle as CO

EMPTY = np.zeros((0, 6), np.int32)
MX_EDGES = (39, 40, 71, 72, 135, 136, 175, 176, 199, 200)
SAT_EDGES = (39, 40, 127, 128)
HUE_EDGES = tuple(b for bound, _ in CO.HUE_BOUNDS[:-1] for b in (bound - 1, bound)) + (0, 1534)
# the palette of the issue, BGR
PALETTE = {
    "red": [(0, 0, 255), (0, 0, 139), (60, 20, 220)], "orange": [(0, 165, 255), (0, 140, 255)], "yellow": [(0, 255, 255), (0, 215, 255)],
    "green": [(0, 128, 0), (0, 255, 0), (34, 139, 34)], "cyan": [(255, 255, 0), (128, 128, 0)],
    "blue": [(255, 0, 0), (128, 0, 0), (189, 96, 21), (225, 105, 65)], "purple": [(238, 130, 238), (128, 0, 128), (255, 0, 255)],
    "pink": [(180, 105, 255), (203, 192, 255)], "brown": [(19, 69, 139), (45, 82, 160), (0, 128, 128)],
    "black": [(0, 0, 0), (30, 30, 30)], "gray": [(128, 128, 128), (192, 192, 192)], "white": [(255, 255, 255), (220, 245, 245)]}


@functools.lru_cache(maxsize=None)
def threshold_set():
    """uint8 [K, 3] BGR: for every maximum in MX_EDGES and 255, every (minimum, middle) and every order of the channels is looked at, and
    one pixel is kept per distinct (maximum, saturation if in SAT_EDGES, hue if in HUE_EDGES, which channels tie at the maximum, colour):
    every threshold of the pixel rule at its value and one beside it, the tie order of the maximum included."""
    px = []
    for mx in MX_EDGES + (255,):
        mn, mid = np.meshgrid(np.arange(mx + 1), np.arange(mx + 1), indexing="ij")
        keep = mid >= mn
        tri = np.stack([np.full(keep.sum(), mx), mid[keep], mn[keep]], axis=1)
        px += [tri[:, list(o)] for o in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]
    px = np.concatenate(px).astype(np.uint8)
    mx, sat, hq = CO.features(px)
    p = px.astype(np.int64)
    ties = (p[:, 0] == mx) * 1 + (p[:, 1] == mx) * 2 + (p[:, 2] == mx) * 4
    chroma = (mx >= 40) & (sat >= 40)
    key = np.stack([mx, np.where(np.isin(sat, SAT_EDGES), sat, -1), np.where(chroma & np.isin(hq, HUE_EDGES), hq, -1), ties, CO.classify(px)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    return np.ascontiguousarray(px[np.sort(first)])


def texture(rng, H, W):
    """A noise frame uint8 [H, W, 3]."""
    return rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


def pixel_frames(hw, seed, ticks=None):
    """[ticks, 1, H, W, 3]: the threshold set laid out pixel after pixel from pixel 5 t of frame t (so that it meets every alignment), over
    as many frames as it needs (at least `ticks`: the set comes round again), the rest of every frame seeded noise."""
    H, W = hw
    ts, rng = threshold_set(), np.random.default_rng(seed)
    per = H * W * 3 // 4                                                      # a quarter of every frame stays noise
    chunks = -(-len(ts) // per)
    n = max(chunks, ticks or 1)
    frames = rng.integers(0, 256, (n, 1, H * W, 3)).astype(np.uint8)
    for t in range(n):
        chunk = ts[(t % chunks) * per:(t % chunks + 1) * per]
        frames[t, 0, 5 * t:5 * t + len(chunk)] = chunk
    return frames.reshape(n, 1, H, W, 3)


def row(x, y, w, h, tid, cls=0):
    """The box with its top-left corner at (x, y), w x h pixels."""
    return [int(x), int(y), int(x + w - 1), int(y + h - 1), int(tid), int(cls)]


def rows_of(*rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def tiles(hw, bw, bh, x0=0, y0=0, first_id=1):
    """Boxes of bw x bh laid side by side from (x0, y0) over the frame (the last column and row hang over its edge): with PIXEL_KW every
    pixel right of x0 and below y0 is in exactly one or two parts of at most 256 pixels, so one pixel named wrongly changes a share."""
    H, W = hw
    out = []
    for y in range(y0, H, bh):
        for x in range(x0, W, bw):
            out.append(row(x, y, bw, bh, first_id + len(out)))
    return out


# the whole box, upper and lower half, nothing cut off: the parts of tiles() cover every pixel
PIXEL_KW = dict(torso_q8=(0, 128), legs_q8=(128, 256), inset_q8=0, min_w=1, min_h=1, max_cover_q8=256, max_tracks=512)


def scripted_stream(seed, ticks, H, W, big=(20, 40), tiny=(3, 5)):
    """One stream of `ticks` ticks (>= 12): (frames [ticks, H, W, 3], rows[tick]).
    id 1 is parked at the bottom-left corner, in front of everything.  id 2 walks for ticks 0..5 and is gone (an ended track with
    samples), with a duplicate row elsewhere on odd ticks; id 3 is too small to be sampled and is gone after tick 3 (an ended track
    without a sample); id 4 enters at tick 6 and leaves through the right edge (clipped, then wholly outside); id 5 stands behind id 1
    and is covered by it; an out-of-bound and an inverted row come along."""
    rng = np.random.default_rng(seed)
    bw, bh = big
    frames = np.stack([texture(rng, H, W) for _ in range(ticks)])
    p2, v2 = rng.integers(0, [W - bw, H - bh - 12]), rng.integers(-4, 5, 2)
    p3 = rng.integers(0, [W - 8, H - 40])
    x4, y4 = W - bw - 14, int(rng.integers(0, H - bh - 12))
    far = (1 << 20) + 1
    rows = []
    for t in range(ticks):
        r = [row(2, H - bh, bw, bh, 1, 1), row(4 + t % 3, H - bh - 3, bw, bh, 5, 0)]
        if t <= 5:
            q = np.clip(p2 + t * v2, 0, [W - bw, H - bh - 12])
            r.append(row(q[0], q[1], bw, bh, 2, 0))
            if t % 2:
                r.append(row(W - bw, 0, bw, bh, 2, 7))                       # the duplicate: never counted
        if t <= 3:
            r.append(row(p3[0] + t, p3[1], tiny[0], tiny[1], 3, 2))
        if t >= 6:
            r.append(row(x4 + 6 * (t - 6), y4, bw, bh, 4, 0))
        if t == 2:
            r += [[far, 0, far + 5, 9, 9, 0], [30, 30, 10, 40, 8, 0]]        # out of bound, inverted
        order = rng.permutation(len(r)) if t % 3 == 2 and not t % 2 else np.arange(len(r))      # (the duplicate stays behind its original)
        rows.append(rows_of(*[r[i] for i in order]))
    return frames, rows


def scripted_case(name, hw, streams, ticks, splits, cap=16, seed=0, big=(20, 40), **kw):
    H, W = hw
    per = [scripted_stream(seed * 100 + s, ticks, H, W, big=big) for s in range(streams)]
    frames = np.stack([p[0] for p in per], axis=1)                           # [ticks, S, H, W, 3]
    rows = [[per[s][1][t] for s in range(streams)] for t in range(ticks)]
    calls = [(np.ascontiguousarray(frames[a:b]), rows[a:b]) for a, b in splits]
    return dict(name=name, hw=hw, streams=streams, kw=kw, cap=cap, calls=calls)


def simple_case(name, hw, kw, cap, ticks, seed=0, frames=None):
    """ticks = [[rows of stream 0, rows of stream 1, ...] per tick] over noise frames (or `frames`), one call."""
    rng = np.random.default_rng(seed)
    S = len(ticks[0])
    if frames is None:
        frames = np.stack([np.stack([texture(rng, *hw) for _ in range(S)]) for _ in ticks]) if ticks else np.zeros((0, S) + tuple(hw) + (3,), np.uint8)
    return dict(name=name, hw=hw, streams=S, kw=kw, cap=cap, calls=[(frames, [[rows_of(*r) for r in tick] for tick in ticks])])


def planted_scene(hw=(96, 128), ticks=12, seed=21):
    """(frames [ticks, 1, H, W, 3], rows[tick][0]): id 7 in a red torso over blue legs walks to the right over a gray-noise background;
    on the odd ticks a nearer box (id 8, its feet lower) stands in front of it."""
    H, W = hw
    rng = np.random.default_rng(seed)
    g = rng.integers(90, 170, (ticks, 1, H, W, 1))
    frames = np.clip(g + rng.integers(-6, 7, (ticks, 1, H, W, 3)), 0, 255).astype(np.uint8)
    rows = []
    bw, bh = 24, 64
    for t in range(ticks):
        x, y = 6 + 7 * t, 10 + t % 3
        f = frames[t, 0]
        f[y + 8:y + 34, x:x + bw] = np.array([20, 25, 200]) + rng.integers(-15, 16, (26, bw, 3))                 # the jacket
        f[y + 34:y + bh, x:x + bw] = np.array([190, 60, 25]) + rng.integers(-15, 16, (bh - 34, bw, 3))           # the trousers
        r = [row(x, y, bw, bh, 7)]
        if t % 2:
            r.append(row(x - 4, y + 6, bw + 8, bh, 8))
        rows.append([rows_of(*r)])
    return frames, rows


def _cases():
    small = dict(forget_after=2)
    out = [scripted_case("scripted 72x101, two calls", (72, 101), 2, 13, [(0, 5), (5, 13)], seed=1, max_tracks=8, **small),
           scripted_case("scripted 96x128, defaults but the table", (96, 128), 1, 12, [(0, 12)], seed=2, max_tracks=6, forget_after=2, max_cover_q8=200)]
    # four tracks vanish together and only one final fits per call: deferral
    four = [row(2 + 24 * i, 4, 20, 40, 10 + i) for i in range(4)]
    out.append(simple_case("deferral at cap 1", (72, 101), dict(max_tracks=8, **small), 1, [[four], [[]], [[]], [[]], [[]]], seed=3))
    # three ids for two slots: the stream stops at tick 1, the other stream goes on
    a, b, c = row(2, 4, 20, 40, 1), row(30, 4, 20, 40, 2), row(60, 4, 20, 40, 3)
    out.append(simple_case("capacity stop", (72, 101), dict(max_tracks=2, **small), 4, [[[a, b], [a]], [[a, b, c], [a, b]], [[a], [a]]], seed=4))
    # forget_after 0: id 1 expires at tick 1, is emitted there, and id 2 takes its slot in the same call
    out.append(simple_case("slot reused within a call", (72, 101), dict(max_tracks=4, forget_after=0), 4, [[[a]], [[b]], [[b, c]]], seed=5))
    return out


CASES = _cases()


def oracles_for(case):
    return [CO.ColoursOracle(case["hw"], stream=s, **case["kw"]) for s in range(case["streams"])]


def run_oracle(case):
    """([packed result per call], oracles)."""
    oracles = oracles_for(case)
    return [CO.run_bank(oracles, frames, rows, case["cap"]) for frames, rows in case["calls"]], oracles
