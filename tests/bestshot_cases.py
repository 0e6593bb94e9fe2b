"""Frames and seeded scenes shared by tests/test_bestshot_oracle.py (are they non-vacuous?) and tests/test_gpu_bestshot.py (does the
device agree?).  A case is dict(name, hw, streams, kw, cap, calls): kw = the stage's parameters, calls = [(frames [ticks, S, H, W, 3]
uint8, rows[tick][stream] = [n, 6] int32)] -- one entry per update call."""
import numpy as np

import bestshot_oracle as BO

EMPTY = np.zeros((0, 6), np.int32)


def texture(rng, H, W, blur=0):
    """A noise frame uint8 [H, W, 3]; blur > 0: that many passes of a 3 x 3 box mean (integer, wrapped at the edges)."""
    f = rng.integers(0, 256, (H, W, 3)).astype(np.int64)
    for _ in range(blur):
        f = sum(np.roll(np.roll(f, dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) // 9
    return f.astype(np.uint8)


def row(x, y, w, h, tid, cls=0):
    """The box with its top-left corner at (x, y), w x h pixels."""
    return [int(x), int(y), int(x + w - 1), int(y + h - 1), int(tid), int(cls)]


def rows_of(*rows):
    return np.array(rows, np.int32).reshape(-1, 6)


def scripted_stream(seed, ticks, H, W, big=(20, 30), tiny=(3, 5)):
    """One stream of `ticks` ticks (>= 12): (frames [ticks, H, W, 3], rows[tick]).
    id 1 is parked at the bottom-left corner, in front of everything; ticks 3 and 4 show the SAME sharp frame, the others are blurred: a
    replacement at tick 3, an exact tie at tick 4.  id 2 walks for ticks 0..5 and is gone (an ended track with a shot), with a duplicate
    row elsewhere on odd ticks; id 3 is too small to be a candidate and is gone after tick 3 (an ended track without a shot); id 4
    enters at tick 6 and leaves through the right edge (clipped, then wholly outside); an out-of-bound and an inverted row come along."""
    rng = np.random.default_rng(seed)
    bw, bh = big
    sharp = texture(rng, H, W)
    frames = np.stack([sharp if t in (3, 4) else texture(rng, H, W, blur=1 + t % 2) for t in range(ticks)])
    p2, v2 = rng.integers(0, [W - bw, H - bh - 12]), rng.integers(-4, 5, 2)
    p3 = rng.integers(0, [W - 8, H - 40])
    x4, y4 = W - bw - 14, int(rng.integers(0, H - bh - 12))
    far = (1 << 20) + 1
    rows = []
    for t in range(ticks):
        r = [row(2, H - bh, bw, bh, 1, 1)]
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


def scripted_case(name, hw, streams, ticks, splits, cap=16, seed=0, big=(20, 30), **kw):
    H, W = hw
    per = [scripted_stream(seed * 100 + s, ticks, H, W, big=big) for s in range(streams)]
    frames = np.stack([p[0] for p in per], axis=1)                           # [ticks, S, H, W, 3]
    rows = [[per[s][1][t] for s in range(streams)] for t in range(ticks)]
    calls = [(np.ascontiguousarray(frames[a:b]), rows[a:b]) for a, b in splits]
    return dict(name=name, hw=hw, streams=streams, kw=kw, cap=cap, calls=calls)


def simple_case(name, hw, kw, cap, ticks, seed=0):
    """ticks = [[rows of stream 0, rows of stream 1, ...] per tick] over noise frames, one call."""
    rng = np.random.default_rng(seed)
    S = len(ticks[0])
    frames = np.stack([np.stack([texture(rng, *hw) for _ in range(S)]) for _ in ticks]) if ticks else np.zeros((0, S) + tuple(hw) + (3,), np.uint8)
    return dict(name=name, hw=hw, streams=S, kw=kw, cap=cap, calls=[(frames, [[rows_of(*r) for r in tick] for tick in ticks])])


def _cases():
    small = dict(thumb=(16, 24), forget_after=2, min_w=8, min_h=16)
    out = [scripted_case("scripted 72x101, 16x24 thumbnails, two calls", (72, 101), 2, 13, [(0, 5), (5, 13)], seed=1, max_tracks=8, **small),
           scripted_case("scripted 96x128, 64x128 thumbnails", (96, 128), 1, 12, [(0, 12)], seed=2, max_tracks=6, forget_after=2)]
    # four tracks vanish together and only one final fits per call: deferral
    four = [row(2 + 24 * i, 4, 20, 30, 10 + i) for i in range(4)]
    out.append(simple_case("deferral at cap 1", (72, 101), dict(max_tracks=8, **small), 1, [[four], [[]], [[]], [[]], [[]]], seed=3))
    # three ids for two slots: the stream stops at tick 1, the other stream goes on
    a, b, c = row(2, 4, 20, 30, 1), row(30, 4, 20, 30, 2), row(60, 4, 20, 30, 3)
    out.append(simple_case("capacity stop", (72, 101), dict(max_tracks=2, **small), 4, [[[a, b], [a]], [[a, b, c], [a, b]], [[a], [a]]], seed=4))
    # forget_after 0: id 1 expires at tick 1, is emitted there, and id 2 takes its slot in the same call
    out.append(simple_case("slot reused within a call", (72, 101), dict(max_tracks=4, **dict(small, forget_after=0)), 4, [[[a]], [[b]], [[b, c]]], seed=5))
    return out


CASES = _cases()


def oracles_for(case):
    return [BO.BestShotOracle(case["hw"], stream=s, **case["kw"]) for s in range(case["streams"])]


def run_oracle(case):
    """([packed result per call], oracles)."""
    oracles = oracles_for(case)
    return [BO.run_bank(oracles, frames, rows, case["cap"]) for frames, rows in case["calls"]], oracles
