"""Geometry and seeded scenes shared by tests/test_zones_oracle.py (are they non-vacuous?) and tests/test_gpu_zones.py (does the device
agree?).  Everything is integer pixels; a scene is frames[s] = list of rows [n, 6] int32 per stream."""
import numpy as np

import zones_oracle as ZO

SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10)]
TRIANGLE = [(20, 20), (180, 40), (90, 170)]
ELL = [(0, 0), (120, 0), (120, 50), (50, 50), (50, 160), (0, 160)]             # concave
LINES = [((100, -20), (100, 220)), ((0, 200), (200, 0))]


def star32(cx=100, cy=100, r_out=90, r_in=35):
    """A 32-vertex concave polygon: 16 spikes on an integer grid."""
    pts = []
    for i in range(32):
        r = r_out if i % 2 == 0 else r_in
        a = 2 * np.pi * i / 32
        pts.append((int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))))
    return pts


def box(px, py, w=1, h=4):
    """A box whose bottom-centre anchor is exactly (px, py)."""
    return [px - w, py - h, px + w, py]


def rows_at(points, ids=None, cls=0):
    """rows [n, 6] with bottom anchors at `points`; ids default 1.."""
    ids = ids if ids is not None else range(1, len(points) + 1)
    return np.array([box(x, y) + [i, cls] for (x, y), i in zip(points, ids)], np.int32).reshape(-1, 6)


def walkers(seed, n_frames, n_ids, gap_max, span=(-30, 230), speed=18):
    """One stream of random walkers bouncing through `span`, each hidden for random stretches of up to gap_max frames, rows shuffled
    per frame, a duplicate row of an id now and then (at another place: only the first may count)."""
    rng = np.random.default_rng(seed)
    lo, hi = span
    pos = rng.integers(lo, hi, (n_ids, 2)).astype(np.int64)
    vel = rng.integers(-speed, speed + 1, (n_ids, 2)).astype(np.int64)
    ids = rng.choice(np.arange(1, 10 * n_ids + 10), n_ids, replace=False)
    hidden = np.zeros(n_ids, np.int64)
    frames = []
    for _ in range(n_frames):
        pos += vel
        for d in range(2):
            out = (pos[:, d] < lo) | (pos[:, d] > hi)
            vel[out, d] *= -1
            pos[:, d] = np.clip(pos[:, d], lo, hi)
        start = (hidden == 0) & (rng.random(n_ids) < 0.08)
        hidden[start] = rng.integers(1, gap_max + 1, int(start.sum()))
        vis = np.nonzero(hidden == 0)[0]
        hidden[hidden > 0] -= 1
        rows = [box(int(pos[i, 0]), int(pos[i, 1]), 3, 12) + [int(ids[i]), int(ids[i]) % 3] for i in vis]
        if len(vis) and rng.random() < 0.3:
            i = int(rng.choice(vis))
            rows.append(box(int(rng.integers(lo, hi)), int(rng.integers(lo, hi)), 3, 12) + [int(ids[i]), 7])
            keep = len(rows) - 1
            p = rng.permutation(len(rows) - 1)                                 # the duplicate stays behind its original
            rows = [rows[j] for j in p] + [rows[keep]]
        else:
            rows = [rows[j] for j in rng.permutation(len(rows))]
        frames.append(np.array(rows, np.int32).reshape(-1, 6))
    return frames


GEOMETRY = [([TRIANGLE, ELL, star32(), [(150, 150), (220, 150), (220, 220), (150, 220)]], LINES),
            ([ELL], LINES[:1]),
            ([star32(60, 60, 50, 20), TRIANGLE], LINES[1:])]


def bank_scene(streams, n_frames, n_ids=6, seed=0, forget_after=3):
    """(geometry[s], frames[s]) for `streams` streams; geometry cycles through GEOMETRY."""
    geo = [GEOMETRY[s % len(GEOMETRY)] for s in range(streams)]
    frames = [walkers(seed * 1000 + s, n_frames, n_ids, forget_after + 3) for s in range(streams)]
    return geo, frames


def oracles_for(geo, **kw):
    return [ZO.ZonesOracle(z, l, **kw) for z, l in geo]


def kinds_seen(events):
    """{(kind, sign of value for CROSS else 0)} over an events array [F, cap, 8] with n_events honoured by zero rows."""
    ev = events.reshape(-1, 8)
    ev = ev[ev[:, 0] != 0]
    return {(int(k), int(np.sign(v)) if k == ZO.CROSS else 0) for k, v in zip(ev[:, 0], ev[:, 5])}


ALL_KINDS = {(ZO.ENTER, 0), (ZO.EXIT, 0), (ZO.LOST, 0), (ZO.CROSS, 1), (ZO.CROSS, -1)}
