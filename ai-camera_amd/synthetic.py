"""Deterministic synthetic workload.

The reference ships no weights and its only clip cannot be decoded here, so the
benchmark and the parity tests drive the hot path with seeded scenes:

* ``Scene`` -- `n` rectangles ("persons") moving with constant velocity and
  reflecting at the frame borders; optional detection gaps (occlusion), late
  births, per-frame jitter and shuffled detection order.  It yields, per frame,
  the planted boxes (xyxy, fp32), confidences, class ids and identity labels.
* ``Scene.render`` -- `uint8[H,W,3]` BGR frames: uniform-noise background,
  regenerated per 16-frame block, each rectangle filled with its identity's
  fixed 8x8 tile pattern.
* ``identity_features`` -- unit-norm appearance vectors per identity with small
  per-frame noise, for tracker-only tests (no ReID net involved).

Pure NumPy (PCG64), no GPU, no reference code: the same seed gives the same
bytes in the build container and on the GPU box.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

PERSON_CLASS_ID = 0  # 'person' in the COCO table of src/config.py:36


@dataclass
class Scene:
    seed: int = 0
    n_targets: int = 30
    width: int = 1280
    height: int = 720
    w_range: tuple = (40.0, 80.0)
    h_range: tuple = (120.0, 200.0)
    y_range: tuple = (50.0, 500.0)
    speed: float = 3.0
    jitter: float = 0.0           # per-frame uniform box noise (px)
    gaps: list = field(default_factory=list)   # (target, first_frame, last_frame) not detected
    births: dict = field(default_factory=dict)  # target -> first frame it exists
    shuffle: bool = False         # shuffle detection order per frame
    conf_range: tuple = (0.5, 0.95)

    def __post_init__(self):
        rng = np.random.default_rng(self.seed)
        n = self.n_targets
        self.w = rng.uniform(*self.w_range, n).astype(np.float32)
        self.h = rng.uniform(*self.h_range, n).astype(np.float32)
        self.x0 = (50.0 + rng.uniform(0, 1, n) * (self.width - 130.0 - self.w)).astype(np.float32)
        self.y0 = rng.uniform(*self.y_range, n).astype(np.float32)
        self.y0 = np.minimum(self.y0, self.height - self.h - 1).astype(np.float32)
        self.vx = rng.uniform(-self.speed, self.speed, n).astype(np.float32)
        self.vy = rng.uniform(-self.speed, self.speed, n).astype(np.float32)
        self.tiles = rng.integers(0, 256, (n, 8, 8, 3), dtype=np.uint8)
        self._gap = {}
        for t, a, b in self.gaps:
            self._gap.setdefault(int(t), []).append((int(a), int(b)))

    # -- geometry ---------------------------------------------------------------------
    @staticmethod
    def _reflect(p, lo, hi):
        """Position of a point bouncing in [lo, hi] after unfolding (vectorised)."""
        span = np.maximum(hi - lo, 1e-3)
        q = np.mod(p - lo, 2 * span)
        return lo + np.where(q > span, 2 * span - q, q)

    def boxes_at(self, frame: int) -> np.ndarray:
        """All `n` target boxes (xyxy fp32) at `frame`, whether detected or not."""
        f = np.float32(frame)
        x = self._reflect(self.x0 + self.vx * f, 0.0, self.width - self.w)
        y = self._reflect(self.y0 + self.vy * f, 0.0, self.height - self.h)
        return np.stack([x, y, x + self.w, y + self.h], axis=1).astype(np.float32)

    def visible(self, frame: int) -> np.ndarray:
        vis = np.ones(self.n_targets, dtype=bool)
        for t, first in self.births.items():
            if frame < first:
                vis[int(t)] = False
        for t, spans in self._gap.items():
            for a, b in spans:
                if a <= frame <= b:
                    vis[t] = False
        return vis

    def detections(self, frame: int):
        """(boxes_xyxy fp32 [N,4], conf fp32 [N], class_ids int32 [N], identity int32 [N])."""
        rng = np.random.default_rng((self.seed + 1) * 1_000_003 + frame)
        ids = np.nonzero(self.visible(frame))[0].astype(np.int32)
        b = self.boxes_at(frame)[ids]
        if self.jitter > 0:
            b = b + rng.uniform(-self.jitter, self.jitter, b.shape).astype(np.float32)
        conf = rng.uniform(*self.conf_range, len(ids)).astype(np.float32)
        if self.shuffle:
            p = rng.permutation(len(ids))
            ids, b, conf = ids[p], b[p], conf[p]
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, self.width)
        b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, self.height)
        cls = np.full(len(ids), PERSON_CLASS_ID, dtype=np.int32)
        return b.astype(np.float32), conf, cls, ids

    # -- pixels -----------------------------------------------------------------------
    def background(self, frame: int) -> np.ndarray:
        rng = np.random.default_rng((self.seed + 7) * 7_000_003 + frame // 16)
        return rng.integers(0, 256, (self.height, self.width, 3), dtype=np.uint8)

    def render(self, frame: int, background: np.ndarray | None = None) -> np.ndarray:
        img = (self.background(frame) if background is None else background).copy()
        boxes = self.boxes_at(frame)
        vis = self.visible(frame)
        for t in range(self.n_targets):
            if not vis[t]:
                continue
            x1, y1, x2, y2 = (int(v) for v in boxes[t])
            x1, y1 = max(0, x1), max(0, y1)
            x2, y2 = min(self.width, x2), min(self.height, y2)
            if x2 <= x1 or y2 <= y1:
                continue
            reps = ((y2 - y1 + 7) // 8, (x2 - x1 + 7) // 8, 1)
            img[y1:y2, x1:x2] = np.tile(self.tiles[t], reps)[: y2 - y1, : x2 - x1]
        return img

    def render_batch(self, first: int, count: int) -> np.ndarray:
        out = np.empty((count, self.height, self.width, 3), dtype=np.uint8)
        bg, bg_block = None, None
        for i in range(count):
            f = first + i
            if bg_block != f // 16:
                bg, bg_block = self.background(f), f // 16
            out[i] = self.render(f, bg)
        return out


def identity_features(identities, frame: int, dim: int = 512, seed: int = 0,
                      noise: float = 0.01, normalise: bool = True) -> np.ndarray:
    """fp32 [N,dim] appearance vectors: fixed unit prototype per identity + seeded
    per-component Gaussian noise of sigma `noise` (0.01 at dim 512 -> same-identity
    cosine distance ~0.05, different identities ~1)."""
    identities = np.asarray(identities, dtype=np.int64)
    out = np.empty((len(identities), dim), dtype=np.float32)
    for k, ident in enumerate(identities):
        proto = np.random.default_rng(seed * 7919 + 17 + int(ident)).standard_normal(dim)
        proto /= np.linalg.norm(proto)
        n = np.random.default_rng((seed + 3) * 104_729 + int(ident) * 8191 + frame).standard_normal(dim)
        v = proto + noise * n
        if normalise:
            v = v / np.linalg.norm(v)
        out[k] = v.astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------------------- a moving camera
def _smooth_noise(rng, height, width, cells=(32, 16, 8), amps=(1.0, 0.5, 0.25)):
    """Three octaves of bilinearly interpolated lattice noise, scaled to 0..255 (fp64 [height, width, 3])."""
    out = np.zeros((height, width, 3))
    for cell, amp in zip(cells, amps):
        gh, gw = height // cell + 2, width // cell + 2
        lat = rng.uniform(0.0, 1.0, (gh, gw, 3))
        y, x = np.arange(height) / cell, np.arange(width) / cell
        y0, x0 = y.astype(int), x.astype(int)
        fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
        a, b = lat[y0][:, x0], lat[y0][:, x0 + 1]
        c, d = lat[y0 + 1][:, x0], lat[y0 + 1][:, x0 + 1]
        out += amp * ((a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy)
    out -= out.min()
    return out * (255.0 / out.max())


@dataclass
class PanningScene:
    """A camera moving over a fixed world: a seeded smooth texture larger than the frame, sampled under a known similarity per frame.

    A static world point seen at pixel X in frame f - 1 is seen at ``true_warp(f) @ [X, 1]`` in frame f:
    ``zoom * R(rot_deg) (X - centre) + centre + pan``, the same step every frame (its inverse after ``reverse_at``).  Integer pans without rotation or zoom are sampled
    exactly (nearest = a slice of the texture), everything else bilinearly.  Persons are rectangles that move with constant velocity in
    WORLD coordinates (``speed`` 0: they stand still in the world) and carry their own texture patch."""
    seed: int = 0
    width: int = 640
    height: int = 360
    pan: tuple = (8.0, -4.0)       # image motion of the background per frame (px)
    rot_deg: float = 0.0
    zoom: float = 1.0
    n_targets: int = 4
    w_range: tuple = (30.0, 50.0)
    h_range: tuple = (70.0, 110.0)
    speed: float = 0.0
    tiled: bool = False            # persons filled with a fixed 8x8 tile pattern, as Scene's (what the trained detector knows)
    reverse_at: int = -1           # >= 0: the camera sweeps back (the inverse step) for every frame after this one
    pad: int = 512                 # texture margin around frame 0 on every side
    gaps: list = field(default_factory=list)   # (target, first_frame, last_frame) not detected
    conf_range: tuple = (0.8, 0.95)

    def __post_init__(self):
        rng = np.random.default_rng(self.seed)
        self.texture = np.floor(_smooth_noise(rng, self.height + 2 * self.pad, self.width + 2 * self.pad) + 0.5).astype(np.uint8)
        n = self.n_targets
        self.w = rng.uniform(*self.w_range, n).astype(np.float32)
        self.h = rng.uniform(*self.h_range, n).astype(np.float32)
        self.x0 = rng.uniform(0.05 * self.width, 0.95 * self.width - self.w).astype(np.float32)     # world = frame 0 coordinates
        self.y0 = rng.uniform(0.05 * self.height, 0.95 * self.height - self.h).astype(np.float32)
        self.vx = rng.uniform(-self.speed, self.speed, n).astype(np.float32)
        self.vy = rng.uniform(-self.speed, self.speed, n).astype(np.float32)
        self.patches = [np.floor(_smooth_noise(rng, int(np.ceil(h)) + 1, int(np.ceil(w)) + 1, cells=(8, 4, 2)) + 0.5).astype(np.uint8)
                        for w, h in zip(self.w, self.h)]
        if self.tiled:
            self.patches = [np.tile(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), (p.shape[0] // 8 + 1, p.shape[1] // 8 + 1, 1))
                            for p in self.patches]
        th = np.deg2rad(self.rot_deg)
        a, b = self.zoom * np.cos(th), self.zoom * np.sin(th)
        cx, cy = (self.width - 1) / 2.0, (self.height - 1) / 2.0
        self.step = np.array([[a, -b, cx - (a * cx - b * cy) + self.pan[0]], [b, a, cy - (b * cx + a * cy) + self.pan[1]], [0, 0, 1.0]])
        self.integer = self.rot_deg == 0 and self.zoom == 1 and all(float(p).is_integer() for p in self.pan)
        self._gap = {}
        for t, a0, b0 in self.gaps:
            self._gap.setdefault(int(t), []).append((int(a0), int(b0)))

    def true_warp(self, frame: int) -> np.ndarray:
        """fp64 [2, 3]: frame - 1 pixel coordinates -> frame pixel coordinates (the identity for frame 0)."""
        if frame <= 0:
            return np.eye(3)[:2]
        back = 0 <= self.reverse_at < frame
        return (np.linalg.inv(self.step) if back else self.step)[:2].copy()

    def world_to_frame(self, frame: int) -> np.ndarray:
        fwd = frame if self.reverse_at < 0 else min(frame, self.reverse_at)
        return np.linalg.matrix_power(np.linalg.inv(self.step), frame - fwd) @ np.linalg.matrix_power(self.step, fwd)

    def boxes_at(self, frame: int) -> np.ndarray:
        """Person boxes (xyxy fp32) in the pixel coordinates of `frame`: the bounding box of the transformed world rectangle."""
        g = self.world_to_frame(frame)
        x, y = self.x0 + self.vx * np.float32(frame), self.y0 + self.vy * np.float32(frame)
        cs = np.stack([np.stack([x, y]), np.stack([x + self.w, y]), np.stack([x, y + self.h]), np.stack([x + self.w, y + self.h])])   # [4, 2, n]
        p = np.einsum("ij,kjn->kin", g[:2, :2], cs.astype(np.float64)) + g[:2, 2][None, :, None]
        return np.stack([p[:, 0].min(0), p[:, 1].min(0), p[:, 0].max(0), p[:, 1].max(0)], axis=1).astype(np.float32)

    def visible(self, frame: int) -> np.ndarray:
        vis = np.ones(self.n_targets, dtype=bool)
        for t, spans in self._gap.items():
            for a, b in spans:
                if a <= frame <= b:
                    vis[t] = False
        return vis

    def detections(self, frame: int):
        """(boxes_xyxy fp32 [N,4], conf fp32 [N], class_ids int32 [N], identity int32 [N]) as Scene.detections; boxes that leave the
        frame are dropped."""
        rng = np.random.default_rng((self.seed + 1) * 1_000_003 + frame)
        b = self.boxes_at(frame)
        conf = rng.uniform(*self.conf_range, self.n_targets).astype(np.float32)
        inside = (b[:, 0] >= 0) & (b[:, 1] >= 0) & (b[:, 2] <= self.width) & (b[:, 3] <= self.height)
        ids = np.nonzero(self.visible(frame) & inside)[0].astype(np.int32)
        return b[ids], conf[ids], np.full(len(ids), PERSON_CLASS_ID, dtype=np.int32), ids

    def background(self, frame: int) -> np.ndarray:
        g = self.world_to_frame(frame)
        if self.integer:
            ox, oy = self.pad - int(round(g[0, 2])), self.pad - int(round(g[1, 2]))
            if not (0 <= ox <= 2 * self.pad and 0 <= oy <= 2 * self.pad):
                raise ValueError("the camera left the texture (raise pad)")
            return self.texture[oy:oy + self.height, ox:ox + self.width].copy()
        inv = np.linalg.inv(g)
        ys, xs = np.mgrid[0:self.height, 0:self.width].astype(np.float64)
        wx = inv[0, 0] * xs + inv[0, 1] * ys + inv[0, 2] + self.pad
        wy = inv[1, 0] * xs + inv[1, 1] * ys + inv[1, 2] + self.pad
        if wx.min() < 0 or wy.min() < 0 or wx.max() > self.texture.shape[1] - 1 or wy.max() > self.texture.shape[0] - 1:
            raise ValueError("the camera left the texture (raise pad)")
        x0 = np.minimum(wx.astype(int), self.texture.shape[1] - 2)
        y0 = np.minimum(wy.astype(int), self.texture.shape[0] - 2)
        fx, fy = (wx - x0)[..., None], (wy - y0)[..., None]
        t = self.texture.astype(np.float64)
        v = (t[y0, x0] * (1 - fx) + t[y0, x0 + 1] * fx) * (1 - fy) + (t[y0 + 1, x0] * (1 - fx) + t[y0 + 1, x0 + 1] * fx) * fy
        return np.floor(v + 0.5).astype(np.uint8)

    def render(self, frame: int) -> np.ndarray:
        img = self.background(frame)
        boxes = self.boxes_at(frame)
        for t in range(self.n_targets):
            x1, y1, x2, y2 = (int(v) for v in np.floor(boxes[t]))
            cx1, cy1, cx2, cy2 = max(0, x1), max(0, y1), min(self.width, x2), min(self.height, y2)
            if cx2 <= cx1 or cy2 <= cy1:
                continue
            p = self.patches[t]
            yy = np.minimum(np.arange(cy1 - y1, cy2 - y1), p.shape[0] - 1)
            xx = np.minimum(np.arange(cx1 - x1, cx2 - x1), p.shape[1] - 1)
            img[cy1:cy2, cx1:cx2] = p[yy][:, xx]
        return img

    def render_batch(self, first: int, count: int) -> np.ndarray:
        return np.stack([self.render(first + i) for i in range(count)])
