"""NumPy specification of the camera-motion estimator (TEST INFRASTRUCTURE): ``csrc/kernels_gmc.hip`` reproduces it bit for bit.

``estimate(prev_bgr, cur_bgr, boxes_xyxy_cur, s=4) -> (warp fp32[2, 3], stats)``.  The warp maps previous-frame pixel coordinates to
current-frame ones (the convention of ``BoTSORT.update(warp=)``); rows are ``r00 r01 t0 / r10 r11 t1``.  Upstream BoT-SORT estimates
this affine with OpenCV (sparse optical flow or ORB + RANSAC): neither deterministic nor a device path.  Here every step up to the sums
of the fit is integer, so no result depends on the order of a parallel sum; a short fp64 sequence with a stated order follows.

1. Gray level: ``g = (sum over the s x s cell of 29 B + 150 G + 77 R) >> (8 + 2 log2 s)``, s in {2, 4}; size (H // s, W // s).
2. Blocks: 16 x 16 gray pixels, origins ``(R + 16 i, R + 16 j)``, R = 8, while the 32 x 32 search window stays inside the level.
3. A block is skipped when its rectangle in frame pixels ``[s x0, s (x0 + 16)) x [s y0, s (y0 + 16))`` intersects a detection box of
   the current frame (``x1 < bx1 and x2 > bx0 and y1 < by1 and y2 > by0``, fp32), or when the texture of the previous level over the
   block, ``sum |g[y, x+1] - g[y, x]| + |g[y+1, x] - g[y, x]|`` (512 differences), is below TEX_MIN = 256: under a mean of half a level
   per difference the truncation of step 1 (up to one level) decides the SAD surface, not the scene.  A flat block has texture 0.
4. SAD of the previous block against the current level at every (dy, dx) in [-8, 8]^2; the minimum wins, ties go to the first in
   (dy, dx) order (index ``17 (dy + 8) + dx + 8``).  A minimum with |dy| = 8 or |dx| = 8 discards the block.
5. Sub-pixel step per axis in 1/16 gray pixel from the SADs m, z, p around the minimum (equiangular fit): ``den = max(m, p) - z``;
   0 if ``den <= 0`` or ``z == 0``, else ``sign(m - p) * ((8 |m - p|) // den)``.  (z = 0 is an exact match: the fit would still move
   it by the asymmetry of the two slopes, and a pan by whole gray pixels would no longer be estimated exactly.)
6. Similarity ``[[a, -b, tx], [b, a, ty]]`` in 1/16 gray pixel; block centre ``p = (16 x0 + 120, 16 y0 + 120)``, ``q = p + d``.
   Fewer than ``min_inliers`` (8) kept blocks: fail.  Start set: the kept blocks within 64 (L-infinity) of the per-axis lower median
   displacement ``sorted[(n - 1) // 2]``.  Three rounds, each: n = |inliers| (n < min_inliers: fail); int64 sums Spx Spy Sqx Sqy,
   Spp = sum |p|^2, Sd = sum p.q, Sc = sum p x q; the exact integers ``V = n Spp - Spx^2 - Spy^2``, ``D = n Sd - Spx Sqx - Spy Sqy``,
   ``C = n Sc - (Spx Sqy - Spy Sqx)`` (V <= 0: fail); then in fp64, one rounding per operation, no fused multiply-add:
       a = D / V;  b = C / V;  mpx = Spx / n; mpy = Spy / n; mqx = Sqx / n; mqy = Sqy / n
       tx = mqx - (a * mpx - b * mpy);  ty = mqy - (b * mpx + a * mpy)
   After rounds one and two the inliers are recomputed over ALL kept blocks:
       rx = ((a * px - b * py) + tx) - qx;  ry = ((b * px + a * py) + ty) - qy;  inlier iff max(|rx|, |ry|) <= 16.
   The third round's fit is the result.  A failure, or no predecessor, gives the identity and ``ok = 0``.
7. To frame pixels, ``X = s u / 16 + c`` with ``c = (s - 1) / 2`` (pixel centres), ``k = s / 16``:
       t0 = (((tx * k) + c) - a * c) + b * c;   t1 = (((ty * k) + c) - b * c) - a * c
   and ``[a, -b, t0, b, a, t1]`` is rounded to fp32 once.
8. stats: ``ok, blocks, kept, inliers`` (what the device reports, int32[4]) and, oracle only, ``masked, flat, border`` (blocks each
   rule of steps 3 and 4 removed), ``start`` (size of the start set: ``start < kept`` = the median gate removed blocks;
   ``inliers < start`` = the residual gate did), ``rounds`` (fits completed) and ``degenerate`` (1: the fit stopped on ``V <= 0``,
   which needs fewer than two distinct block centres, i.e. ``min_inliers = 1``).

Working range: the start gate of 4 gray pixels around the median bounds the spread of the displacement field over the frame, i.e.
about 1.4 degrees of rotation or 2.5 % of zoom per frame at 640 x 360 (the spread is half the diagonal times the angle / the zoom),
and the translation must stay inside the search, |d| < 8 s frame pixels.  Beyond either the result is the identity with ok = 0.
"""
from __future__ import annotations

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

R = 8                 # search radius and grid origin (gray pixels)
B = 16                # block side
TEX_MIN = 256
START_GATE = 64       # 1/16 gray pixel
INLIER_GATE = 16.0
MIN_INLIERS = 8
IDENTITY = np.array([[1, 0, 0], [0, 1, 0]], dtype=np.float32)


def gray_level(bgr, s=4):
    """uint8 [H // s, W // s]."""
    assert s in (2, 4)
    bgr = np.asarray(bgr)
    h, w = bgr.shape[0] // s, bgr.shape[1] // s
    v = bgr[:h * s, :w * s].astype(np.int64)
    y = 29 * v[..., 0] + 150 * v[..., 1] + 77 * v[..., 2]
    y = y.reshape(h, s, w, s).sum(axis=(1, 3))
    return (y >> (8 + 2 * (s.bit_length() - 1))).astype(np.uint8)


def grid(gh, gw):
    """Block counts (nby, nbx)."""
    nby = (gh - 2 * B) // B + 1 if gh >= 2 * B else 0
    nbx = (gw - 2 * B) // B + 1 if gw >= 2 * B else 0
    return nby, nbx


def _step(m, z, p):
    den = max(m, p) - z
    if den <= 0 or z == 0:
        return 0
    d = m - p
    q = (8 * abs(d)) // den
    return q if d > 0 else -q


def match_blocks(gp, gc, boxes, s):
    """Steps 2-5.  Returns (px, py, dx, dy int64 arrays of the kept blocks in grid order, counts dict)."""
    gh, gw = gp.shape
    nby, nbx = grid(gh, gw)
    boxes = np.zeros((0, 4), np.float32) if boxes is None else np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    gpi, gci = gp.astype(np.int64), gc.astype(np.int64)
    cnt = dict(blocks=nby * nbx, masked=0, flat=0, border=0)
    out = []
    for j in range(nby):
        for i in range(nbx):
            x0, y0 = R + B * i, R + B * j
            bx0, by0, bx1, by1 = (np.float32(v) for v in (s * x0, s * y0, s * (x0 + B), s * (y0 + B)))
            if len(boxes) and np.any((boxes[:, 0] < bx1) & (boxes[:, 2] > bx0) & (boxes[:, 1] < by1) & (boxes[:, 3] > by0)):
                cnt["masked"] += 1
                continue
            t = gpi[y0:y0 + B + 1, x0:x0 + B + 1]
            tex = int(np.abs(t[:B, 1:] - t[:B, :B]).sum() + np.abs(t[1:, :B] - t[:B, :B]).sum())
            if tex < TEX_MIN:
                cnt["flat"] += 1
                continue
            win = sliding_window_view(gci[y0 - R:y0 + B + R, x0 - R:x0 + B + R], (B, B))     # [17, 17, 16, 16]
            sad = np.abs(win - gpi[y0:y0 + B, x0:x0 + B]).sum(axis=(2, 3))
            k = int(np.argmin(sad))                                # first minimum in (dy, dx) order
            ky, kx = divmod(k, 2 * R + 1)
            if ky in (0, 2 * R) or kx in (0, 2 * R):
                cnt["border"] += 1
                continue
            z = int(sad[ky, kx])
            sx = _step(int(sad[ky, kx - 1]), z, int(sad[ky, kx + 1]))
            sy = _step(int(sad[ky - 1, kx]), z, int(sad[ky + 1, kx]))
            out.append((16 * x0 + 120, 16 * y0 + 120, 16 * (kx - R) + sx, 16 * (ky - R) + sy))
    a = np.array(out, dtype=np.int64).reshape(-1, 4)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], cnt


def fit_similarity(px, py, dx, dy, min_inliers=MIN_INLIERS):
    """Step 6.  Returns (ok, (a, b, tx, ty) fp64, inliers, rounds)."""
    return _fit(px, py, dx, dy, min_inliers, {})


def _fit(px, py, dx, dy, min_inliers, info):
    kept = len(px)
    info.update(start=0, degenerate=0)
    if kept < min_inliers:
        return 0, None, 0, 0
    mx, my = np.sort(dx)[(kept - 1) // 2], np.sort(dy)[(kept - 1) // 2]
    inl = (np.abs(dx - mx) <= START_GATE) & (np.abs(dy - my) <= START_GATE)
    qx, qy = px + dx, py + dy
    info["start"] = int(inl.sum())
    n = 0
    for rnd in range(3):
        n = int(inl.sum())
        if n < min_inliers:
            return 0, None, n, rnd
        P, Q, U, W = (int(v[inl].sum()) for v in (px, py, qx, qy))
        spp = int((px[inl] * px[inl] + py[inl] * py[inl]).sum())
        sd = int((px[inl] * qx[inl] + py[inl] * qy[inl]).sum())
        sc = int((px[inl] * qy[inl] - py[inl] * qx[inl]).sum())
        V = n * spp - P * P - Q * Q
        D = n * sd - P * U - Q * W
        C = n * sc - (P * W - Q * U)
        assert max(abs(V), abs(D), abs(C)) < 2 ** 62
        if V <= 0:
            info["degenerate"] = 1
            return 0, None, n, rnd
        f = np.float64
        a, b = f(D) / f(V), f(C) / f(V)
        mpx, mpy, mqx, mqy = f(P) / f(n), f(Q) / f(n), f(U) / f(n), f(W) / f(n)
        tx = mqx - (a * mpx - b * mpy)
        ty = mqy - (b * mpx + a * mpy)
        if rnd < 2:
            fx, fy = px.astype(f), py.astype(f)
            rx = ((a * fx - b * fy) + tx) - qx.astype(f)
            ry = ((b * fx + a * fy) + ty) - qy.astype(f)
            inl = np.maximum(np.abs(rx), np.abs(ry)) <= INLIER_GATE
    return 1, (a, b, tx, ty), n, 3


def to_frame(a, b, tx, ty, s):
    """Step 7."""
    f = np.float64
    k, c = f(s) / f(16), f(s - 1) / f(2)
    t0 = (((tx * k) + c) - a * c) + b * c
    t1 = (((ty * k) + c) - b * c) - a * c
    return np.array([[a, -b, t0], [b, a, t1]], dtype=np.float64).astype(np.float32)


def estimate_gray(gp, gc, boxes, s=4, min_inliers=MIN_INLIERS):
    """estimate() on two gray levels (gp None: no predecessor)."""
    nby, nbx = grid(*gc.shape)
    stats = dict(ok=0, blocks=nby * nbx, kept=0, inliers=0, masked=0, flat=0, border=0, rounds=0, start=0, degenerate=0)
    if gp is None:
        return IDENTITY.copy(), stats
    px, py, dx, dy, cnt = match_blocks(gp, gc, boxes, s)
    stats.update(cnt, kept=len(px))
    info = {}
    ok, sim, n, rounds = _fit(px, py, dx, dy, min_inliers, info)
    stats.update(info, ok=ok, inliers=n, rounds=rounds)
    return (to_frame(*sim, s) if ok else IDENTITY.copy()), stats


def estimate(prev_bgr, cur_bgr, boxes_xyxy_cur=None, s=4, min_inliers=MIN_INLIERS):
    gp = None if prev_bgr is None else gray_level(prev_bgr, s)
    return estimate_gray(gp, gray_level(cur_bgr, s), boxes_xyxy_cur, s, min_inliers)


def stats4(st):
    """What the device reports per frame."""
    return np.array([st["ok"], st["blocks"], st["kept"], st["inliers"]], dtype=np.int32)


class Stream:
    """The estimator over a stream: keeps the previous gray level, as the device object does."""

    def __init__(self, s=4, min_inliers=MIN_INLIERS):
        self.s, self.min_inliers, self.prev = s, min_inliers, None

    def reset(self):
        self.prev = None

    def apply(self, frame_bgr, boxes_xyxy=None):
        g = gray_level(frame_bgr, self.s)
        w, st = estimate_gray(self.prev, g, boxes_xyxy, self.s, self.min_inliers)
        self.prev = g
        return w, st


def corner_error(w, true, height, width):
    """Largest distance (px) between the images of the four frame corners under two 2x3 affines."""
    c = np.array([[0, 0, 1], [width - 1, 0, 1], [0, height - 1, 1], [width - 1, height - 1, 1]], dtype=np.float64)
    d = c @ np.asarray(w, np.float64).T - c @ np.asarray(true, np.float64).T
    return float(np.sqrt((d * d).sum(1)).max())
