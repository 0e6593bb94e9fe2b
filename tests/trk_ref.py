"""DeepSORT association costs in float64, and the planted inputs that make every gallery row count.  Plain NumPy, nothing from the
package under test.  Made for checking trk_assoc_all_kernel, cosine_min_mfma_kernel and trk_epoch_prep_kernel cell by cell through
TrackerCore.import_state / last_costs and aic_appearance_cost; tests/test_trk_ref.py checks on the CPU that this reference reproduces
the fixtures the real reference wrote (tests/golden/costs.npz, kf.npz, kf_dt.npz) and that the builders deliver the conditions such
device tests lean on.

Reference (all float64 on the fp32 inputs as given):
  predict64      F P F^T + Q(h), x <- F x                               kalman_filter.py:85-120
  project64      S = H P H^T + R(h)                                     kalman_filter.py:122-151
  maha64         d^T S^-1 d, solved by numpy.linalg.solve               kalman_filter.py:206-249
  update64       K = P H^T S^-1, x + K d, P - K S K^T                   kalman_filter.py:153-204
  iou_cost64     1 - IoU of mean_to_tlwh64(mean) against the detections matching.py:13-106, track.py:133-151
  app64          min over live gallery rows of max(0, 1 - <g/max(|g|,1e-7), d/max(|d|,1e-7)>), 1e5 for an empty gallery or a
                 featureless detection; also the minimising row and the gap to the runner-up       matching.py:109-217

Planted galleries (plant()).  One track per gallery length in GLENS: the edges of the 16-row MFMA tile, of the 64-row block of
cosine_min_mfma_kernel's grid.y, of the 7 x 16-row batch of trk_epoch_prep_kernel and of the 128-row step of trk_assoc_all_kernel, up to
the budget of 130.  Rows and detection features are Gaussian vectors scaled by factors in 0.1 .. 5.  For every detection j and track t
the row (j + 7 t) mod glen[t] is overwritten by detection j's feature plus 20 % noise (cosine distance ~ 0.02, never below 5e-3); a later detection
that lands on the same row wins, so with n >= glen every row ends up as the plant of exactly one detection.  The exceptions: one
all-zero gallery row (ZERO_ROW), one all-zero detection feature (ZERO_DET) and two featureless detections (FEATURELESS), all three
below index 31 so that, at n = 161, the rows they would have planted are planted by the detection one gallery length later.
For dim >= 30 random rows are far from every detection (runner-up >= plant + 0.1), so a dropped, misindexed or stale row moves a
cell by ~0.1 or more; tests/test_trk_ref.py asserts exactly that on this module's output."""
from dataclasses import dataclass

import numpy as np

INFTY = 1e5                                   # linear_assignment.py:9
CHI2_4 = 9.487729036781154                    # kalman_filter.py:16
STD_POS, STD_VEL = 1.0 / 20, 1.0 / 160        # kalman_filter.py:52-53
U = 2.0 ** -24

BUDGET = 130
GLENS = (0, 1, 15, 16, 17, 63, 64, 65, 111, 112, 113, 127, 128, 129, 130)
N_FULL = 161                                  # five 32-detection chunks plus one
ZERO_ROW = (4, 16)                            # (track, row): the glen = 17 track, the one row of its second tile
ZERO_DET = 10
FEATURELESS = (3, 20)
PLANT_NOISE = 0.2
# The scene a tracker is seeded on before the galleries are planted (synthetic.Scene arguments): fifteen people in a 320 x 320 frame.
# Small on purpose: 1 - IoU is checked against float64 with an ABSOLUTE bound of 1e-6, and exact fp32 arithmetic only keeps that where
# one rounding of a corner x + w (2^-24 * 512 = 3e-5 px here, 1.2e-4 px at x > 1024) is small against the box sides; at 1280 x 720 the
# fp32 NumPy restatement itself is 2.3e-6 away from float64.  The crowding also puts more pairs inside the gate and into overlap.
SCENE = dict(seed=11, n_targets=15, jitter=1.0, width=320, height=320, w_range=(40.0, 80.0), h_range=(100.0, 160.0), y_range=(10.0, 150.0))
PLANT_MAX, PLANT_GAP = 0.05, 0.1              # every planted minimum <= PLANT_MAX, its runner-up >= PLANT_GAP above it


# ------------------------------------------------------------------------------------------------------------------ Kalman, fp64
def motion_matrix(dt=1.0):
    f = np.eye(8)
    for i in range(4):
        f[i, 4 + i] = float(np.float32(dt))   # the filter's motion matrix is fp32 (kalman_filter.py:41-44)
    return f


_H = np.eye(4, 8)


def predict64(mean, cov, dt=1.0):
    """mean [..., 8], cov [..., 8, 8] -> the predicted pair in float64."""
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    f = motion_matrix(dt)
    h = m[..., 3]
    one = np.ones_like(h)
    std = np.stack([STD_POS * h, STD_POS * h, 1e-2 * one, STD_POS * h, STD_VEL * h, STD_VEL * h, 1e-5 * one, STD_VEL * h], -1)
    q = std[..., :, None] * std[..., None, :] * np.eye(8)
    return m @ f.T, f @ p @ f.T + q


def project64(mean, cov):
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    h = m[..., 3]
    one = np.ones_like(h)
    std = np.stack([STD_POS * h, STD_POS * h, 1e-1 * one, STD_POS * h], -1)
    r = std[..., :, None] * std[..., None, :] * np.eye(4)
    return m[..., :4], p[..., :4, :4] + r


def maha64(mean, cov, xyah, only_position=False):
    """Squared Mahalanobis distance [T, n] of every measurement to every track's projected state."""
    pm, s = project64(mean, cov)
    z = np.asarray(xyah, np.float64)
    k = 2 if only_position else 4
    out = np.empty((len(pm), len(z)))
    for t in range(len(pm)):
        d = (z[:, :k] - pm[t, :k]).T                              # [k, n]
        try:
            np.linalg.cholesky(s[t, :k, :k])
        except np.linalg.LinAlgError:                             # kalman_filter.py:241-247: S not positive definite (h == 0) rejects everything
            out[t] = np.inf
            continue
        out[t] = np.sum(d * np.linalg.solve(s[t, :k, :k], d), axis=0)
    return out


def update64(mean, cov, z):
    """One track: mean [8], cov [8, 8], z [4] (xyah)."""
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    pm, s = project64(m, p)
    k = np.linalg.solve(s, (p @ _H.T).T).T                         # S is symmetric: K = P H^T S^-1
    return m + k @ (np.asarray(z, np.float64) - pm), p - k @ s @ k.T


# ------------------------------------------------------------------------------------------------------------------ boxes, fp64
def tlwh_to_xyah64(tlwh):
    """detection.py:36-47."""
    b = np.asarray(tlwh, np.float64).reshape(-1, 4)
    a = np.divide(b[:, 2], b[:, 3], out=np.zeros(len(b)), where=b[:, 3] > 0)
    return np.stack([b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2, a, b[:, 3]], 1)


def mean_to_tlwh64(mean):
    """track.py:133-151: w = a h when h > 0 else 0, h clamped at 0."""
    m = np.asarray(mean, np.float64).reshape(-1, 8)
    h = np.maximum(m[:, 3], 0.0)
    w = np.where(m[:, 3] > 0, m[:, 2] * m[:, 3], 0.0)
    return np.stack([m[:, 0] - w / 2, m[:, 1] - h / 2, w, h], 1)


def iou_cost64(trk_tlwh, det_tlwh):
    a, b = np.asarray(trk_tlwh, np.float64).reshape(-1, 1, 4), np.asarray(det_tlwh, np.float64).reshape(1, -1, 4)
    iw = np.maximum(0.0, np.minimum(a[..., 0] + a[..., 2], b[..., 0] + b[..., 2]) - np.maximum(a[..., 0], b[..., 0]))
    ih = np.maximum(0.0, np.minimum(a[..., 1] + a[..., 3], b[..., 1] + b[..., 3]) - np.maximum(a[..., 1], b[..., 1]))
    inter = iw * ih
    union = a[..., 2] * a[..., 3] + b[..., 2] * b[..., 3] - inter
    return 1.0 - inter / np.maximum(union, 1e-7)


def iou_fp32_bound(trk_tlwh, det_tlwh):
    """|fp32 - float64| per cell of 1 - IoU evaluated in fp32 on fp32 boxes (u = 2^-24).
      corners   x + w and y + h round once: u X, u Y with X, Y the largest corner of the pair
      iw, ih    a difference of two corners, rounded: off by 2 u X + u iw and 2 u Y + u ih
      I = iw ih off by dI <= ih 2 u X + iw 2 u Y + 3 u I
      U         the union holds either box, and ih <= both heights, iw <= both widths, so ih / U <= 1 / max(w), iw / U <= 1 / max(h):
                dI / U <= e = 2 u (X / max(w) + Y / max(h)) + 3 u
                U itself: two areas (each <= U) rounded, two sums rounded, and the same dI: dU / U <= e + 8 u
      I / U     <= 1, so it moves by dI / U + dU / U + u (division) <= 2 e + 9 u; the final 1 - x rounds once more."""
    a, b = np.asarray(trk_tlwh, np.float64).reshape(-1, 1, 4), np.asarray(det_tlwh, np.float64).reshape(1, -1, 4)
    x = np.maximum(np.abs(a[..., 0]) + a[..., 2], np.abs(b[..., 0]) + b[..., 2])
    y = np.maximum(np.abs(a[..., 1]) + a[..., 3], np.abs(b[..., 1]) + b[..., 3])
    e = 2 * U * (x / np.maximum(np.maximum(a[..., 2], b[..., 2]), 1e-30) + y / np.maximum(np.maximum(a[..., 3], b[..., 3]), 1e-30)) + 3 * U
    return 2 * e + 10 * U


# ------------------------------------------------------------------------------------------------------------------ appearance, fp64
def unit64(x):
    x = np.asarray(x, np.float64)
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-7)


def app64(galleries, det_feat, has_feat):
    """galleries: list of [glen_t, dim] arrays in FIFO order.  Returns (cost, argmin, gap), each [T, n]: the minimum over the live rows,
    the row that attains it (-1 where the cost is 1e5) and runner-up minus minimum (inf for a one-row gallery)."""
    d = unit64(det_feat)
    has = np.asarray(has_feat).astype(bool)
    t, n = len(galleries), len(d)
    cost, arg, gap = np.full((t, n), INFTY), np.full((t, n), -1, np.int64), np.full((t, n), np.inf)
    for i, g in enumerate(galleries):
        if len(g) == 0:
            continue
        c = np.maximum(0.0, 1.0 - unit64(g) @ d.T)                 # [glen, n]
        order = np.argsort(c, axis=0, kind="stable")
        best = np.take_along_axis(c, order[:1], 0)[0]
        cost[i, has], arg[i, has] = best[has], order[0][has]
        if len(g) > 1:
            gap[i, has] = (np.take_along_axis(c, order[1:2], 0)[0] - best)[has]
    return cost, arg, gap


def split_galleries(flat, glen):
    o = np.concatenate([[0], np.cumsum(glen)])
    return [np.asarray(flat)[o[i]:o[i + 1]] for i in range(len(glen))]


def frame64(mean, cov, galleries, det_tlwh, det_feat, has_feat, predict=True):
    """Everything one frame's association reads, from the state BEFORE predict(): dict of the predicted mean / cov and the three
    [T, n] matrices (+ argmin / gap of the appearance matrix)."""
    m, p = predict64(mean, cov) if predict else (np.asarray(mean, np.float64), np.asarray(cov, np.float64))
    app, arg, gap = app64(galleries, det_feat, has_feat)
    return dict(mean=m, cov=p, maha=maha64(m, p, tlwh_to_xyah64(det_tlwh)), iou=iou_cost64(mean_to_tlwh64(m), det_tlwh), app=app, argmin=arg,
                gap=gap)


def app_bound(dim):
    """|fp32 kernel - fp64| on one cosine distance.  Each unit vector: the sum of squares, the square root and the division put
    (dim/2 + 2) u relative on every element at most (a dim-term sum of non-negative terms in ANY order is within (dim - 1) u, halved
    by the root); the dot product of two vectors of norm <= 1 adds dim roundings of partial sums bounded by sum|a_k b_k| <= 1
    (Cauchy-Schwarz); 1 - dot rounds once more on a value below 2.  (dim + 4) u + dim u + 2 u, rounded up to (2 dim + 8) u."""
    return (2 * dim + 8) * U


# ------------------------------------------------------------------------------------------------------------------ builders
@dataclass
class Case:
    dim: int
    n: int
    glen: np.ndarray          # [T]
    galleries: list           # T arrays [glen_t, dim] fp32
    det_feat: np.ndarray      # [n, dim] fp32
    has_feat: np.ndarray      # [n] uint8
    planted: np.ndarray       # [T, n] bool: cell (t, j) still has its planted row

    @property
    def flat(self):
        return np.concatenate(self.galleries).astype(np.float32) if self.glen.sum() else np.zeros((0, self.dim), np.float32)

    def padded(self, fill=None):
        """[T, BUDGET, dim] for aic_appearance_cost; rows past glen from `fill` ([BUDGET, dim]) or zero."""
        out = np.zeros((len(self.glen), BUDGET, self.dim), np.float32)
        for t, g in enumerate(self.galleries):
            if fill is not None:
                out[t] = fill
            out[t, :len(g)] = g
        return out


def plant(dim, n=N_FULL, seed=0, glens=GLENS):
    rng = np.random.default_rng(1000 * dim + seed)
    det = rng.standard_normal((n, dim)) * rng.uniform(0.1, 5.0, (n, 1))
    has = np.ones(n, np.uint8)
    for j in FEATURELESS:
        if j < n:
            has[j] = 0
    if ZERO_DET < n:
        det[ZERO_DET] = 0.0
    det = det.astype(np.float32)
    glen = np.asarray(glens, np.int32)
    gal, planted = [], np.zeros((len(glen), n), bool)
    for t, g in enumerate(glen):
        rows = rng.standard_normal((g, dim)) * rng.uniform(0.1, 5.0, (g, 1))
        owner = np.full(g, -1)
        for j in range(n):
            if g == 0 or not has[j] or j == ZERO_DET:
                continue
            r = (j + 7 * t) % g
            d = det[j].astype(np.float64)
            rms = np.sqrt(np.mean(d * d))
            rows[r] = (d + PLANT_NOISE * rms * rng.standard_normal(dim)) / rms * rng.uniform(0.1, 5.0)
            owner[r] = j
        if (t, g) == (ZERO_ROW[0], ZERO_ROW[1] + 1):
            rows[ZERO_ROW[1]] = 0.0
            owner[ZERO_ROW[1]] = -1
        planted[t, owner[owner >= 0]] = True
        gal.append(rows.astype(np.float32))
    return Case(dim, n, glen, gal, det, has, planted)


def poison_rows(case):
    """[BUDGET, dim]: exact copies of detection features (distance 0), cycling over the detections that carry a non-zero feature."""
    live = [j for j in range(case.n) if case.has_feat[j] and case.det_feat[j].any()]
    return np.stack([case.det_feat[live[r % len(live)]] for r in range(BUDGET)]).astype(np.float32) if live else np.ones((BUDGET, case.dim), np.float32)


def boxes(mean, cov, n, seed=0):
    """n detection boxes (tlwh fp32) around the PREDICTED boxes of the tracks: detection j belongs to track j mod T, ring j // T; ring 0
    sits on the track (inside the gate, overlapping), each further ring is 0.12 h further out and a little off in size, so that the
    Mahalanobis gate and the IoU overlap both have both outcomes."""
    rng = np.random.default_rng(77 + seed)
    m, _ = predict64(mean, cov)
    t = len(m)
    out = np.empty((n, 4), np.float32)
    for j in range(n):
        i, k = j % t, j // t
        cx, cy, a, h = m[i, :4]
        th = rng.uniform(0, 2 * np.pi)
        r = (0.01 + 0.12 * k) * h
        cx, cy = cx + r * np.cos(th), cy + r * np.sin(th)
        h2 = h * (1 + 0.01 * k * rng.uniform(-1, 1))
        w2 = a * h2 * (1 + 0.01 * k * rng.uniform(-1, 1))
        out[j] = (cx - w2 / 2, cy - h2 / 2, w2, h2)
    return out


def state_dict(exported, case, galleries=None):
    """The dict TrackerCore.import_state takes: integer fields, mean and cov of `exported` (export_arrays() of a real run), galleries of
    `case` (or `galleries`: [T * BUDGET, dim], all full -- the poison state)."""
    st = {k: np.array(v) for k, v in exported.items()}
    t = len(st["track_id"])
    assert t == len(case.glen)
    if galleries is None:
        st["gallery_len"], st["galleries"] = case.glen.copy(), case.flat
    else:
        st["gallery_len"], st["galleries"] = np.full(t, BUDGET, np.int32), np.asarray(galleries, np.float32)
    st["dim"], st["next_track_id"] = case.dim, int(st["track_id"].max()) + 1
    return st


def seed_frames(scene, frames=5):
    """tlwh fp32 [N, 4], conf, class ids of the scene's first frames: what the seed run of a tracker is fed (no features: the
    galleries are planted afterwards)."""
    out = []
    for f in range(frames):
        b, conf, cls, _ = scene.detections(f)
        out.append((np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float32), conf, cls))
    return out


def follow_up(galleries, n, frame, dim):
    """Detection features of a LATER frame of the three-frame device test, from the galleries exported before it (FIFO order): detection
    j looks like a row of track j mod T -- the NEWEST row for j < T (after an eviction it sits where the ring's head was), the OLDEST for
    T <= j < 2 T (the ring's head itself), any row beyond -- so a ring read that does not wrap shows.  One featureless detection."""
    rng = np.random.default_rng(5000 + 10 * dim + frame)
    t = len(galleries)
    feat = (rng.standard_normal((n, dim)) * rng.uniform(0.1, 5.0, (n, 1)))
    for j in range(n):
        g = np.asarray(galleries[j % t], np.float64)
        if len(g) == 0:
            continue
        r = len(g) - 1 if j < t else 0 if j < 2 * t else (37 * j + 11 * frame) % len(g)
        rms = max(np.sqrt(np.mean(g[r] * g[r])), 1e-30)
        feat[j] = (g[r] + PLANT_NOISE * rms * rng.standard_normal(dim)) / rms * rng.uniform(0.1, 5.0)
    has = np.ones(n, np.uint8)
    if n > 5:
        has[5] = 0
    return feat.astype(np.float32), has


def own_rows(case, ident_feat):
    """The case with row glen // 2 of every gallery replaced by the track's own identity feature (scaled): detections that carry
    identity features then match by appearance, and the row outlives sixteen evictions of a full gallery."""
    rng = np.random.default_rng(99)
    gal = [g.copy() for g in case.galleries]
    for t, g in enumerate(gal):
        if len(g):
            g[len(g) // 2] = ident_feat[t] * np.float32(rng.uniform(0.1, 5.0))
    return Case(case.dim, case.n, case.glen, gal, case.det_feat, case.has_feat, np.zeros_like(case.planted))
