"""NumPy/SciPy restatement of OC-SORT's ``OCSort.update()`` (TEST INFRASTRUCTURE).

Written from the algorithm as published by the OC-SORT authors (``trackers/ocsort_tracker/ocsort.py``: ``KalmanBoxTracker``,
``OCSort.update``, ``k_previous_obs``, ``speed_direction``; ``association.py``: ``associate``; ``kalmanfilter.py``:
``KalmanFilterNew.update / freeze / unfreeze``).  It is the specification the device tracker (``csrc/kernels_ocsort.hip``)
reproduces bit for bit: ids, rows, class, score, every counter AND the Kalman state (the 7x7 filter products below are ordered fp32
sums, the order the kernel uses, so no tolerance is needed).

Deliberate changes from upstream (also in DESIGN.md, section 17):
  1. IoU is this project's (no ``+1`` pixel, union floored at 1e-7, fp32), not ``iou_batch``'s 0/0.
  2. The filter is fp32 with a stated operation order (upstream: fp64 filterpy).  ``inv(S)`` is restated as a 4x4 Cholesky
     factorisation and two triangular solves per gain row (``K_i = S^-1 P[i, :4]``); the Joseph form
     ``(I - KH) P (I - KH)^T + K R K^T`` is kept, each product an ordered sum over the four measured states.
  3. Track ids are counted per tracker from ``first_track_id``.  The class of a track is that of its last matched
     detection (upstream ignores classes).
  4. ``lap.lapjv(extend_cost=True)`` is SciPy's ``linear_sum_assignment`` on the rectangular fp32 matrix (rows = detections,
     columns = tracks, as upstream): same objective, ties by SciPy's rules.
  5. ``arccos`` is a fixed fp32 routine: ``pi/2 - |acos(c)| = asin(c)`` and ``asin32`` below is the single-precision Cephes
     polynomial, a fixed sequence of fp32 multiplies and adds and one square root.  Its largest error against fp64
     ``np.arcsin`` on a grid of 2^21 + 1 points of [-1, 1] is 1.64e-7 (measured by tests/test_ocsort_oracle.py, which asserts 3.28e-7);
     it is odd and non-decreasing on that grid.
  6. "The track has an observation" / "has a velocity" are flags, not upstream's ``last_observation.sum() < 0`` sign test (which
     misfires for a real box with negative coordinates).
  7. The lists of unmatched detections and tracks handed to the BYTE and OCR stages are in ascending order (upstream appends the
     pairs it dropped for IoU below the threshold at the end, a permutation that can only matter for ties).
  8. A track whose predicted box is not finite (NaN or infinite: a zero-area box makes ``h = s / w = 0 / 0``) is dropped right
     after the predict step.  Upstream drops on NaN only (and misaligns its arrays on an infinite one).
  9. Detections arrive as tlwh like everywhere in this project; ``x2 = fp32(x + w)``, ``y2 = fp32(y + h)`` once.
 10. ``lsap_fast = False`` (a test switch, ``aic_ocsort_option``) skips upstream's read-off in stage 1 and sends every problem to the
     LSAP.  The two agree whenever the entries at or below the threshold cannot outweigh a read-off pair (always when the other
     entries are zero); they need NOT agree in general: iou = [[.35, .29], [.29, 0]] reads off (0, 0), the LSAP prefers the
     anti-diagonal (0.58 > 0.35) and the IoU check then drops both pairs.  Both modes are specified here and the device follows each.

Every threshold is rounded to fp32 once and every comparison is made in fp32.

Recording hook (tests/ocsort_edge_cases.py): ``OCSort(record=[])`` appends one dict per non-empty association problem -- frame, stage
("stage1" / "byte" / "ocr"), the IoU matrix, the OCM term (stage 1), the cost matrix, the threshold, how it was solved ("read_off" /
"lsap" / "gate_shut": the BYTE / OCR gate ``max > th`` stayed shut) and the rows' detection indices and columns' track ids.  It
changes no result.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

F32 = np.float32
NEW, OBSERVED, FROZEN = 0, 1, 2                   # filter: never updated / last update was an observation / frozen at the first miss
BYTE_LOW = F32(0.1)                               # ocsort.py: inds_low = scores > 0.1

# ----------------------------------------------------------------------------------------------------------------- asin, fp32
PIO2 = F32(1.5707963267948966)
PI = F32(3.141592653589793)
ASIN_C = tuple(F32(c) for c in (4.2163199048e-2, 2.4181311049e-2, 4.5470025998e-2, 7.4953002686e-2, 1.6666752422e-1))


def asin32(x):
    """asin for fp32 x in [-1, 1] as a fixed sequence of fp32 operations (Cephes asinf), elementwise.
    a = |x|; big = a > 0.5; z = big ? 0.5 * (1 - a) : a * a; t = big ? sqrt(z) : a;
    p = ((((c0 z + c1) z + c2) z + c3) z + c4) z t + t; big: p = pi/2 - (p + p); sign of x."""
    x = np.asarray(x, dtype=F32)
    a = np.abs(x)
    big = a > F32(0.5)
    z = np.where(big, F32(0.5) * (F32(1) - a), a * a).astype(F32)
    t = np.where(big, np.sqrt(z), a).astype(F32)
    p = ASIN_C[0] * z + ASIN_C[1]
    p = p * z + ASIN_C[2]
    p = p * z + ASIN_C[3]
    p = p * z + ASIN_C[4]
    p = (p * z) * t + t
    p = np.where(big, PIO2 - (p + p), p).astype(F32)
    return np.where(x < 0, -p, p).astype(F32)


# ----------------------------------------------------------------------------------------------------------------- boxes
def bbox_to_z(b):
    """convert_bbox_to_z: [x1, y1, x2, y2] -> [x, y, s, r], r = w / (h + 1e-6)."""
    w, h = F32(b[2] - b[0]), F32(b[3] - b[1])
    return np.array([b[0] + w / F32(2), b[1] + h / F32(2), w * h, w / (h + F32(1e-6))], dtype=F32)


def x_to_bbox(x):
    """convert_x_to_bbox: w = sqrt(s * r), h = s / w."""
    with np.errstate(all="ignore"):
        w = np.sqrt(F32(x[2] * x[3]))
        h = F32(x[2] / w)
        return np.array([x[0] - w / F32(2), x[1] - h / F32(2), x[0] + w / F32(2), x[1] + h / F32(2)], dtype=F32)


def iou_matrix(a, b):
    """[len(a), len(b)] fp32 IoU of xyxy boxes: inter / max(area_a + area_b - inter, 1e-7)."""
    a = np.asarray(a, dtype=F32).reshape(-1, 4)
    b = np.asarray(b, dtype=F32).reshape(-1, 4)
    A, B = a[:, None, :], b[None, :, :]
    iw = np.maximum(F32(0), np.minimum(A[..., 2], B[..., 2]) - np.maximum(A[..., 0], B[..., 0]))
    ih = np.maximum(F32(0), np.minimum(A[..., 3], B[..., 3]) - np.maximum(A[..., 1], B[..., 1]))
    inter = iw * ih
    uni = (A[..., 2] - A[..., 0]) * (A[..., 3] - A[..., 1]) + (B[..., 2] - B[..., 0]) * (B[..., 3] - B[..., 1]) - inter
    return (inter / np.maximum(uni, F32(1e-7))).astype(F32)


def speed_direction(b1, b2):
    """Unit direction (dy, dx) from the centre of b1 to the centre of b2."""
    cx1, cy1 = (b1[0] + b1[2]) / F32(2), (b1[1] + b1[3]) / F32(2)
    cx2, cy2 = (b2[0] + b2[2]) / F32(2), (b2[1] + b2[3]) / F32(2)
    dy, dx = F32(cy2 - cy1), F32(cx2 - cx1)
    norm = np.sqrt(F32(dx * dx + dy * dy)) + F32(1e-6)
    return np.array([dy / norm, dx / norm], dtype=F32)


# ----------------------------------------------------------------------------------------------------------------- the filter
R_DIAG = np.array([1, 1, 10, 10], dtype=F32)
Q_DIAG = np.array([1, 1, 1, 1, 0.01, 0.01, 1e-4], dtype=F32)
P0_DIAG = np.array([10, 10, 10, 10, 1e4, 1e4, 1e4], dtype=F32)


def kf7_predict(x, P):
    """x = F x, P = F (P F^T) + Q; every element an ordered fp32 sum."""
    x, P = x.copy(), P.copy()
    x[:3] = x[:3] + x[4:7]
    t1 = P.copy()
    t1[:, :3] = P[:, :3] + P[:, 4:7]
    t2 = t1.copy()
    t2[:3, :] = t1[:3, :] + t1[4:7, :]
    t2[np.arange(7), np.arange(7)] += Q_DIAG
    return x, t2


def _chol4(S):
    L = np.zeros((4, 4), dtype=F32)
    with np.errstate(all="ignore"):
        for j in range(4):
            d = S[j, j]
            for k in range(j):
                d = F32(d - L[j, k] * L[j, k])
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 4):
                s = S[i, j]
                for k in range(j):
                    s = F32(s - L[i, k] * L[j, k])
                L[i, j] = s / L[j, j]
    return L


def _solve4(L, B):
    """Rows of B [n, 4] -> rows of S^-1 b: forward then backward substitution, the order of trk_math.hpp."""
    n = B.shape[0]
    y = np.zeros((n, 4), dtype=F32)
    x = np.zeros((n, 4), dtype=F32)
    with np.errstate(all="ignore"):
        for i in range(4):
            s = B[:, i].copy()
            for k in range(i):
                s = s - L[i, k] * y[:, k]
            y[:, i] = s / L[i, i]
        for i in range(3, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 4):
                s = s - L[k, i] * x[:, k]
            x[:, i] = s / L[i, i]
    return x


def kf7_update(x, P, z):
    """Joseph-form update with measurement z = [x, y, s, r]."""
    with np.errstate(all="ignore"):
        S = P[:4, :4].copy()
        S[np.arange(4), np.arange(4)] += R_DIAG
        K = _solve4(_chol4(S), P[:, :4])                         # [7, 4]
        y = (np.asarray(z, dtype=F32) - x[:4]).astype(F32)
        dot = K[:, 0] * y[0] + K[:, 1] * y[1]
        dot = dot + K[:, 2] * y[2]
        dot = dot + K[:, 3] * y[3]
        xn = (x + dot).astype(F32)

        def ksum(Kr, M):                                          # [7, 4] x [4, m] -> [7, m], ((k0 m0 + k1 m1) + k2 m2) + k3 m3
            acc = Kr[:, 0:1] * M[0:1, :] + Kr[:, 1:2] * M[1:2, :]
            acc = acc + Kr[:, 2:3] * M[2:3, :]
            return acc + Kr[:, 3:4] * M[3:4, :]
        B = P - ksum(K, P[:4, :])                                 # (I - KH) P
        C = B - ksum(B[:, :4], K.T)                               # ... (I - KH)^T:  B[i][j] - sum_b B[i][b] K[j][b]
        Pn = C + ksum(K * R_DIAG[None, :], K.T)                   # + K R K^T
    return xn, Pn.astype(F32)


class KalmanBoxTracker:
    def __init__(self, bbox, score, cls, track_id, delta_t):
        self.x = np.zeros(7, dtype=F32)
        self.x[:4] = bbox_to_z(bbox)
        self.P = np.diag(P0_DIAG).astype(F32)
        self.kstate = NEW
        self.saved = None                                         # (x, P) frozen at the first missed frame
        self.id, self.cls, self.score = track_id, int(cls), F32(score)
        self.age = self.hits = self.hit_streak = self.time_since_update = 0
        self.has_obs = False
        self.last_observation = np.full(4, -1, dtype=F32)
        self.observations = {}
        self.velocity = np.zeros(2, dtype=F32)
        self.has_vel = False
        self.delta_t = delta_t
        self.oru_gap = 0                                          # gap of the last ORU replay (test hook)

    def predict(self):
        if F32(self.x[6] + self.x[2]) <= 0:
            self.x[6] = 0
        self.x, self.P = kf7_predict(self.x, self.P)
        self.age += 1
        if self.time_since_update > 0:
            self.hit_streak = 0
        self.time_since_update += 1
        return x_to_bbox(self.x)

    def previous_obs(self):
        """k_previous_obs(observations, age, delta_t): (box, valid)."""
        if not self.has_obs:
            return np.full(4, -1, dtype=F32), False
        for dt in range(self.delta_t, 0, -1):
            if self.age - dt in self.observations:
                return self.observations[self.age - dt], True
        return self.last_observation, True

    def update(self, bbox, score=None, cls=None, oru=True):
        if bbox is None:
            if self.kstate == OBSERVED:                           # KalmanFilterNew.freeze
                self.saved = (self.x.copy(), self.P.copy())
                self.kstate = FROZEN
            return
        bbox = np.asarray(bbox, dtype=F32)
        if self.has_obs:
            prev, _ = self.previous_obs()
            self.velocity = speed_direction(prev, bbox)
            self.has_vel = True
        if self.kstate == FROZEN and oru:
            self.unfreeze(bbox)
        self.kstate = OBSERVED
        self.last_observation = bbox.copy()
        self.has_obs = True
        self.observations[self.age] = bbox.copy()
        for k in [k for k in self.observations if k <= self.age - self.delta_t]:   # a ring of delta_t ages is all that is ever read
            del self.observations[k]
        self.time_since_update = 0
        self.hits += 1
        self.hit_streak += 1
        self.score, self.cls = F32(score), int(cls)
        self.x, self.P = kf7_update(self.x, self.P, bbox_to_z(bbox))

    def unfreeze(self, bbox):
        """ORU: back to the frozen filter, then `gap` virtual observations on the straight line from the last observation to the
        new one: update, then predict except after the last (KalmanFilterNew.predict: no area-velocity check there)."""
        self.x, self.P = self.saved[0].copy(), self.saved[1].copy()
        gap = self.time_since_update                              # frames from the last observation to this one
        self.oru_gap = gap
        for i, z in enumerate(virtual_boxes(self.last_observation, bbox, gap)):
            self.x, self.P = kf7_update(self.x, self.P, z)
            if i != gap - 1:
                self.x, self.P = kf7_predict(self.x, self.P)


def virtual_boxes(last_box, new_box, gap):
    """The z = [x, y, s, r] of the `gap` virtual observations of unfreeze(): linear in (x, y, w, h) of the two z forms."""
    with np.errstate(all="ignore"):
        x1, y1, s1, r1 = bbox_to_z(last_box)
        x2, y2, s2, r2 = bbox_to_z(new_box)
        w1, h1 = np.sqrt(F32(s1 * r1)), np.sqrt(F32(s1 / r1))
        w2, h2 = np.sqrt(F32(s2 * r2)), np.sqrt(F32(s2 / r2))
        g = F32(gap)
        dx, dy, dw, dh = F32((x2 - x1) / g), F32((y2 - y1) / g), F32((w2 - w1) / g), F32((h2 - h1) / g)
        out = []
        for i in range(gap):
            k = F32(i + 1)
            x, y, w, h = F32(x1 + k * dx), F32(y1 + k * dy), F32(w1 + k * dw), F32(h1 + k * dh)
            out.append(np.array([x, y, w * h, w / h], dtype=F32))
    return out


# ----------------------------------------------------------------------------------------------------------------- association
def linear_assignment(cost):
    """Pairs (row, col) of SciPy's rectangular LSAP on the fp32 matrix (change 4)."""
    r, c = linear_sum_assignment(np.asarray(cost, dtype=F32).astype(np.float64))
    return list(zip(r.tolist(), c.tolist()))


def read_off(iou, thr):
    """Upstream's shortcut: a = iou > thr has at most one entry per row and column (and one at all): the pairs, else None."""
    a = iou > thr
    if a.size and a.sum(1).max() == 1 and a.sum(0).max() == 1:
        return [(int(r), int(c)) for r, c in zip(*np.where(a))]
    return None


def ocm_term(dets, scores, prev, valid, vel, inertia):
    """[N, T] fp32: inertia * valid_t * asin(clip(vel_t . dir(prev_t -> d))) / pi * score_d."""
    d = np.asarray(dets, dtype=F32).reshape(-1, 4)
    p = np.asarray(prev, dtype=F32).reshape(-1, 4)
    v = np.asarray(vel, dtype=F32).reshape(-1, 2)
    dx = ((d[:, 0] + d[:, 2]) / F32(2))[:, None] - ((p[:, 0] + p[:, 2]) / F32(2))[None, :]
    dy = ((d[:, 1] + d[:, 3]) / F32(2))[:, None] - ((p[:, 1] + p[:, 3]) / F32(2))[None, :]
    norm = np.sqrt(dx * dx + dy * dy) + F32(1e-6)
    c = v[None, :, 1] * (dx / norm) + v[None, :, 0] * (dy / norm)
    c = np.minimum(np.maximum(c, F32(-1)), F32(1))
    t = ((asin32(c) / PI) * F32(inertia)) * np.asarray(scores, dtype=F32)[:, None]
    return np.where(np.asarray(valid, dtype=bool)[None, :], t, F32(0)).astype(F32)


def associate(dets, scores, trks, thr, vel, prev, valid, inertia, lsap_fast=True, stats=None, record=None):
    """Stage 1.  Returns det -> track (or -1) for each detection.  `record` (a list, test hook) takes one dict per non-empty problem."""
    n, t = len(dets), len(trks)
    m = np.full(n, -1, dtype=np.int64)
    if n == 0 or t == 0:
        return m
    iou = iou_matrix(dets, trks)
    pairs = read_off(iou, thr) if lsap_fast else None
    ocm = ocm_term(dets, scores, prev, valid, vel, inertia) if pairs is None or record is not None else None
    cost = None if ocm is None else -(iou + ocm)
    if record is not None:
        record.append(dict(stage="stage1", iou=iou.copy(), ocm=ocm, cost=cost, th=F32(thr), solved="lsap" if pairs is None else "read_off"))
    if pairs is None:
        pairs = linear_assignment(cost)
        if stats is not None:
            stats["n_lsap"] += 1
            stats["max_side"] = max(stats["max_side"], n, t)
    elif stats is not None:
        stats["n_fast"] += 1
    for r, c in pairs:
        if not iou[r, c] < thr:
            m[r] = c
    return m


class OCSort:
    def __init__(self, det_thresh=0.6, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False,
                 first_track_id=1, lsap_fast=True, oru=True, record=None):
        self.det_thresh, self.iou_threshold, self.inertia = F32(det_thresh), F32(iou_threshold), F32(inertia)
        self.max_age, self.min_hits, self.delta_t, self.use_byte = int(max_age), int(min_hits), int(delta_t), bool(use_byte)
        self.trackers = []
        self.frame_count = 0
        self.next_id = first_track_id
        self.lsap_fast, self.oru = lsap_fast, oru
        self.record = record                                      # test hook: a list that takes every non-empty association problem
        self.stats = dict(n_fast=0, n_lsap=0, max_side=0, n_oru=0, max_gap=0, n_ocr=0, n_byte=0)

    def _second(self, iou, rows, cols, take, stage=None):
        """BYTE / OCR stage: gate on the best IoU, LSAP on -iou, keep pairs at or above the threshold."""
        shut = iou.size == 0 or not iou.max() > self.iou_threshold
        if self.record is not None and iou.size:
            self.record.append(dict(frame=self.frame_count, stage=stage, iou=iou.copy(), ocm=None, cost=-iou, th=self.iou_threshold,
                                    solved="gate_shut" if shut else "lsap", dets=np.array(rows), tracks=[self.trackers[c].id for c in cols]))
        if shut:
            return 0
        self.stats["n_lsap"] += 1
        self.stats["max_side"] = max(self.stats["max_side"], *iou.shape)
        k = 0
        for r, c in linear_assignment(-iou):
            if iou[r, c] < self.iou_threshold:
                continue
            take(rows[r], cols[c])
            k += 1
        return k

    def update(self, tlwh, scores, cls):
        """One frame: tlwh [N, 4], scores [N], class ids [N] in detection order.  Returns the output tracks (upstream's order: the
        track list reversed)."""
        self.frame_count += 1
        tlwh = np.asarray(tlwh, dtype=F32).reshape(-1, 4)
        scores = np.asarray(scores, dtype=F32).reshape(-1)
        cls = np.asarray(cls).reshape(-1)
        box = np.stack([tlwh[:, 0], tlwh[:, 1], tlwh[:, 0] + tlwh[:, 2], tlwh[:, 1] + tlwh[:, 3]], 1).astype(F32) if len(tlwh) else np.zeros((0, 4), F32)
        hi = np.flatnonzero(scores > self.det_thresh)
        lo = np.flatnonzero((scores > BYTE_LOW) & (scores < self.det_thresh)) if self.use_byte else np.zeros(0, np.int64)

        trks, keep = [], []
        for t in self.trackers:
            b = t.predict()
            if np.all(np.isfinite(b)):                            # change 8
                keep.append(t)
                trks.append(b)
        self.trackers = keep
        T = len(keep)
        trks = np.array(trks, dtype=F32).reshape(-1, 4)
        vel = np.array([t.velocity for t in keep], dtype=F32).reshape(-1, 2)
        po = [t.previous_obs() for t in keep]
        prev = np.array([p[0] for p in po], dtype=F32).reshape(-1, 4)
        valid = np.array([p[1] for p in po], dtype=bool)
        last = np.array([t.last_observation for t in keep], dtype=F32).reshape(-1, 4)

        tdet = np.full(T, -1, dtype=np.int64)                     # track -> detection (index into the frame)
        m = associate(box[hi], scores[hi], trks, self.iou_threshold, vel, prev, valid, self.inertia, self.lsap_fast, self.stats, self.record)
        if self.record and "frame" not in self.record[-1]:
            self.record[-1].update(frame=self.frame_count, dets=hi.copy(), tracks=[t.id for t in keep])
        for r, c in enumerate(m):
            if c >= 0:
                tdet[c] = hi[r]
        dfree = np.ones(len(scores), dtype=bool)
        dfree[tdet[tdet >= 0]] = False

        def take(d, t):
            tdet[t] = d
            dfree[d] = False

        if self.use_byte and len(lo) > 0:
            ut = np.flatnonzero(tdet < 0)
            if len(ut):
                self.stats["n_byte"] += self._second(iou_matrix(box[lo], trks[ut]), lo, ut, take, "byte")
        ud = np.array([d for d in hi if dfree[d]], dtype=np.int64)
        ut = np.flatnonzero(tdet < 0)
        if len(ud) and len(ut):
            self.stats["n_ocr"] += self._second(iou_matrix(box[ud], last[ut]), ud, ut, take, "ocr")

        for t, d in zip(keep, tdet):
            if d < 0:
                t.update(None)
            else:
                was = t.kstate
                t.update(box[d], scores[d], cls[d], oru=self.oru)
                if was == FROZEN and self.oru:
                    self.stats["n_oru"] += 1
                    self.stats["max_gap"] = max(self.stats["max_gap"], t.oru_gap)
        for d in hi:
            if dfree[d]:
                self.trackers.append(KalmanBoxTracker(box[d], scores[d], cls[d], self.next_id, self.delta_t))
                self.next_id += 1
        out = [t for t in reversed(self.trackers)
               if t.time_since_update < 1 and (t.hit_streak >= self.min_hits or self.frame_count <= self.min_hits)]
        self.trackers = [t for t in self.trackers if not t.time_since_update > self.max_age]
        return out

    def update_xyxy(self, boxes_xyxy, scores, cls):
        b = np.asarray(boxes_xyxy, dtype=F32).reshape(-1, 4)
        tlwh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1) if len(b) else np.zeros((0, 4), F32)
        return self.update(tlwh, scores, cls)

    # ---- what the device returns
    @staticmethod
    def rows(tracks):
        """tracks6 rows: rint(x1 y1 x2 y2) of the last observation (of the filter's box for a track that has none), id, cls; scores."""
        out, conf = [], []
        for t in tracks:
            b = t.last_observation if t.has_obs else x_to_bbox(t.x)
            out.append((int(np.rint(b[0])), int(np.rint(b[1])), int(np.rint(b[2])), int(np.rint(b[3])), t.id, t.cls))
            conf.append(t.score)
        return np.array(out, dtype=np.int32).reshape(-1, 6), np.array(conf, dtype=F32)

    def export(self):
        """Live tracks in list order as aic_ocsort_export returns them."""
        ts = self.trackers
        i32 = lambda f: np.array([f(t) for t in ts], np.int32)
        return dict(track_id=i32(lambda t: t.id), age=i32(lambda t: t.age), hits=i32(lambda t: t.hits),
                    hit_streak=i32(lambda t: t.hit_streak), time_since_update=i32(lambda t: t.time_since_update),
                    cls=i32(lambda t: t.cls), frozen=i32(lambda t: t.kstate == FROZEN), has_obs=i32(lambda t: t.has_obs),
                    score=np.array([t.score for t in ts], F32),
                    last_observation=np.array([t.last_observation for t in ts], F32).reshape(-1, 4),
                    velocity=np.array([t.velocity for t in ts], F32).reshape(-1, 2),
                    mean=np.array([t.x for t in ts], F32).reshape(-1, 7), cov=np.array([t.P for t in ts], F32).reshape(-1, 7, 7))
