"""NumPy/SciPy restatement of BoT-SORT's ``BoTSORT.update()`` with ReID (TEST INFRASTRUCTURE).

Written from the algorithm as published by the BoT-SORT authors (Aharon, Orfaig, Bobrovsky 2022; ``tracker/bot_sort.py``: ``STrack``,
``BoTSORT.update``; ``tracker/matching.py``: ``iou_distance``, ``fuse_score``, ``embedding_distance``; ``tracker/kalman_filter.py``:
the xywh filter), with upstream's list semantics.  It is the specification the device tracker (``csrc/kernels_botsort.hip``)
reproduces bit for bit: ids, rows, class, score, state, list order, every counter, the Kalman state AND the smoothed features (every
product below is an ordered fp32 sum, the order the kernel uses, so no tolerance is needed anywhere).

Deliberate changes from upstream (also in DESIGN.md, section 18):
  1. IoU is this project's (no ``+1`` pixel, union floored at 1e-7, fp32), not ``cython_bbox``'s.
  2. The xywh filter is fp32 with a stated operation order (upstream: fp64 NumPy / SciPy).  The noise terms are
     ``(fp32(weight) * side)^2`` in fp32; ``cho_solve`` is a 4x4 Cholesky factorisation and two triangular solves per gain row
     (``K_i = S^-1 P[i, :4]``); ``P - K S K^T`` is kept, ``(S K_j^T)`` first, both products ordered sums over the four measured states.
  3. Track ids are counted per tracker from ``first_track_id``.  The class of a track is that of its last matched
     detection.
  4. ``lap.lapjv(extend_cost=True, cost_limit=thresh)`` is SciPy's ``linear_sum_assignment`` on lap's extended square matrix,
     exactly as ``tests/bytetrack_oracle.py`` change 4.
  5. Camera motion is an INPUT (a 2x3 affine per frame, ``None`` = no warp); upstream's estimators (ORB / ECC / sparse optical flow)
     are left out.  ``kron(I4, R) P kron(I4, R)^T`` is evaluated as ``(A P) A^T`` with two-term ordered sums.
  6. A 512-term dot product is ``wave_sum`` below: 64 partial sums (lane l takes elements 256 c + 4 l + q, in the order c, q)
     folded by a butterfly (distances 32, 16, 8, 4, 2, 1).  ``|f|`` is the square root of the same sum over ``f * f``.
  7. A detection's feature is normalised once (upstream normalises it again inside ``update_features``: a no-op up to rounding).
     A detection whose normalised feature is not finite in every element (a zero embedding gives 0 / 0, one overflowed element
     inf / inf) counts as having no feature (``has_feature``): it is never compared, never enters a smoothed vector and does not set
     ``has_feat``; it still matches by IoU.  Upstream would carry the NaN into the track's smoothed feature for good.  ``d_emb`` is
     set to 1 unless ``d_emb <= appearance_thresh`` (upstream: where ``d_emb > appearance_thresh``; the same for every finite value,
     and no detection brings a NaN).  The 50-deep feature deque is never read by upstream's algorithm and is left out.
  8. Only high-band detections carry a feature; a low-band detection's feature is never read (as upstream, which embeds the high band
     only).
  9. Output: EVERY track of the tracked list, as upstream's ``output_stracks = [track for track in self.tracked_stracks]`` (its
     ``is_activated`` filter is commented out there), so a new track shows from its first frame.  ByteTrack here outputs the
     activated ones only.

Every threshold is rounded to fp32 once and every comparison is made in fp32.
"""
from __future__ import annotations

import numpy as np

from bytetrack_oracle import (LOST, NEW, REMOVED, SECOND_THRESH, TRACKED, UNCONFIRMED_THRESH, fuse_score, joint_stracks,
                              linear_assignment, remove_duplicate_stracks, sub_stracks)
from ocsort_oracle import _chol4, _solve4
from oracle.deepsort_oracle import iou_cost_matrix

F32 = np.float32
W_POS, W_VEL = F32(1.0 / 20), F32(1.0 / 160)
W_POS0, W_VEL0 = F32(0.1), F32(0.0625)            # initiate: 2 / 20 and 10 / 160


# ----------------------------------------------------------------------------------------------------------------- ordered sums
def wave_sum(prod):
    """Sum of the last axis of fp32 `prod` [..., D] in the kernel's order (change 6)."""
    prod = np.asarray(prod, dtype=F32)
    d = prod.shape[-1]
    n = -(-d // 256) * 256
    p = np.zeros(prod.shape[:-1] + (n,), dtype=F32)
    p[..., :d] = prod
    p = p.reshape(prod.shape[:-1] + (n // 256, 64, 4))
    acc = np.zeros(prod.shape[:-1] + (64,), dtype=F32)
    for c in range(n // 256):
        for q in range(4):
            acc = acc + p[..., c, :, q]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def normalise(f):
    f = np.asarray(f, dtype=F32)
    with np.errstate(all="ignore"):
        return (f / np.sqrt(wave_sum(f * f))[..., None]).astype(F32)


def has_feature(unit):
    """Change 7: a normalised row counts as a feature only if every element is finite."""
    return bool(np.isfinite(unit).all())


# ----------------------------------------------------------------------------------------------------------------- the xywh filter
def _sides(mean):
    return np.array([mean[2], mean[3], mean[2], mean[3]], dtype=F32)


def kf_initiate(xywh):
    z = np.asarray(xywh, dtype=F32)
    mean = np.zeros(8, dtype=F32)
    mean[:4] = z
    std = np.concatenate([W_POS0 * _sides(z), W_VEL0 * _sides(z)]).astype(F32)
    return mean, np.diag(std * std).astype(F32)


def kf_predict(mean, cov):
    """x = F x, P = F (P F^T) + Q; Q from the sides BEFORE the step; every element an ordered fp32 sum."""
    std = np.concatenate([W_POS * _sides(mean), W_VEL * _sides(mean)]).astype(F32)
    x = mean.copy()
    x[:4] = x[:4] + x[4:]
    t1 = cov.copy()
    t1[:, :4] = cov[:, :4] + cov[:, 4:]
    t2 = t1.copy()
    t2[:4, :] = t1[:4, :] + t1[4:, :]
    t2[np.arange(8), np.arange(8)] += std * std
    return x, t2.astype(F32)


def kf_update(mean, cov, xywh):
    with np.errstate(all="ignore"):
        std = (W_POS * _sides(mean)).astype(F32)
        S = cov[:4, :4].copy()
        S[np.arange(4), np.arange(4)] += std * std
        K = _solve4(_chol4(S), cov[:, :4])                        # [8, 4], K_i = S^-1 P[i, :4]
        y = (np.asarray(xywh, dtype=F32) - mean[:4]).astype(F32)
        dot = np.zeros(8, dtype=F32)
        for a in range(4):
            dot = dot + K[:, a] * y[a]
        xn = (mean + dot).astype(F32)
        acc = np.zeros((8, 8), dtype=F32)
        for a in range(4):
            u = np.zeros(8, dtype=F32)                            # (S K_j^T)[a], per column j
            for c in range(4):
                u = u + S[a, c] * K[:, c]
            acc = acc + K[:, a:a + 1] * u[None, :]
        return xn, (cov - acc).astype(F32)


def kf_warp(mean, cov, warp):
    """mean <- kron(I4, R) mean, mean[:2] += t, cov <- (A cov) A^T with A = kron(I4, R); warp = [R | t] (2x3)."""
    w = np.asarray(warp, dtype=F32).reshape(2, 3)
    i = np.arange(8)
    ra, rb = w[i & 1, 0], w[i & 1, 1]                             # row i of A: ra at column i & ~1, rb at column i | 1
    m = (ra * mean[i & ~1] + rb * mean[i | 1]).astype(F32)
    m[0] = m[0] + w[0, 2]
    m[1] = m[1] + w[1, 2]
    T = (ra[:, None] * cov[i & ~1, :] + rb[:, None] * cov[i | 1, :]).astype(F32)
    P = (T[:, i & ~1] * ra[None, :] + T[:, i | 1] * rb[None, :]).astype(F32)
    return m, P


def mean_to_tlwh(mean):
    return np.array([mean[0] - mean[2] / F32(2), mean[1] - mean[3] / F32(2), mean[2], mean[3]], dtype=F32)


def tlwh_to_xywh(t):
    t = np.asarray(t, dtype=F32)
    return np.array([t[0] + t[2] / F32(2), t[1] + t[3] / F32(2), t[2], t[3]], dtype=F32)


# ----------------------------------------------------------------------------------------------------------------- STrack
class STrack:
    def __init__(self, tlwh, score, cls, feat=None, alpha=F32(0.9)):
        self._tlwh = np.asarray(tlwh, dtype=F32)
        self.score = F32(score)
        self.cls = int(cls)
        self.mean, self.covariance = None, None
        self.is_activated = False
        self.track_id = 0
        self.state = NEW
        self.frame_id = 0
        self.start_frame = 0
        self.alpha = F32(alpha)
        self.smooth_feat = None
        self.curr_feat = None
        unit = None if feat is None else normalise(feat)
        if unit is not None and has_feature(unit):
            self.update_features(unit)

    def update_features(self, f):
        """f is unit length (change 7)."""
        self.curr_feat = f
        if self.smooth_feat is None:
            self.smooth_feat = f.copy()
        else:
            s = (self.alpha * self.smooth_feat + (F32(1) - self.alpha) * f).astype(F32)
            self.smooth_feat = normalise(s)

    @property
    def end_frame(self):
        return self.frame_id

    @property
    def tlwh(self):
        return self._tlwh.copy() if self.mean is None else mean_to_tlwh(self.mean)

    def predict(self):
        mean = self.mean.copy()
        if self.state != TRACKED:
            mean[6] = 0
            mean[7] = 0
        self.mean, self.covariance = kf_predict(mean, self.covariance)

    def warp(self, w):
        self.mean, self.covariance = kf_warp(self.mean, self.covariance, w)

    def activate(self, track_id, frame_id):
        self.track_id = track_id
        self.mean, self.covariance = kf_initiate(tlwh_to_xywh(self._tlwh))
        self.state = TRACKED
        if frame_id == 1:
            self.is_activated = True
        self.frame_id = frame_id
        self.start_frame = frame_id

    def update(self, det, frame_id):
        """STrack.update and STrack.re_activate(new_id=False): the same assignments."""
        self.mean, self.covariance = kf_update(self.mean, self.covariance, tlwh_to_xywh(det.tlwh))
        if det.curr_feat is not None:
            self.update_features(det.curr_feat)
        self.state = TRACKED
        self.is_activated = True
        self.frame_id = frame_id
        self.score = det.score
        self.cls = det.cls

    def mark_lost(self):
        self.state = LOST

    def mark_removed(self):
        self.state = REMOVED


def iou_distance(atracks, btracks):
    return iou_cost_matrix([a.tlwh for a in atracks], [b.tlwh for b in btracks])


# ----------------------------------------------------------------------------------------------------------------- BoTSORT
class BoTSORT:
    def __init__(self, track_high_thresh=0.6, track_low_thresh=0.1, new_track_thresh=0.7, match_thresh=0.8, proximity_thresh=0.5,
                 appearance_thresh=0.25, track_buffer=30, frame_rate=30, fuse_score=True, with_reid=True, feat_alpha=0.9,
                 first_track_id=1):
        self.tracked_stracks, self.lost_stracks = [], []
        self.frame_id = 0
        self.high, self.low, self.new_thresh = F32(track_high_thresh), F32(track_low_thresh), F32(new_track_thresh)
        self.match_thresh, self.proximity, self.appearance = F32(match_thresh), F32(proximity_thresh), F32(appearance_thresh)
        self.fuse, self.with_reid, self.alpha = bool(fuse_score), bool(with_reid), F32(feat_alpha)
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        self.next_id = first_track_id
        self.n_appearance = 0                     # matched pairs (stages 1 and 3) whose winning term was d_emb (d_emb < d_iou)
        self.last_costs = None                    # (d_iou, d_emb, cost) of the last first association (test hook)

    def fused_cost(self, tracks, dets):
        """min(d_iou, gated d_emb) [T, N] fp32 and the matrix of pairs where d_emb won."""
        d_iou = iou_distance(tracks, dets)
        far = d_iou > self.proximity
        if self.fuse:
            d_iou = fuse_score(d_iou, dets)
        d_emb = np.ones_like(d_iou)
        if self.with_reid and d_iou.size:
            for i, t in enumerate(tracks):
                for j, d in enumerate(dets):
                    if far[i, j] or t.smooth_feat is None or d.curr_feat is None:
                        continue
                    e = np.maximum(F32(0), F32(1) - wave_sum(t.smooth_feat * d.curr_feat)) / F32(2)
                    if e <= self.appearance:
                        d_emb[i, j] = e
        return d_iou, d_emb, np.minimum(d_iou, d_emb).astype(F32)

    def update(self, tlwh, scores, cls, features=None, warp=None):
        """One frame: tlwh [N, 4], scores [N], class ids [N], features [N, D] or None (or a list with None entries), warp 2x3 or None."""
        self.frame_id += 1
        tlwh = np.asarray(tlwh, dtype=F32).reshape(-1, 4)
        scores = np.asarray(scores, dtype=F32).reshape(-1)
        cls = np.asarray(cls).reshape(-1)
        activated, refind, lost, removed = [], [], [], []

        def feat(i):
            return None if features is None or not self.with_reid or features[i] is None else features[i]
        remain = scores > self.high
        second = (scores > self.low) & (scores < self.high)
        detections = [STrack(tlwh[i], scores[i], cls[i], feat(i), self.alpha) for i in np.flatnonzero(remain)]
        detections_second = [STrack(tlwh[i], scores[i], cls[i]) for i in np.flatnonzero(second)]

        unconfirmed, tracked = [], []
        for t in self.tracked_stracks:
            (tracked if t.is_activated else unconfirmed).append(t)

        pool = joint_stracks(tracked, self.lost_stracks)
        for t in pool:
            t.predict()
        if warp is not None:
            for t in pool + unconfirmed:
                t.warp(warp)

        # first association: pool x high band, min(IoU distance, gated appearance distance)
        d_iou, d_emb, dists = self.fused_cost(pool, detections)
        self.last_costs = (d_iou, d_emb, dists)
        matches, u_track, u_detection = linear_assignment(dists, self.match_thresh)
        for it, idet in matches:
            self.n_appearance += int(d_emb[it, idet] < d_iou[it, idet])
            track, det = pool[it], detections[idet]
            (activated if track.state == TRACKED else refind).append(track)
            track.update(det, self.frame_id)

        # second association: the remaining Tracked tracks x low band, IoU only
        r_tracked = [pool[i] for i in u_track if pool[i].state == TRACKED]
        matches, u_track, _ = linear_assignment(iou_distance(r_tracked, detections_second), SECOND_THRESH)
        for it, idet in matches:
            r_tracked[it].update(detections_second[idet], self.frame_id)
            activated.append(r_tracked[it])
        for it in u_track:
            r_tracked[it].mark_lost()
            lost.append(r_tracked[it])

        # unconfirmed tracks x the high band left over, the same fused cost
        detections = [detections[i] for i in u_detection]
        d_iou, d_emb, dists = self.fused_cost(unconfirmed, detections)
        matches, u_unconfirmed, u_detection = linear_assignment(dists, UNCONFIRMED_THRESH)
        for it, idet in matches:
            self.n_appearance += int(d_emb[it, idet] < d_iou[it, idet])
            unconfirmed[it].update(detections[idet], self.frame_id)
            activated.append(unconfirmed[it])
        for it in u_unconfirmed:
            unconfirmed[it].mark_removed()
            removed.append(unconfirmed[it])

        for inew in u_detection:
            track = detections[inew]
            if track.score < self.new_thresh:
                continue
            track.activate(self.next_id, self.frame_id)
            self.next_id += 1
            activated.append(track)

        for track in self.lost_stracks:
            if self.frame_id - track.end_frame > self.max_time_lost:
                track.mark_removed()
                removed.append(track)

        self.tracked_stracks = [t for t in self.tracked_stracks if t.state == TRACKED]
        self.tracked_stracks = joint_stracks(self.tracked_stracks, activated)
        self.tracked_stracks = joint_stracks(self.tracked_stracks, refind)
        self.lost_stracks = sub_stracks(self.lost_stracks, self.tracked_stracks)
        self.lost_stracks.extend(lost)
        self.lost_stracks = sub_stracks(self.lost_stracks, removed)
        self.tracked_stracks, self.lost_stracks = remove_duplicate_stracks(self.tracked_stracks, self.lost_stracks)
        return list(self.tracked_stracks)                         # change 9

    def update_xyxy(self, boxes_xyxy, scores, cls, features=None, warp=None):
        b = np.asarray(boxes_xyxy, dtype=F32).reshape(-1, 4)
        tlwh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1) if len(b) else np.zeros((0, 4), F32)
        return self.update(tlwh, scores, cls, features, warp)

    # ---- what the device returns
    @staticmethod
    def rows(tracks):
        """rint(x1 y1 x2 y2) of the track box with w, h clamped at 0, id, cls; and the scores."""
        out, conf = [], []
        for t in tracks:
            x1, y1, w, h = mean_to_tlwh(t.mean)
            w, h = max(F32(0), w), max(F32(0), h)
            out.append((int(np.rint(x1)), int(np.rint(y1)), int(np.rint(x1 + w)), int(np.rint(y1 + h)), t.track_id, t.cls))
            conf.append(t.score)
        return np.array(out, dtype=np.int32).reshape(-1, 6), np.array(conf, dtype=F32)

    def export(self, dim=512):
        """Live tracks in list order (tracked, then lost) as aic_botsort_export returns them."""
        ts = self.tracked_stracks + self.lost_stracks
        sf = np.zeros((len(ts), dim), dtype=F32)
        for i, t in enumerate(ts):
            if t.smooth_feat is not None:
                sf[i] = t.smooth_feat
        return dict(track_id=np.array([t.track_id for t in ts], np.int32), state=np.array([t.state for t in ts], np.int32),
                    is_activated=np.array([t.is_activated for t in ts], np.int32),
                    start_frame=np.array([t.start_frame for t in ts], np.int32),
                    end_frame=np.array([t.end_frame for t in ts], np.int32), cls=np.array([t.cls for t in ts], np.int32),
                    score=np.array([t.score for t in ts], F32),
                    mean=np.array([t.mean for t in ts], F32).reshape(-1, 8),
                    cov=np.array([t.covariance for t in ts], F32).reshape(-1, 8, 8),
                    has_feat=np.array([t.smooth_feat is not None for t in ts], np.int32), smooth_feat=sf,
                    n_tracked=len(self.tracked_stracks))
