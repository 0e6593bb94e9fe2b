"""NumPy/SciPy restatement of ByteTrack's ``BYTETracker.update()`` (TEST INFRASTRUCTURE).

A line-by-line restatement of the ByteTrack authors' ``yolox/tracker/byte_tracker.py`` (``STrack``, ``BYTETracker``,
``joint_stracks``, ``sub_stracks``, ``remove_duplicate_stracks``) and ``yolox/tracker/matching.py`` (``linear_assignment``,
``iou_distance``, ``fuse_score``), with the same list semantics.  It is the specification the device tracker
(``csrc/kernels_bytetrack.hip``) reproduces: ids, rows, class, score, state and list order bit for bit, the Kalman state within the
tolerance of the DeepSORT chain (the update's K S K^T is a BLAS product here, an ordered fp32 sum on the device).

Deliberate changes from upstream (also in DESIGN.md, section "ByteTrack"):
  1. IoU is this project's (``matching.py`` form of the reference: no ``+1`` pixel, union floored at 1e-7, fp32), not
     ``cython_bbox``'s.
  2. The Kalman filter is the reference DeepSORT's fp32 filter (``oracle/deepsort_oracle.py``: the arithmetic the device
     already reproduces), not ByteTrack's fp64 ``multi_predict``.
  3. Track ids are counted per tracker from ``first_track_id``, not by a process-wide counter (as SURVEY F8 decided for
     DeepSORT).
  4. ``lap.lapjv(cost, extend_cost=True, cost_limit=thresh)`` is restated as SciPy's ``linear_sum_assignment`` on lap's
     extended square matrix (side T + N, fp32: top-left the costs, bottom-right 0, every other entry fp32(thresh / 2)), so
     ties are settled by SciPy's rules, not lapjv's.  The objective is the one lapjv minimises.

Every threshold is rounded to fp32 once and every comparison is made in fp32.
"""
from __future__ import annotations

import numpy as np
from scipy.optimize import linear_sum_assignment

from oracle.deepsort_oracle import (iou_cost_matrix, kf_initiate, kf_predict, kf_update, mean_to_tlwh,
                                    tlwh_to_xyah)

NEW, TRACKED, LOST, REMOVED = 0, 1, 2, 3          # basetrack.py TrackState

SECOND_THRESH = np.float32(0.5)                   # byte_tracker.py: second association
UNCONFIRMED_THRESH = np.float32(0.7)              # byte_tracker.py: unconfirmed tracks
DUPLICATE_DIST = np.float32(0.15)                 # byte_tracker.py: remove_duplicate_stracks


class STrack:
    def __init__(self, tlwh, score, cls):
        self._tlwh = np.asarray(tlwh, dtype=np.float32)
        self.score = np.float32(score)
        self.cls = int(cls)
        self.mean, self.covariance = None, None
        self.is_activated = False
        self.track_id = 0
        self.state = NEW
        self.frame_id = 0
        self.start_frame = 0
        self.tracklet_len = 0

    @property
    def end_frame(self):
        return self.frame_id

    @property
    def tlwh(self):
        if self.mean is None:
            return self._tlwh.copy()
        return mean_to_tlwh(self.mean)

    def predict(self):
        mean = self.mean.copy()
        if self.state != TRACKED:
            mean[7] = 0
        self.mean, self.covariance = kf_predict(mean, self.covariance)

    def activate(self, track_id, frame_id):
        self.track_id = track_id
        self.mean, self.covariance = kf_initiate(tlwh_to_xyah(self._tlwh))
        self.tracklet_len = 0
        self.state = TRACKED
        if frame_id == 1:
            self.is_activated = True
        self.frame_id = frame_id
        self.start_frame = frame_id

    def re_activate(self, new_track, frame_id):
        self.mean, self.covariance = kf_update(self.mean, self.covariance, tlwh_to_xyah(new_track.tlwh))
        self.tracklet_len = 0
        self.state = TRACKED
        self.is_activated = True
        self.frame_id = frame_id
        self.score = new_track.score
        self.cls = new_track.cls

    def update(self, new_track, frame_id):
        self.frame_id = frame_id
        self.tracklet_len += 1
        self.mean, self.covariance = kf_update(self.mean, self.covariance, tlwh_to_xyah(new_track.tlwh))
        self.state = TRACKED
        self.is_activated = True
        self.score = new_track.score
        self.cls = new_track.cls

    def mark_lost(self):
        self.state = LOST

    def mark_removed(self):
        self.state = REMOVED


# --------------------------------------------------------------------------- matching.py
def linear_assignment(cost, thresh):
    """lap.lapjv(cost, extend_cost=True, cost_limit=thresh) as SciPy on lap's extended matrix (change 4)."""
    cost = np.asarray(cost, dtype=np.float32)
    t, n = cost.shape
    if cost.size == 0:
        return [], list(range(t)), list(range(n))
    ext = extended_matrix(cost, thresh)
    rows, cols = linear_sum_assignment(ext.astype(np.float64))
    x = np.full(t, -1, dtype=np.int64)
    for r, c in zip(rows, cols):
        if r < t and c < n:
            x[r] = c
    matches = [(i, int(x[i])) for i in range(t) if x[i] >= 0]
    taken = set(int(c) for c in x if c >= 0)
    return matches, [i for i in range(t) if x[i] < 0], [j for j in range(n) if j not in taken]


def extended_matrix(cost, thresh):
    """lap's extend_cost / cost_limit square matrix, fp32."""
    t, n = cost.shape
    ext = np.full((t + n, t + n), np.float32(np.float32(thresh) / np.float32(2)), dtype=np.float32)
    ext[t:, n:] = 0
    ext[:t, :n] = cost
    return ext


def iou_distance(atracks, btracks):
    """matching.py iou_distance with this project's IoU (change 1); [T, N] fp32."""
    return iou_cost_matrix([a.tlwh for a in atracks], [b.tlwh for b in btracks])


def fuse_score(cost, detections):
    if cost.size == 0:
        return cost
    s = np.array([d.score for d in detections], dtype=np.float32)[None, :]
    return (np.float32(1) - (np.float32(1) - cost) * s).astype(np.float32)


# --------------------------------------------------------------------------- byte_tracker.py list helpers
def joint_stracks(tlista, tlistb):
    exists, res = {}, []
    for t in tlista:
        exists[t.track_id] = 1
        res.append(t)
    for t in tlistb:
        if not exists.get(t.track_id, 0):
            exists[t.track_id] = 1
            res.append(t)
    return res


def sub_stracks(tlista, tlistb):
    stracks = {t.track_id: t for t in tlista}
    for t in tlistb:
        if stracks.get(t.track_id, 0):
            del stracks[t.track_id]
    return list(stracks.values())


def remove_duplicate_stracks(stracksa, stracksb):
    pdist = iou_distance(stracksa, stracksb)
    dupa, dupb = set(), set()
    if pdist.size:
        for p, q in zip(*np.where(pdist < DUPLICATE_DIST)):
            timep = stracksa[p].frame_id - stracksa[p].start_frame
            timeq = stracksb[q].frame_id - stracksb[q].start_frame
            if timep > timeq:
                dupb.add(q)
            else:
                dupa.add(p)
    return ([t for i, t in enumerate(stracksa) if i not in dupa], [t for i, t in enumerate(stracksb) if i not in dupb])


# --------------------------------------------------------------------------- BYTETracker
class BYTETracker:
    def __init__(self, track_thresh=0.5, track_buffer=30, match_thresh=0.8, mot20=False, frame_rate=30, low_thresh=0.1,
                 first_track_id=1):
        self.tracked_stracks, self.lost_stracks = [], []
        self.frame_id = 0
        self.track_thresh = np.float32(track_thresh)
        self.low_thresh = np.float32(low_thresh)
        self.det_thresh = np.float32(track_thresh + 0.1)
        self.match_thresh = np.float32(match_thresh)
        self.fuse = not mot20
        self.max_time_lost = int(frame_rate / 30.0 * track_buffer)
        self.next_id = first_track_id

    def update(self, tlwh, scores, cls):
        """One frame: tlwh [N, 4] fp32, scores [N], class ids [N], in detection order. Returns the output tracks."""
        self.frame_id += 1
        tlwh = np.asarray(tlwh, dtype=np.float32).reshape(-1, 4)
        scores = np.asarray(scores, dtype=np.float32).reshape(-1)
        cls = np.asarray(cls).reshape(-1)
        activated, refind, lost, removed = [], [], [], []

        remain = scores > self.track_thresh
        second = (scores > self.low_thresh) & (scores < self.track_thresh)
        detections = [STrack(tlwh[i], scores[i], cls[i]) for i in np.flatnonzero(remain)]
        detections_second = [STrack(tlwh[i], scores[i], cls[i]) for i in np.flatnonzero(second)]

        unconfirmed, tracked = [], []
        for t in self.tracked_stracks:
            (tracked if t.is_activated else unconfirmed).append(t)

        # step 2: first association, with high score detections
        pool = joint_stracks(tracked, self.lost_stracks)
        for t in pool:
            t.predict()
        dists = iou_distance(pool, detections)
        if self.fuse:
            dists = fuse_score(dists, detections)
        matches, u_track, u_detection = linear_assignment(dists, self.match_thresh)
        for it, idet in matches:
            track, det = pool[it], detections[idet]
            if track.state == TRACKED:
                track.update(det, self.frame_id)
                activated.append(track)
            else:
                track.re_activate(det, self.frame_id)
                refind.append(track)

        # step 3: second association, with low score detections
        r_tracked = [pool[i] for i in u_track if pool[i].state == TRACKED]
        dists = iou_distance(r_tracked, detections_second)
        matches, u_track, _ = linear_assignment(dists, SECOND_THRESH)
        for it, idet in matches:
            track, det = r_tracked[it], detections_second[idet]
            if track.state == TRACKED:
                track.update(det, self.frame_id)
                activated.append(track)
            else:
                track.re_activate(det, self.frame_id)
                refind.append(track)
        for it in u_track:
            track = r_tracked[it]
            if not track.state == LOST:
                track.mark_lost()
                lost.append(track)

        # unconfirmed tracks (usually tracks with only their first frame)
        detections = [detections[i] for i in u_detection]
        dists = iou_distance(unconfirmed, detections)
        if self.fuse:
            dists = fuse_score(dists, detections)
        matches, u_unconfirmed, u_detection = linear_assignment(dists, UNCONFIRMED_THRESH)
        for it, idet in matches:
            unconfirmed[it].update(detections[idet], self.frame_id)
            activated.append(unconfirmed[it])
        for it in u_unconfirmed:
            unconfirmed[it].mark_removed()
            removed.append(unconfirmed[it])

        # step 4: init new tracks
        for inew in u_detection:
            track = detections[inew]
            if track.score < self.det_thresh:
                continue
            track.activate(self.next_id, self.frame_id)
            self.next_id += 1
            activated.append(track)

        # step 5: update state
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
        return [t for t in self.tracked_stracks if t.is_activated]

    def update_xyxy(self, boxes_xyxy, scores, cls):
        b = np.asarray(boxes_xyxy, dtype=np.float32).reshape(-1, 4)
        tlwh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1) if len(b) else np.zeros((0, 4), np.float32)
        return self.update(tlwh, scores, cls)

    # ---- what the device returns
    @staticmethod
    def rows(tracks):
        """Output rows as aic_tracker_outputs: rint(x1 y1 x2 y2) of mean_to_tlwh with w, h clamped at 0, id, cls; and the scores."""
        out, conf = [], []
        for t in tracks:
            x1, y1, w, h = mean_to_tlwh(t.mean)
            w, h = max(np.float32(0), w), max(np.float32(0), h)
            out.append((int(np.rint(x1)), int(np.rint(y1)), int(np.rint(x1 + w)), int(np.rint(y1 + h)), t.track_id, t.cls))
            conf.append(t.score)
        return (np.array(out, dtype=np.int32).reshape(-1, 6), np.array(conf, dtype=np.float32))

    def export(self):
        """Live tracks in list order (tracked, then lost) as aic_bytetrack_export returns them."""
        ts = self.tracked_stracks + self.lost_stracks
        return dict(track_id=np.array([t.track_id for t in ts], np.int32), state=np.array([t.state for t in ts], np.int32),
                    is_activated=np.array([t.is_activated for t in ts], np.int32),
                    start_frame=np.array([t.start_frame for t in ts], np.int32),
                    end_frame=np.array([t.end_frame for t in ts], np.int32), cls=np.array([t.cls for t in ts], np.int32),
                    score=np.array([t.score for t in ts], np.float32),
                    mean=np.array([t.mean for t in ts], np.float32).reshape(-1, 8),
                    cov=np.array([t.covariance for t in ts], np.float32).reshape(-1, 8, 8),
                    n_tracked=len(self.tracked_stracks))
