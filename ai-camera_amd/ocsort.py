"""OC-SORT (OCSort.update of the OC-SORT authors' ocsort.py) on the device.

No appearance model: one frame costs the detector and a small association.  SORT's 7-state filter on [x, y, s, r], the velocity
direction term (OCM), the last-observation stage (OCR) and the virtual-trajectory replay of a re-found track (ORU) run in
csrc/kernels_ocsort.hip (k frames per launch, the track table resident in HBM); the specification is tests/ocsort_oracle.py, the
deliberate changes from upstream are listed there and in DESIGN.md ("OC-SORT").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config
from .bytetrack import TrackerBank, frame_rows, output_tuples


def ocsort_params(det_thresh=0.6, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False,
                  max_tracks=512, first_track_id=1):
    """aic_ocsort_params (upstream's defaults)."""
    return L.OCSortParams(det_thresh=float(det_thresh), iou_threshold=float(iou_threshold), inertia=float(inertia),
                          max_age=int(max_age), min_hits=int(min_hits), delta_t=int(delta_t), use_byte=int(bool(use_byte)),
                          max_tracks=int(max_tracks), first_track_id=int(first_track_id))


class OCSort:
    """update(boxes_xyxy, scores, class_ids) -> [(x1, y1, x2, y2, track_id, class_name, conf), ...] as DeepSORT.update: the tracks
    updated in the frame with hit_streak >= min_hits (or frame <= min_hits), their last observation, in upstream's order (the
    track list reversed).  Association is class-agnostic, as upstream; a track's class is that of its last detection."""

    def __init__(self, det_thresh=0.6, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False, device=0,
                 max_tracks=512, first_track_id=1):
        self.params = ocsort_params(det_thresh, max_age, min_hits, iou_threshold, delta_t, inertia, use_byte, max_tracks,
                                    first_track_id)
        self.max_tracks = max_tracks
        self._h = C.c_void_p()
        L.call("aic_ocsort_create", config.resolve_device(device), C.byref(self.params), C.byref(self._h))
        self.frame_count = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_ocsort_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"lsap_fast" (0: stage 1 never takes the read-off), "epoch_frames" (0..16: same results)."""
        L.call("aic_ocsort_option", self._h, key.encode(), int(value))

    def update_batch_arrays(self, frames, cap_rows=None):
        """frames: list of (boxes_xyxy [n,4], scores [n], class_ids [n]).  Returns per frame (rows [m,6] int32, conf [m] fp32)."""
        k = len(frames)
        if k == 0:
            return []
        boxes = [np.asarray(b, dtype=np.float32).reshape(-1, 4) for b, _, _ in frames]
        scores = [np.asarray(s, dtype=np.float32).reshape(-1) for _, s, _ in frames]
        cids = [np.asarray(c).reshape(-1).astype(np.int32) for _, _, c in frames]
        counts = np.array([len(b) for b in boxes], dtype=np.int32)
        for b, s, c in zip(boxes, scores, cids):
            if not (len(b) == len(s) == len(c)):
                raise ValueError("boxes, scores and class ids differ in length")
        cap = int(cap_rows if cap_rows is not None else self.max_tracks or 512)
        xyxy = np.ascontiguousarray(np.concatenate(boxes) if counts.sum() else np.zeros((0, 4), np.float32))
        conf = np.ascontiguousarray(np.concatenate(scores) if counts.sum() else np.zeros(0, np.float32))
        cls = np.ascontiguousarray(np.concatenate(cids) if counts.sum() else np.zeros(0, np.int32))
        n_out = np.zeros(k, np.int32)
        out6 = np.zeros((k, cap, 6), np.int32)
        oconf = np.zeros((k, cap), np.float32)
        L.call("aic_ocsort_update_batch", self._h, k, L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), cap, L.ptr(n_out),
               L.ptr(out6), L.ptr(oconf))
        self.frame_count += k
        return frame_rows(n_out, out6, oconf, cap, 0, k)

    _tuples = staticmethod(output_tuples)

    def update(self, boxes_xyxy, scores, class_ids):
        """One frame (OCSort.update). Empty inputs (np.array([])) are accepted."""
        rows, conf = self.update_batch_arrays([(boxes_xyxy, scores, class_ids)])[0]
        return self._tuples(rows, conf)

    def update_batch(self, boxes_xyxy, scores, class_ids):
        """k frames in one call (per-frame lists of arrays): a list of k update() results."""
        return [self._tuples(r, c) for r, c in self.update_batch_arrays(list(zip(boxes_xyxy, scores, class_ids)))]

    def counters(self):
        """Since creation: stage-1 problems read off / problems through the LSAP, the largest side the LSAP met, ORU replays and
        their longest gap, pairs made by the OCR and the BYTE stage."""
        nf, nl, no, nr, nb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        ms, mg = C.c_int32(), C.c_int32()
        L.call("aic_ocsort_counters", self._h, C.byref(nf), C.byref(nl), C.byref(ms), C.byref(no), C.byref(mg), C.byref(nr), C.byref(nb))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value, n_oru=no.value, max_gap=mg.value, n_ocr=nr.value,
                    n_byte=nb.value)

    KEYS = ("track_id", "age", "hits", "hit_streak", "time_since_update", "cls", "frozen", "has_obs", "score", "last_observation",
            "velocity", "mean", "cov")

    def export(self):
        """Live tracks in list order: dict of arrays (KEYS)."""
        n = C.c_int32()
        L.call("aic_ocsort_export", self._h, 0, *([None] * 13), C.byref(n))
        m = n.value
        out = {k: np.zeros(m, np.int32) for k in self.KEYS[:8]}
        out.update(score=np.zeros(m, np.float32), last_observation=np.zeros((m, 4), np.float32), velocity=np.zeros((m, 2), np.float32),
                   mean=np.zeros((m, 7), np.float32), cov=np.zeros((m, 7, 7), np.float32))
        L.call("aic_ocsort_export", self._h, m, *(L.ptr(out[k]) for k in self.KEYS), C.byref(n))
        return out


class OCSortBank(TrackerBank):
    """OCSortBank(streams, **OCSort's arguments): the OC-SORT state of `streams` cameras on one device (bytetrack.TrackerBank)."""
    _abi = "aic_ocsort_bank"

    def __init__(self, streams, det_thresh=0.6, max_age=30, min_hits=3, iou_threshold=0.3, delta_t=3, inertia=0.2, use_byte=False, device=0,
                 max_tracks=512, first_track_id=1):
        self.params = ocsort_params(det_thresh, max_age, min_hits, iou_threshold, delta_t, inertia, use_byte, max_tracks,
                                    first_track_id)
        self.max_tracks = max_tracks
        self._create(streams, device)

    def counters(self, stream):
        """OCSort.counters() of one stream."""
        nf, nl, no, nr, nb = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        ms, mg = C.c_int32(), C.c_int32()
        L.call("aic_ocsort_bank_counters", self._h, int(stream), C.byref(nf), C.byref(nl), C.byref(ms), C.byref(no), C.byref(mg),
               C.byref(nr), C.byref(nb))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value, n_oru=no.value, max_gap=mg.value, n_ocr=nr.value,
                    n_byte=nb.value)

    def export(self, stream):
        """OCSort.export() of one stream; raises for a stopped stream."""
        n = C.c_int32()
        L.call("aic_ocsort_bank_export", self._h, int(stream), 0, *([None] * 13), C.byref(n))
        m = n.value
        out = {k: np.zeros(m, np.int32) for k in OCSort.KEYS[:8]}
        out.update(score=np.zeros(m, np.float32), last_observation=np.zeros((m, 4), np.float32), velocity=np.zeros((m, 2), np.float32),
                   mean=np.zeros((m, 7), np.float32), cov=np.zeros((m, 7, 7), np.float32))
        L.call("aic_ocsort_bank_export", self._h, int(stream), m, *(L.ptr(out[k]) for k in OCSort.KEYS), C.byref(n))
        return out
