"""ByteTrack (BYTETracker.update of the ByteTrack authors' yolox/tracker/byte_tracker.py) on the device.

No appearance model: one frame costs the detector and a small association.  The recurrence runs in
csrc/kernels_bytetrack.hip (k frames per launch, the track table resident in HBM); its specification is
tests/bytetrack_oracle.py, the deliberate changes from upstream are listed in DESIGN.md ("ByteTrack").
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config


def bytetrack_params(track_thresh=0.5, track_buffer=30, match_thresh=0.8, mot20=False, frame_rate=30, low_thresh=0.1,
                     max_tracks=512, first_track_id=1, new_track_thresh=None):
    """aic_bytetrack_params (ByteTrack's MOT17 defaults); new_track_thresh defaults to track_thresh + 0.1."""
    return L.ByteTrackParams(track_thresh=float(track_thresh), low_thresh=float(low_thresh),
                             new_track_thresh=float(track_thresh + 0.1 if new_track_thresh is None else new_track_thresh),
                             match_thresh=float(match_thresh), track_buffer=int(track_buffer), frame_rate=int(frame_rate),
                             fuse_score=0 if mot20 else 1, max_tracks=int(max_tracks), first_track_id=int(first_track_id))


def output_tuples(rows, conf):
    """Output rows and scores of one frame as DeepSORT.update's tuples (x1, y1, x2, y2, track_id, class_name, conf)."""
    return [(r[0], r[1], r[2], r[3], r[4], config.class_name(r[5]), cf) for r, cf in zip(rows.tolist(), conf.tolist())]


def frame_rows(n_out, out6, oconf, cap, first, count):
    """Frames [first, first + count) of an update call's flat outputs as a list of (rows [m,6] int32, conf [m] fp32)."""
    res = []
    for f in range(first, first + count):
        m = min(int(n_out[f]), cap)
        res.append((out6[f, :m].copy(), oconf[f, :m].copy()))
    return res


_EXPORT = (("track_id", np.int32, ()), ("state", np.int32, ()), ("is_activated", np.int32, ()), ("start_frame", np.int32, ()),
           ("end_frame", np.int32, ()), ("cls", np.int32, ()), ("score", np.float32, ()), ("mean", np.float32, (8,)), ("cov", np.float32, (8, 8)))


def export_tracks(abi, *lead, feature_dim=None):
    """aic_bytetrack_export and its kin (`abi`, called with the leading arguments `lead`): the live tracks in list order (tracked list,
    then lost list) as a dict of arrays + n_tracked (the tracked list's length); with feature_dim, BoT-SORT's two columns on top."""
    cols = _EXPORT + ((("has_feat", np.int32, ()), ("smooth_feat", np.float32, (feature_dim,))) if feature_dim else ())
    n, nt = C.c_int32(), C.c_int32()
    L.call(abi, *lead, 0, *([None] * len(cols)), C.byref(n), C.byref(nt))
    out = {k: np.zeros((n.value,) + shape, dt) for k, dt, shape in cols}
    L.call(abi, *lead, n.value, *(L.ptr(v) for v in out.values()), C.byref(n), C.byref(nt))
    out["n_tracked"] = nt.value
    return out


class BYTETracker:
    """update(boxes_xyxy, scores, class_ids) -> [(x1, y1, x2, y2, track_id, class_name, conf), ...] as DeepSORT.update, for the
    activated tracks of the tracked list (ByteTrack's output_stracks).  Association is class-agnostic, as upstream."""

    def __init__(self, track_thresh=0.5, track_buffer=30, match_thresh=0.8, mot20=False, frame_rate=30, low_thresh=0.1, device=0,
                 max_tracks=512, first_track_id=1):
        self.params = bytetrack_params(track_thresh, track_buffer, match_thresh, mot20, frame_rate, low_thresh, max_tracks,
                                       first_track_id)
        self.max_tracks = max_tracks
        self._h = C.c_void_p()
        L.call("aic_bytetrack_create", config.resolve_device(device), C.byref(self.params), C.byref(self._h))
        self.frame_id = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_bytetrack_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"lsap_fast" (0/1), "epoch_frames" (0..16): same results either way."""
        L.call("aic_bytetrack_option", self._h, key.encode(), int(value))

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
        L.call("aic_bytetrack_update_batch", self._h, k, L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), cap, L.ptr(n_out),
               L.ptr(out6), L.ptr(oconf))
        self.frame_id += k
        return frame_rows(n_out, out6, oconf, cap, 0, k)

    _tuples = staticmethod(output_tuples)

    def update(self, boxes_xyxy, scores, class_ids):
        """One frame (BYTETracker.update). Empty inputs (np.array([])) are accepted."""
        rows, conf = self.update_batch_arrays([(boxes_xyxy, scores, class_ids)])[0]
        return self._tuples(rows, conf)

    def update_batch(self, boxes_xyxy, scores, class_ids):
        """k frames in one call (per-frame lists of arrays): a list of k update() results."""
        return [self._tuples(r, c) for r, c in self.update_batch_arrays(list(zip(boxes_xyxy, scores, class_ids)))]

    def counters(self):
        """Assignment problems since creation: read off as the unique optimum / through the LSAP, and the largest extended side met."""
        nf, nl, ms = C.c_int64(), C.c_int64(), C.c_int32()
        L.call("aic_bytetrack_counters", self._h, C.byref(nf), C.byref(nl), C.byref(ms))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value)

    def export(self):
        """Live tracks in list order (tracked list, then lost list): dict of arrays + n_tracked (the tracked list's length)."""
        return export_tracks("aic_bytetrack_export", self._h)


class TrackerBank:
    """What BYTETrackerBank, OCSortBank and BoTSORTBank share: `streams` independent streams on one device, one kernel block per stream and
    launch.  Every stream computes exactly what the single class fed the same frames computes; a stream that meets a capacity
    error stops alone (`failed`), the others go on, and reset(stream) starts it afresh."""
    _abi = None                                                  # "aic_bytetrack_bank" / "aic_ocsort_bank"

    def _create(self, streams, device):
        self.streams = int(streams)
        self.failed = {}                                         # stream -> message
        self._device = device
        self._h = C.c_void_p()
        L.call(self._abi + "_create", config.resolve_device(device), C.byref(self.params), self.streams, C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(L.load(), self._abi + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"lsap_fast" (0/1), "epoch_frames" (0..16), for the whole bank: same results either way."""
        L.call(self._abi + "_option", self._h, key.encode(), int(value))

    def reset(self, stream):
        """The stream as after creation (no tracks, ids from first_track_id again), a stop cleared: a camera reconnecting."""
        L.call(self._abi + "_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def update_arrays(self, per_stream_frames, cap_rows=None):
        """per_stream_frames: `streams` lists of (boxes_xyxy [n,4], scores [n], class_ids [n]), any length each.  Returns `streams`
        lists of (rows [m,6] int32, conf [m] fp32) per frame, None in place of a stopped stream's list."""
        if len(per_stream_frames) != self.streams:
            raise ValueError(f"{len(per_stream_frames)} frame lists for a bank of {self.streams} streams")
        flat = [fr for frames in per_stream_frames for fr in frames]
        fps = np.array([len(frames) for frames in per_stream_frames], dtype=np.int32)
        k = len(flat)
        boxes = [np.asarray(b, dtype=np.float32).reshape(-1, 4) for b, _, _ in flat]
        scores = [np.asarray(s, dtype=np.float32).reshape(-1) for _, s, _ in flat]
        cids = [np.asarray(c).reshape(-1).astype(np.int32) for _, _, c in flat]
        for b, s, c in zip(boxes, scores, cids):
            if not (len(b) == len(s) == len(c)):
                raise ValueError("boxes, scores and class ids differ in length")
        counts = np.array([len(b) for b in boxes], dtype=np.int32)
        cap = int(cap_rows if cap_rows is not None else self.max_tracks or 512)
        some = bool(counts.sum())
        xyxy = np.ascontiguousarray(np.concatenate(boxes) if some else np.zeros((0, 4), np.float32))
        conf = np.ascontiguousarray(np.concatenate(scores) if some else np.zeros(0, np.float32))
        cls = np.ascontiguousarray(np.concatenate(cids) if some else np.zeros(0, np.int32))
        n_out = np.zeros(max(k, 1), np.int32)
        out6 = np.zeros((max(k, 1), cap, 6), np.int32)
        oconf = np.zeros((max(k, 1), cap), np.float32)
        status = np.zeros(self.streams, np.int32)
        L.call(self._abi + "_update", self._h, L.ptr(fps), L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), cap, L.ptr(n_out),
               L.ptr(out6), L.ptr(oconf), L.ptr(status))
        return self._unpack(fps, n_out, out6, oconf, status, cap)

    def _unpack(self, fps, n_out, out6, oconf, status, cap):
        """The flat outputs of a bank update as `streams` lists of (rows, conf) per frame; a stopped stream is noted and gets None."""
        res, f = [], 0
        for s in range(self.streams):
            if status[s] and s not in self.failed:
                self.failed[s] = f"stream {s} stopped with libaicam error {int(status[s])} (reset({s}) starts it afresh)"
            k = int(fps[s])
            res.append(None if status[s] else frame_rows(n_out, out6, oconf, cap, f, k))
            f += k
        return res

    def update(self, per_stream_detections):
        """One tick: `streams` entries (boxes_xyxy, scores, class_ids), None = no frame from that camera this tick.  Returns
        `streams` lists of (x1, y1, x2, y2, track_id, class_name, conf) tuples ([] without a frame), None for a stopped stream."""
        got = self.update_arrays([[] if d is None else [d] for d in per_stream_detections])
        return [None if g is None else (output_tuples(*g[0]) if g else []) for g in got]


class BYTETrackerBank(TrackerBank):
    """BYTETrackerBank(streams, **BYTETracker's arguments): the ByteTrack state of `streams` cameras on one device."""
    _abi = "aic_bytetrack_bank"

    def __init__(self, streams, track_thresh=0.5, track_buffer=30, match_thresh=0.8, mot20=False, frame_rate=30, low_thresh=0.1, device=0,
                 max_tracks=512, first_track_id=1):
        self.params = bytetrack_params(track_thresh, track_buffer, match_thresh, mot20, frame_rate, low_thresh, max_tracks,
                                       first_track_id)
        self.max_tracks = max_tracks
        self._create(streams, device)

    def counters(self, stream):
        """BYTETracker.counters() of one stream."""
        nf, nl, ms = C.c_int64(), C.c_int64(), C.c_int32()
        L.call("aic_bytetrack_bank_counters", self._h, int(stream), C.byref(nf), C.byref(nl), C.byref(ms))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value)

    def export(self, stream):
        """BYTETracker.export() of one stream; raises for a stopped stream."""
        return export_tracks("aic_bytetrack_bank_export", self._h, int(stream))
