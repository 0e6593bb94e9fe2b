"""BoT-SORT with ReID (BoTSORT.update of the BoT-SORT authors' tracker/bot_sort.py) on the device.

ByteTrack's score bands and life cycle, a Kalman filter on [cx, cy, w, h], one exponentially smoothed appearance vector per track and
a first association on min(IoU distance, gated cosine distance / 2).  The recurrence runs in csrc/kernels_botsort.hip (k frames per
launch, the track table and the smoothed features resident in HBM); its specification is tests/botsort_oracle.py, the deliberate
changes from upstream are listed there and in DESIGN.md section 18.  Camera motion is an input (`warp`); gmc.CameraMotion estimates
it on the device, and a BoT-SORT pipeline does so itself with gmc=2 or 4.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config
from .bytetrack import TrackerBank, export_tracks, frame_rows, output_tuples
from .xcam import CameraLinks


def botsort_params(track_high_thresh=0.6, track_low_thresh=0.1, new_track_thresh=0.7, match_thresh=0.8, proximity_thresh=0.5,
                   appearance_thresh=0.25, track_buffer=30, frame_rate=30, fuse_score=True, with_reid=True, feat_alpha=0.9,
                   feature_dim=512, max_tracks=512, first_track_id=1):
    """aic_botsort_params (upstream's defaults)."""
    return L.BoTSORTParams(track_high_thresh=float(track_high_thresh), track_low_thresh=float(track_low_thresh),
                           new_track_thresh=float(new_track_thresh), match_thresh=float(match_thresh),
                           proximity_thresh=float(proximity_thresh), appearance_thresh=float(appearance_thresh),
                           feat_alpha=float(feat_alpha), track_buffer=int(track_buffer), frame_rate=int(frame_rate),
                           fuse_score=1 if fuse_score else 0, with_reid=1 if with_reid else 0, feature_dim=int(feature_dim),
                           max_tracks=int(max_tracks), first_track_id=int(first_track_id))


def _pack_frames(frames, feature_dim):
    """The frame tuples of BoTSORT.update_batch_arrays as the C ABI's flat arrays: counts, xyxy, conf, cls, feat, valid, warps."""
    frames = [tuple(f) + (None,) * (6 - len(f)) for f in frames]
    boxes = [np.asarray(f[0], dtype=np.float32).reshape(-1, 4) for f in frames]
    scores = [np.asarray(f[1], dtype=np.float32).reshape(-1) for f in frames]
    cids = [np.asarray(f[2]).reshape(-1).astype(np.int32) for f in frames]
    counts = np.array([len(b) for b in boxes], dtype=np.int32)
    for b, s, c in zip(boxes, scores, cids):
        if not (len(b) == len(s) == len(c)):
            raise ValueError("boxes, scores and class ids differ in length")
    total = int(counts.sum())
    with_feat = [f[3] is not None for f in frames]
    if any(with_feat) and not all(w or n == 0 for w, n in zip(with_feat, counts)):
        raise ValueError("features must be given for every frame of a call or for none")
    feat = None
    if any(with_feat) and total:
        fs = [np.asarray(f[3], dtype=np.float32).reshape(n, feature_dim) for f, n in zip(frames, counts) if n]
        feat = np.ascontiguousarray(np.concatenate(fs))
    valid = None
    if any(f[5] is not None for f in frames):
        valid = np.ascontiguousarray(np.concatenate([np.ones(n, np.int32) if f[5] is None else
                                                     np.asarray(f[5]).reshape(n).astype(np.int32) for f, n in zip(frames, counts)]))
    warps = None
    if any(f[4] is not None for f in frames):
        eye = np.array([[1, 0, 0], [0, 1, 0]], np.float32)
        warps = np.ascontiguousarray(np.stack([eye if f[4] is None else np.asarray(f[4], dtype=np.float32).reshape(2, 3)
                                               for f in frames]))
    xyxy = np.ascontiguousarray(np.concatenate(boxes) if total else np.zeros((0, 4), np.float32))
    conf = np.ascontiguousarray(np.concatenate(scores) if total else np.zeros(0, np.float32))
    cls = np.ascontiguousarray(np.concatenate(cids) if total else np.zeros(0, np.int32))
    return counts, xyxy, conf, cls, feat, valid, warps


class BoTSORT:
    """update(boxes_xyxy, scores, class_ids, features=None, warp=None) -> [(x1, y1, x2, y2, track_id, class_name, conf), ...] as
    DeepSORT.update, for every track of the tracked list (upstream's output_stracks).  features [n, feature_dim] are raw embeddings
    (normalised on the device; read for the high band only), warp a 2x3 affine [R | t] of the camera motion."""

    def __init__(self, device=0, **params):
        self.params = botsort_params(**params)
        self.max_tracks = self.params.max_tracks
        self.feature_dim = self.params.feature_dim or 512
        self._h = C.c_void_p()
        L.call("aic_botsort_create", config.resolve_device(device), C.byref(self.params), C.byref(self._h))
        self.frame_id = 0

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_botsort_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"lsap_fast" (0/1), "epoch_frames" (0..16): same results either way."""
        L.call("aic_botsort_option", self._h, key.encode(), int(value))

    def update_batch_arrays(self, frames, cap_rows=None):
        """frames: list of (boxes_xyxy [n,4], scores [n], class_ids [n][, features [n,dim] or None[, warp 2x3 or None[, valid [n] or
        None]]]).  Features are all-or-nothing over a call; a frame without a warp gets the identity.  Returns per frame
        (rows [m,6] int32, conf [m] fp32)."""
        k = len(frames)
        if k == 0:
            return []
        counts, xyxy, conf, cls, feat, valid, warps = _pack_frames(frames, self.feature_dim)
        cap = int(cap_rows if cap_rows is not None else self.max_tracks or 512)
        n_out = np.zeros(k, np.int32)
        out6 = np.zeros((k, cap, 6), np.int32)
        oconf = np.zeros((k, cap), np.float32)
        L.call("aic_botsort_update_batch", self._h, k, L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), L.ptr(feat), L.ptr(valid),
               L.ptr(warps), cap, L.ptr(n_out), L.ptr(out6), L.ptr(oconf))
        self.frame_id += k
        return frame_rows(n_out, out6, oconf, cap, 0, k)

    _tuples = staticmethod(output_tuples)

    def update(self, boxes_xyxy, scores, class_ids, features=None, warp=None):
        """One frame (BoTSORT.update). Empty inputs (np.array([])) are accepted."""
        rows, conf = self.update_batch_arrays([(boxes_xyxy, scores, class_ids, features, warp)])[0]
        return self._tuples(rows, conf)

    def counters(self):
        """Assignment problems since creation: read off as the unique optimum / through the LSAP, the largest extended side met, and
        the matched pairs whose winning term was the appearance distance; cost_cycles / kernel_cycles are shader-clock totals of the
        appearance pass of the fused cost (the dot products) and of the whole epoch kernel."""
        nf, nl, ms, na, cc, ck = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.call("aic_botsort_counters", self._h, C.byref(nf), C.byref(nl), C.byref(ms), C.byref(na), C.byref(cc), C.byref(ck))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value, n_appearance=na.value, cost_cycles=cc.value,
                    kernel_cycles=ck.value)

    def export(self):
        """Live tracks in list order (tracked list, then lost list): dict of arrays + n_tracked (the tracked list's length)."""
        return export_tracks("aic_botsort_export", self._h, feature_dim=self.feature_dim)


class BoTSORTBank(CameraLinks, TrackerBank):
    """BoTSORTBank(streams, device=0, **BoTSORT's parameters): the BoT-SORT state of `streams` cameras on one device, one kernel block
    per stream and launch.  Every stream has its own table, smoothed features and ids and computes exactly what a BoTSORT fed the same
    frames computes; a stream that meets a capacity error stops alone, and reset(stream) starts it afresh.  link_cameras() links the
    identities of the cameras' activated tracks by their smoothed features on the device (xcam.py; cosine distance within
    config.DEEPSORT_MAX_DIST unless a CrossCamera with another threshold is handed over); global_ids(stream, track_ids) reads them."""
    _abi = "aic_botsort_bank"

    def __init__(self, streams, device=0, **params):
        self.params = botsort_params(**params)
        self.max_tracks = self.params.max_tracks
        self.feature_dim = self.params.feature_dim or 512
        self._create(streams, device)

    def update_arrays(self, per_stream_frames, cap_rows=None):
        """per_stream_frames: `streams` lists of BoTSORT.update_batch_arrays' frame tuples, any length each; features are all-or-nothing
        over the call.  Returns `streams` lists of (rows [m,6] int32, conf [m] fp32) per frame, None in place of a stopped stream's."""
        if len(per_stream_frames) != self.streams:
            raise ValueError(f"{len(per_stream_frames)} frame lists for a bank of {self.streams} streams")
        flat = [fr for frames in per_stream_frames for fr in frames]
        fps = np.array([len(frames) for frames in per_stream_frames], dtype=np.int32)
        k = len(flat)
        counts, xyxy, conf, cls, feat, valid, warps = _pack_frames(flat, self.feature_dim)
        cap = int(cap_rows if cap_rows is not None else self.max_tracks or 512)
        n_out = np.zeros(max(k, 1), np.int32)
        out6 = np.zeros((max(k, 1), cap, 6), np.int32)
        oconf = np.zeros((max(k, 1), cap), np.float32)
        status = np.zeros(self.streams, np.int32)
        L.call("aic_botsort_bank_update", self._h, L.ptr(fps), L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), L.ptr(feat),
               L.ptr(valid), L.ptr(warps), cap, L.ptr(n_out), L.ptr(out6), L.ptr(oconf), L.ptr(status))
        return self._unpack(fps, n_out, out6, oconf, status, cap)

    def update(self, per_stream_detections):
        """One tick: `streams` entries (boxes_xyxy, scores, class_ids[, features[, warp]]), None = no frame from that camera this
        tick.  Returns `streams` lists of (x1, y1, x2, y2, track_id, class_name, conf) tuples, None for a stopped stream."""
        got = self.update_arrays([[] if d is None else [d] for d in per_stream_detections])
        return [None if g is None else (output_tuples(*g[0]) if g else []) for g in got]

    def counters(self, stream):
        """BoTSORT.counters() of one stream."""
        nf, nl, ms, na, cc, ck = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.call("aic_botsort_bank_counters", self._h, int(stream), C.byref(nf), C.byref(nl), C.byref(ms), C.byref(na), C.byref(cc),
               C.byref(ck))
        return dict(n_fast=nf.value, n_lsap=nl.value, max_side=ms.value, n_appearance=na.value, cost_cycles=cc.value,
                    kernel_cycles=ck.value)

    def export(self, stream):
        """BoTSORT.export() of one stream; raises for a stopped stream."""
        return export_tracks("aic_botsort_bank_export", self._h, int(stream), feature_dim=self.feature_dim)
