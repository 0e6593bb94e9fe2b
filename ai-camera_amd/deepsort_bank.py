"""A bank of DeepSORT streams on one device (aic_deepsort_bank_*, csrc/deepsort_bank.hpp): `streams` cameras per launch of the device
association (csrc/kernels_trk_dev.hip), one kernel block per stream.  Every stream has its own track table, Kalman state, galleries and
ids and computes exactly what a core.tracker_core.TrackerCore with option("device_assoc", 1) fed the same frames computes.

Device association only: nn_budget > 0, max_tracks <= 512, feature_dim a multiple of 4.  The galleries are resident:
2 * max_tracks * nn_budget * feature_dim * 4 bytes per stream (210 MB at the defaults), so the number of streams is a memory decision.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config
from .bytetrack import TrackerBank
from .xcam import CameraLinks


def deepsort_bank_params(max_cosine_distance=0.2, nn_budget=100, max_iou_distance=0.7, max_age=70, n_init=3, max_tracks=512,
                         feature_dim=512, first_track_id=1):
    """aic_tracker_params of a bank (the reference's defaults, src/config.py:23-29)."""
    return L.TrackerParams(float(max_cosine_distance), float(max_iou_distance), int(nn_budget) if nn_budget else 0, int(max_age),
                           int(n_init), int(max_tracks), int(feature_dim), int(first_track_id))


class DeepSORTBank(CameraLinks, TrackerBank):
    """DeepSORTBank(streams, device=0, **deepsort_bank_params): the DeepSORT state of `streams` cameras.  A stream that exhausts
    max_tracks stops alone (`failed`), the others go on, and reset(stream) starts it afresh.  link_cameras() links the identities of
    the cameras' confirmed tracks on the device (xcam.py) within max_cosine_distance; global_ids(stream, track_ids) reads them."""
    _abi = "aic_deepsort_bank"

    def _link_threshold(self):
        return self.params.max_cosine_distance

    def __init__(self, streams, device=0, **params):
        self.params = deepsort_bank_params(**params)
        self.max_tracks = self.params.max_tracks or 512
        self.feature_dim = self.params.feature_dim or 512
        self._create(streams, device)

    @classmethod
    def _borrow(cls, handle, params, streams, device, feature_dim):
        """The bank a TrackingPipeline.deepsort_bank pipeline owns (aic_pipeline_deepsort_bank): close() destroys nothing."""
        b = cls.__new__(cls)
        b.params, b._h, b._borrowed = params, handle, True
        b.streams, b.failed, b._device = int(streams), {}, device
        b.max_tracks, b.feature_dim = params.max_tracks or 512, int(feature_dim)
        return b

    def close(self):
        if getattr(self, "_borrowed", False):
            self._h = C.c_void_p()
        else:
            super().close()

    def option(self, key, value):
        """"lsap_fast" (0/1), "wave_cascade" (0/1), "epoch_frames" (0..16), for the whole bank: same results either way."""
        L.call(self._abi + "_option", self._h, key.encode(), int(value))

    def update_arrays(self, per_stream_frames, cap_rows=None):
        """per_stream_frames: `streams` lists of TrackerCore.update_batch's frame tuples (tlwh [n,4], conf [n], class ids [n], feats
        [n,feature_dim] or None[, has_feat [n] or None]), any length each; each frame is a predict() + update().  Returns `streams`
        lists of (rows [m,6] int32, conf [m] fp32) per frame, None in place of a stopped stream's list."""
        if len(per_stream_frames) != self.streams:
            raise ValueError(f"{len(per_stream_frames)} frame lists for a bank of {self.streams} streams")
        flat = [tuple(fr) + (None,) * (5 - len(fr)) for frames in per_stream_frames for fr in frames]
        fps = np.array([len(frames) for frames in per_stream_frames], dtype=np.int32)
        k = len(flat)
        counts = np.array([len(np.asarray(f[0]).reshape(-1, 4)) for f in flat], dtype=np.int32)
        tot = int(counts.sum())
        any_feat = any(f[3] is not None and n for f, n in zip(flat, counts))
        tlwh, conf, cls = np.zeros((tot, 4), np.float32), np.zeros(tot, np.float32), np.zeros(tot, np.int32)
        feats = np.zeros((tot, self.feature_dim), np.float32) if any_feat else None
        valid = np.zeros(tot, np.int32)
        o = 0
        for f, n in zip(flat, counts):
            if n:
                tlwh[o:o + n], conf[o:o + n], cls[o:o + n] = np.asarray(f[0]).reshape(-1, 4), f[1], f[2]
                if f[3] is not None:
                    feats[o:o + n] = np.asarray(f[3]).reshape(n, self.feature_dim)
                    valid[o:o + n] = 1 if f[4] is None else np.asarray(f[4]).reshape(n).astype(np.int32)
            o += n
        cap = int(cap_rows if cap_rows is not None else self.max_tracks)
        n_out = np.zeros(max(k, 1), np.int32)
        out6 = np.zeros((max(k, 1), cap, 6), np.int32)
        oconf = np.zeros((max(k, 1), cap), np.float32)
        status = np.zeros(self.streams, np.int32)
        L.call("aic_deepsort_bank_update", self._h, L.ptr(fps), L.ptr(counts), L.ptr(tlwh), L.ptr(conf), L.ptr(cls), L.ptr(feats),
               L.ptr(valid), cap, L.ptr(n_out), L.ptr(out6), L.ptr(oconf), L.ptr(status))
        return self._unpack(fps, n_out, out6, oconf, status, cap)

    def update(self, per_stream_detections):
        """One tick: `streams` entries (tlwh, conf, class_ids, feats[, has_feat]), None = no frame from that camera this tick.  Returns
        `streams` lists of (x1, y1, x2, y2, track_id, class_name, conf) tuples, None for a stopped stream."""
        got = self.update_arrays([[] if d is None else [d] for d in per_stream_detections])
        return [None if g is None else ([(r[0], r[1], r[2], r[3], r[4], config.class_name(r[5]), cf)
                                         for r, cf in zip(g[0][0].tolist(), g[0][1].tolist())] if g else []) for g in got]

    def counters(self, stream):
        """(assignment problems settled by the unique-optimum check, solved by the wave LSAP) of one stream, since create / its reset."""
        a, b = C.c_int64(), C.c_int64()
        L.call("aic_deepsort_bank_counters", self._h, int(stream), C.byref(a), C.byref(b))
        return a.value, b.value

    def export(self, stream):
        """TrackerCore.export_arrays() of one stream; raises for a stopped stream."""
        n = C.c_int32()
        L.call("aic_deepsort_bank_export", self._h, int(stream), 0, *([None] * 10), C.byref(n))
        t = n.value
        a = {k: np.zeros(t, np.int32) for k in ("track_id", "state", "hits", "age", "time_since_update", "cls", "gallery_len")}
        conf, mean, cov = np.zeros(t, np.float32), np.zeros((t, 8), np.float32), np.zeros((t, 8, 8), np.float32)
        L.call("aic_deepsort_bank_export", self._h, int(stream), t, L.ptr(a["track_id"]), L.ptr(a["state"]), L.ptr(a["hits"]), L.ptr(a["age"]),
               L.ptr(a["time_since_update"]), L.ptr(a["cls"]), L.ptr(conf), L.ptr(a["gallery_len"]), L.ptr(mean), L.ptr(cov), C.byref(n))
        a.update(conf=conf, mean=mean, cov=cov)
        return a

    def export_gallery(self, stream, index, gallery_len):
        """The gallery of live track `index` of the stream in FIFO order: [gallery_len, feature_dim] raw embeddings."""
        out = np.zeros((int(gallery_len), self.feature_dim), np.float32)
        if gallery_len:
            L.call("aic_deepsort_bank_export_gallery", self._h, int(stream), int(index), L.ptr(out), int(gallery_len))
        return out
