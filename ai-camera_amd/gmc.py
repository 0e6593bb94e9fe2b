"""Camera-motion estimation on the device (csrc/kernels_gmc.hip): the 2x3 affine that BoT-SORT's ``warp`` argument takes.

Upstream's ``GMC.apply`` runs OpenCV (sparse optical flow or ORB + RANSAC) on the host; here a gray pyramid level, integer block
matching with an integer sub-pixel step and a robust similarity fit from exact integer sums run in three kernels, and equal inputs give
equal bits.  The specification is tests/gmc_oracle.py.  Working range per frame: a translation below
8 * downscale pixels, about 1.4 degrees of rotation or 2.5 % of zoom; beyond it, and for a stream's first frame, the identity.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config


class CameraMotion:
    """apply(frame_bgr, boxes_xyxy=None) -> float32[2, 3]: previous-frame pixel coordinates -> current-frame ones (the shape of
    upstream's GMC.apply).  `stats` holds (ok, blocks, blocks that entered the fit, inliers) of the last call's frames."""

    def __init__(self, height, width, downscale=4, min_inliers=8, device=0):
        self.height, self.width, self.downscale = int(height), int(width), int(downscale)
        self.params = L.GmcParams(downscale=self.downscale, min_inliers=int(min_inliers))
        self._h = C.c_void_p()
        L.call("aic_gmc_create", config.resolve_device(device), self.height, self.width, C.byref(self.params), C.byref(self._h))
        self.stats = np.zeros((0, 4), np.int32)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_gmc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """The next frame is a stream's first."""
        L.call("aic_gmc_reset", self._h)

    def apply_batch(self, frames, boxes_list=None):
        """frames: uint8 [k, H, W, 3] BGR (NumPy), or (device address, k) of such frames in HBM; boxes_list: per frame [n, 4] xyxy or
        None.  Returns float32 [k, 2, 3]."""
        if isinstance(frames, tuple):
            src, k, mem = L.ptr(int(frames[0])), int(frames[1]), L.DEVICE
        else:
            f = np.ascontiguousarray(frames, dtype=np.uint8)
            if f.ndim == 3:
                f = f[None]
            if f.shape[1:] != (self.height, self.width, 3):
                raise ValueError(f"frames must be [k, {self.height}, {self.width}, 3], not {f.shape}")
            src, k, mem = L.ptr(f), len(f), L.HOST
        counts = boxes = None
        if boxes_list is not None:
            if len(boxes_list) != k:
                raise ValueError("one box array (or None) per frame")
            bl = [np.zeros((0, 4), np.float32) if b is None else np.asarray(b, dtype=np.float32).reshape(-1, 4) for b in boxes_list]
            counts = np.array([len(b) for b in bl], dtype=np.int32)
            boxes = np.ascontiguousarray(np.concatenate(bl) if k else np.zeros((0, 4), np.float32))
            if not len(boxes):
                boxes = np.zeros((1, 4), np.float32)
        warps = np.zeros((k, 2, 3), np.float32)
        stats = np.zeros((k, 4), np.int32)
        L.call("aic_gmc_estimate_batch", self._h, src, k, mem, L.ptr(counts), L.ptr(boxes), L.ptr(warps), L.ptr(stats))
        self.stats = stats
        return warps

    def apply(self, frame_bgr, boxes_xyxy=None):
        return self.apply_batch(np.asarray(frame_bgr)[None], None if boxes_xyxy is None else [boxes_xyxy])[0]


class CameraMotionBank:
    """The estimator of `streams` cameras of one frame size (aic_gmc_bank_*).  apply_ticks(frames, boxes_list=None) takes whole ticks,
    tick-major (frame t * streams + s = tick t of camera s), and returns float32 [ticks * streams, 2, 3]; every camera's rows are what
    a CameraMotion fed that camera's frames returns.  reset(stream): that camera's next frame is its first."""

    def __init__(self, streams, height, width, downscale=4, min_inliers=8, device=0):
        self.streams = int(streams)
        self.height, self.width, self.downscale = int(height), int(width), int(downscale)
        self.params = L.GmcParams(downscale=self.downscale, min_inliers=int(min_inliers))
        self._h = C.c_void_p()
        L.call("aic_gmc_bank_create", config.resolve_device(device), self.height, self.width, C.byref(self.params), self.streams,
               C.byref(self._h))
        self.stats = np.zeros((0, 4), np.int32)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_gmc_bank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream):
        L.call("aic_gmc_bank_reset", self._h, int(stream))

    def apply_ticks(self, frames, boxes_list=None):
        """frames: uint8 [ticks * streams, H, W, 3] BGR (NumPy), or (device address, frames) of such frames in HBM; boxes_list: per
        frame [n, 4] xyxy or None."""
        if isinstance(frames, tuple):
            src, k, mem = L.ptr(int(frames[0])), int(frames[1]), L.DEVICE
        else:
            f = np.ascontiguousarray(frames, dtype=np.uint8)
            if f.ndim != 4 or f.shape[1:] != (self.height, self.width, 3):
                raise ValueError(f"frames must be [k, {self.height}, {self.width}, 3], not {f.shape}")
            src, k, mem = L.ptr(f), len(f), L.HOST
        if k % self.streams:
            raise ValueError(f"{k} frames are no whole ticks of {self.streams} cameras")
        counts = boxes = None
        if boxes_list is not None:
            if len(boxes_list) != k:
                raise ValueError("one box array (or None) per frame")
            bl = [np.zeros((0, 4), np.float32) if b is None else np.asarray(b, dtype=np.float32).reshape(-1, 4) for b in boxes_list]
            counts = np.array([len(b) for b in bl], dtype=np.int32)
            boxes = np.ascontiguousarray(np.concatenate(bl) if k else np.zeros((0, 4), np.float32))
            if not len(boxes):
                boxes = np.zeros((1, 4), np.float32)
        warps = np.zeros((k, 2, 3), np.float32)
        stats = np.zeros((k, 4), np.int32)
        L.call("aic_gmc_bank_estimate", self._h, src, k // self.streams, mem, L.ptr(counts), L.ptr(boxes), L.ptr(warps), L.ptr(stats))
        self.stats = stats
        return warps
