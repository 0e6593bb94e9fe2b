"""Cross-camera identities for the cameras of one tracker bank (aic_xcam_*, csrc/xcam.hpp, csrc/kernels_xcam.hip): what the gallery
exchange does between ranks (distributed.py), inside one process.  A link pass packs every stream's shard on the device, finds every
live row's nearest row of another camera and applies the global-id policy of csrc/global_id.cpp with world = streams.  The bank's own
association never reads the result."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config


class CrossCamera:
    """CrossCamera(streams, t_max, dim, max_cosine_distance=0.2, device=0): the identities of `streams` cameras.  t_max (1..512) rows per
    camera go into a pass: the first t_max eligible tracks in list order.  A global id is (generation << 44 | stream << 32 | track id)
    of the identity's first sighting; two tracks of different cameras that are each other's nearest neighbour within the threshold
    adopt the smaller one."""

    archive = None

    def __init__(self, streams, t_max, dim, max_cosine_distance=config.DEEPSORT_MAX_DIST, device=0):
        self.streams, self.t_max, self.dim = int(streams), int(t_max), int(dim)
        self.max_cosine_distance = float(max_cosine_distance)
        self._h = C.c_void_p()
        L.call("aic_xcam_create", config.resolve_device(device), self.streams, self.t_max, self.dim, self.max_cosine_distance, C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_xcam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"tile": 32 / 64 = rows per tile of the nearest kernel, 0 = by size.  Same results either way.  "min_gap" (default 1): an
        archived row answers a new track only when its last deposit is more than min_gap passes old."""
        L.call("aic_xcam_option", self._h, str(key).encode(), int(value))

    def attach_archive(self, archive):
        """Every link pass from now on ends with three more steps (archive.py; None detaches): the pass's rows whose key the archive does
        not hold are searched in it, a match within the threshold that is older than min_gap passes gives the new track the archived
        row's identity (one new track per archived row: the nearest), and every valid row of the pass is deposited."""
        L.call("aic_xcam_attach_archive", self._h, None if archive is None else archive._h)
        self.archive = archive

    def returning(self):
        """The last pass's returning tracks: [(stream, track id, archived key, distance)], ascending shard row."""
        n = C.c_int32()
        L.call("aic_xcam_returning", self._h, None, None, None, None, 0, C.byref(n))
        st, ti, ak, di = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.int64), np.zeros(n.value, np.float32)
        L.call("aic_xcam_returning", self._h, L.ptr(st), L.ptr(ti), L.ptr(ak), L.ptr(di), n.value, C.byref(n))
        return [(int(a), int(b), int(c), float(d)) for a, b, c, d in zip(st, ti, ak, di)]

    def _link(self, name, *args):
        n = C.c_int32()
        L.call(name, self._h, *args, C.byref(n))
        return n.value

    def link_bank(self, bank):
        """One pass over a DeepSORTBank or BoTSORTBank, between its update calls.  Returns the identities merged by this call."""
        if bank._abi not in ("aic_deepsort_bank", "aic_botsort_bank"):
            raise TypeError("only DeepSORT and BoT-SORT banks carry appearance vectors")
        return self._link("aic_xcam_link_" + bank._abi[4:], bank._h)

    def link_pipeline(self, pipe):
        """The pass for the bank of a TrackingPipeline.botsort_bank / deepsort_bank pipeline, between run calls."""
        n = C.c_int32()
        L.call("aic_pipeline_link_cameras", pipe._h, self._h, C.byref(n))
        return n.value

    def link_shards(self, shards, n_valid=None):
        """The pass on caller-made shards: fp32 [streams, t_max, 2 + dim] = (valid, track id, unit embedding) as a NumPy array, or a
        torch tensor on the device.  n_valid [streams] (optional) = the valid prefix of every stream."""
        nv = None if n_valid is None else np.ascontiguousarray(n_valid, dtype=np.int32).reshape(self.streams)
        shape = (self.streams, self.t_max, 2 + self.dim)
        if isinstance(shards, np.ndarray):
            a = L.as_f32(shards)
            if a.shape != shape:
                raise ValueError(f"shards of shape {a.shape}, expected {shape}")
            return self._link("aic_xcam_link_shards", L.ptr(a), L.ptr(nv), L.HOST)
        if tuple(shards.shape) != shape or not shards.is_contiguous() or str(shards.dtype) != "torch.float32":
            raise ValueError(f"device shards must be a contiguous float32 tensor of shape {shape}")
        mem = L.DEVICE if shards.is_cuda else L.HOST
        return self._link("aic_xcam_link_shards", C.c_void_p(shards.data_ptr()), L.ptr(nv), mem)

    def tables(self):
        """(track_id, near_row, near_dist) of the last pass over all streams * t_max rows, as distributed.annotate's."""
        n = self.streams * self.t_max
        ids, nr, nd = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        L.call("aic_xcam_tables", self._h, L.ptr(ids), L.ptr(nr), L.ptr(nd))
        return ids, nr, nd

    def shards(self):
        """The last pass's shard array, fp32 [streams, t_max, 2 + dim]."""
        out = np.zeros((self.streams, self.t_max, 2 + self.dim), np.float32)
        L.call("aic_xcam_shards", self._h, L.ptr(out))
        return out

    def global_ids(self, stream, track_ids):
        """int64 global ids of the stream's local track ids; -1 = never seen in a pass."""
        t = np.ascontiguousarray(track_ids, dtype=np.int32).reshape(-1)
        out = np.full(len(t), -1, np.int64)
        L.call("aic_xcam_global_ids", self._h, int(stream), L.ptr(t), len(t), L.ptr(out))
        return out

    def size(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.call("aic_xcam_size", self._h, C.byref(a), C.byref(b), C.byref(c))
        return dict(tracks=a.value, identities=b.value, links=c.value)

    def forget_stream(self, stream):
        """The camera's local ids start over (its bank stream was reset): its keys of now are never met again."""
        L.call("aic_xcam_forget_stream", self._h, int(stream))


class CameraLinks:
    """What DeepSORTBank and BoTSORTBank add to TrackerBank: link_cameras() / global_ids() through an attached CrossCamera."""
    xcam = None

    def _link_threshold(self):
        return config.DEEPSORT_MAX_DIST

    def link_cameras(self, xcam=None, archive=None):
        """One cross-camera pass over the bank, between update calls.  The first call creates and keeps a CrossCamera (t_max = max_tracks:
        every eligible track takes part) unless one is handed over; returns the identities merged by this call.  archive: an
        IdentityArchive to attach to it (CrossCamera.attach_archive); it stays attached."""
        if xcam is not None:
            self.xcam = xcam
        if self.xcam is None:
            self.xcam = CrossCamera(self.streams, self.max_tracks or 512, self.feature_dim, self._link_threshold(), device=self._device)
        if archive is not None and self.xcam.archive is not archive:
            self.xcam.attach_archive(archive)
        return self.xcam.link_bank(self)

    def global_ids(self, stream, track_ids):
        if self.xcam is None:
            raise RuntimeError("link_cameras() has not run yet")
        return self.xcam.global_ids(stream, track_ids)

    def reset(self, stream):
        super().reset(stream)
        if self.xcam is not None:
            self.xcam.forget_stream(stream)
