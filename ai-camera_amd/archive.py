"""The identity archive (aic_archive_*, csrc/archive.hpp, csrc/kernels_archive.hip): appearance rows of tracks that
have ended, kept on the device as int8 codes with one scale a row and searched with int8 MFMA.  It answers "where has this person been
seen?" and, attached to a CrossCamera, gives a returning person the identity they had."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config

_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1


class ArchiveFilter(C.Structure):
    _fields_ = [("exclude_camera", C.c_int32), ("max_distance", C.c_float), ("t_lo", C.c_int64), ("t_hi", C.c_int64),
                ("exclude_key", C.c_int64)]


def _rows(a, dim):
    """(pointer, n, mem) of fp32 rows [n, dim]: a NumPy array, or a contiguous float32 torch tensor on the host or the device."""
    if isinstance(a, np.ndarray) or not hasattr(a, "data_ptr"):
        a = L.as_f32(a).reshape(-1, dim)
        return a, L.ptr(a), len(a), L.HOST
    if a.dim() != 2 or a.shape[1] != dim or not a.is_contiguous() or str(a.dtype) != "torch.float32":
        raise ValueError(f"rows must be a contiguous float32 tensor of shape [n, {dim}]")
    return a, C.c_void_p(a.data_ptr()), int(a.shape[0]), L.DEVICE if a.is_cuda else L.HOST


class IdentityArchive:
    """IdentityArchive(capacity, dim, device=0): up to `capacity` (1..2^24) rows of `dim` (a multiple of 4 in 4..1024) elements.  A row is
    known by an int64 key >= 0 and carries a camera and the ticks of its first and last deposit; a full archive evicts the row that was
    deposited longest ago."""

    def __init__(self, capacity, dim, device=0):
        self.capacity, self.dim = int(capacity), int(dim)
        self._h = C.c_void_p()
        L.call("aic_archive_create", config.resolve_device(device), self.capacity, self.dim, C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_archive_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def pitch(self):
        return (self.dim + 63) // 64 * 64

    def put(self, keys, cameras, tick, rows):
        """Upsert rows [n, dim] (NumPy, or a torch tensor on the device) under keys [n] at `tick`.  A row that is all zero or not finite
        fails the call and nothing of it is stored."""
        k = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cameras, np.int32), k.shape))
        keep, p, n, mem = _rows(rows, self.dim)
        if n != len(k):
            raise ValueError(f"{n} rows for {len(k)} keys")
        L.call("aic_archive_put", self._h, L.ptr(k), L.ptr(c), int(tick), p, n, mem)

    def remove(self, key):
        L.call("aic_archive_remove", self._h, int(key))

    def search(self, queries, k=1, exclude_camera=-1, since=None, until=None, exclude_key=-1, max_distance=float("inf")):
        """The k nearest eligible rows of every query [n, dim]: (keys int64, slots int32, dist fp32), each [n, k], nearest first; missing
        places hold -1, -1 and 1e5.  Filters (a scalar, or one value per query): the row's camera differs from exclude_camera, its last
        deposit lies in [since, until], its key differs from exclude_key, and its distance is at most max_distance."""
        keep, p, n, mem = _rows(queries, self.dim)
        per = lambda x, t: np.broadcast_to(np.asarray(x, t), (n,))      # noqa: E731
        f = (ArchiveFilter * max(n, 1))()
        ec, lo, hi = per(exclude_camera, np.int32), per(_I64_MIN if since is None else since, np.int64), per(_I64_MAX if until is None else until, np.int64)
        ek, md = per(exclude_key, np.int64), per(max_distance, np.float32)
        for i in range(n):
            f[i] = ArchiveFilter(int(ec[i]), float(md[i]), int(lo[i]), int(hi[i]), int(ek[i]))
        keys, slots, dist = np.full((n, k), -1, np.int64), np.full((n, k), -1, np.int32), np.full((n, k), 1e5, np.float32)
        L.call("aic_archive_search", self._h, p, n, mem, int(k), C.cast(f, C.c_void_p), L.ptr(keys), L.ptr(slots), L.ptr(dist))
        return keys, slots, dist

    def size(self):
        a, b = C.c_int64(), C.c_int64()
        L.call("aic_archive_size", self._h, C.byref(a), C.byref(b))
        return a.value

    def high_water(self):
        a, b = C.c_int64(), C.c_int64()
        L.call("aic_archive_size", self._h, C.byref(a), C.byref(b))
        return b.value

    def block_rows(self, n_queries=1):
        """The slots one block of a search of n_queries owns at the present high-water mark (tests, measurements)."""
        r = C.c_int32()
        L.call("aic_archive_block_rows", self._h, int(n_queries), C.byref(r))
        return r.value

    def export(self):
        """dict of the slots below the high-water mark: keys (-1 = free), cameras, t_first, t_last, scales, rows int8 [n, pitch]."""
        n = self.high_water()
        out = dict(keys=np.zeros(n, np.int64), cameras=np.zeros(n, np.int32), t_first=np.zeros(n, np.int64), t_last=np.zeros(n, np.int64),
                   scales=np.zeros(n, np.float32), rows=np.zeros((n, self.pitch), np.int8))
        m = C.c_int64()
        L.call("aic_archive_export", self._h, *(L.ptr(out[k]) for k in ("keys", "cameras", "t_first", "t_last", "scales", "rows")), C.byref(m))
        assert m.value == n
        return out

    def import_(self, d):
        a = {k: np.ascontiguousarray(d[k], dtype=t) for k, t in (("keys", np.int64), ("cameras", np.int32), ("t_first", np.int64),
                                                                ("t_last", np.int64), ("scales", np.float32), ("rows", np.int8))}
        n = len(a["keys"])
        if a["rows"].shape != (n, self.pitch) or any(len(a[k]) != n for k in a):
            raise ValueError(f"an export of another shape: rows {a['rows'].shape}, expected ({n}, {self.pitch})")
        L.call("aic_archive_import", self._h, *(L.ptr(a[k]) for k in ("keys", "cameras", "t_first", "t_last", "scales", "rows")), n)

    def clear(self):
        L.call("aic_archive_clear", self._h)

    def save(self, path):
        """The export as an .npz (with the dimension, which load() checks)."""
        with open(path, "wb") as fh:
            np.savez(fh, dim=np.int64(self.dim), **self.export())

    def load(self, path):
        with np.load(path) as z:
            if int(z["dim"]) != self.dim:
                raise ValueError(f"{path} holds rows of dimension {int(z['dim'])}, the archive has {self.dim}")
            self.import_({k: z[k] for k in ("keys", "cameras", "t_first", "t_last", "scales", "rows")})
