"""What the analytics classes (BestShots, TrackColours, HeatMaps, SceneWatch, LeftObjects, ZoneCounter) share in front of a library call: the
memory of an argument, nested row lists made flat, the counts that travel with the rows, tracker tuples made rows.
Each class keeps its own checks; what differs between them is an argument here, not a copy there."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import config


def memory(a, what, dtype):
    """(pointer, AIC_HOST / AIC_DEVICE, keep-alive) of a NumPy array or a contiguous torch tensor."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, dtype=dtype)
        return L.ptr(a), L.HOST, a
    if str(a.dtype) != "torch." + np.dtype(dtype).name or not a.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {np.dtype(dtype).name} tensor")
    if a.is_cuda:
        import torch
        torch.cuda.current_stream(a.device).synchronize()  # the library reads it on its own stream
    return C.c_void_p(a.data_ptr()), L.DEVICE if a.is_cuda else L.HOST, a


def flat_rows(rows, ticks, streams):
    """rows[tick][stream] = [n, 6] -> (ONE int32 array [rows, 6] in that order, counts [ticks * streams])."""
    if len(rows) != ticks or any(len(r) != streams for r in rows):
        raise ValueError(f"rows must be [ticks = {ticks}][streams = {streams}] arrays")
    flat = [np.asarray(r, dtype=np.int32).reshape(-1, 6) for tick in rows for r in tick]
    counts = np.array([len(r) for r in flat], np.int32)
    return np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros((0, 6), np.int32)), counts


def n_rows_of(r_keep):
    return r_keep.size // 6 if isinstance(r_keep, np.ndarray) else r_keep.numel() // 6


def _beside_rows(host_counts, rows, r_mem):
    """counts and rows travel together: host counts go where the rows are.  -> (pointer, keep-alive)"""
    if r_mem == L.DEVICE:
        import torch
        keep = torch.from_numpy(host_counts).to(rows.device)
        return C.c_void_p(keep.data_ptr()), keep
    return L.ptr(host_counts), host_counts


def counts_for(rows, counts, r_mem, ticks, streams, need_total):
    """The counts of the slot stages' update, beside rows (the tensor or array memory() kept).  Device counts stay where they are: the
    library fetches them for its checks, and their total is read back only when the class needs it (need_total).  Host counts are summed
    and checked against the rows.  -> (pointer, keep-alive, total or None)"""
    n_rows, total = n_rows_of(rows), None
    if getattr(counts, "is_cuda", False):
        if r_mem != L.DEVICE:
            raise ValueError("counts on the device need rows on the device")
        c_ptr, _, c_keep = memory(counts, "counts", np.int32)
        n_counts = counts.numel()
        if need_total:
            total = int(counts.sum().item())
        host = None
    else:
        host = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        n_counts, total = len(host), int(host.sum())
    if total is not None and n_rows < total:
        raise ValueError(f"{n_rows} rows, counts sum to {total}")
    if host is not None:
        c_ptr, c_keep = _beside_rows(host, rows, r_mem)
    if n_counts != ticks * streams:
        raise ValueError("counts must name every frame of the call")
    return c_ptr, c_keep, total


def counts_on_host(rows, counts, r_mem, ticks, streams):
    """The counts of the cell stages' update (scene watch, left objects): they slice their per-row outputs, so the counts are wanted on
    the host wherever they lie, and are checked here.  -> (pointer, keep-alive, host counts)"""
    host = counts.cpu().numpy() if hasattr(counts, "is_cuda") else counts
    host = np.ascontiguousarray(host, dtype=np.int32).reshape(-1)
    if len(host) != ticks * streams:
        raise ValueError("counts must name every frame of the call")
    n_rows, total = n_rows_of(rows), int(host.sum())
    if (host < 0).any() or n_rows < total:
        raise ValueError(f"{n_rows} rows, counts sum to {total}")
    if r_mem == L.DEVICE and getattr(counts, "is_cuda", False):
        c_ptr, _, c_keep = memory(counts, "counts", np.int32)
    else:
        c_ptr, c_keep = _beside_rows(host, rows, r_mem)
    return c_ptr, c_keep, host


def rows_from_tuples(tracks):
    """tracks[i][j] = a list of the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) the trackers return -> [i][j] int32 [n, 6]."""
    ids = {n: i for i, n in enumerate(config.CLASSES)}
    return [[np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in fr], np.int64).reshape(-1, 6).astype(np.int32) for fr in outer]
            for outer in tracks]
