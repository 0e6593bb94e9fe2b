"""Zone entries, dwell and line crossings per camera, on the device (aic_zones_*, csrc/zones.hpp, csrc/kernels_zones.hip; DESIGN.md
section 27): what an operator reads off the tracks -- how many are in this area now, how many came in and went out through that door,
how long each stayed.  One tracker-agnostic stage over the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32), for a bank of
1..256 cameras per call.  Exact integer arithmetic; tests/zones_oracle.py is the specification."""
from __future__ import annotations

import ctypes as C
import json
from collections import namedtuple

import numpy as np

from . import _bank_io as IO
from . import _lib as L
from . import config

ENTER, EXIT, LOST, CROSS = 1, 2, 3, 4
KINDS = {ENTER: "enter", EXIT: "exit", LOST: "lost", CROSS: "cross"}
MAX_ZONES = MAX_LINES = MAX_VERTS = 32
MAX_ROWS = MAX_TRACKS = 512
COORD_MAX = 1 << 20

ZoneResult = namedtuple("ZoneResult", "n_events events occupancy status frames_per_stream")
ZoneResult.__doc__ = """Flat, stream-major (stream 0's frames, then stream 1's, ...): n_events [F] true counts, events [F, cap_events, 8] =
kind, index, track id, cls, frame, value, doubled anchor x, y (truncated at cap_events), occupancy [F, 32], status [streams] = 0 or the
code a stream stopped with, frames_per_stream [streams]."""


def load_zones_file(path_or_obj, n_cameras):
    """The CLI's --zones file: {"cameras": [{"zones": [[[x, y], ...], ...], "lines": [[[x, y], [x, y]], ...]}, ...]} -> `n_cameras`
    pairs (zones, lines) of integer arrays.  One entry serves every camera; otherwise the file names exactly n_cameras of them."""
    if isinstance(path_or_obj, (str, bytes)):
        with open(path_or_obj) as f:
            doc = json.load(f)
    else:
        doc = path_or_obj
    cams = doc.get("cameras") if isinstance(doc, dict) else None
    if not isinstance(cams, list) or not cams:
        raise ValueError('a zones file is {"cameras": [{"zones": [...], "lines": [...]}, ...]} with at least one camera')
    if len(cams) == 1:
        cams = cams * int(n_cameras)
    if len(cams) != int(n_cameras):
        raise ValueError(f"the zones file names {len(cams)} cameras, the run has {n_cameras} (one entry would serve all)")
    out = []
    for i, cam in enumerate(cams):
        if not isinstance(cam, dict) or set(cam) - {"zones", "lines"}:
            raise ValueError(f"camera {i}: an object with \"zones\" and \"lines\" only")
        out.append(check_geometry(cam.get("zones", []), cam.get("lines", []), what=f"camera {i}: "))
    return out


def _int_points(pts, what):
    a = np.asarray(pts)
    if a.ndim != 2 or a.shape[1] != 2 or a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and np.all(a == np.round(a))):
        raise ValueError(what + "points are [x, y] pairs of integer pixels")
    a = a.astype(np.int64)
    if np.any(np.abs(a) > COORD_MAX):
        raise ValueError(what + "a coordinate is outside +-2^20")
    return a.astype(np.int32)


def check_geometry(zones, lines, what=""):
    """(zones, lines) as lists of int32 arrays [n_vert, 2] / [2, 2], or ValueError: the limits of aic_zones_set."""
    if len(zones) > MAX_ZONES or len(lines) > MAX_LINES:
        raise ValueError(what + "at most 32 zones and 32 lines per camera")
    zs = [_int_points(z, what) for z in zones]
    for z in zs:
        if not 3 <= len(z) <= MAX_VERTS:
            raise ValueError(what + "a zone has 3..32 vertices")
    ls = [_int_points(l, what) for l in lines]
    for l in ls:
        if len(l) != 2:
            raise ValueError(what + "a line is two points")
    return zs, ls


class ZoneCounter:
    """ZoneCounter(streams=1, max_tracks=512, forget_after=70, anchor="bottom", device=0): zones and lines of `streams` cameras.
    anchor: "bottom" = the bottom centre of a box (feet on the ground), "centre" = its centre.  A track unseen for more than
    forget_after frames is forgotten (LOST events for the zones it was in).  The device is first touched by update()."""

    def __init__(self, streams=1, max_tracks=512, forget_after=70, anchor="bottom", device=0):
        if anchor not in ("bottom", "centre", "center"):
            raise ValueError("anchor must be 'bottom' or 'centre'")
        self.streams, self.max_tracks, self.forget_after, self.anchor = int(streams), int(max_tracks), int(forget_after), anchor
        self.failed = {}                                         # stream -> message
        self.n_zones, self.n_lines = [0] * self.streams, [0] * self.streams
        self._h = C.c_void_p()
        L.call("aic_zones_create", config.resolve_device(device), self.streams, self.max_tracks, self.forget_after,
               0 if anchor == "bottom" else 1, C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_zones_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"frames_per_launch": 0 = a call's frames in one launch (default), k = at most k frames of a stream per launch.  Same results."""
        L.call("aic_zones_option", self._h, str(key).encode(), int(value))

    def set_zones(self, stream, zones=(), lines=()):
        """zones: polygons [[x, y], ...] of 3..32 integer-pixel vertices; lines: [[ax, ay], [bx, by]], directed A->B (+1 = a track ends on
        the left of A->B in a y-up frame, i.e. cross(B - A, p - A) >= 0).  Between updates; the stream's state and counters start over."""
        zs, ls = check_geometry(zones, lines)
        nv = np.array([len(z) for z in zs], np.int32)
        xy = np.ascontiguousarray(np.concatenate(zs) if zs else np.zeros((0, 2), np.int32))
        lx = np.ascontiguousarray(np.stack(ls) if ls else np.zeros((0, 2, 2), np.int32))
        L.call("aic_zones_set", self._h, int(stream), len(zs), L.ptr(nv) if zs else None, L.ptr(xy) if zs else None, len(ls), L.ptr(lx) if ls else None)
        self.n_zones[int(stream)], self.n_lines[int(stream)] = len(zs), len(ls)
        self.failed.pop(int(stream), None)

    def reset(self, stream):
        """The stream's table and counters as after set_zones, a stop cleared: a camera reconnecting."""
        L.call("aic_zones_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def _run(self, fps, counts, rows_ptr, mem, cap):
        F = int(fps.sum())
        n_events = np.zeros(F, np.int32)
        events = np.zeros((F, cap, 8), np.int32)
        occ = np.zeros((F, MAX_ZONES), np.int32)
        status = np.zeros(self.streams, np.int32)
        L.call("aic_zones_update", self._h, L.ptr(fps), L.ptr(counts), rows_ptr, mem, cap, L.ptr(n_events), L.ptr(events), L.ptr(occ), L.ptr(status))
        for s in np.nonzero(status)[0]:
            self.failed.setdefault(int(s), f"stream {s} stopped with libaicam error {int(status[s])} (reset({s}) starts it afresh)")
        return ZoneResult(n_events, events, occ, status, fps)

    def update(self, frames, counts=None, frames_per_stream=None, cap_events=256):
        """frames: `streams` lists of rows [n, 6] int32 arrays (x1 y1 x2 y2 id cls), any length each, a frame per entry.  Or ONE array /
        torch tensor (host or device) [rows, 6] int32 holding every frame's rows stream-major, with counts [F] and frames_per_stream
        [streams].  Returns a ZoneResult; a stream that stopped is noted in .failed and delivers nothing until reset()."""
        cap = int(cap_events)
        if counts is None:
            if len(frames) != self.streams:
                raise ValueError(f"{len(frames)} frame lists for a counter of {self.streams} streams")
            fps = np.array([len(fr) for fr in frames], np.int32)
            flat = [np.asarray(r, dtype=np.int32).reshape(-1, 6) for fr in frames for r in fr]
            cnt = np.array([len(r) for r in flat], np.int32)
            rows = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros((0, 6), np.int32))
            return self._run(fps, cnt, L.ptr(rows) if len(rows) else None, L.HOST, cap)
        cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        fps = np.ascontiguousarray(frames_per_stream if frames_per_stream is not None else [len(cnt)], dtype=np.int32).reshape(-1)
        if len(fps) != self.streams or int(fps.sum()) != len(cnt):
            raise ValueError("frames_per_stream must name every stream and sum to len(counts)")
        total = int(cnt.sum())
        if isinstance(frames, np.ndarray):
            rows = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1, 6)
            if len(rows) < total:
                raise ValueError(f"{len(rows)} rows, counts sum to {total}")
            return self._run(fps, cnt, L.ptr(rows) if total else None, L.HOST, cap)
        if str(frames.dtype) != "torch.int32" or not frames.is_contiguous() or frames.numel() < total * 6:
            raise ValueError("device rows must be a contiguous int32 tensor of at least sum(counts) * 6 elements")
        if frames.is_cuda:
            import torch
            torch.cuda.current_stream(frames.device).synchronize()      # the rows are read on the library's own stream
        return self._run(fps, cnt, C.c_void_p(frames.data_ptr()) if total else None, L.DEVICE if frames.is_cuda else L.HOST, cap)

    def update_tuples(self, frames, cap_events=256):
        """As update(), from the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) DeepSORT.update and the other trackers return:
        `streams` lists of frames, a frame being a list of tuples."""
        return self.update(IO.rows_from_tuples(frames), cap_events=cap_events)

    def counters(self, stream):
        """dict(zone_in, zone_out [n_zones], line_pos, line_neg [n_lines]): cumulative int64 counts since set_zones / reset."""
        a = [np.zeros(MAX_ZONES, np.int64) for _ in range(4)]
        L.call("aic_zones_counters", self._h, int(stream), *(L.ptr(x) for x in a))
        nz, nl = self.n_zones[int(stream)], self.n_lines[int(stream)]
        return dict(zone_in=a[0][:nz], zone_out=a[1][:nz], line_pos=a[2][:nl], line_neg=a[3][:nl])

    @staticmethod
    def event_lists(result):
        """The events of a ZoneResult per stream and frame: [[ [event row, ...] per frame ] per stream], truncated rows only."""
        out, f = [], 0
        for n in result.frames_per_stream:
            out.append([result.events[i, :min(int(result.n_events[i]), result.events.shape[1])] for i in range(f, f + int(n))])
            f += int(n)
        return out
