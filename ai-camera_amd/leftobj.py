"""Left objects: abandoned and removed items per camera (aic_left_*, csrc/left.hpp, csrc/kernels_left.hip).
One tracker-agnostic stage over the frames and the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32) for a bank of 1..256
cameras per call: the cells that stayed changed while nobody stood on them, their 8-connected blobs, and per camera a table of objects
that appear, are alarmed as LEFT or REMOVED and end.  Integer arithmetic only; tests/left_oracle.py is the specification."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _bank_io as IO
from . import _lib as L
from . import config
from .scene import SceneWatch

APPEARED, RAISED, ENDED = 1, 2, 3
EVENT_NAMES = {APPEARED: "appeared", RAISED: "raised", ENDED: "ended"}
LEFT, REMOVED = 1, 2
KIND_NAMES = ("", "LEFT", "REMOVED")
MAX_ROWS = 512
RECORD_FIELDS = ("frame", "ready", "n_cand", "n_blobs", "n_objects", "n_alarmed", "flags", "dropped")
OBJECT_FIELDS = ("uid", "kind", "alarmed", "x0", "y0", "x1", "y1", "owner", "born", "area", "seen", "missing")
EVENT_FIELDS = ("tick", "stream", "type", "uid", "kind", "x0", "y0", "x1", "y1", "owner", "area", "age")
OPTIONS = ("fast_shift", "slow_shift", "thresh", "warmup", "decay", "min_ticks", "absorb_ticks", "pad_cells", "owner_window", "min_cells",
           "max_cells", "alarm_hold", "gone_ticks", "ticks_per_launch", "launch_budget_mb")


class LeftResult:
    """records int32 [ticks, S, 8] (RECORD_FIELDS; every field is also an attribute, a [ticks, S] view); objects int32 [ticks, S,
    max_objects, 12] (OBJECT_FIELDS; uid 0 = a free slot); events int32 [n, 12] (EVENT_FIELDS) in tick, stream, slot order; n_events:
    how many the call raised; overflow: more than cap_events, the list is cut (the state is not); cand u8 / labels int32 [ticks, S, Hc, Wc]
    or None."""

    def __init__(self, records, objects, events, n_events, cand=None, labels=None):
        self.records, self.objects, self.events, self.n_events, self.cand, self.labels = records, objects, events, int(n_events), cand, labels
        self.overflow = self.n_events > len(events)

    def __getattr__(self, name):
        if name in RECORD_FIELDS:
            return self.records[..., RECORD_FIELDS.index(name)]
        raise AttributeError(name)

    def alarmed(self, stream, tick):
        """[dict(uid, kind, box, owner, age)] of the alarmed objects of one frame, in slot order."""
        age = int(self.records[tick, stream, 0])
        return [dict(uid=int(o[0]), kind=KIND_NAMES[int(o[1])], box=[int(v) for v in o[3:7]], owner=int(o[7]), age=age - int(o[8]))
                for o in self.objects[tick, stream] if o[0] and o[2]]

    def events_of(self, stream, tick):
        e = self.events
        return e[(e[:, 0] == tick) & (e[:, 1] == stream)]

    def prims(self, stream, tick, pl=None):
        """A visualization.PrimList segment for render.Renderer: every live object a rectangle, labelled `LEFT 7 <- 12` (kind, uid,
        owner) once alarmed."""
        from . import visualization
        pl = pl if pl is not None else visualization.PrimList()
        for o in self.objects[tick, stream]:
            if not o[0]:
                continue
            x0, y0, x1, y1 = (int(v) for v in o[3:7])
            if o[2]:
                color = (0, 0, 255) if o[1] == LEFT else (0, 165, 255)
                label = f"{KIND_NAMES[int(o[1])]} {int(o[0])}" + (f" <- {int(o[7])}" if o[7] >= 0 else "")
                visualization.labelled_box(pl, x0, y0, x1, y1, color, label, 2)
            else:
                pl.outline(x0, y0, x1, y1, (0, 255, 255))
        return pl


class LeftObjects:
    """LeftObjects(streams, frame_hw, cell=8, max_objects=32, device=0, **options): options are the thresholds of OPTIONS (option).
    The device is first touched by update."""

    def __init__(self, streams, frame_hw, cell=8, max_objects=32, device=0, **options):
        self.streams, self.frame_h, self.frame_w, self.cell = int(streams), int(frame_hw[0]), int(frame_hw[1]), int(cell)
        self.max_objects = int(max_objects)
        cfg = L.LeftConfig(self.streams, self.frame_h, self.frame_w, self.cell, self.max_objects)
        self._h = C.c_void_p()
        L.call("aic_left_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))
        self.grid_h, self.grid_w = self.frame_h // self.cell, self.frame_w // self.cell
        try:
            for k, v in options.items():
                self.option(k, v)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_left_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """A threshold of the specification, or "ticks_per_launch" / "launch_budget_mb" (same results).  None sizes a buffer: they may
        change between calls."""
        L.call("aic_left_option", self._h, str(key).encode(), int(value))

    def reset(self, stream=None):
        """The stream (None: every stream) starts again at age 0, its objects forgotten and its uids from 1."""
        L.call("aic_left_reset", self._h, -1 if stream is None else int(stream))

    def update(self, frames, rows=None, counts=None, cap_events=256, want_masks=False):
        """frames: uint8 [ticks, streams, H, W, 3] BGR, tick-major, a NumPy array or a torch tensor (host or device, any alignment).
        rows (optional): per tick, per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6]
        holding them in that order, with counts [ticks * streams].  Returns a LeftResult; with want_masks it carries cand and labels."""
        shape = tuple(frames.shape)
        if len(shape) != 5 or shape[1:] != (self.streams, self.frame_h, self.frame_w, 3):
            raise ValueError(f"frames of shape {shape}, not [ticks, {self.streams}, {self.frame_h}, {self.frame_w}, 3]")
        ticks, S, M = shape[0], self.streams, self.max_objects
        cap_events = int(cap_events)
        f_ptr, f_mem, f_keep = SceneWatch._memory(frames, "frames", np.uint8)
        r_ptr = c_ptr = None
        r_mem = L.HOST
        if rows is not None:
            if counts is None:
                rows, counts = IO.flat_rows(rows, ticks, S)
            r_ptr, r_mem, r_keep = SceneWatch._memory(rows, "rows", np.int32)
            c_ptr, c_keep, _ = IO.counts_on_host(r_keep, counts, r_mem, ticks, S)
        rec = np.zeros((ticks, S, 8), np.int32)
        obj = np.zeros((ticks, S, M, 12), np.int32)
        ev = np.zeros((max(cap_events, 0), 12), np.int32)
        n_ev, status = C.c_int32(0), C.c_int32(0)
        cand = np.zeros((ticks, S, self.grid_h, self.grid_w), np.uint8) if want_masks else None
        labels = np.full((ticks, S, self.grid_h, self.grid_w), -1, np.int32) if want_masks else None
        L.call("aic_left_update", self._h, f_ptr if ticks else None, f_mem, ticks, c_ptr if ticks else None, r_ptr, r_mem, cap_events, L.ptr(rec),
               L.ptr(obj), L.ptr(ev), C.byref(n_ev), C.byref(status), L.ptr(cand), L.ptr(labels))
        return LeftResult(rec, obj, ev[:min(n_ev.value, len(ev))], n_ev.value, cand, labels)

    def export(self, stream):
        """dict(fast, slow, still, last_id, last_tick: int32 [Hc, Wc]; slots int32 [max_objects, 12]; age, uids: int) of one stream.
        Changes nothing."""
        planes = [np.zeros((self.grid_h, self.grid_w), np.int32) for _ in range(5)]
        slots, sc = np.zeros((self.max_objects, 12), np.int32), np.zeros(4, np.int32)
        L.call("aic_left_export", self._h, int(stream), *(L.ptr(p) for p in planes), L.ptr(slots), L.ptr(sc))
        return dict(fast=planes[0], slow=planes[1], still=planes[2], last_id=planes[3], last_tick=planes[4], slots=slots, age=int(sc[0]),
                    uids=int(sc[1]), scalars=sc)
