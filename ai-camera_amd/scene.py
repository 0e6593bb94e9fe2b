"""Scene watch: motion masks, an activity gate and tamper alarms per camera (aic_scene_*, csrc/scene.hpp, csrc/kernels_scene.hip;
DESIGN.md section 39).  One tracker-agnostic stage over the frames -- and, optionally, the rows every tracker here delivers (x1 y1 x2 y2
id cls, int32) -- for a bank of 1..256 cameras per call.  Integer arithmetic only; tests/scene_oracle.py is the specification."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _bank_io as IO
from . import _lib as L
from . import config

KINDS = ("dark", "bright", "defocus", "scene", "frozen")
DARK, BRIGHT, DEFOCUS, SCENE, FROZEN = (1 << i for i in range(5))
MAX_ROWS = 512
RECORD_FIELDS = ("frame", "ready", "active", "n_moving", "n_raw", "x0", "y0", "x1", "y1", "mean_luma", "sharp", "ref_q8", "n_changed", "cond",
                 "alarms", "edges")
OPTIONS = ("thresh", "noise_k_q4", "warmup", "big_thresh", "learn_shift", "slow_extra", "dev_init_q8", "min_neighbours", "dark_luma",
           "bright_luma", "min_ref_q8", "defocus_q8", "scene_q16", "ref_shift", "hold", "gate_cells", "gate_hold", "ticks_per_launch",
           "launch_budget_mb")


def alarm_names(bits):
    """The names of the alarm (or condition) bits set."""
    return [k for i, k in enumerate(KINDS) if int(bits) >> i & 1]


class SceneResult:
    """records int32 [ticks, S, 16] (RECORD_FIELDS; every field is also an attribute, a [ticks, S] view: .active, .alarms, .n_moving,
    ...); masks u8 [ticks, S, Hc, Wc] (bit 0 clean, bit 1 raw) or None; row_motion int32 [rows] (256 * moving / covered cells of the
    row's box, -1 = invalid or empty) or None; row_offsets [ticks * S + 1] into it."""

    def __init__(self, records, masks, row_motion, row_offsets):
        self.records, self.masks, self.row_motion, self.row_offsets = records, masks, row_motion, row_offsets

    def __getattr__(self, name):
        if name in RECORD_FIELDS:
            return self.records[..., RECORD_FIELDS.index(name)]
        raise AttributeError(name)

    @property
    def motion_box(self):
        """[ticks, S, 4] = x0 y0 x1 y1 of the clean cells in pixels (x1 y1 exclusive), all -1 = none."""
        return self.records[..., 5:9]

    def rows_of(self, tick, stream):
        """row_motion of one frame's rows."""
        i = tick * self.records.shape[1] + stream
        return self.row_motion[self.row_offsets[i]:self.row_offsets[i + 1]]

    def events(self):
        """[(tick, stream, kind, raised)] of every alarm edge, in tick, stream, kind order; a raised edge before a cleared one."""
        out = []
        edges = self.records[..., 15]
        for t, s in zip(*np.nonzero(edges)):
            e = int(edges[t, s])
            out += [(int(t), int(s), k, True) for i, k in enumerate(KINDS) if e >> i & 1]
            out += [(int(t), int(s), k, False) for i, k in enumerate(KINDS) if e >> (8 + i) & 1]
        return out


class SceneWatch:
    """SceneWatch(streams, frame_hw, cell=8, device=0, **options): options are the thresholds of OPTIONS (set_option).  The device is
    first touched by update."""

    def __init__(self, streams, frame_hw, cell=8, device=0, **options):
        self.streams, self.frame_h, self.frame_w, self.cell = int(streams), int(frame_hw[0]), int(frame_hw[1]), int(cell)
        cfg = L.SceneConfig(self.streams, self.frame_h, self.frame_w, self.cell)
        self._h = C.c_void_p()
        L.call("aic_scene_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))
        self.grid_h, self.grid_w = self.frame_h // self.cell, self.frame_w // self.cell
        try:
            for k, v in options.items():
                self.set_option(k, v)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        """A threshold of the specification, or "ticks_per_launch" (0 = as many ticks per launch as the budget allows, k = at most k) /
        "launch_budget_mb" (same results).  None sizes a buffer: they may change between calls."""
        L.call("aic_scene_option", self._h, str(key).encode(), int(value))

    def reset(self, stream=None):
        """The stream (None: every stream) starts again at age 0: a camera reconnecting or re-aimed."""
        L.call("aic_scene_reset", self._h, -1 if stream is None else int(stream))

    _memory = staticmethod(IO.memory)                            # (leftobj.py and callers reach it by this name)

    def update(self, frames, rows=None, counts=None, want_masks=False):
        """frames: uint8 [ticks, streams, H, W, 3] BGR, tick-major, a NumPy array or a torch tensor (host or device, any alignment).
        rows (optional): per tick, per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6]
        holding them in that order, with counts [ticks * streams] (an array, or a tensor in the same memory as the rows).  Returns a
        SceneResult."""
        shape = tuple(frames.shape)
        if len(shape) != 5 or shape[1:] != (self.streams, self.frame_h, self.frame_w, 3):
            raise ValueError(f"frames of shape {shape}, not [ticks, {self.streams}, {self.frame_h}, {self.frame_w}, 3]")
        ticks, S = shape[0], self.streams
        f_ptr, f_mem, f_keep = self._memory(frames, "frames", np.uint8)
        r_ptr = c_ptr = rm = offsets = None
        r_mem = L.HOST
        if rows is not None:
            if counts is None:
                rows, counts = IO.flat_rows(rows, ticks, S)
            r_ptr, r_mem, r_keep = self._memory(rows, "rows", np.int32)
            c_ptr, c_keep, host_counts = IO.counts_on_host(r_keep, counts, r_mem, ticks, S)
            total = int(host_counts.sum())
            offsets = np.concatenate([[0], np.cumsum(host_counts)]).astype(np.int64)
            rm = np.full(max(total, 1), -1, np.int32)
        rec = np.zeros((ticks, S, 16), np.int32)
        masks = np.zeros((ticks, S, self.grid_h, self.grid_w), np.uint8) if want_masks else None
        L.call("aic_scene_update", self._h, f_ptr if ticks else None, f_mem, ticks, c_ptr if ticks else None, r_ptr, r_mem, L.ptr(rec), L.ptr(masks),
               L.ptr(rm) if ticks else None)
        return SceneResult(rec, masks, None if rm is None else rm[:int(offsets[-1])], offsets)

    def export(self, stream):
        """dict(bg, dev, prev: int32 [Hc, Wc]; age, quiet, ref_q8, alarms: int; on, off: int32 [5]) of one stream.  Changes nothing."""
        planes = [np.zeros((self.grid_h, self.grid_w), np.int32) for _ in range(3)]
        sc = np.zeros(16, np.int32)
        L.call("aic_scene_export", self._h, int(stream), *(L.ptr(p) for p in planes), L.ptr(sc))
        return dict(bg=planes[0], dev=planes[1], prev=planes[2], age=int(sc[0]), quiet=int(sc[1]), ref_q8=int(sc[2]), alarms=int(sc[3]),
                    on=sc[4:9].copy(), off=sc[9:14].copy(), scalars=sc)
