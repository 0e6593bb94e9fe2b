"""Heat maps: footfall, dwell, flow and paths per camera, on the device (aic_heat_*, csrc/heat.hpp, csrc/kernels_heat.hip; DESIGN.md
section 49): where people go.  One tracker-agnostic stage over the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32), for a
bank of 1..256 cameras per call; only render() touches frames.  Integer arithmetic only; tests/heat_oracle.py is the specification."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _bank_io as IO
from . import _lib as L
from . import config

LIVE, EXPIRED, FLUSHED = 0, 1, 2
REASONS = {LIVE: "live", EXPIRED: "expired", FLUSHED: "flushed"}
MAX_ROWS = MAX_TRACKS = 512
LAYERS = ("visits", "dwell", "starts", "ends", "dir0", "dir1", "dir2", "dir3", "dir4", "dir5", "dir6", "dir7")
ANCHORS = {"foot": 0, "centre": 1}
SCALES = {"linear": 0, "log": 1}
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "cells", "start_fx", "start_fy", "end_fx", "end_fy",
                "path", "max_step", "moving", "last_cell")

HeatResult = namedtuple("HeatResult", "n_final events row_tags pending status failed")
HeatResult.__doc__ = """n_final [S]; events [S, cap, 16] (EVENT_FIELDS) -- the n_final[s] first of stream s are filled, the rest zero;
row_tags [rows of the call, 4] = cell index, ticks in that cell, step (doubled pixels), octant or -1 per counted row (-1, 0, 0, -1 for a
row that is not counted); pending [S] = ENDED tracks still waiting for room (drain() fetches them); status [S] = 0 or the code a stream
stopped with; failed = {stream: message}."""


def layer_index(layer):
    """A layer's number from its name or number."""
    if isinstance(layer, str):
        if layer not in LAYERS:
            raise ValueError(f"no such layer: {layer} (one of {', '.join(LAYERS)})")
        return LAYERS.index(layer)
    if not 0 <= int(layer) < len(LAYERS):
        raise ValueError(f"layer {layer} outside 0..11")
    return int(layer)


def layer_mask(names=None):
    """The bit mask of a list of layer names or numbers; None: all twelve."""
    if names is None:
        return (1 << len(LAYERS)) - 1
    mask = 0
    for n in names:
        mask |= 1 << layer_index(n)
    if not mask:
        raise ValueError("no layer named")
    return mask


def event_dict(ev):
    """One 16-int event as a dict: EVENT_FIELDS, and `why` = the reason's name."""
    d = dict(zip(EVENT_FIELDS, (int(v) for v in ev[:16])))
    d["why"] = REASONS[d["reason"]]
    return d


def paths(result):
    """One dict per ended track of a HeatResult, stream by stream in emission order: event_dict plus start / end in pixels (floats),
    length = the path in pixels and straightness = the start-to-end Chebyshev distance over the path (None for a track that never moved)."""
    out = []
    for s, n in enumerate(result.n_final):
        for k in range(int(n)):
            d = event_dict(result.events[s, k])
            d["start"], d["end"] = (d["start_fx"] / 2, d["start_fy"] / 2), (d["end_fx"] / 2, d["end_fy"] / 2)
            d["length"] = d["path"] / 2
            direct = max(abs(d["end_fx"] - d["start_fx"]), abs(d["end_fy"] - d["start_fy"]))
            d["straightness"] = direct / d["path"] if d["path"] else None
            out.append(d)
    return out


def colour_table():
    """uint8 [256, 3] BGR: the default colour ramp (no device)."""
    t = np.zeros((256, 3), np.uint8)
    L.call("aic_heat_lut", L.ptr(t))
    return t


class HeatMaps:
    """HeatMaps(streams, frame_hw, cell=16, max_tracks=128, forget_after=70, anchor="foot", min_move=4, device=None).  cell: 4, 8, 16 or
    32 pixels; anchor: "foot" (the middle of the box's bottom edge) or "centre"; min_move: the step, in doubled pixels, from which a
    sighting counts as movement.  The device is first touched by update / drain / flush / layers / load_layers / decay / render."""

    def __init__(self, streams, frame_hw, cell=16, max_tracks=128, forget_after=70, anchor="foot", min_move=4, device=None):
        self.streams, self.frame_h, self.frame_w, self.max_tracks, self.cell = int(streams), int(frame_hw[0]), int(frame_hw[1]), int(max_tracks), int(cell)
        if anchor not in ANCHORS:
            raise ValueError(f"anchor must be one of {', '.join(ANCHORS)}")
        self.failed, self._alpha = {}, 160                       # stream -> message; the alpha_q8 option as set
        cfg = L.HeatConfig(self.streams, self.frame_h, self.frame_w, self.cell, self.max_tracks, int(forget_after), ANCHORS[anchor], int(min_move))
        self._h = C.c_void_p()
        L.call("aic_heat_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))
        self.grid_h, self.grid_w = -(-self.frame_h // self.cell), -(-self.frame_w // self.cell)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_heat_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"scale" ("linear" / "log" or 0 / 1), "alpha_q8" (0..256), "floor" (0..255), "chunk_frames" for render; "ticks_per_launch",
        "launch_budget_mb" for update.  Same results."""
        if key == "scale" and isinstance(value, str):
            if value not in SCALES:
                raise ValueError(f"scale must be one of {', '.join(SCALES)}")
            value = SCALES[value]
        L.call("aic_heat_option", self._h, str(key).encode(), int(value))
        if key == "alpha_q8":
            self._alpha = int(value)

    def reset(self, stream):
        """The stream forgets everything, its layers and pending finals included; a stop is cleared: a camera reconnecting."""
        L.call("aic_heat_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def _outputs(self, cap, rows=0):
        S = self.streams
        tags = np.zeros((rows, 4), np.int32)
        tags[:, 0], tags[:, 3] = -1, -1
        return np.zeros(S, np.int32), np.zeros((S, cap, 16), np.int32), tags, np.zeros(S, np.int32), np.zeros(S, np.int32)

    def _result(self, out):
        for s in np.nonzero(out[4])[0]:
            self.failed.setdefault(int(s), f"stream {s} stopped with libaicam error {int(out[4][s])} (reset({s}) starts it afresh)")
        return HeatResult(*out, dict(self.failed))

    def update(self, rows, counts=None, ticks=None, cap=16):
        """rows: per tick, per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6] holding them
        tick-major, with counts [ticks * streams] (an array, or a tensor in the same memory as the rows).  An empty list only drains.
        Returns a HeatResult; a stream that stopped is noted in .failed and delivers nothing until reset()."""
        cap = int(cap)
        if counts is None:
            ticks = len(rows)
            rows, counts = IO.flat_rows(rows, ticks, self.streams)
        elif ticks is None:
            n = counts.numel() if hasattr(counts, "numel") else len(counts)
            if n % self.streams:
                raise ValueError("counts must name every frame of the call")
            ticks = n // self.streams
        r_ptr, r_mem, r_keep = IO.memory(rows, "rows", np.int32)
        c_ptr, c_keep, total = IO.counts_for(r_keep, counts, r_mem, ticks, self.streams, need_total=True)   # row_tags is sized by it
        out = self._outputs(cap, total)
        L.call("aic_heat_update", self._h, ticks, c_ptr if ticks else None, r_ptr, r_mem, cap, *(L.ptr(x) for x in out))
        return self._result(out)

    def update_tuples(self, tracks, cap=16):
        """As update(), from the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) the trackers return: tracks[tick][stream] is a list
        of tuples."""
        return self.update(IO.rows_from_tuples(tracks), cap=cap)

    def drain(self, cap=16):
        """The ENDED tracks still waiting (result.pending of an earlier call), at most cap per stream."""
        out = self._outputs(int(cap))
        L.call("aic_heat_update", self._h, 0, None, None, L.HOST, int(cap), *(L.ptr(x) for x in out))
        return self._result(out)

    def flush(self, stream=None, cap=None):
        """Every live track of the stream (None: of every stream) ends with reason FLUSHED and is handed over with everything pending:
        the end of a run.  cap defaults to max_tracks, which takes them all."""
        cap = self.max_tracks if cap is None else int(cap)
        out = self._outputs(cap)
        L.call("aic_heat_flush", self._h, -1 if stream is None else int(stream), cap, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[3]), L.ptr(out[4]))
        return self._result(out)

    def export(self, stream):
        """events [n, 16] of every track the stream holds, in slot order, live ones with reason LIVE.  Changes nothing."""
        n = C.c_int32()
        ev = np.zeros((self.max_tracks, 16), np.int32)
        L.call("aic_heat_export", self._h, int(stream), C.byref(n), L.ptr(ev))
        return ev[:n.value].copy()

    def layers(self, stream, names=None):
        """{name: int32 [GH, GW]} of the stream's layers (names: a list of layer names or numbers; None: all twelve)."""
        mask = layer_mask(names)
        ls = [l for l in range(12) if mask >> l & 1]
        out = np.zeros((len(ls), self.grid_h, self.grid_w), np.int32)
        L.call("aic_heat_export_layers", self._h, int(stream), mask, L.ptr(out))
        return {LAYERS[l]: out[k] for k, l in enumerate(ls)}

    def load_layers(self, stream, layers):
        """{name or number: int32 [GH, GW]} replaces those layers of the stream (values 0..2^30): yesterday's map carried on.  Takes
        effect in call order, as reset() does."""
        items = sorted((layer_index(k), np.asarray(v)) for k, v in layers.items())
        if not items:
            raise ValueError("no layer named")
        for _, v in items:
            if v.shape != (self.grid_h, self.grid_w) or not np.issubdtype(v.dtype, np.integer):
                raise ValueError(f"a layer must be an integer array [{self.grid_h}, {self.grid_w}]")
            if v.size and (int(v.min()) < 0 or int(v.max()) > 1 << 30):
                raise ValueError("a layer value outside 0..2^30")
        arr = np.ascontiguousarray(np.stack([v for _, v in items]), dtype=np.int32)
        L.call("aic_heat_import_layers", self._h, int(stream), layer_mask([l for l, _ in items]), L.ptr(arr))

    def decay(self, shift=1, stream=None, names=None):
        """v >>= shift (1..31; 31 clears) on the named layers (None: all) of the stream (None: of every stream): ageing."""
        L.call("aic_heat_decay", self._h, -1 if stream is None else int(stream), layer_mask(names), int(shift))

    def set_colour_table(self, table):
        """uint8 [256, 3] BGR replaces the colour ramp of render()."""
        t = np.ascontiguousarray(table, dtype=np.uint8)
        if t.shape != (256, 3):
            raise ValueError("the colour table must be [256, 3] BGR")
        L.call("aic_heat_set_lut", self._h, L.ptr(t))

    @staticmethod
    def colour_table():
        """The default colour ramp, uint8 [256, 3] BGR."""
        return colour_table()

    def render(self, frames, cameras=None, layer="dwell"):
        """Blends the layer of each frame's camera into uint8 [n, H, W, 3] BGR frames: in place for a torch tensor on the device (returned),
        a rendered copy for a NumPy array.  cameras [n] names each frame's camera (None: frame f shows camera f % streams)."""
        shape = tuple(frames.shape)
        if len(shape) != 4 or shape[1:] != (self.frame_h, self.frame_w, 3):
            raise ValueError(f"frames of shape {shape}, not [n, {self.frame_h}, {self.frame_w}, 3]")
        n = shape[0]
        cams = None
        if cameras is not None:
            cams = np.ascontiguousarray(cameras, dtype=np.int32).reshape(-1)
            if len(cams) != n:
                raise ValueError("cameras must name every frame")
        if isinstance(frames, np.ndarray):
            frames = np.array(frames, dtype=np.uint8, order="C", copy=True)
        f_ptr, f_mem, f_keep = IO.memory(frames, "frames", np.uint8)
        L.call("aic_heat_render", self._h, f_ptr if n else None, n, f_mem, None if cams is None else L.ptr(cams), layer_index(layer))
        return f_keep

    def images(self, streams=None, layer="dwell"):
        """uint8 [n, H, W, 3]: the plain heat image of each named stream (None: all) -- alpha 256 over black frames, ready for
        JpegEncoder.  The stage's own alpha_q8 is put back afterwards."""
        streams = list(range(self.streams)) if streams is None else [int(s) for s in streams]
        frames = np.zeros((len(streams), self.frame_h, self.frame_w, 3), np.uint8)
        L.call("aic_heat_option", self._h, b"alpha_q8", 256)
        try:
            return self.render(frames, cameras=streams, layer=layer)
        finally:
            L.call("aic_heat_option", self._h, b"alpha_q8", self._alpha)
