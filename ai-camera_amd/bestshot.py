"""Best shots: the best crop of every track, kept on the device, per camera (aic_bestshot_*, csrc/bestshot.hpp,
csrc/kernels_bestshot.hip): the picture an operator is shown for "this is person 4711 again".  One
tracker-agnostic stage over the frames and the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32), for a bank of 1..256
cameras per call.  Integer arithmetic only; tests/bestshot_oracle.py is the specification."""
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
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "has_shot", "best_frame", "score", "x0", "y0",
                "x1", "y1", "slot")

BestShotResult = namedtuple("BestShotResult", "n_final events thumbs pending status failed")
BestShotResult.__doc__ = """n_final [S]; events [S, cap, 16] (EVENT_FIELDS, then 0), thumbs [S, cap, TH, TW, 3] BGR -- the n_final[s] first
of stream s are filled, the rest zero; pending [S] = ENDED tracks still waiting for room (drain() fetches them); status [S] = 0 or the
code a stream stopped with; failed = {stream: message}."""


def finals(result):
    """[(event dict, thumbnail [TH, TW, 3] BGR)] of a BestShotResult, stream by stream in emission order."""
    out = []
    for s, n in enumerate(result.n_final):
        for k in range(int(n)):
            out.append((dict(zip(EVENT_FIELDS, (int(v) for v in result.events[s, k]))), result.thumbs[s, k]))
    return out


def write_ppm(path, thumb_bgr):
    """A thumbnail as a binary P6 file (RGB)."""
    t = np.ascontiguousarray(thumb_bgr[:, :, ::-1])
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (t.shape[1], t.shape[0]))
        f.write(t.tobytes())


def write_jpeg(path, data):
    """A thumbnail's JFIF file as encode_finals() delivered it."""
    with open(path, "wb") as f:
        f.write(data)


def encode_finals(result, encoder):
    """The JFIF file (bytes; None for one beyond the encoder's max_bytes) of every final of a BestShotResult, in finals() order: all
    thumbnails go through one JpegEncoder.encode call (jpeg.py; more than its max_images: one call per max_images)."""
    thumbs = [t for _, t in finals(result)]
    out = []
    for lo in range(0, len(thumbs), encoder.max_images):
        out += encoder.encode(np.stack(thumbs[lo:lo + encoder.max_images]))
    return out


class BestShots:
    """BestShots(streams, frame_hw, thumb=(64, 128), max_tracks=128, forget_after=70, region="box", head_q8=64, pad=0, min_w=8,
    min_h=16, device=0).  thumb = (width, height), multiples of 8 in 16..128 x 16..256; region "box" or "head" (the upper head_q8 / 256
    of the box, as the renderer's head mode).  The device is first touched by update / drain / flush; the resident thumbnails take
    streams * max_tracks * TH * TW * 3 bytes there."""

    def __init__(self, streams, frame_hw, thumb=(64, 128), max_tracks=128, forget_after=70, region="box", head_q8=64, pad=0, min_w=8,
                 min_h=16, device=0):
        if region not in ("box", "head"):
            raise ValueError("region must be 'box' or 'head'")
        self.streams, self.frame_h, self.frame_w = int(streams), int(frame_hw[0]), int(frame_hw[1])
        self.thumb_w, self.thumb_h, self.max_tracks = int(thumb[0]), int(thumb[1]), int(max_tracks)
        self.failed = {}                                         # stream -> message
        cfg = L.BestShotConfig(self.streams, self.frame_h, self.frame_w, self.thumb_w, self.thumb_h, self.max_tracks, int(forget_after),
                               0 if region == "box" else 1, int(head_q8), int(pad), int(min_w), int(min_h))
        self._h = C.c_void_p()
        L.call("aic_bestshot_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_bestshot_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"ticks_per_launch": 0 = as many ticks per launch as the budget allows (default), k = at most k; "launch_budget_mb"; "stats" 0 / 1
        (counters()).  Same results."""
        L.call("aic_bestshot_option", self._h, str(key).encode(), int(value))

    def counters(self):
        """After option("stats", 1): dict(rows, candidates, stored) since creation -- rows handed in, candidates scored, candidate
        thumbnails the could-still-win filter let through."""
        v = [C.c_int64() for _ in range(3)]
        L.call("aic_bestshot_counters", self._h, *(C.byref(x) for x in v))
        return dict(rows=v[0].value, candidates=v[1].value, stored=v[2].value)

    def reset(self, stream):
        """The stream forgets everything, pending finals included; a stop is cleared: a camera reconnecting."""
        L.call("aic_bestshot_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def _outputs(self, cap):
        S = self.streams
        return (np.zeros(S, np.int32), np.zeros((S, cap, 16), np.int32), np.zeros((S, cap, self.thumb_h, self.thumb_w, 3), np.uint8),
                np.zeros(S, np.int32), np.zeros(S, np.int32))

    def _result(self, out):
        for s in np.nonzero(out[4])[0]:
            self.failed.setdefault(int(s), f"stream {s} stopped with libaicam error {int(out[4][s])} (reset({s}) starts it afresh)")
        return BestShotResult(*out, dict(self.failed))

    def update(self, frames, rows, counts=None, cap=16):
        """frames: uint8 [ticks, streams, H, W, 3] BGR, tick-major, a NumPy array or a torch tensor (host or device).  rows: per tick,
        per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6] holding them in that order, with
        counts [ticks * streams] (an array, or a tensor in the same memory as the rows).  ticks = 0 only drains.  Returns a
        BestShotResult; a stream that stopped is noted in .failed and delivers nothing until reset()."""
        cap = int(cap)
        shape = tuple(frames.shape)
        if len(shape) != 5 or shape[1:] != (self.streams, self.frame_h, self.frame_w, 3):
            raise ValueError(f"frames of shape {shape}, not [ticks, {self.streams}, {self.frame_h}, {self.frame_w}, 3]")
        ticks = shape[0]
        f_ptr, f_mem, f_keep = IO.memory(frames, "frames", np.uint8)
        if counts is None:
            rows, counts = IO.flat_rows(rows, ticks, self.streams)
        r_ptr, r_mem, r_keep = IO.memory(rows, "rows", np.int32)
        c_ptr, c_keep, _ = IO.counts_for(r_keep, counts, r_mem, ticks, self.streams, need_total=False)
        out = self._outputs(cap)
        L.call("aic_bestshot_update", self._h, f_ptr if ticks else None, f_mem, ticks, c_ptr if ticks else None, r_ptr, r_mem, cap,
               *(L.ptr(x) for x in out))
        return self._result(out)

    def update_tuples(self, frames, tracks, cap=16):
        """As update(), from the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) the trackers return: tracks[tick][stream] is a list
        of tuples."""
        return self.update(frames, IO.rows_from_tuples(tracks), cap=cap)

    def drain(self, cap=16):
        """The ENDED tracks still waiting (result.pending of an earlier call), at most cap per stream."""
        out = self._outputs(int(cap))
        L.call("aic_bestshot_update", self._h, None, L.HOST, 0, None, None, L.HOST, int(cap), *(L.ptr(x) for x in out))
        return self._result(out)

    def flush(self, stream=None, cap=None):
        """Every live track of the stream (None: of every stream) ends with reason FLUSHED and is handed over with everything pending:
        the end of a run.  cap defaults to max_tracks, which takes them all."""
        cap = self.max_tracks if cap is None else int(cap)
        out = self._outputs(cap)
        L.call("aic_bestshot_flush", self._h, -1 if stream is None else int(stream), cap, *(L.ptr(x) for x in out))
        return self._result(out)

    def export(self, stream):
        """(events [n, 16], thumbs [n, TH, TW, 3]) of every track the stream holds, in slot order, live ones with reason LIVE.  Changes
        nothing."""
        n = C.c_int32()
        ev = np.zeros((self.max_tracks, 16), np.int32)
        th = np.zeros((self.max_tracks, self.thumb_h, self.thumb_w, 3), np.uint8)
        L.call("aic_bestshot_export", self._h, int(stream), C.byref(n), L.ptr(ev), L.ptr(th))
        return ev[:n.value].copy(), th[:n.value].copy()
