"""Clothing colours: what each track wears, per camera, on the device (aic_colours_*, csrc/colours.hpp, csrc/kernels_colours.hip;
DESIGN.md section 45): the description an operator searches by -- "the person in the red jacket and dark trousers".  One
tracker-agnostic stage over the frames and the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32), for a bank of 1..256
cameras per call.  Integer arithmetic only; tests/colours_oracle.py is the specification."""
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
NAMES = ("black", "gray", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown")
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "samples_upper", "samples_lower", "top_upper",
                "second_upper", "top_lower", "second_lower", "slot")

ColourResult = namedtuple("ColourResult", "n_final events row_tags pending status failed")
ColourResult.__doc__ = """n_final [S]; events [S, cap, 48] (EVENT_FIELDS, 0, 0, hist_upper[12], hist_lower[12], 8 zeros) -- the n_final[s]
first of stream s are filled, the rest zero; row_tags [rows of the call, 4] = top_upper, top_lower and their q8 shares per row (-1 for a
row that is not counted); pending [S] = ENDED tracks still waiting for room (drain() fetches them); status [S] = 0 or the code a stream
stopped with; failed = {stream: message}."""


def name_of(bin_):
    """The colour's name, None for -1."""
    return NAMES[bin_] if bin_ >= 0 else None


def event_dict(ev):
    """One 48-int event as a dict: EVENT_FIELDS, hist_upper / hist_lower (lists of 12 q8 shares), and upper / lower / upper_second /
    lower_second = the names beside the bin numbers (None for -1)."""
    d = dict(zip(EVENT_FIELDS, (int(v) for v in ev[:14])))
    d["hist_upper"], d["hist_lower"] = [int(v) for v in ev[16:28]], [int(v) for v in ev[28:40]]
    d["upper"], d["upper_second"] = name_of(d["top_upper"]), name_of(d["second_upper"])
    d["lower"], d["lower_second"] = name_of(d["top_lower"]), name_of(d["second_lower"])
    return d


def finals(result):
    """[event dict] of a ColourResult, stream by stream in emission order."""
    return [event_dict(result.events[s, k]) for s, n in enumerate(result.n_final) for k in range(int(n))]


def matches(event, upper=None, lower=None, min_share_q8=64):
    """Does a track's descriptor (an event dict, or 48 ints) answer "upper in red, lower in blue or black"?  A name or a tuple of names
    matches a part if it is the part's top, or its second, with that bin's hist >= min_share_q8.  None asks nothing of the part."""
    ev = event if isinstance(event, dict) else event_dict(event)
    for want, part in ((upper, "upper"), (lower, "lower")):
        if want is None:
            continue
        names = (want,) if isinstance(want, str) else tuple(want)
        unknown = [n for n in names if n not in NAMES]
        if unknown:
            raise ValueError(f"no such colour: {unknown[0]} (one of {', '.join(NAMES)})")
        hist = ev["hist_" + part]
        if not any(b >= 0 and NAMES[b] in names and hist[b] >= min_share_q8 for b in (ev["top_" + part], ev["second_" + part])):
            return False
    return True


def classify(bgr):
    """uint8 [..., 3] BGR -> uint8 [...] colour bins: the host's copy of the pixel rule (no device)."""
    a = np.ascontiguousarray(bgr, dtype=np.uint8)
    if a.shape[-1:] != (3,):
        raise ValueError("pixels must be [..., 3] BGR")
    out = np.zeros(a.shape[:-1], np.uint8)
    L.call("aic_colours_classify", L.ptr(a) if a.size else None, a.size // 3, L.ptr(out) if a.size else None)
    return out


class TrackColours:
    """TrackColours(streams, frame_hw, max_tracks=128, forget_after=70, torso_q8=(51, 128), legs_q8=(141, 230), inset_q8=64, min_w=4,
    min_h=4, max_cover_q8=64, device=0).  torso_q8 / legs_q8: the part's top and bottom as q8 fractions of the box height; inset_q8:
    what is cut off the box on either side; a part smaller than min_w x min_h after clipping, or covered by more than max_cover_q8 by
    one nearer box, is not sampled.  The device is first touched by update / drain / flush."""

    def __init__(self, streams, frame_hw, max_tracks=128, forget_after=70, torso_q8=(51, 128), legs_q8=(141, 230), inset_q8=64, min_w=4,
                 min_h=4, max_cover_q8=64, device=0):
        self.streams, self.frame_h, self.frame_w, self.max_tracks = int(streams), int(frame_hw[0]), int(frame_hw[1]), int(max_tracks)
        self.failed = {}                                         # stream -> message
        cfg = L.ColoursConfig(self.streams, self.frame_h, self.frame_w, self.max_tracks, int(forget_after), int(torso_q8[0]), int(torso_q8[1]),
                              int(legs_q8[0]), int(legs_q8[1]), int(inset_q8), int(min_w), int(min_h), int(max_cover_q8))
        self._h = C.c_void_p()
        L.call("aic_colours_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_colours_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"ticks_per_launch": 0 = as many ticks per launch as the budget allows (default), k = at most k; "launch_budget_mb".  Same
        results."""
        L.call("aic_colours_option", self._h, str(key).encode(), int(value))

    def reset(self, stream):
        """The stream forgets everything, pending finals included; a stop is cleared: a camera reconnecting."""
        L.call("aic_colours_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def _outputs(self, cap, rows=0):
        S = self.streams
        return (np.zeros(S, np.int32), np.zeros((S, cap, 48), np.int32), np.full((rows, 4), -1, np.int32), np.zeros(S, np.int32),
                np.zeros(S, np.int32))

    def _result(self, out):
        for s in np.nonzero(out[4])[0]:
            self.failed.setdefault(int(s), f"stream {s} stopped with libaicam error {int(out[4][s])} (reset({s}) starts it afresh)")
        return ColourResult(*out, dict(self.failed))

    def update(self, frames, rows, counts=None, cap=16):
        """frames: uint8 [ticks, streams, H, W, 3] BGR, tick-major, a NumPy array or a torch tensor (host or device).  rows: per tick,
        per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6] holding them in that order, with
        counts [ticks * streams] (an array, or a tensor in the same memory as the rows).  ticks = 0 only drains.  Returns a
        ColourResult; a stream that stopped is noted in .failed and delivers nothing until reset()."""
        cap = int(cap)
        shape = tuple(frames.shape)
        if len(shape) != 5 or shape[1:] != (self.streams, self.frame_h, self.frame_w, 3):
            raise ValueError(f"frames of shape {shape}, not [ticks, {self.streams}, {self.frame_h}, {self.frame_w}, 3]")
        ticks = shape[0]
        f_ptr, f_mem, f_keep = IO.memory(frames, "frames", np.uint8)
        if counts is None:
            rows, counts = IO.flat_rows(rows, ticks, self.streams)
        r_ptr, r_mem, r_keep = IO.memory(rows, "rows", np.int32)
        c_ptr, c_keep, total = IO.counts_for(r_keep, counts, r_mem, ticks, self.streams, need_total=True)   # row_tags is sized by it
        out = self._outputs(cap, total)
        L.call("aic_colours_update", self._h, f_ptr if ticks else None, f_mem, ticks, c_ptr if ticks else None, r_ptr, r_mem, cap,
               *(L.ptr(x) for x in out))
        return self._result(out)

    def update_tuples(self, frames, tracks, cap=16):
        """As update(), from the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) the trackers return: tracks[tick][stream] is a list
        of tuples."""
        return self.update(frames, IO.rows_from_tuples(tracks), cap=cap)

    def drain(self, cap=16):
        """The ENDED tracks still waiting (result.pending of an earlier call), at most cap per stream."""
        out = self._outputs(int(cap))
        L.call("aic_colours_update", self._h, None, L.HOST, 0, None, None, L.HOST, int(cap), *(L.ptr(x) for x in out))
        return self._result(out)

    def flush(self, stream=None, cap=None):
        """Every live track of the stream (None: of every stream) ends with reason FLUSHED and is handed over with everything pending:
        the end of a run.  cap defaults to max_tracks, which takes them all."""
        cap = self.max_tracks if cap is None else int(cap)
        out = self._outputs(cap)
        L.call("aic_colours_flush", self._h, -1 if stream is None else int(stream), cap, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[3]), L.ptr(out[4]))
        return self._result(out)

    def export(self, stream):
        """events [n, 48] of every track the stream holds, in slot order, live ones with reason LIVE.  Changes nothing."""
        n = C.c_int32()
        ev = np.zeros((self.max_tracks, 48), np.int32)
        L.call("aic_colours_export", self._h, int(stream), C.byref(n), L.ptr(ev))
        return ev[:n.value].copy()
