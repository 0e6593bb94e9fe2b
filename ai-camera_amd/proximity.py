"""Proximity: ground plane, speed, pairs and parties per camera, on the device (aic_prox_*, csrc/prox.hpp, csrc/kernels_prox.hip; DESIGN.md
section 55): who is with whom, how fast, where on the floor.  One tracker-agnostic stage over the rows every tracker here delivers (x1 y1
x2 y2 id cls, int32), for a bank of 1..256 cameras per call; no frames.  Integer arithmetic only; tests/prox_oracle.py is the
specification."""
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
METRICS = {"ground": 0, "body": 1}
LINK, UNLINK = 1, 2
KINDS = {LINK: "link", UNLINK: "unlink"}
GAITS = ("none", "still", "moving", "running")
F_VALID, F_FIRST, F_NONEMPTY, F_PLACED, F_NEW = 1, 2, 4, 8, 16
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "links", "dist", "max_v_q8", "v_q8", "party_ticks",
                "max_party", "gx", "gy", "gait")
RECORD_FIELDS = ("frame", "n_counted", "n_placed", "n_near_pairs", "largest_near", "n_linked_pairs", "n_parties", "n_singles", "largest_party",
                 "n_units", "n_running", "n_still", "n_link", "n_unlink", "zero0", "zero1")
TAG_FIELDS = ("gx", "gy", "v_q8", "gait", "party", "party_size", "n_near", "flags")
PAIR_EVENT_FIELDS = ("kind", "frame", "id_lo", "id_hi", "duration", "distance", "ticks", "zero")
OPTIONS = ("forget_after", "metric", "near", "height_ratio_q8", "link_ticks", "unlink_ticks", "speed_shift", "still_speed", "run_speed")


def event_dict(ev):
    """One 16-int ended-track event as a dict: EVENT_FIELDS, `why` = the reason's name, `gait_name`, and speed / max_speed = v_q8 / 256."""
    d = dict(zip(EVENT_FIELDS, (int(v) for v in ev[:16])))
    d["why"], d["gait_name"] = REASONS[d["reason"]], GAITS[d["gait"]]
    d["speed"], d["max_speed"] = d["v_q8"] / 256, d["max_v_q8"] / 256
    return d


def pair_event_dict(ev, stream=None):
    """One 8-int pair event as a dict: kind ("link" / "unlink"), frame, ids (lo, hi), duration, distance, ticks (the `on` or `off` count)."""
    k, frame, lo, hi, duration, distance, ticks = (int(v) for v in ev[:7])
    d = dict(kind=KINDS[k], frame=frame, ids=(lo, hi), duration=duration, distance=distance, ticks=ticks)
    if stream is not None:
        d["stream"] = int(stream)
    return d


def homography(pixels, ground):
    """(H int32 [9], shift) for aic_prox_set_ground from n >= 4 correspondences pixels [n, 2] (x, y) -> ground [n, 2] (any unit: it becomes
    the ground unit of `near` and of every distance).

    A float64 DLT fit gives the numerator rows N (2 x 3) and the denominator row D (1 x 3) of g = (N p) / (D p), p = (x, y, 1); the device
    evaluates at p~ = (fx, fy, 2) = 2 p in doubled pixels, which changes neither quotient.  N is scaled by a and D by b = a 2^shift, both
    rounded to the nearest integer, so that every |entry| <= 2^30: shift = clamp(ceil(log2(max|N| / max|D|)), 0, 14), b = 2^30 / max|D|,
    a = b / 2^shift, and where a max|N| would still exceed 2^30 (a ratio beyond 2^14) a = 2^30 / max|N|, b = a 2^shift.

    The bound.  Rounding moves every entry by at most 1/2, so the integer numerator is a (N p~) + e_n and the integer denominator den =
    b (D p~) + e_d with |e_n|, |e_d| <= E = (fx + fy + 2) / 2.  With g = (N p~) / (D p~) = 2^shift a (N p~) / (b (D p~)):
        2^shift (a N p~ + e_n) / den - g = (2^shift e_n - g e_d) / den,
    and the floor division takes away less than 1.  So for a pixel with den > 0
        |integer map - float64 evaluation of the same fit| <= 1 + (2^shift + |g|) E / den
    per coordinate (tests/test_prox_oracle.py asserts this, with 1e-6 (1 + |g|) for the float64 evaluation itself), and a pixel whose
    b (D p~) < -E has den <= 0: it is not placed."""
    px, gr = np.asarray(pixels, np.float64).reshape(-1, 2), np.asarray(ground, np.float64).reshape(-1, 2)
    if len(px) < 4 or len(px) != len(gr):
        raise ValueError("homography needs n >= 4 pixels [n, 2] and as many ground points")
    # Hartley normalisation, then the DLT's null vector
    def norm(p):
        c, s = p.mean(0), np.sqrt(2) / max(np.sqrt(((p - p.mean(0)) ** 2).sum(1)).mean(), 1e-12)
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])
    Tp, Tg = norm(px), norm(gr)
    ph = (Tp @ np.c_[px, np.ones(len(px))].T).T
    gh = (Tg @ np.c_[gr, np.ones(len(gr))].T).T
    A = []
    for (x, y, _), (u, v, _) in zip(ph, gh):
        A.append([-x, -y, -1, 0, 0, 0, u * x, u * y, u])
        A.append([0, 0, 0, -x, -y, -1, v * x, v * y, v])
    h = np.linalg.svd(np.asarray(A))[2][-1].reshape(3, 3)
    M = np.linalg.inv(Tg) @ h @ Tp
    if (M[2] @ np.c_[px, np.ones(len(px))].T).mean() < 0:                    # the denominator is positive where the points are
        M = -M
    return scale_map(M)


def scale_map(M):
    """(H int32 [9], shift) from a float64 3 x 3 map (rows: x numerator, y numerator, denominator), scaled as homography() says."""
    M = np.asarray(M, np.float64).reshape(3, 3)
    mn, md = np.abs(M[:2]).max(), np.abs(M[2]).max()
    if not (np.isfinite(M).all() and mn > 0 and md > 0):
        raise ValueError("a degenerate ground map")
    shift = int(np.clip(np.ceil(np.log2(mn / md)), 0, 14))
    b = (1 << 30) / md
    a = b / (1 << shift)
    if a * mn > 1 << 30:
        a = (1 << 30) / mn
        b = a * (1 << shift)
    H = np.concatenate([np.rint(M[:2] * a).reshape(-1), np.rint(M[2] * b)]).astype(np.int64)
    H = np.clip(H, -(1 << 30), 1 << 30)
    return H.astype(np.int32), shift


class ProximityResult(namedtuple("ProximityResult", "n_final events pending status records row_tags n_pair_events pair_events failed counts ids")):
    """n_final [S]; events [S, cap, 16] (EVENT_FIELDS) -- the n_final[s] first of stream s are filled; pending [S]; status [S]; records
    [ticks, S, 16] (RECORD_FIELDS); row_tags [rows of the call, 8] (TAG_FIELDS); n_pair_events [ticks, S] = the true counts; pair_events
    [ticks, S, cap_pairs, 8] (PAIR_EVENT_FIELDS), zero-filled; failed = {stream: message}; counts [ticks, S] = the rows of each frame; ids [rows of the call] = the rows' track ids."""
    __slots__ = ()

    def tags(self, tick, stream):
        """The row tags [n, 8] of one frame."""
        flat = self.counts.reshape(-1)
        k = tick * self.counts.shape[1] + stream
        lo = int(flat[:k].sum())
        return self.row_tags[lo:lo + int(flat[k])]

    def record(self, tick, stream):
        return dict(zip(RECORD_FIELDS[:14], (int(v) for v in self.records[tick, stream])))

    def pairs(self, tick=None, stream=None):
        """The delivered pair events as a list of pair_event_dict, in order of tick, stream, (row i, row j)."""
        out = []
        T, S = self.n_pair_events.shape
        for t in range(T) if tick is None else (tick,):
            for s in range(S) if stream is None else (stream,):
                for k in range(min(int(self.n_pair_events[t, s]), self.pair_events.shape[2])):
                    out.append(pair_event_dict(self.pair_events[t, s, k], s))
        return out

    def ended(self):
        """One event_dict per ended track, stream by stream in emission order."""
        return [event_dict(self.events[s, k]) for s, n in enumerate(self.n_final) for k in range(int(n))]

    def parties(self, tick, stream):
        """[[id, ...], ...] of one frame's placed rows: parties of size >= 2 first, then the singles; each list sorted, the lists ordered
        by their smallest id."""
        flat = self.counts.reshape(-1)
        k = tick * self.counts.shape[1] + stream
        lo = int(flat[:k].sum())
        groups = {}
        for tid, t in zip(self.ids[lo:lo + int(flat[k])], self.tags(tick, stream)):
            if t[5] > 0:
                groups.setdefault(int(t[4]), []).append(int(tid))
        lists = sorted(sorted(g) for g in groups.values())
        return [g for g in lists if len(g) >= 2] + [g for g in lists if len(g) == 1]


class Proximity:
    """Proximity(streams, frame_hw, max_tracks=128, forget_after=70, metric="body", near=None, height_ratio_q8=384, link_ticks=30,
    unlink_ticks=60, speed_shift=2, still_speed=5, run_speed=70, device=None).  metric "body": distances and speeds relative to body
    height (near and the speeds in per mille of it; no calibration); "ground": through each camera's ground map (set_ground), near and the
    speeds in ground units.  near defaults to 700 ("body") or must be given ("ground").  The device is first touched by update / drain /
    flush."""

    def __init__(self, streams, frame_hw, max_tracks=128, forget_after=70, metric="body", near=None, height_ratio_q8=384, link_ticks=30,
                 unlink_ticks=60, speed_shift=2, still_speed=5, run_speed=70, device=None):
        self.streams, self.frame_h, self.frame_w, self.max_tracks = int(streams), int(frame_hw[0]), int(frame_hw[1]), int(max_tracks)
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {', '.join(METRICS)}")
        if near is None:
            if metric == "ground":
                raise ValueError("metric 'ground' needs near, in ground units")
            near = 700
        self.failed = {}
        cfg = L.ProxConfig(self.streams, self.frame_h, self.frame_w, self.max_tracks, int(forget_after), METRICS[metric], int(near),
                           int(height_ratio_q8), int(link_ticks), int(unlink_ticks), int(speed_shift), int(still_speed), int(run_speed))
        self._h = C.c_void_p()
        L.call("aic_prox_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_prox_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """The rules (OPTIONS; "metric" also by name), legal between calls; "ticks_per_launch", "launch_budget_mb": same results."""
        if key == "metric" and isinstance(value, str):
            if value not in METRICS:
                raise ValueError(f"metric must be one of {', '.join(METRICS)}")
            value = METRICS[value]
        L.call("aic_prox_option", self._h, str(key).encode(), int(value))

    def reset(self, stream):
        """The stream forgets everything, its pairs and pending finals included; a stop is cleared: a camera reconnecting."""
        L.call("aic_prox_reset", self._h, int(stream))
        self.failed.pop(int(stream), None)

    def set_ground(self, H, shift=0, stream=None):
        """The ground map of one stream (None: of all): H [9] int32 and shift, e.g. from homography().  Host only."""
        H = np.ascontiguousarray(H, dtype=np.int64).reshape(-1)
        if H.shape != (9,) or np.abs(H).max() > 1 << 30:
            raise ValueError("H must be 9 integers within +-2^30")
        H = H.astype(np.int32)
        L.call("aic_prox_set_ground", self._h, -1 if stream is None else int(stream), L.ptr(H), int(shift))

    def _result(self, out, ticks, counts, ids=np.zeros(0, np.int32)):
        S = self.streams
        n_final, events, pending, status, records, tags, n_pe, pe = out
        for s in np.nonzero(status)[0]:
            self.failed.setdefault(int(s), f"stream {s} stopped with libaicam error {int(status[s])} (reset({s}) starts it afresh)")
        return ProximityResult(n_final, events, pending, status, records.reshape(ticks, S, 16), tags, n_pe.reshape(ticks, S),
                               pe.reshape(ticks, S, pe.shape[1], 8), dict(self.failed), np.asarray(counts, np.int32).reshape(ticks, S), ids)

    def _outputs(self, cap, cap_pairs, frames=0, rows=0):
        S = self.streams
        return (np.zeros(S, np.int32), np.zeros((S, cap, 16), np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32),
                np.zeros((frames, 16), np.int32), np.zeros((rows, 8), np.int32), np.zeros(frames, np.int32), np.zeros((frames, cap_pairs, 8), np.int32))

    def update(self, rows, counts=None, ticks=None, cap=16, cap_pairs=64):
        """rows: per tick, per stream an [n, 6] int32 array (x1 y1 x2 y2 id cls) -- or ONE array / torch tensor [rows, 6] holding them
        tick-major, with counts [ticks * streams] (an array, or a tensor in the same memory as the rows).  An empty list only drains.
        Returns a ProximityResult; a stream that stopped is noted in .failed and delivers nothing until reset()."""
        cap, cap_pairs = int(cap), int(cap_pairs)
        if counts is None:
            ticks = len(rows)
            rows, counts = IO.flat_rows(rows, ticks, self.streams)
        elif ticks is None:
            n = counts.numel() if hasattr(counts, "numel") else len(counts)
            if n % self.streams:
                raise ValueError("counts must name every frame of the call")
            ticks = n // self.streams
        r_ptr, r_mem, r_keep = IO.memory(rows, "rows", np.int32)
        c_ptr, c_keep, total = IO.counts_for(r_keep, counts, r_mem, ticks, self.streams, need_total=True)
        host_counts = counts.cpu().numpy() if hasattr(counts, "cpu") else np.asarray(counts)
        out = self._outputs(cap, max(cap_pairs, 0), ticks * self.streams, total)
        L.call("aic_prox_update", self._h, ticks, c_ptr if ticks else None, r_ptr, r_mem, cap, cap_pairs, *(L.ptr(x) for x in out))
        ids = (r_keep.cpu().numpy() if hasattr(r_keep, "cpu") else np.asarray(r_keep)).reshape(-1, 6)[:, 4].copy() if total else np.zeros(0, np.int32)
        return self._result(out, ticks, host_counts, ids)

    def update_tuples(self, tracks, cap=16, cap_pairs=64):
        """As update(), from the 7-tuples (x1, y1, x2, y2, track_id, class_name, conf) the trackers return."""
        return self.update(IO.rows_from_tuples(tracks), cap=cap, cap_pairs=cap_pairs)

    def drain(self, cap=16):
        """The ENDED tracks still waiting (result.pending of an earlier call), at most cap per stream."""
        out = self._outputs(int(cap), 0)
        L.call("aic_prox_update", self._h, 0, None, None, L.HOST, int(cap), 0, *(L.ptr(x) for x in out))
        return self._result(out, 0, np.zeros(0, np.int32))

    def flush(self, stream=None, cap=None):
        """Every live track of the stream (None: of every stream) ends with reason FLUSHED and is handed over with everything pending."""
        cap = self.max_tracks if cap is None else int(cap)
        out = self._outputs(cap, 0)
        L.call("aic_prox_flush", self._h, -1 if stream is None else int(stream), cap, *(L.ptr(x) for x in out[:4]))
        return self._result(out, 0, np.zeros(0, np.int32))

    def export(self, stream):
        """events [n, 16] of every track the stream holds, in slot order, live ones with reason LIVE.  Changes nothing."""
        n = C.c_int32()
        ev = np.zeros((self.max_tracks, 16), np.int32)
        L.call("aic_prox_export", self._h, int(stream), C.byref(n), L.ptr(ev))
        return ev[:n.value].copy()

    def export_pairs(self, stream):
        """[n, 6] = id_a id_b linked on off since: the nonzero pair entries among the stream's live slots, in (slot_lo, slot_hi) order."""
        n = C.c_int32()
        out = np.zeros((max(1, self.max_tracks * (self.max_tracks - 1) // 2), 6), np.int32)
        L.call("aic_prox_export_pairs", self._h, int(stream), C.byref(n), L.ptr(out))
        return out[:n.value].copy()
