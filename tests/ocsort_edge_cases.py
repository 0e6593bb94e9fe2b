"""Planted scenes for the OC-SORT kernel (csrc/kernels_ocsort.hip): an IoU on the threshold at each of the three stages, tied optima, scores
on a band edge, the OCM term at its end points, every exit of the observation lookup, a reused slot with a stale ring, non-finite and
shrinking predictions, the life-cycle edges, output coordinates on k + 0.5, the capacity boundary and assignment problems whose side or
size sits on one of the kernel's own switches -- the places the random scenes of tests/test_gpu_ocsort.py never reach.

tests/test_ocsort_edge_cases.py (CPU) holds the oracle (tests/ocsort_oracle.py) to the edge each scene is named for;
tests/test_gpu_ocsort_edges.py (GPU) replays every scene through OCSort and OCSortBank and compares frame by frame, exactly.

The oracle states every filter sum in the kernel's order, so an edge may sit anywhere.  A threshold equality is made with the threshold:
the oracle runs up to the edge frame, the fp32 IoU of the planted pair is read from its record, and iou_threshold is set to that value
(`eq`), to the next fp32 value above it (`below`: the IoU is one ulp below the threshold) or below it (`above`)."""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ocsort_oracle as O  # noqa: E402
from byte_edge_cases import bank_plan, down, up  # noqa: E402,F401
from byte_family_cases import CONFIGS  # noqa: E402,F401

F32 = np.float32
LDS_ARENA_FLOATS = 8428                                          # kernels_ocsort.hip: the static_assert on the LDS arena
NMAX = 512                                                       # trk_dev.hpp: TRK_DEV_NMAX
DTMAX = 8                                                        # ocsort.hpp: OC_DTMAX
DET_THRESH = F32(0.6)


@dataclass
class EdgeScene:
    id: str
    params: dict                                                 # keyword arguments of OCSort (the bank's, after `streams`)
    frames: list                                                 # per frame (boxes_xyxy [n, 4], scores [n], class ids [n])
    edge: int                                                    # the frame (1-based) on which the scene reaches its edge
    chunks: tuple = ()                                           # frames per update call, ragged
    overflow: object = None                                      # one more frame, which needs one slot more than there is
    facts: dict = field(default_factory=dict)                    # what the CPU test needs to find the planted pair

    def oracle(self, lsap_fast=True, record=None):
        kw = {k: v for k, v in self.params.items() if k != "max_tracks"}
        return O.OCSort(lsap_fast=lsap_fast, record=record, **kw)


def B(x, y, w=64, h=128, s=0.9):
    return (x, y, w, h, s)


def frame(*boxes):
    """Boxes (x, y, w, h, score) -> (xyxy, scores, class ids); the class of a detection is its index modulo 3."""
    a = np.array(boxes, F32).reshape(-1, 5)
    xyxy = np.stack([a[:, 0], a[:, 1], a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]], 1).astype(F32)
    return xyxy, a[:, 4].copy(), (np.arange(len(a)) % 3).astype(np.int32)


def ragged(n, edge, k=0):
    """n frames in ragged calls; the edge frame lies inside a call and is not its first frame (where the scene has a frame before it)."""
    sizes = ((3, 1, 2, 4), (2, 3, 1, 5), (1, 4, 2, 3))[k % 3]
    out, f, i = [], 0, 0
    while f < n:
        c = min(sizes[i % 4], n - f)
        if f + 1 == edge and f > 0 and out:                      # the edge frame would open this call: it joins the call before
            out[-1] += 1
            f += 1
            continue
        out.append(c)
        f += c
        i += 1
    assert sum(out) == n
    return tuple(out)


def run_record(params, frames, lsap_fast=True):
    rec = []
    ora = O.OCSort(lsap_fast=lsap_fast, record=rec, **{k: v for k, v in params.items() if k != "max_tracks"})
    for fr in frames:
        ora.update_xyxy(*fr)
    return ora, rec


def problem(rec, frame_no, stage):
    got = [p for p in rec if p["frame"] == frame_no and p["stage"] == stage]
    assert len(got) <= 1
    return got[0] if got else None


def planted_iou(params, frames, edge, stage, det, track):
    """The fp32 IoU of detection `det` (index into the edge frame) and track id `track` in the oracle's own matrix of `stage`."""
    _, rec = run_record(params, frames[:edge])
    p = problem(rec, edge, stage)
    return p["iou"][list(p["dets"]).index(det), p["tracks"].index(track)]


SCENES = []


def add(sid, params, frames, edge, overflow=None, **facts):
    SCENES.append(EdgeScene(sid, params, frames, edge, ragged(len(frames), edge, len(SCENES)), overflow, facts))


# ------------------------------------------------------------------------------------------------------------------ thresholds
SIDES = {"eq": lambda v: F32(v), "below": up, "above": down}     # the IoU is on / one ulp below / one ulp above the threshold


def _threshold_scenes():
    # stage 1: one track walks 16 px a frame; on frame 6 its box comes 24 px ahead of where the filter expects it.  The last observation
    # lies 40 px behind the box (IoU 24 / 104), well under the threshold: OCR cannot rescue a pair that stage 1 drops.
    fr = [frame(B(100 + 16 * f, 100)) for f in range(5)] + [frame(B(100 + 16 * 5 + 24, 100))] + [frame(B(220 + 16 * f, 100)) for f in (0, 1)]
    base = dict(min_hits=1)
    v = planted_iou(base, fr, 6, "stage1", 0, 1)
    for side, th in SIDES.items():
        add("th_stage1_" + side, dict(base, iou_threshold=float(th(v))), fr, 6, stage="stage1", det=0, track=1, iou=v, side=side)
    # OCR: tracks walk 12 px a frame for 8 frames and are unseen for two; on frame 11 a box lies 15 px (8 px: the companion) behind the last
    # observation and 51 px behind the prediction (no overlap).
    walk = lambda f, y: B(100 + 12 * f, y, 40, 100)
    for name, comp, side in (("th_ocr_eq_alone", False, "eq"), ("th_ocr_eq_companion", True, "eq"), ("th_ocr_below_companion", True, "below")):
        ys = (100, 1100) if comp else (100,)
        edge = [B(184 - 15, 100, 40, 100)] + ([B(184 - 8, 1100, 40, 100)] if comp else [])
        fr = [frame(*[walk(f, y) for y in ys]) for f in range(8)] + [frame(), frame()] + [frame(*edge)] * 3
        v = planted_iou(base, fr, 11, "ocr", 0, 1)
        add(name, dict(base, iou_threshold=float(SIDES[side](v))), fr, 11, stage="ocr", det=0, track=1, iou=v, side=side, companion=comp)
    # BYTE: standing tracks; on frame 5 a low-score box lies 15 px (8 px: the companion) beside the prediction
    base = dict(min_hits=1, use_byte=True)
    for name, comp, side in (("th_byte_eq_alone", False, "eq"), ("th_byte_eq_companion", True, "eq"), ("th_byte_below_companion", True, "below")):
        ys = (100, 1100) if comp else (100,)
        stand = frame(*[B(100, y, 40, 100) for y in ys])
        edge = [B(115, 100, 40, 100, 0.3)] + ([B(108, 1100, 40, 100, 0.3)] if comp else [])
        fr = [stand] * 4 + [frame(*edge)] + [stand] * 2
        v = planted_iou(base, fr, 5, "byte", 0, 1)
        add(name, dict(base, iou_threshold=float(SIDES[side](v))), fr, 5, stage="byte", det=0, track=1, iou=v, side=side, companion=comp)
    # OCR against a track born the frame before: last_observation is -1, nothing can match
    fr = [frame(B(100, 100, 40, 100)), frame(B(126, 100, 40, 100))] + [frame(B(100, 100, 40, 100), B(126, 100, 40, 100))] * 2
    add("ocr_no_observation", dict(min_hits=1), fr, 2)


# ------------------------------------------------------------------------------------------------------------------ ties
def _tie_groups(x, y, w, h, s, counts):
    """counts[g] identical boxes at the place of group g (400 px apart), x pixels along."""
    return [B(400 * g + x, y, w, h, s) for g, n in enumerate(counts) for _ in range(n)]


TRACKS_PER_GROUP, DETS_PER_GROUP = (1, 2, 3, 2), (2, 2, 2, 3)       # 2x1, 2x2, 2x3 and 3x2 constant blocks


def _tie_scenes():
    for inertia, sfx in ((0.0, ""), (0.2, "_inertia")):
        born = frame(*_tie_groups(0, 0, 64, 128, 0.9, TRACKS_PER_GROUP))
        over = frame(*_tie_groups(8, 0, 64, 128, 0.9, DETS_PER_GROUP))
        # the boxes walk on: from frame 4 the tracks have a velocity, and identical boxes still tie with the OCM term in the cost
        walk_on = [frame(*_tie_groups(8 * k, 0, 64, 128, 0.9, DETS_PER_GROUP)) for k in (1, 2, 3, 4)]
        add("ties_stage1" + sfx, dict(min_hits=1, inertia=inertia), [born] + walk_on, 2, stage="stage1")
        low = frame(*_tie_groups(8, 0, 64, 128, 0.3, DETS_PER_GROUP))
        add("ties_byte" + sfx, dict(min_hits=1, inertia=inertia, use_byte=True), [born, low, low, over, over], 2, stage="byte")
        # the groups walk 12 px a frame (identical tracks stay identical), are unseen for two frames and meet their boxes on the last observation
        walk = [frame(*_tie_groups(12 * f, 0, 40, 100, 0.9, TRACKS_PER_GROUP)) for f in range(6)]
        back = frame(*_tie_groups(60, 0, 40, 100, 0.9, DETS_PER_GROUP))
        add("ties_ocr" + sfx, dict(min_hits=1, inertia=inertia), walk + [frame(), frame(), back, back, back], 9, stage="ocr")


# ------------------------------------------------------------------------------------------------------------------ scores
def score_edges(det_thresh):
    t = F32(det_thresh)
    return [t, up(t), down(t), O.BYTE_LOW, up(O.BYTE_LOW)]


def _score_scenes():
    for det_thresh, use_byte in ((DET_THRESH, False), (DET_THRESH, True), (F32(0.3), False), (F32(0.3), True)):
        at = [(300 * i, 0) for i in range(5)]
        born = frame(*[B(x, y) for x, y in at])
        edge = [B(x, y, s=s) for (x, y), s in zip(at, score_edges(det_thresh))]
        edge += [B(300 * i, 1000, s=s) for i, s in enumerate(score_edges(det_thresh)[:3])]          # away from every track: only a high one is born
        low = frame(*[B(x, y, s=0.2) for x, y in at])
        after = frame(*([B(x, y) for x, y in at] + [B(300 * i, 1000) for i in range(3)]))
        name = "score_edges" + ("" if det_thresh == DET_THRESH else "_alt") + ("_byte" if use_byte else "")
        # an empty first frame, boxes and no tracks, the edge frame, an empty frame in the middle, a low-only frame
        add(name, dict(min_hits=1, det_thresh=float(det_thresh), use_byte=use_byte), [frame(), born, frame(*edge), frame(), low, after, after], 3)


# ------------------------------------------------------------------------------------------------------------------ OCM
def predicted_box(params, frames):
    """The box the oracle's track 1 predicts for the frame after `frames`."""
    ora, _ = run_record(params, frames)
    t = next(t for t in ora.trackers if t.id == 1)
    return O.x_to_bbox(O.kf7_predict(t.x, t.P)[0])


def _ocm_scenes():
    # the construction of tests/test_ocsort_oracle.py::_ocm_scene: two boxes 16 px left and right of the prediction, equal IoU.  With
    # delta_t = 1 the direction is taken from the last observation, which lies between the two: the term is negative for the left box.
    params = dict(min_hits=1, delta_t=1)
    fr = [frame(B(100 + 8 * f, 100 + 4 * f, 40, 100)) for f in range(4)]
    p = predicted_box(params, fr)
    px, py, w, h = float(p[0]), float(p[1]), float(p[2] - p[0]), float(p[3] - p[1])
    add("ocm_decides", params, fr + [frame(B(px - 16, py, w, h), B(px + 16, py, w, h)), frame(B(px + 24, py + 4, w, h)), frame(B(px + 32, py + 8, w, h))], 5)
    # delta_t = 3: both boxes lie ahead of the observation 3 ages back (age 1: x = 108, centre (128, 150)); a third box is centred on that
    # observation: norm = 1e-6, cosine 0
    params = dict(min_hits=1)
    fr = [frame(B(100 + 8 * f, 100, 40, 100)) for f in range(4)]
    p = predicted_box(params, fr)
    px, py, w, h = float(p[0]), float(p[1]), float(p[2] - p[0]), float(p[3] - p[1])
    left, right = B(px - 16, py, w, h), B(px + 16, py, w, h)
    centred = B(128 - 44, 100, 88, 100)
    add("ocm_same_centre", params, fr + [frame(left, right, centred), frame(B(px + 24, py, w, h), centred), frame(B(px + 32, py, w, h), centred)], 5, det=2)
    # motion along x, 64 px a frame, delta_t = 1: the velocity is (0, 1) exactly; the boxes keep the observations' y, so the direction to
    # each is (0, -1) or (0, +1) exactly and asin32 runs at -1 and +1
    params = dict(min_hits=1, delta_t=1)
    fr = [frame(B(100 + 64 * f, 100, 256, 256)) for f in range(4)]
    px = float(predicted_box(params, fr)[0])
    add("ocm_axis", params, fr + [frame(B(px - 128, 100, 256, 256), B(px + 128, 100, 256, 256)), frame(B(px + 192, 100, 256, 256))], 5)
    # one observation, no velocity yet: the term is computed (has_obs) and is zero for both boxes
    params = dict(min_hits=1)
    fr = [frame(B(100, 100, 40, 100))] * 2
    p = predicted_box(params, fr)
    px, py, w, h = float(p[0]), float(p[1]), float(p[2] - p[0]), float(p[3] - p[1])
    add("ocm_zero_velocity", params, fr + [frame(B(px - 16, py, w, h), B(px + 16, py, w, h))] * 2, 3)


def _ring_scenes():
    """One target on a curve, seen at the ages listed (frame = age + 1; frame 1 is its birth)."""
    at = lambda f: B(100 + 4 * f, 100 + (f * f) // 8, 80, 160)
    for name, dt, ages in (("ring_dt8", DTMAX, (1, 2, 4, 5, 8, 9, 10, 19)), ("ring_dt1", 1, (1, 2, 3, 5, 6))):
        fr = [frame(at(f)) if f == 0 or f in ages else frame() for f in range(max(ages) + 1)]
        add(name, dict(min_hits=1, delta_t=dt), fr, max(ages) + 1, ages=ages)
    # max_age = 1: track 1 (ages 1, 2, 3 observed: every place of the ring written) dies on frame 6; track 2 is born on its slot on frame 7,
    # misses age 1, is seen at age 2 and looks up at age 3: key 1 is an observation of the previous occupant only
    fr = [frame(B(10 * f, 0)) for f in range(4)] + [frame(), frame(), frame(B(1000, 1000)), frame(), frame(B(1000, 1010)), frame(B(1010, 1020)),
                                                    frame(B(1020, 1030))]
    add("slot_reuse_stale_ring", dict(min_hits=1, max_age=1, delta_t=3), fr, 10)


# ------------------------------------------------------------------------------------------------------------------ predictions
def _prediction_scenes():
    # a zero-width box is born as track 3 on frame 4 (past min_hits: a new track is not output, its filter's box has no finite corners) and
    # dropped after the next predict (0 / 0); the same frame brings a new box, which takes its slot
    others = [B(300, 10, 40, 100), B(600, 10, 40, 100)]
    fr = [frame(*others)] * 3 + [frame(B(10, 10, 0, 80), *others)] + [frame(*others, B(900, 10, 40, 100))] * 3
    add("pred_zero_width", dict(), fr, 5)
    # a box that shrinks fast (40 px a frame) and is unseen on frames 5 and 6: the predict of frame 5 steps the area down, that of frame 6
    # would pass zero and clears the area velocity instead (x[6] + x[2] <= 0), and the frozen filter keeps the velocity of frame 5.  On
    # frame 7 the box is refound at 32 x 64 (iou_threshold = 0.01 lets the pair stand).  The ORU replay predicts without that check, so
    # the area steps far below zero inside it, and the closing updates leave (1 - k) s + k z with a negative s: the track, observed and
    # output on frame 7 from its observation, carries a negative area.  The predict of frame 8 takes the branch again, the box is NaN and
    # the track is dropped, its ring filled and its filter unfrozen, while the other track carries on.
    far = B(1500, 100, 40, 100)
    fr = [frame(B(500 - s // 2, 500 - s, s, 2 * s), far) for s in (256, 216, 176, 136)] + [frame(far), frame(far), frame(B(484, 468, 32, 64), far), frame(far), frame(far)]
    add("pred_shrinking", dict(min_hits=1, iou_threshold=0.01), fr, 8)


# ------------------------------------------------------------------------------------------------------------------ life cycle
def _life_scenes():
    a, b = B(0, 0), B(300, 0)
    both = frame(a, b)
    # max_age = 3: both unseen on frames 4..6; on frame 7 track 1 is refound at time_since_update 4 = max_age + 1, track 2 is removed
    add("life_refind_last", dict(min_hits=1, max_age=3), [both] * 3 + [frame()] * 3 + [frame(a), frame(a)], 7)
    # max_age = 1: unseen on frame 4; on frame 5 track 1 is refound with the shortest ORU gap, 2, and track 2 is removed
    add("life_max_age_1", dict(min_hits=1, max_age=1), [both] * 3 + [frame(), frame(a), frame(a)], 5)
    # min_hits = 3: track 1 from frame 1, track 2 from frame 2; track 1 misses frame 5
    fr = [frame(a), both, both, both, frame(B(300, 0)), both, both, both]
    add("life_min_hits", dict(), fr, 4)


# ------------------------------------------------------------------------------------------------------------------ output, capacity
def _output_scenes():
    xyxy = np.array([[10.5, 11.5, 50.5, 111.5], [-3.5, -2.5, 36.5, 97.5], [200.5, 300.5, 241.5, 401.5], [-100.5, 600.5, -61.5, 699.5]], F32)
    fr = []
    for shift in (0, 0, 1, 1):                                   # a corner k + 0.5 with k even and with k odd
        fr.append((xyxy + F32(shift), np.full(4, 0.9, F32), np.arange(4, dtype=np.int32) % 3))
    add("out_rounding", dict(min_hits=1), fr, 2)


def _capacity_scenes():
    at = [(300 * i, 0) for i in range(5)] + [(300 * i, 1000) for i in range(3)]
    five, eight = frame(*[B(x, y) for x, y in at[:5]]), frame(*[B(x, y) for x, y in at])
    # 512 boxes, the largest accepted count: the eight tracks' and 504 below det_thresh
    crowd = [B(x, y) for x, y in at] + [B(40 * (i % 32), 2000 + 40 * (i // 32), 30, 30, 0.05 + 0.5 * (i % 11) / 11) for i in range(NMAX - 8)]
    over = frame(*([B(x, y) for x, y in at] + [B(0, 3000)]))
    add("capacity_boundary", dict(min_hits=1, max_tracks=8), [five, eight, frame(*crowd), eight], 2, overflow=over)


# ------------------------------------------------------------------------------------------------------------------ assignment regimes
REGIMES = ((64, 64), (65, 65), (128, 128), (129, 129), (86, 98), (87, 97), (3, 200), (200, 3))    # detections x tracks of the stage-1 problem


def grid(n, dx=0, dy=0):
    """n boxes of 64 x 128 on a grid of pitch 32 x 64, 16 to a row: neighbours overlap with IoU 1/3, above the threshold."""
    return [B(32 * (i % 16) + dx, 64 * (i // 16) + dy) for i in range(n)]


def _regime_scenes():
    for nd, nt in REGIMES:
        # frame 1: nt births; frame 2: nd boxes half a pitch off the grid, each over up to four tracks with the same IoU; frame 3: back on it
        add(f"regime_{nd}x{nt}", dict(min_hits=1), [frame(*grid(nt)), frame(*grid(nd, 16, 32)), frame(*grid(max(nd, nt)))], 2, shape=(nd, nt))


for _build in (_threshold_scenes, _tie_scenes, _score_scenes, _ocm_scenes, _ring_scenes, _prediction_scenes, _life_scenes, _output_scenes,
               _capacity_scenes, _regime_scenes):
    _build()
SCENES = tuple(SCENES)
assert len({sc.id for sc in SCENES}) == len(SCENES) and all(len(sc.frames) <= 21 for sc in SCENES)


def scene_of(sid):
    return next(s for s in SCENES if s.id == sid)


def chunked(sid):
    """The scene's frames as its ragged update calls."""
    sc, out, f = scene_of(sid), [], 0
    for n in sc.chunks:
        out.append(sc.frames[f:f + n])
        f += n
    assert f == len(sc.frames), (sid, f)
    return out


# ------------------------------------------------------------------------------------------------------------------ the oracle's trace
_TRACES = {}


def oracle_trace(sid, lsap_fast=True, extra=()):
    """The oracle over the scene (and the frames `extra` behind it) -> (per-frame records, the oracle); computed once.  A record holds
      problems     the non-empty association problems of the frame, as the oracle's recording hook gives them
      rows, conf   the output; raw = the unrounded x1 y1 x2 y2 behind the rows, out_ids = their track ids
      export       the oracle's export() after the frame; stats = its counters after the frame; ids = the live track ids
      lookup       track id -> (age, exit, box) of k_previous_obs at the predict: exit 1 = the observation delta_t ages back, 2 = a younger one,
                   3 = the last observation, 0 = the track has no observation
      zeroed       ids of the tracks whose predict cleared the area velocity (x[6] + x[2] <= 0)
      dropped      ids of the tracks dropped for a non-finite prediction;  n_dets = detections in the frame"""
    key = (sid, bool(lsap_fast), len(extra))
    if key in _TRACES:
        return _TRACES[key]
    sc = scene_of(sid)
    rec = []
    ora = sc.oracle(lsap_fast, rec)
    inner_predict, inner_prev = O.KalmanBoxTracker.predict, O.KalmanBoxTracker.previous_obs
    cur, trace = {}, []

    def predict(self):
        if F32(self.x[6] + self.x[2]) <= 0:
            cur["zeroed"].append(self.id)
        b = inner_predict(self)
        if not np.all(np.isfinite(b)):
            cur["dropped"].append(self.id)
        return b

    def previous_obs(self):
        box, valid = inner_prev(self)
        if self.id not in cur["lookup"]:                          # the call of the frame's predict (update() looks up again, at the same age)
            ex = 0
            if valid:
                ex = 3
                for dt in range(self.delta_t, 0, -1):
                    if self.age - dt in self.observations:
                        ex = 1 if dt == self.delta_t else 2
                        break
            cur["lookup"][self.id] = (self.age, ex, np.array(box, F32))
        return box, valid

    O.KalmanBoxTracker.predict, O.KalmanBoxTracker.previous_obs = predict, previous_obs
    try:
        for fr in list(sc.frames) + list(extra):
            cur = dict(zeroed=[], dropped=[], lookup={})
            n0 = len(rec)
            out = ora.update_xyxy(*fr)
            rows, conf = O.OCSort.rows(out)
            raw = np.array([t.last_observation if t.has_obs else O.x_to_bbox(t.x) for t in out], F32).reshape(-1, 4)
            trace.append(dict(frame=ora.frame_count, problems=rec[n0:], rows=rows, conf=conf, raw=raw, out_ids=[t.id for t in out],
                              export={k: np.array(v, copy=True) for k, v in ora.export().items()}, stats=dict(ora.stats),
                              ids=[t.id for t in ora.trackers], n_dets=len(fr[0]), **cur))
    finally:
        O.KalmanBoxTracker.predict, O.KalmanBoxTracker.previous_obs = inner_predict, inner_prev
    _TRACES[key] = (trace, ora)
    return _TRACES[key]


def stage_problem(rec, stage):
    got = [p for p in rec["problems"] if p["stage"] == stage]
    assert len(got) <= 1
    return got[0] if got else None


def optimal_assignments_at_least_two(cost):
    """Whether the rectangular LSAP on `cost` has two different optimal assignments: forbid each pair of one optimum in turn and solve again."""
    from scipy.optimize import linear_sum_assignment
    import math
    c = np.asarray(cost, F32).astype(np.float64)
    r, k = linear_sum_assignment(c)
    best = math.fsum(c[r, k])
    big = float(np.abs(c).sum() + 1.0)
    for i, j in zip(r, k):
        d = c.copy()
        d[i, j] = big
        r2, k2 = linear_sum_assignment(d)
        if math.fsum(d[r2, k2]) == best:
            return True
    return False
