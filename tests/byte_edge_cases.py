"""Planted scenes for the BYTE skeleton (csrc/byte_epoch.hpp): duplicates, costs on a threshold, tied optima, scores on a band edge,
slot reuse, empty frames and the capacity boundary -- the places the random scenes of tests/byte_family_cases.py never reach.

tests/test_byte_edge_cases.py (CPU) holds the NumPy oracles to the edge each scene is named for; tests/test_gpu_byte_edges.py (GPU)
replays every scene through the public ByteTrack and BoT-SORT classes, alone and as a bank, and compares frame by frame.

Every box has integer corners and power-of-two sides where a cost has to be exact, so that a = w / h, the areas and the IoU are exact
in fp32.  ByteTrack's update is only close to the oracle's (LAPACK against an ordered sum), so its scenes are of two classes:
  exact   no track that takes part in the edge decision has been updated before the edge frame (initiate and predict are bit-exact);
  margin  the scene needs updates (the duplicate scenes); its edge is an integer one (end - start), and every float decision after a
          first update keeps MARGIN_* away from its threshold (asserted on the oracle by the CPU test).
BoT-SORT's oracle states every sum in the kernel's order: there an edge may sit anywhere."""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from byte_family_cases import CONFIGS, KINDS  # noqa: E402,F401

F32 = np.float32
DIM = 64
MARGIN_COST = 1e-3                                               # a cost of updated tracks to its threshold; a duplicate distance to 0.15
MARGIN_PIXEL = 0.01                                              # an unrounded output coordinate of an updated track to k + 0.5
# band edges per tracker at the defaults, and at the non-default set of score_edges_alt: (high, low, new)
BANDS = {"default": {"bytetrack": (F32(0.5), F32(0.1), F32(0.5 + 0.1)), "botsort": (F32(0.6), F32(0.1), F32(0.7))},
         "alt": {"bytetrack": (F32(0.3), F32(0.2), F32(0.3 + 0.1)), "botsort": (F32(0.3), F32(0.2), F32(0.4))}}
MATCH, SECOND, UNCONF, DUP = F32(0.8), F32(0.5), F32(0.7), F32(0.15)
STAGE_THRESH = {1: MATCH, 2: SECOND, 3: UNCONF}


def up(x, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(np.inf), dtype=F32)
    return x


def down(x, k=1):
    x = F32(x)
    for _ in range(k):
        x = np.nextafter(x, F32(-np.inf), dtype=F32)
    return x


# ------------------------------------------------------------------------------------------------------------------ cost arithmetic
def iou_cost(track_tlwh, det_tlwh):
    """The oracles' 1 - IoU of one box against another, fp32."""
    from oracle.deepsort_oracle import iou_cost_matrix
    return iou_cost_matrix([np.asarray(track_tlwh, F32)], [np.asarray(det_tlwh, F32)])[0, 0]


def fused(d, s):
    """fuse_score of one entry: 1 - (1 - d) * s in fp32."""
    return F32(F32(1) - F32(F32(1) - F32(d)) * F32(s))


def crossing(cost_of, x0, step):
    """The first fp32 value behind x0 in direction `step` (up / down) at which cost_of(x) leaves cost_of(x0), at most 8 ulps away."""
    c0, x = cost_of(F32(x0)), F32(x0)
    for _ in range(8):
        x = step(x)
        if cost_of(x) != c0:
            return x
    raise AssertionError("the cost does not move within 8 ulps")


# ------------------------------------------------------------------------------------------------------------------ scenes
def box(x, y, w, h, s, ident):
    return (F32(x), F32(y), F32(w), F32(h), F32(s), int(ident))


@dataclass
class EdgeScene:
    id: str
    build: object                                                # kind -> list of frames, a frame a list of box()
    chunks: tuple                                                # frames per update call, ragged
    cls: str = "exact"                                           # ByteTrack's class: "exact" or "margin"
    bands: str = "default"
    kw: dict = field(default_factory=dict)                       # track_buffer, max_tracks, with_reid
    overflow: object = None                                      # kind -> one more frame, which needs one slot more than there is

    def params(self, kind):
        """Keyword arguments of the public single class (the bank's, after `streams`)."""
        high, low, new = BANDS[self.bands][kind]
        kw = {k: v for k, v in self.kw.items() if k != "with_reid"}
        if kind == "bytetrack":
            if self.bands != "default":
                kw.update(track_thresh=float(high), low_thresh=float(low))      # new_track_thresh = track_thresh + 0.1, as upstream
            return kw
        kw.update(feature_dim=DIM, with_reid=self.kw.get("with_reid", True))
        if self.bands != "default":
            kw.update(track_high_thresh=float(high), track_low_thresh=float(low), new_track_thresh=float(new))
        return kw

    def oracle(self, kind):
        import botsort_oracle
        import bytetrack_oracle
        kw = {k: v for k, v in self.params(kind).items() if k not in ("max_tracks", "feature_dim")}
        return bytetrack_oracle.BYTETracker(**kw) if kind == "bytetrack" else botsort_oracle.BoTSORT(**kw)


W, H = 64, 128                                                   # the small power-of-two box
FAR = box(3000, 1000, 200, 400, 0.9, 90)                          # the bystander


def _dup(L, born, a_x, last):
    """B (ident 0) walks 100 px per frame for L frames and then coasts, Lost; A (ident 1) stands at a_x from frame `born` on."""
    def build(kind):
        out = []
        for f in range(1, last + 1):
            fr = [FAR]
            if f <= L:
                fr.append(box(100 * (f - 1), 0, 200, 400, 0.9, 0))
            if f >= born:
                fr.append(box(a_x, 0, 200, 400, 0.9, 1))
            out.append(fr)
        return out
    return build


def _dup_many(kind):
    """Row y = 100: a lost walker B over two standing tracks, A1 younger than B (A1 is dropped) and A2 older (B is dropped).
    Row y = 2000: two lost walkers C1 (age 7) and C2 (born a frame later: age 6) under one standing track D of age 7:
    the tie with C1 drops D, C2 is dropped by D.  Both drop flags are therefore written from several pairs of one frame."""
    L, f_hit = 8, 13
    out = []
    for f in range(1, 17):
        fr = [FAR]
        if f <= L:
            fr.append(box(100 * (f - 1), 100, 200, 400, 0.9, 0))                 # B
            fr.append(box(100 * (f - 1), 2000, 200, 400, 0.9, 10))               # C1
            if f >= 2:
                fr.append(box(100 * (f - 1) + 0.25, 2016, 200, 400, 0.9, 11))    # C2 (a quarter pixel off: its rows stay clear of k + 0.5)
        fr.append(box(1150, 108, 200, 400, 0.9, 2))                              # A2, from frame 1
        if f >= 10:
            fr.append(box(1150, 92, 200, 400, 0.9, 1))                           # A1
        if f >= f_hit - 7:
            fr.append(box(1150, 2008, 200, 400, 0.9, 12))                        # D: age 7 on the frame the walkers arrive
        out.append(fr)
    return out


def _cost_eq(stage, side):
    """One track and a box inside it whose stage-`stage` cost is its threshold (side 0), or the next fp32 cost below (-1) / above (+1).
    Stage 1: 16 x 128 in 64 x 128 (IoU 1/4) at score fp32(0.8); stage 2: 32 x 128 (IoU 1/2) at 0.3; stage 3: an unconfirmed track born on
    frame 2 and a 24 x 128 box (IoU 3/8) at the score that gives fp32(0.7)."""
    def build(kind):
        track = (0, 0, W, H)
        if stage == 1:
            s = F32(0.8)
            if side:
                s = crossing(lambda v: fused(F32(0.75), v), s, down if side > 0 else up)     # a lower score is a higher cost
            probe = box(0, 0, 16, H, s, 21)
        elif stage == 2:
            w = F32(32)
            if side:
                w = crossing(lambda v: iou_cost(track, (0, 0, v, H)), w, down if side > 0 else up)
            probe = box(0, 0, w, H, 0.3, 21)
        else:
            s = STAGE3_SCORE
            if side:
                s = crossing(lambda v: fused(F32(0.625), v), s, down if side > 0 else up)
            probe = box(0, 0, 24, H, s, 21)
        born = [[FAR, box(0, 0, W, H, 0.9, 20)]]
        if stage == 3:
            born = [[FAR]] + born                                 # born on frame 2: unconfirmed
        # afterwards, a box exactly on the track that stands there then: at stage 3 the unmet probe has become a track of its own
        after = [FAR, box(0, 0, 24 if stage == 3 and side >= 0 else W, H, 0.9, 22)]
        return born + [[FAR, probe], after, after]
    return build


def _stage3_score():
    """The fp32 score s with 1 - (3 / 8) s == fp32(0.7), searched around 0.8."""
    for k in range(-16, 17):
        s = up(F32(0.8), k) if k >= 0 else down(F32(0.8), -k)
        if fused(F32(0.625), s) == UNCONF:
            return s
    raise AssertionError("no fp32 score puts the stage-3 cost on 0.7")


STAGE3_SCORE = _stage3_score()


def _tie_pattern(x0, y0, s, first_ident, tracks):
    """Three tied problems side by side: two identical boxes over one track, two identical tracks under one box, and two tracks and two
    boxes with four equal costs.  tracks=True gives the boxes the tracks are born from, False the boxes that meet them."""
    if tracks:
        return [box(x0, y0, W, H, s, first_ident), box(x0 + 400, y0, W, H, s, first_ident + 1), box(x0 + 400, y0, W, H, s, first_ident + 1),
                box(x0 + 800, y0, W, H, s, first_ident + 2), box(x0 + 816, y0, W, H, s, first_ident + 3)]
    return [box(x0, y0, W, H, s, first_ident), box(x0, y0, W, H, s, first_ident), box(x0 + 400, y0, W, H, s, first_ident + 1),
            box(x0 + 808, y0 - 8, W, H, s, first_ident + 2), box(x0 + 808, y0 + 8, W, H, s, first_ident + 3)]


def _ties(kind):
    """Frame 1: the tracks of a stage-1 pattern (y = 0) and of a stage-2 pattern (y = 1000); frame 2: high boxes over the first, low boxes
    over the second; frame 3: one high box per place."""
    again = [box(x, y, W, H, 0.9, 60 + i) for i, (x, y) in enumerate([(0, 0), (400, 0), (800, 0), (816, 0), (0, 1000), (400, 1000), (800, 1000), (816, 1000)])]
    return [_tie_pattern(0, 0, 0.9, 30, True) + _tie_pattern(0, 1000, 0.9, 40, True),
            _tie_pattern(0, 0, 0.9, 50, False) + _tie_pattern(0, 1000, 0.3, 54, False), again, again]


def _ties_unconfirmed(kind):
    """The pattern at stage 3: the tracks are born on frame 2, unconfirmed, and meet their boxes on frame 3."""
    again = [FAR] + [box(x, 0, W, H, 0.9, 60 + i) for i, x in enumerate((0, 400, 800, 816))]
    return [[FAR], [FAR] + _tie_pattern(0, 0, 0.9, 30, True), [FAR] + _tie_pattern(0, 0, 0.9, 50, False), again, again]


def _score_edges(bands):
    def build(kind):
        """Frame 2 puts the nine scores down: high -/0/+ and low -/0/+ over six tracks, new -/0/+ away from any track."""
        high, low, new = BANDS[bands][kind]
        at = [(300 * i, 0) for i in range(6)]
        born = [box(x, y, W, H, 0.9, i) for i, (x, y) in enumerate(at)]
        scores = [down(high), high, up(high), down(low), low, up(low)]
        edge = [box(x, y, W, H, s, i) for i, ((x, y), s) in enumerate(zip(at, scores))]
        edge += [box(300 * i, 1000, W, H, s, 6 + i) for i, s in enumerate((down(new), new, up(new)))]
        after = born + [box(300 * i, 1000, W, H, 0.9, 6 + i) for i in range(3)]
        return [born, edge, after, after]
    return build


def _slots_frames(kind):
    T = [box(300 * i, 0, W, H, 0.9, i) for i in range(5)]
    low = [box(300 * i, 0, W, H, 0.3, i) for i in range(3)]
    new = [box(300 * i, 1000, W, H, 0.9, 20 + i) for i in range(8)]
    return T, low, new


def _slots(kind):
    """track_buffer = 3, max_tracks = 8.
     1 T1..T5 are born              2 + U1 (unconfirmed, slot 5)        3 U1 unmet: removed; V1 born on the slot U1 leaves
     4 low boxes only, over T1..T3: T4, T5 lost, V1 removed             5 no detections: T1..T3 lost
     6 T1 refound; a low box over the lost T2 meets nothing; T4, T5 are max_time_lost old and stay
     7 T4 is refound (it is still there); T5 is removed; T2, T3 are max_time_lost old and stay
     8 T2 is refound, T3 removed    9 T1, T4, T2 + four new: one slot left
    10 one of the four unmet (its slot is freed), two new: exactly full"""
    T, low, new = _slots_frames(kind)
    live = [T[0], T[3], T[1]]
    return [T, T + [new[6]], T + [new[7]], low, [], [T[0], low[1]], [T[0], T[3]], live, live + new[:4], live + new[:3] + [new[6], new[7]]]


def _slots_overflow(kind):
    """Frame 11: the two unconfirmed tracks of frame 10 are unmet (two slots freed), three boxes are new: one slot short."""
    T, low, new = _slots_frames(kind)
    return [T[0], T[3], T[1]] + new[:3] + [box(300 * i, 2000, W, H, 0.9, 40 + i) for i in range(3)]


SCENES = (EdgeScene("dup_drop_tracked", _dup(8, 10, 1150, 16), (5, 1, 8, 2), cls="margin"),
          EdgeScene("dup_drop_lost", _dup(3, 4, 625, 15), (2, 7, 1, 5), cls="margin", kw=dict(with_reid=False)),
          EdgeScene("dup_tie", _dup(6, 7, 1000, 16), (4, 6, 3, 3), cls="margin"),
          EdgeScene("dup_many", _dup_many, (9, 5, 2), cls="margin"),
          EdgeScene("cost_eq_stage1", _cost_eq(1, 0), (3, 1)), EdgeScene("cost_eq_stage1_below", _cost_eq(1, -1), (4,)),
          EdgeScene("cost_eq_stage1_above", _cost_eq(1, 1), (2, 1, 1)),
          EdgeScene("cost_eq_stage2", _cost_eq(2, 0), (3, 1)), EdgeScene("cost_eq_stage2_below", _cost_eq(2, -1), (2, 1, 1)),
          EdgeScene("cost_eq_stage2_above", _cost_eq(2, 1), (4,)),
          EdgeScene("cost_eq_stage3", _cost_eq(3, 0), (4, 1)), EdgeScene("cost_eq_stage3_below", _cost_eq(3, -1), (3, 2)),
          EdgeScene("cost_eq_stage3_above", _cost_eq(3, 1), (1, 4)),
          EdgeScene("ties", _ties, (3, 1)), EdgeScene("ties_unconfirmed", _ties_unconfirmed, (1, 3, 1)),
          EdgeScene("score_edges", _score_edges("default"), (3, 1)), EdgeScene("score_edges_alt", _score_edges("alt"), (2, 1, 1), bands="alt"),
          EdgeScene("slots_and_empties", _slots, (3, 4, 3), cls="margin", kw=dict(track_buffer=3, max_tracks=8), overflow=_slots_overflow))
# the frames (1-based) on which each scene reaches its edge: the chunk plans put them inside a call, never first in one
EDGE_FRAMES = {"dup_drop_tracked": (13,), "dup_drop_lost": (12,), "dup_tie": (12,), "dup_many": (13,), "ties": (2,), "ties_unconfirmed": (3,),
               "score_edges": (2,), "score_edges_alt": (2,), "slots_and_empties": (3, 5, 7, 10)}
EDGE_FRAMES.update({f"cost_eq_stage{st}{sfx}": (3 if st == 3 else 2,) for st in (1, 2, 3) for sfx in ("", "_below", "_above")})
# one bank per tracker: every scene a stream; frames of stream s in call c = BANK_CALLS[(s + c) % len] (+ 2 from the third call on):
# ragged, and every stream is absent from one of the first two calls, while it still has frames to come
BANK_CALLS = (3, 1, 2, 3, 2)
_FRAMES = {}


def scene_of(sid):
    return next(s for s in SCENES if s.id == sid)


def pack(frame, f, kind):
    """A list of box() as the tuple the classes and the oracles take: (xyxy, scores, cls) and, for BoT-SORT, (features, warp)."""
    from conftest import pkg
    a = np.array([b[:5] for b in frame], F32).reshape(-1, 5)
    ident = np.array([b[5] for b in frame], np.int64)
    xyxy = np.stack([a[:, 0], a[:, 1], a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]], 1).astype(F32)
    cls = (ident % 3).astype(np.int32)
    if kind == "bytetrack":
        return xyxy, a[:, 4].copy(), cls
    ft = (pkg("synthetic").identity_features(ident, f, dim=DIM, seed=7) * F32(1.5 + 0.01 * f)).astype(F32).reshape(-1, DIM)
    return xyxy, a[:, 4].copy(), cls, ft, None


def frames_of(sid, kind):
    """Per frame (boxes, scores, cls) for ByteTrack, (boxes, scores, cls, raw 64-float features, None) for BoT-SORT; computed once."""
    if (sid, kind) not in _FRAMES:
        _FRAMES[sid, kind] = [pack(fr, f, kind) for f, fr in enumerate(scene_of(sid).build(kind))]
    return _FRAMES[sid, kind]


def overflow_of(sid, kind):
    sc = scene_of(sid)
    return pack(sc.overflow(kind), len(frames_of(sid, kind)), kind)


def chunked(sid, kind):
    """The scene's frames as its ragged update calls."""
    frames, out, f = frames_of(sid, kind), [], 0
    for n in scene_of(sid).chunks:
        out.append(frames[f:f + n])
        f += n
    assert f == len(frames), (sid, f, len(frames))
    return out


def bank_plan(lengths):
    """Frames per call and stream until every stream is through."""
    pos, plan = [0] * len(lengths), []
    while any(p < n for p, n in zip(pos, lengths)):
        c = len(plan)
        call = [0 if c == (s + 1) % 2 else min(BANK_CALLS[(s + c) % len(BANK_CALLS)] + 2 * (c >= 2), lengths[s] - pos[s]) for s in range(len(lengths))]
        pos = [p + c for p, c in zip(pos, call)]
        plan.append(call)
    return plan


# ------------------------------------------------------------------------------------------------------------------ the read-off
def read_off(cost, th):
    """The unique-optimum condition of byte_assign: no entry equals th, every row and every column holds at most one entry below it."""
    cost, th = np.asarray(cost, F32), F32(th)
    below = cost < th
    return bool(not (cost == th).any() and (below.sum(1) <= 1).all() and (below.sum(0) <= 1).all())


# ------------------------------------------------------------------------------------------------------------------ the oracles
def oracle_trace(kind, sid, extra=()):
    """The oracle over the scene (and the frames `extra` behind it) -> (per-frame records, the oracle).  A record holds
      problems    the non-empty assignment problems: dict(stage, cost, th, matches, ids = the track ids of the rows)
      dup         dict(dist = the duplicate check's IoU distances [tracked, lost], pairs = [(tracked id, lost id, age, age)] below 0.15,
                  dropped_tracked, dropped_lost = track ids)
      rows, conf  the output; raw = the unrounded x1 y1 x2 y2 of the output tracks, out_ids their ids
      updated     ids of the tracks that had taken a detection BEFORE this frame; updated_after: with this frame's
      tracked, lost, unconfirmed, removed   ids after the frame (removed: in this frame)"""
    import botsort_oracle
    import bytetrack_oracle
    mod = bytetrack_oracle if kind == "bytetrack" else botsort_oracle
    ora = scene_of(sid).oracle(kind)
    inner_la, inner_dup = mod.linear_assignment, mod.remove_duplicate_stracks
    updated, cur, trace = set(), {}, []
    taking = ("update", "re_activate") if kind == "bytetrack" else ("update",)
    inner_take = {n: getattr(mod.STrack, n) for n in taking}

    def la(cost, thresh):
        res = inner_la(cost, thresh)
        cur["calls"].append((np.array(cost, F32, copy=True), F32(thresh), list(res[0]), list(res[1])))
        return res

    def dup(a, b):
        dist = np.array(mod.iou_distance(a, b), F32).reshape(len(a), len(b))
        ra, rb = inner_dup(a, b)
        age = lambda t: t.frame_id - t.start_frame
        cur["dup"] = dict(dist=dist, ids=([t.track_id for t in a], [t.track_id for t in b]),
                          pairs=[(a[p].track_id, b[q].track_id, age(a[p]), age(b[q])) for p, q in zip(*np.where(dist < DUP))],
                          dropped_tracked=[t.track_id for t in a if t not in ra], dropped_lost=[t.track_id for t in b if t not in rb])
        return ra, rb

    def taker(name):
        def take(self, *a, **k):
            cur["took"].add(self.track_id)
            return inner_take[name](self, *a, **k)
        return take

    mod.linear_assignment, mod.remove_duplicate_stracks = la, dup
    for n in taking:
        setattr(mod.STrack, n, taker(n))
    try:
        for fr in list(frames_of(sid, kind)) + list(extra):
            tracked, lost = list(ora.tracked_stracks), list(ora.lost_stracks)
            pool = [t for t in tracked if t.is_activated] + lost
            unconfirmed = [t for t in tracked if not t.is_activated]
            was_tracked = {t.track_id for t in pool if t.state == mod.TRACKED}
            cur = dict(calls=[], took=set(), dup=None)
            out = ora.update_xyxy(*fr)
            (c1, t1, m1, u1), (c2, t2, m2, _), (c3, t3, m3, _) = cur["calls"]
            rows2 = [pool[i].track_id for i in u1 if pool[i].track_id in was_tracked]
            problems = [dict(stage=st, cost=c, th=t, matches=m, ids=ids)
                        for st, c, t, m, ids in ((1, c1, t1, m1, [t.track_id for t in pool]), (2, c2, t2, m2, rows2),
                                                 (3, c3, t3, m3, [t.track_id for t in unconfirmed])) if c.size]
            for p in problems:
                assert len(p["ids"]) == p["cost"].shape[0] and p["th"] == STAGE_THRESH[p["stage"]], (sid, p["stage"])
            rows, conf = ora.rows(out)
            raw = []
            for t in out:
                x1, y1, w, h = mod.mean_to_tlwh(t.mean)
                w, h = max(F32(0), w), max(F32(0), h)
                raw.append((x1, y1, x1 + w, y1 + h))
            trace.append(dict(frame=ora.frame_id, problems=problems, dup=cur["dup"], rows=rows, conf=conf,
                              raw=np.array(raw, F32).reshape(-1, 4), out_ids=[t.track_id for t in out], updated=frozenset(updated),
                              updated_after=frozenset(updated | cur["took"]),
                              tracked=[t.track_id for t in ora.tracked_stracks], lost=[t.track_id for t in ora.lost_stracks],
                              unconfirmed=[t.track_id for t in ora.tracked_stracks if not t.is_activated],
                              removed=[t.track_id for t in tracked + lost if t.state == mod.REMOVED], n_dets=len(fr[0])))
            updated |= cur["took"]
    finally:
        mod.linear_assignment, mod.remove_duplicate_stracks = inner_la, inner_dup
        for n in taking:
            setattr(mod.STrack, n, inner_take[n])
    return trace, ora
