"""Planted scenes for what BoT-SORT adds to the BYTE skeleton (BsVariant of csrc/kernels_botsort.hip, the feature arithmetic of
csrc/kf8wh_math.hpp, botsort_normalize_kernel): the proximity veto and the appearance gate on their thresholds, an appearance distance
equal to the IoU distance, the clamp at 0, a slot's first feature against the smoothed update, the has_feat life cycle, the one pair of
a problem that needs a dot product on the 64-pair group boundaries of cost_pass, the camera-motion warp before the costs, and features
whose normalised row is not finite.  The skeleton's own edges are tests/byte_edge_cases.py's.

tests/test_botsort_edge_cases.py (CPU) holds the oracle to the edge each scene is named for; tests/test_gpu_botsort_edges.py (GPU)
replays every scene through the public BoTSORT and BoTSORTBank classes and compares bit for bit.

Exact features: with dim 64 and raw entries of +-0.25 the squared sum is 4, its root 2 and the unit feature +-1/8; two such features
that differ in m signs have the ordered dot product (64 - 2m) / 64 and the appearance distance e = m / 64, both exact in fp32.  A slot
that has taken one feature holds it verbatim.  Boxes have integer corners and power-of-two sides, a track that has only met boxes equal
to its own has an exact mean, so IoU 1/4 and 3/4 are exact too.  A threshold is a parameter: it is set to the planted cost or to its
fp32 neighbour; for a smoothed feature the cost is taken from the oracle's own first pass (Scene.kw as a function of that pass)."""
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import botsort_oracle as O  # noqa: E402
from byte_edge_cases import H, MATCH, UNCONF, W, bank_plan, crossing, down, fused, iou_cost, read_off, up  # noqa: E402,F401
from byte_family_cases import CONFIGS  # noqa: E402,F401

F32 = np.float32
DIM = 64
NEAR = 0.875                                                     # a proximity_thresh that keeps an IoU of 1/4 (distance 0.75) near
RESCUE_W, RESCUE_S = 16, F32(0.7)                                # a 16 x 128 box in a 64 x 128 track at score 0.7: fused distance 0.825 > 0.8
GROUP = 64                                                       # pairs per wavefront of cost_pass
SWEEP = 8 * GROUP                                                # pairs per sweep of the block: NW (csrc/trk_wave.hpp) wavefronts


# ------------------------------------------------------------------------------------------------------------------ features
def signs(k):
    """Row k of the 64 x 64 Walsh matrix: rows of different k are orthogonal (appearance distance 1/2)."""
    return np.array([(-1) ** bin(i & k).count("1") for i in range(DIM)], F32)


def feat(k, m=0):
    """The raw feature of identity k with its first m signs flipped: e(feat(k, a), feat(k, b)) = |a - b| / 64."""
    v = signs(k)
    v[:m] *= -1
    return (F32(0.25) * v).astype(F32)


def blend(first, second, alpha=F32(0.9)):
    """The smoothed unit feature of a slot that took raw `first` and then raw `second`, as the oracle states it."""
    return O.normalise(alpha * O.normalise(first) + (F32(1) - alpha) * O.normalise(second))


def _self_dot_above_one():
    """(k, m) such that s = blend(feat(k), feat(k, m)) has an ordered self-dot above 1 and is its own normalisation: handed back as a raw
    feature it meets the slot that holds it at 1 - dot < 0."""
    for m in range(1, 33):
        s = blend(feat(9), feat(9, m))
        if O.wave_sum(s * s) > 1 and np.array_equal(O.normalise(s), s):
            return 9, m
    raise AssertionError("no blend with a self-dot above 1")


CLAMP_K, CLAMP_M = _self_dot_above_one()


# ------------------------------------------------------------------------------------------------------------------ scenes
def det(x, y, w, h, s, ft, cls=0):
    """One detection; ft = its raw feature, or None for a row without one (valid = 0: an empty crop)."""
    return dict(box=(F32(x), F32(y), F32(w), F32(h)), s=F32(s), cls=int(cls), ft=None if ft is None else np.asarray(ft, F32))


def on(x, y, ft, s=0.9, cls=0):
    return det(x, y, W, H, s, ft, cls)


def rescue(x, y, ft, cls=0):
    """Inside the 64 x 128 track at (x, y): IoU 1/4, and a fused distance above match_thresh -- it matches by appearance or not at all."""
    return det(x, y, RESCUE_W, H, RESCUE_S, ft, cls)


FAR = on(3000, 1000, feat(63))                                    # the bystander


@dataclass
class Scene:
    id: str
    build: object                                                # () -> list of frames; a frame a list of det() or (list of det(), warp 2x3)
    chunks: tuple                                                # frames per update call, ragged
    edge: tuple                                                  # the frames (1-based) on which the scene reaches its edge
    kw: object = None                                            # parameters that differ from the defaults; or a function () -> dict

    def params(self):
        kw = self.kw() if callable(self.kw) else dict(self.kw or {})
        return dict(kw, feature_dim=DIM)

    def oracle(self, **over):
        kw = {k: v for k, v in self.params().items() if k not in ("max_tracks", "feature_dim")}
        kw.update(over)
        return O.BoTSORT(**kw)


_FRAMES, _TRACES = {}, {}
# a row without a feature still carries DIM floats to the device: these, which would match anything of identity 9 if they were read
UNREAD = feat(CLAMP_K)


def scene_of(sid):
    return next(s for s in SCENES if s.id == sid)


def frames_of(sid, sign=1):
    """Per frame the tuple BoTSORT.update_batch_arrays takes: (xyxy, scores, cls, raw features [n, 64], warp or None, valid or None).
    sign = -1 negates every feature: every dot product, cost and decision stays, every smoothed feature comes out negated, bit for bit."""
    if (sid, sign) not in _FRAMES:
        out = []
        for fr in scene_of(sid).build():
            dets, warp = fr if isinstance(fr, tuple) else (fr, None)
            a = np.array([d["box"] for d in dets], F32).reshape(-1, 4)
            xyxy = np.stack([a[:, 0], a[:, 1], a[:, 0] + a[:, 2], a[:, 1] + a[:, 3]], 1).astype(F32)
            ft = np.array([(UNREAD if d["ft"] is None else d["ft"]) * F32(sign) for d in dets], F32).reshape(-1, DIM)
            valid = np.array([d["ft"] is not None for d in dets], np.int32)
            out.append((xyxy, np.array([d["s"] for d in dets], F32), np.array([d["cls"] for d in dets], np.int32), ft,
                        None if warp is None else np.asarray(warp, F32).reshape(2, 3), None if valid.all() else valid))
        _FRAMES[sid, sign] = out
    return _FRAMES[sid, sign]


def oracle_args(fr):
    """A frame of frames_of as the oracle's update_xyxy takes it: a row with valid = 0 has the feature None."""
    b, s, c, ft, warp, valid = fr
    return b, s, c, [ft[i] if valid is None or valid[i] else None for i in range(len(b))], warp


def chunked(sid, sign=1):
    frames, out, f = frames_of(sid, sign), [], 0
    for n in scene_of(sid).chunks:
        out.append(frames[f:f + n])
        f += n
    assert f == len(frames), (sid, f, len(frames))
    return out


def run_oracle(ora, frames):
    """`ora` over the frames -> per-frame records:
      stages   {1, 3: dict(d_iou = the fused IoU distance, d_emb = the gated appearance distance, cost, need = the pairs that are near and
               have a feature on both sides (the kernel's dot products), ids = the rows' track ids, th, matches)}, non-empty problems only
      problems every non-empty assignment problem of the frame as dict(cost, th) (stages 1, 2, 3)
      rows, conf, n_app (after the frame), tracks = {id: dict(state, has_feat, smooth, mean)} of the live tracks after the frame"""
    inner_la = O.linear_assignment
    inner_cost = ora.fused_cost
    cur, trace = {}, []

    def la(cost, thresh):
        res = inner_la(cost, thresh)
        cur["la"].append((np.array(cost, F32, copy=True), F32(thresh), [tuple(m) for m in res[0]]))
        return res

    def cost(tracks, dets):
        d_iou, d_emb, c = inner_cost(tracks, dets)
        plain = O.iou_distance(tracks, dets)
        need = np.zeros(d_iou.shape, bool)
        for i, t in enumerate(tracks):
            for j, d in enumerate(dets):
                need[i, j] = ora.with_reid and not plain[i, j] > ora.proximity and t.smooth_feat is not None and d.curr_feat is not None
        cur["fc"].append(dict(d_iou=d_iou.copy(), d_emb=d_emb.copy(), cost=c.copy(), need=need, plain=np.asarray(plain, F32).reshape(d_iou.shape),
                              ids=[t.track_id for t in tracks]))
        return d_iou, d_emb, c

    O.linear_assignment, ora.fused_cost = la, cost
    try:
        for fr in frames:
            cur = dict(la=[], fc=[])
            out = ora.update_xyxy(*oracle_args(fr))
            (c1, t1, m1), (c2, t2, _), (c3, t3, m3) = cur["la"]
            stages = {}
            for st, fc, th, m in ((1, cur["fc"][0], t1, m1), (3, cur["fc"][1], t3, m3)):
                if fc["cost"].size:
                    stages[st] = dict(fc, th=th, matches=m)
            rows, conf = ora.rows(out)
            live = ora.tracked_stracks + ora.lost_stracks
            trace.append(dict(frame=ora.frame_id, stages=stages, problems=[dict(cost=c, th=t) for c, t in ((c1, t1), (c2, t2), (c3, t3)) if c.size],
                              rows=rows, conf=conf, n_app=ora.n_appearance,
                              tracks={t.track_id: dict(state=t.state, has_feat=t.smooth_feat is not None, mean=t.mean.copy(),
                                                       smooth=None if t.smooth_feat is None else t.smooth_feat.copy()) for t in live}))
    finally:
        O.linear_assignment = inner_la
        del ora.fused_cost
    return trace


def oracle_trace(sid, sign=1):
    """The scene's oracle run, once: (trace, oracle)."""
    if (sid, sign) not in _TRACES:
        ora = scene_of(sid).oracle()
        _TRACES[sid, sign] = (run_oracle(ora, frames_of(sid, sign)), ora)
    return _TRACES[sid, sign]


# ---- 1. the proximity veto on its threshold: d_iou = 0.75 against proximity_thresh 0.75 and its neighbours; e = 4 / 64 far below the gate
def _prox():
    after = [FAR, on(0, 0, feat(1))]
    return [[FAR, on(0, 0, feat(1))], [FAR, rescue(0, 0, feat(1, 4))], after, after]


# ---- 2. the appearance gate on its threshold: e = 16 / 64 against appearance_thresh 0.25 and its neighbours ...
def _app():
    after = [FAR, on(0, 0, feat(2))]
    return [[FAR, on(0, 0, feat(2))], [FAR, rescue(0, 0, feat(2, 16))], after, after]


# ... and on a smoothed feature: the slot has taken feat(3) and feat(3, 8); feat(3, 12) meets it at e near 0.16
def _app_smooth():
    after = [FAR, on(0, 0, feat(3))]
    return [[FAR, on(0, 0, feat(3))], [FAR, on(0, 0, feat(3, 8))], [FAR, rescue(0, 0, feat(3, 12))], after, after]


SMOOTH_EDGE = 3


def smooth_e():
    """The planted cost of the smoothed scenes, from a first pass at the default appearance_thresh."""
    if "e" not in _TRACES:
        ora = O.BoTSORT(proximity_thresh=NEAR)
        rec = run_oracle(ora, frames_of("app_smooth_eq"))[SMOOTH_EDGE - 1]
        e = rec["stages"][1]["d_emb"][rec["stages"][1]["ids"].index(2), 1]
        assert F32(0) < e < F32(0.25)
        _TRACES["e"] = F32(e)
    return _TRACES["e"]


def _app_smooth_kw(side):
    return lambda: dict(proximity_thresh=NEAR, appearance_thresh=float((down, F32, up)[side + 1](smooth_e())))


# ---- 3. e equal to the IoU distance (no score fusion): a 48 x 128 box in the track, IoU 3/4; the twin at e = 15 / 64 is counted
def _tie(m):
    def build():
        after = [FAR, on(0, 0, feat(4))]
        return [[FAR, on(0, 0, feat(4))], [FAR, det(0, 0, 48, H, 0.9, feat(4, m))], after, after]
    return build


# ---- 4. the clamp and the range: e = 0 from an identical first feature, e = 0 through max(0, 1 - dot) with dot > 1 on a smoothed feature,
# e = 1 from the opposite feature; scores of 1 make the fused IoU distance 0, so that a negative e would be counted
def _clamp():
    k, m = CLAMP_K, CLAMP_M
    tracks = [on(0, 0, feat(5)), on(300, 0, feat(k)), on(600, 0, feat(6))]
    second = [on(0, 0, None), on(300, 0, feat(k, m)), on(600, 0, None)]
    edge = [on(0, 0, feat(5), s=1.0), on(300, 0, blend(feat(k), feat(k, m)), s=1.0), on(600, 0, -feat(6), s=1.0)]
    after = [on(0, 0, feat(5, 2)), on(300, 0, feat(k, 2)), on(600, 0, feat(6, 2))]
    return [[FAR] + tracks, [FAR] + second, [FAR] + edge, [FAR] + after, [FAR] + after]


# ---- 5. the has_feat life cycle.  Row y = 0: stage 1, slot with / without a feature against a detection with / without; y = 400: the same
# at stage 3 (tracks born on frame 2); y = 800: two stage-2 matches whose rows carry a feature, a lost track found again, and an
# unconfirmed tracks X (with a feature) and X0 (without) whose slots are freed on frame 3 and handed to Y (born without a feature)
# and Z (born with one) in the same call
def _presence():
    ks = {"p": (10, 11, 12, 13), "u": (14, 15, 16, 17)}
    P = [(300 * i, 0) for i in range(4)]
    U = [(300 * i, 400) for i in range(4)]
    low, low0, R, X, Y, Z, X0 = (0, 800), (300, 800), (600, 800), (900, 800), (1200, 800), (1500, 800), (1800, 800)
    wf = lambda k, m, have: feat(k, m) if have else None
    f1 = [on(*P[i], wf(ks["p"][i], 0, i < 2)) for i in range(4)] + [on(*low, feat(20)), on(*low0, None), on(*R, feat(22)), FAR]
    f2 = ([on(*P[i], wf(ks["p"][i], 6, i in (0, 2))) for i in range(4)] + [on(*low, feat(20, 3)), on(*low0, None)]
          + [on(*X, feat(23)), on(*X0, None)] + [on(*U[i], wf(ks["u"][i], 0, i < 2)) for i in range(4)] + [FAR])
    f3 = ([on(*P[i], wf(ks["p"][i], 9, i in (0, 1, 3))) for i in range(4)] + [on(*low, feat(20, 20), s=0.3), on(*low0, feat(21), s=0.3)]
          + [on(*U[i], wf(ks["u"][i], 5, i in (0, 2))) for i in range(4)] + [on(*Y, None), on(*Z, feat(25)), FAR])
    f4 = ([on(*P[i], feat(ks["p"][i], 2)) for i in range(4)] + [on(*low, feat(20, 1)), on(*low0, feat(21, 1)), on(*R, feat(22, 10))]
          + [on(*U[i], feat(ks["u"][i], 2)) for i in range(4)] + [on(*Y, feat(24)), on(*Z, feat(25, 4)), FAR])
    return [f1, f2, f3, f4, f4]


# ---- 6. the one pair of a problem that needs a dot product, at pair index p of an nr x nc stage-1 problem.  Track r meets detection c
# (of the high band, which is every detection) as a rescue; every other detection sits on a track of its own, where one side lacks a
# feature (even tracks are born without one, the detections over odd tracks come without one), or stands alone and becomes a track
def _pairs(nr, nc, p):
    def build():
        r, c = divmod(p, nc)
        at = lambda i: (300 * (i % 8), 400 * (i // 8))
        born = [on(*at(i), feat(i + 1) if (i % 2 or i == r) else None, cls=i % 3) for i in range(nr)]
        others = [i for i in range(nr) if i != r] + list(range(nr, nc))       # the places of the detections that are not planted
        edge = []
        for j in range(nc):
            if j == c:
                edge.append(rescue(*at(r), feat(r + 1, 4), cls=r % 3))
                continue
            i = others.pop(0)
            edge.append(on(*at(i), feat(i + 1, 2) if (i % 2 == 0 or i >= nr) else None, cls=i % 3))
        after = [on(*at(i), feat(i + 1, 3), cls=i % 3) for i in range(max(nr, nc))]
        return [born, edge, after]
    return build


PAIR_PROBLEMS = ((8, 8), (5, 13), (23, 23))
PAIR_INDEX = {(nr, nc): tuple(sorted({p for p in (0, GROUP - 1, GROUP, SWEEP - 1, SWEEP, nr * nc - 1) if p < nr * nc})) for nr, nc in PAIR_PROBLEMS}
PAIR_CHUNKS = ((2, 1), (3,))


# ---- 7. the camera-motion warp before the costs: an identity rotation and an integer translation (exact) carry a tracked walker A, an
# unconfirmed track B (born on frame 4) and a lost walker C (last met on frame 2) onto the rescues of frame 5, a thousand pixels away
WARP = np.array([[1, 0, 1000], [0, 1, 500]], F32)
WARP_EDGE = 5


def _warp():
    A = lambda f: on(8 * (f - 1), 0, feat(30, f % 3))
    C = lambda f: on(8 * (f - 1), 800, feat(31, f % 2))
    B = on(0, 400, feat(32))
    edge = [rescue(1000 + 24 + 32, 500, feat(30, 3)), rescue(1000 + 24, 900, feat(32, 5)), rescue(1000 + 24 + 8, 1300, feat(31, 4))]
    after = [on(1000 + 32, 500, feat(30)), on(1000, 900, feat(32)), on(1000 + 8, 1300, feat(31))]
    far = on(4000, 1500, feat(63))                               # where the warp takes the bystander
    return [[FAR, A(1), C(1)], [FAR, A(2), C(2)], [FAR, A(3)], ([FAR, A(4), B], None), ([far] + edge, WARP), [far] + after, [far] + after]


# ---- 8. a feature whose normalised row is not finite, on a high-band detection (valid = 1) next to a track that has a smoothed feature;
# an ordinary detection on the track competes for it.  Frame 3: the bad row overlaps the track (IoU 3/5) and must be left over, to be born
# without a feature; frame 5: a bad row sits alone on the track and matches by IoU, the smoothed feature untouched; three frames follow
def bad_feature(kind, k):
    f = feat(k, 2)
    if kind == "zero":
        f[:] = 0
    else:
        f[{"inf": 7, "nan": 9}[kind]] = {"inf": np.inf, "nan": np.nan}[kind]
    return f


NONFINITE_EDGE = (3, 5)


def _nonfinite(kind):
    def build():
        T, N = (0, 0), (16, 0)
        tail = [FAR, on(*T, feat(40, 1)), on(*N, feat(41, 1))]
        return [[FAR, on(*T, feat(40))], [FAR, on(*T, feat(40, 4))], [FAR, on(*N, bad_feature(kind, 40)), on(*T, feat(40, 2))],
                [FAR, on(*T, feat(40, 3)), on(*N, feat(41))], [FAR, on(*T, bad_feature(kind, 40)), on(*N, feat(41, 2))], tail, tail, tail]
    return build


def _edge_kw(name, x, side):
    return {"proximity_thresh": NEAR, name: float((down, F32, up)[side + 1](F32(x)))}


SIDES = (("_below", -1), ("_eq", 0), ("_above", 1))
SCENES = tuple(
    [Scene("prox" + sfx, _prox, ch, (2,), _edge_kw("proximity_thresh", 0.75, side)) for (sfx, side), ch in zip(SIDES, ((3, 1), (4,), (2, 1, 1)))]
    + [Scene("app" + sfx, _app, ch, (2,), _edge_kw("appearance_thresh", 0.25, side)) for (sfx, side), ch in zip(SIDES, ((4,), (2, 1, 1), (3, 1)))]
    + [Scene("app_smooth" + sfx, _app_smooth, ch, (SMOOTH_EDGE,), _app_smooth_kw(side)) for (sfx, side), ch in zip(SIDES, ((4, 1), (1, 4), (5,)))]
    + [Scene("app_ties_iou", _tie(16), (3, 1), (2,), dict(fuse_score=False, appearance_thresh=0.5)),
       Scene("app_under_iou", _tie(15), (4,), (2,), dict(fuse_score=False, appearance_thresh=0.5)),
       Scene("clamp_and_range", _clamp, (1, 4), (3,), dict(appearance_thresh=1.0)),
       Scene("feature_presence", _presence, (4, 1), (2, 3, 4))]
    + [Scene(f"pair_groups_{nr}x{nc}_{p}", _pairs(nr, nc, p), PAIR_CHUNKS[i % 2], (2,), dict(proximity_thresh=NEAR))
       for nr, nc in PAIR_PROBLEMS for i, p in enumerate(PAIR_INDEX[nr, nc])]
    + [Scene("warp_first", _warp, (3, 4), (WARP_EDGE,), dict(proximity_thresh=NEAR))]
    + [Scene("nonfinite_" + kind, _nonfinite(kind), ch, NONFINITE_EDGE, dict(proximity_thresh=NEAR))
       for kind, ch in (("zero", (1, 7)), ("inf", (3, 4, 1)), ("nan", (1, 5, 2)))])


def groups():
    """The scenes by parameter set: a bank has one.  A scene alone with its parameters runs as two streams, under different plans."""
    out = {}
    for sc in SCENES:
        out.setdefault(repr(sorted(sc.params().items())), []).append(sc.id)
    return [g * 2 if len(g) == 1 else g for g in out.values()]
