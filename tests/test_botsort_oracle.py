"""The BoT-SORT specification (tests/botsort_oracle.py) against hand-worked answers and fp64 evaluations of the same formulas, and the
scene that shows what the appearance term buys: a crossing that the IoU-only tracker swaps and the ReID tracker does not.  No GPU."""
import numpy as np

import botsort_oracle as bo
from botsort_oracle import LOST, TRACKED, BoTSORT, STrack
from conftest import pkg

F32 = np.float32


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F32)


def track(tlwh, feat=None, score=0.9):
    t = STrack(tlwh, score, 0, feat)
    t.activate(1, 1)
    return t


# ---------------------------------------------------------------------------------------------------- ordered sums
def test_wave_sum_and_normalise_against_fp64():
    rng = np.random.default_rng(0)
    for d in (4, 8, 256, 512, 772):
        a, b = unit(rng.standard_normal(d)), unit(rng.standard_normal(d))
        got = bo.wave_sum(a * b)
        assert got.dtype == F32
        # gamma_n * sum |a_i b_i| <= 512 * 2^-24 for unit vectors (plus the rounding of the products)
        assert abs(float(got) - float(a.astype(np.float64) @ b.astype(np.float64))) < 1e-4 / 2
    f = rng.standard_normal((3, 512)).astype(F32)
    n = bo.normalise(f)
    assert np.allclose(np.linalg.norm(n.astype(np.float64), axis=1), 1, atol=1e-6)
    assert np.array_equal(n[1], bo.normalise(f[1]))              # batched == row by row: the order does not depend on the shape


# ---------------------------------------------------------------------------------------------------- the fused cost
def test_pair_rescued_by_appearance():
    # IoU 0.25 (not far at proximity 0.8), score 0.7: fused IoU distance 1 - 0.25 * 0.7 = 0.825 > match_thresh; cosine 0.8 -> d_emb = 0.1
    o = BoTSORT(proximity_thresh=0.8)
    t = track([0, 0, 100, 100], [1, 0, 0, 0])
    d = STrack([60, 0, 100, 100], 0.7, 0, [0.8, 0.6, 0, 0])
    d_iou, d_emb, cost = o.fused_cost([t], [d])
    assert np.isclose(d_iou[0, 0], 0.825, atol=1e-6) and d_iou[0, 0] > o.match_thresh
    assert np.isclose(d_emb[0, 0], 0.1, atol=1e-6) and cost[0, 0] == d_emb[0, 0]
    matches, _, _ = bo.linear_assignment(cost, o.match_thresh)
    assert matches == [(0, 0)]
    # the same pair without the appearance term is not matched
    o0 = BoTSORT(proximity_thresh=0.8, with_reid=False)
    assert bo.linear_assignment(o0.fused_cost([t], [d])[2], o0.match_thresh)[0] == []


def test_good_appearance_vetoed_by_far_and_missing_feature():
    o = BoTSORT()                                                 # proximity 0.5: IoU distance 0.75 is far
    t = track([0, 0, 100, 100], [1, 0, 0, 0])
    same = STrack([60, 0, 100, 100], 0.7, 0, [1, 0, 0, 0])
    d_iou, d_emb, cost = o.fused_cost([t], [same])
    assert d_emb[0, 0] == 1 and cost[0, 0] == d_iou[0, 0]
    # near, but the detection has no feature / the track has none
    near = STrack([10, 0, 100, 100], 0.9, 0, None)
    d_iou, d_emb, cost = o.fused_cost([t], [near])
    assert d_emb[0, 0] == 1 and cost[0, 0] == d_iou[0, 0]
    t0 = track([0, 0, 100, 100], None)
    assert o.fused_cost([t0], [STrack([10, 0, 100, 100], 0.9, 0, [1, 0, 0, 0])])[1][0, 0] == 1
    # near with a feature, but a different person: cosine 0 -> d_emb 0.5 > appearance_thresh -> 1
    other = STrack([10, 0, 100, 100], 0.9, 0, [0, 1, 0, 0])
    assert o.fused_cost([t], [other])[1][0, 0] == 1
    # near, same person: the far veto is taken BEFORE score fusion (raw IoU distance 18 / 110 < 0.5)
    good = STrack([10, 0, 100, 100], 0.61, 0, [1, 0, 0, 0])
    d_iou, d_emb, cost = o.fused_cost([t], [good])
    assert d_emb[0, 0] == 0 and cost[0, 0] == 0 and d_iou[0, 0] > 0.45


def test_low_band_feature_is_never_read():
    o = BoTSORT()
    bad = np.full((1, 8), np.nan, F32)
    o.update(np.array([[0, 0, 50, 100]], F32), [0.9], [0], [unit(np.arange(8) + 1.0)])
    out = o.update(np.array([[1, 0, 50, 100]], F32), [0.4], [0], bad)        # second association: IoU only
    assert len(out) == 1 and np.isfinite(out[0].smooth_feat).all() and out[0].frame_id == 2


def test_ema_after_two_updates():
    rng = np.random.default_rng(1)
    f = [rng.standard_normal(512).astype(F32) for _ in range(3)]
    t = STrack([0, 0, 10, 10], 0.9, 0, f[0])
    for x in f[1:]:
        t.update_features(bo.normalise(x))
    s = f[0].astype(np.float64) / np.linalg.norm(f[0])
    for x in f[1:]:
        s = 0.9 * s + 0.1 * x.astype(np.float64) / np.linalg.norm(x)
        s /= np.linalg.norm(s)
    assert np.abs(t.smooth_feat - s).max() < 1e-6 and t.smooth_feat.dtype == F32


# ---------------------------------------------------------------------------------------------------- the xywh filter
def _f64_filter():
    Fm = np.eye(8)
    Fm[:4, 4:] = np.eye(4)
    H = np.eye(4, 8)
    sides = lambda m: np.array([m[2], m[3], m[2], m[3]])
    wp, wv = float(bo.W_POS), float(bo.W_VEL)

    def initiate(z):
        std = np.r_[2 * wp * sides(z), 10 * wv * sides(z)]
        return np.r_[z, np.zeros(4)], np.diag(std ** 2)

    def predict(m, P):
        std = np.r_[wp * sides(m), wv * sides(m)]
        return Fm @ m, Fm @ P @ Fm.T + np.diag(std ** 2)

    def update(m, P, z):
        S = H @ P @ H.T + np.diag((wp * sides(m)) ** 2)
        K = P @ H.T @ np.linalg.inv(S)
        return m + K @ (z - H @ m), P - K @ S @ K.T
    return initiate, predict, update


def test_filter_against_fp64():
    initiate, predict, update = _f64_filter()
    rng = np.random.default_rng(2)
    z = np.array([320.5, 240.25, 61.0, 153.0])
    m32, P32 = bo.kf_initiate(z.astype(F32))
    m64, P64 = initiate(z)
    assert np.allclose(m32, m64) and np.allclose(P32, P64, rtol=1e-6)
    assert np.isclose(P32[0, 0], (0.1 * 61) ** 2, rtol=1e-6) and np.isclose(P32[5, 5], (0.0625 * 153) ** 2, rtol=1e-6)
    for step in range(40):
        m32, P32 = bo.kf_predict(m32, P32)
        m64, P64 = predict(m64, P64)
        assert m32.dtype == F32 and P32.dtype == F32
        if step % 5 != 4:                                         # a miss every fifth frame
            z = z + np.array([2.0, -1.0, 0.1, 0.2]) + rng.uniform(-1, 1, 4)
            m32, P32 = bo.kf_update(m32, P32, z.astype(F32))
            m64, P64 = update(m64, P64, z.astype(F32).astype(np.float64))
        assert np.allclose(m32, m64, rtol=1e-4, atol=1e-2), step
        assert np.allclose(P32, P64, rtol=1e-3, atol=1e-3), step
    assert abs(m32[4] - 2.0) < 0.5 and abs(m32[5] + 1.0) < 0.5     # the velocity was learnt


def test_warp_against_fp64_kron():
    rng = np.random.default_rng(3)
    m, P = bo.kf_initiate(np.array([100, 50, 40, 90], F32))
    for _ in range(3):
        m, P = bo.kf_predict(m, P)
        m, P = bo.kf_update(m, P, (m[:4] + F32(1)).astype(F32))
    th = 0.02
    w = np.array([[np.cos(th), -np.sin(th), 3.5], [np.sin(th), np.cos(th), -2.25]])
    m2, P2 = bo.kf_warp(m, P, w)
    A = np.kron(np.eye(4), w[:, :2].astype(F32).astype(np.float64))
    want_m = A @ m.astype(np.float64)
    want_m[:2] += w[:, 2]
    assert np.allclose(m2, want_m, rtol=1e-6, atol=1e-5)
    assert np.allclose(P2, A @ P.astype(np.float64) @ A.T, rtol=1e-5, atol=1e-5)
    mi, Pi = bo.kf_warp(m, P, [[1, 0, 0], [0, 1, 0]])
    assert np.array_equal(mi, m) and np.array_equal(Pi, P)        # the identity changes nothing


# ---------------------------------------------------------------------------------------------------- life cycle
BOX = np.array([[100, 100, 50, 120]], F32)


def test_lost_track_reactivated_keeps_its_id_and_takes_the_feature():
    o = BoTSORT()
    f = unit(np.arange(16) + 1.0)
    o.update(BOX, [0.9], [0], [f])
    assert [t.track_id for t in o.tracked_stracks] == [1] and o.tracked_stracks[0].is_activated
    for _ in range(5):
        assert o.update(np.zeros((0, 4)), [], []) == []
    assert [t.state for t in o.lost_stracks] == [LOST]
    out = o.update(BOX, [0.9], [2], [unit(np.arange(16)[::-1] + 1.0)])
    assert [(t.track_id, t.state, t.cls, t.frame_id) for t in out] == [(1, TRACKED, 2, 7)] and o.lost_stracks == []
    assert not np.array_equal(out[0].smooth_feat, f) and np.isclose(np.linalg.norm(out[0].smooth_feat), 1, atol=1e-6)


def test_lost_track_times_out():
    o = BoTSORT(track_buffer=3)
    o.update(BOX, [0.9], [0])
    for k in range(4):                                            # lost at frame 2 (end_frame 1): removed when frame - 1 > 3
        o.update(np.zeros((0, 4)), [], [])
        assert len(o.lost_stracks) == (1 if k < 3 else 0), k
    out = o.update(BOX, [0.9], [0])
    assert [t.track_id for t in out] == [2]


def test_unconfirmed_track_is_shown_then_removed():
    o = BoTSORT()
    o.update(np.zeros((0, 4)), [], [])
    out = o.update(BOX, [0.9], [0])                               # born after frame 1: not activated, but output (change 9)
    assert [(t.track_id, t.is_activated) for t in out] == [(1, False)]
    assert o.update(np.zeros((0, 4)), [], []) == [] and o.lost_stracks == [] and o.tracked_stracks == []
    # a detection below new_track_thresh in the high band starts nothing
    assert o.update(BOX, [0.65], [0]) == []


# ---------------------------------------------------------------------------------------------------- what the appearance term buys
# Two persons of the same size walk towards each other, turn round while nobody detects them (frames GAP) and walk back.  The filters
# coast on: after the gap each prediction lies nearer to the OTHER person's detection, and all four boxes overlap with IoU > 0.5, so
# the appearance term is allowed to speak.  Only the seed and these parameters are committed.
CROSSING = dict(seed=0, frames=60, turn=20, gap=(14, 26), x0=(370.0, 420.0), speed=1.0, y=200.0, w=60.0, h=150.0, jitter=0.3)


def crossing_scene(seed, frames, turn, gap, x0, speed, y, w, h, jitter):
    """Per frame: (boxes_xyxy [n,4], scores [n], cls [n], identities [n]) and the ground truth (boxes, identities) of every frame."""
    rng = np.random.default_rng(seed)
    dets, gt = [], []
    for f in range(frames):
        d = speed * (f if f <= turn else 2 * turn - f)
        xs = np.array([x0[0] + d, x0[1] - d])
        b = np.stack([xs, np.full(2, y), xs + w, np.full(2, y) + h], 1)
        gt.append((b.astype(F32), np.arange(2)))
        b = (b + rng.uniform(-jitter, jitter, b.shape)).astype(F32)
        s = rng.uniform(0.75, 0.95, 2).astype(F32)
        keep = np.arange(2) if not gap[0] <= f <= gap[1] else np.zeros(0, np.int64)
        dets.append((b[keep], s[keep], np.zeros(len(keep), np.int32), keep))
    return dets, gt


def run_crossing(make, with_feat=True):
    """Feeds the scene to make()'s tracker (anything with update_xyxy returning tracks, or rows); -> per-frame output tuples."""
    syn = pkg("synthetic")
    dets, gt = crossing_scene(**CROSSING)
    trk = make()
    outs = []
    for f, (b, s, c, ident) in enumerate(dets):
        feats = syn.identity_features(ident, f, dim=512, seed=5) if with_feat else None
        rows, _ = BoTSORT.rows(trk.update_xyxy(b, s, c, feats))
        outs.append([tuple(r) for r in rows.tolist()])
    return outs, gt, trk


def ids_by_position(out):
    return [r[4] for r in sorted(out, key=lambda r: r[0])]


def test_crossing_swaps_without_reid_and_not_with_it():
    mm = pkg("mot_metrics")
    outs0, gt, _ = run_crossing(lambda: BoTSORT(with_reid=False))
    outs1, _, trk1 = run_crossing(lambda: BoTSORT(with_reid=True))
    before, after = CROSSING["gap"][0] - 1, CROSSING["frames"] - 1
    assert ids_by_position(outs0[before]) == [1, 2] and ids_by_position(outs1[before]) == [1, 2]
    assert ids_by_position(outs0[after]) == [2, 1]                # motion alone: the identities are exchanged
    assert ids_by_position(outs1[after]) == [1, 2]                # with appearance: kept
    assert mm.evaluate(gt, outs0)["idsw"] == 2
    m1 = mm.evaluate(gt, outs1)
    assert m1["idsw"] == 0 and m1["fp"] == 0
    assert trk1.n_appearance > 0                                  # the appearance distance decided pairs
    assert trk1.next_id == 3                                      # and nobody was re-born under a new id
