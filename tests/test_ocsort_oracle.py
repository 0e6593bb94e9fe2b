"""The OC-SORT oracle (tests/ocsort_oracle.py) on hand-built scenes: each test pins one rule of OCSort.update()."""
import itertools

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import ocsort_oracle as O
from ocsort_oracle import FROZEN, OBSERVED, OCSort

F32 = np.float32


def box(x, y, w=40.0, h=100.0):
    return np.array([x, y, x + w, y + h], F32)


def step(trk, boxes, scores, cls=None):
    b = np.array(boxes, F32).reshape(-1, 4)
    return trk.update_xyxy(b, np.array(scores, F32), np.zeros(len(b), np.int32) if cls is None else cls)


def ids(out):
    return [t.id for t in out]


def test_output_from_frame_one_then_needs_min_hits():
    trk = OCSort()
    for f in range(3):                                            # frame_count <= min_hits: output at once, new tracks too
        assert ids(step(trk, [box(10 + f, 10), box(300, 10)], [0.9, 0.8])) == [2, 1]    # upstream's order: the list reversed
    for _ in range(2):
        step(trk, [], [])
    # frame 6: a new track (id 3) is not output; the old ones lost their streak (missed two frames) and need min_hits again
    assert ids(step(trk, [box(12, 10), box(300, 10), box(600, 10)], [0.9, 0.8, 0.9])) == []
    assert ids(step(trk, [box(12, 10), box(300, 10), box(600, 10)], [0.9, 0.8, 0.9])) == []
    out = step(trk, [box(12, 10), box(300, 10), box(600, 10)], [0.9, 0.8, 0.9])
    assert ids(out) == [2, 1] and [t.hit_streak for t in out] == [3, 3]       # the new one was born with hit_streak 0: 2 so far
    out = step(trk, [box(12, 10), box(300, 10), box(600, 10)], [0.9, 0.8, 0.9])
    assert ids(out) == [3, 2, 1] and [t.hit_streak for t in out] == [3, 4, 4]


def test_new_track_hit_streak_counts_updates_only():
    trk = OCSort(min_hits=2)
    for _ in range(3):
        step(trk, [], [])
    assert ids(step(trk, [box(10, 10)], [0.9])) == []             # born: hit_streak 0
    assert ids(step(trk, [box(10, 10)], [0.9])) == []             # first update: 1
    assert ids(step(trk, [box(10, 10)], [0.9])) == [1]            # second update: 2 = min_hits


def test_low_score_starts_nothing_and_use_byte_keeps_track_alive():
    trk = OCSort()
    assert step(trk, [box(10, 10)], [0.5]) == [] and trk.trackers == []
    assert step(trk, [box(10, 10)], [0.6]) == [] and trk.trackers == []       # s > det_thresh, strictly
    for use_byte in (False, True):
        trk = OCSort(use_byte=use_byte)
        step(trk, [box(10, 10)], [0.9])
        step(trk, [box(10, 10)], [0.9])
        out = step(trk, [box(11, 10)], [0.3])
        t = trk.trackers[0]
        if use_byte:
            assert ids(out) == [1] and t.time_since_update == 0 and t.score == F32(0.3) and trk.stats["n_byte"] == 1
        else:
            assert out == [] and t.time_since_update == 1 and t.kstate == FROZEN
    trk = OCSort(use_byte=True)                                   # the band is open at 0.1
    step(trk, [box(10, 10)], [0.9])
    assert step(trk, [box(10, 10)], [0.1]) == []


def _ocm_scene(inertia):
    """A track moving right, then two detections left and right of its prediction with the same IoU."""
    trk = OCSort(inertia=inertia, min_hits=1)
    for f in range(4):
        step(trk, [box(100 + 8 * f, 100)], [0.9])
    t = trk.trackers[0]
    x = t.x.copy()
    x[:3] = x[:3] + x[4:7]
    px = float(O.x_to_bbox(x)[0])                                 # the predicted box's x1 at the next frame
    w = float(O.x_to_bbox(x)[2] - O.x_to_bbox(x)[0])
    py = float(O.x_to_bbox(x)[1])
    h = float(O.x_to_bbox(x)[3] - O.x_to_bbox(x)[1])
    d = 16.0                                                      # exactly representable offsets: the two IoUs are equal
    left = np.array([px - d, py, px - d + w, py + h], F32)
    right = np.array([px + d, py, px + d + w, py + h], F32)
    return trk, left, right


def test_ocm_direction_breaks_an_iou_tie():
    trk, left, right = _ocm_scene(0.2)
    pred = O.x_to_bbox(O.kf7_predict(trk.trackers[0].x, trk.trackers[0].P)[0])
    iou = O.iou_matrix([left, right], [pred])[:, 0]
    assert abs(float(iou[0]) - float(iou[1])) < 2e-6 and iou[0] > 0.3
    step(trk, [left, right], [0.9, 0.9])
    assert np.array_equal(trk.trackers[0].last_observation, right)       # the direction of motion wins
    assert trk.stats["n_lsap"] >= 1
    # reversed detection order: still the one on the right
    trk, left, right = _ocm_scene(0.2)
    step(trk, [right, left], [0.9, 0.9])
    assert np.array_equal(trk.trackers[0].last_observation, right)


def test_without_inertia_the_tie_follows_scipy():
    trk, left, right = _ocm_scene(0.0)
    pred = O.x_to_bbox(O.kf7_predict(trk.trackers[0].x, trk.trackers[0].P)[0])
    iou = O.iou_matrix([left, right], [pred])
    r, c = linear_sum_assignment(-iou.astype(np.float64))
    want = [left, right][int(r[0])]
    step(trk, [left, right], [0.9, 0.9])
    assert np.array_equal(trk.trackers[0].last_observation, want)


def test_ocr_rematches_by_last_observation():
    trk = OCSort(min_hits=1)
    for f in range(10):                                           # steady motion to the right, 12 px a frame
        step(trk, [box(100 + 12 * f, 100)], [0.9])
    assert len(trk.trackers) == 1
    t = trk.trackers[0]
    last = t.last_observation.copy()
    step(trk, [], [])
    step(trk, [], [])                                             # the prediction runs on: 3 frames ahead at the next update
    pred = O.x_to_bbox(O.kf7_predict(t.x, t.P)[0])
    assert O.iou_matrix([last], [pred])[0, 0] < 0.3               # it has left the target, which stopped where it was last seen
    n0 = trk.stats["n_ocr"]
    out = step(trk, [last], [0.9])
    assert trk.stats["n_ocr"] == n0 + 1 and ids(out) == [1] and len(trk.trackers) == 1
    assert t.time_since_update == 0 and trk.stats["n_oru"] == 1 and trk.stats["max_gap"] == 3


@pytest.mark.parametrize("g", [1, 2, 5, 12])
def test_oru_replays_the_virtual_trajectory(g):
    def run(oru):
        trk = OCSort(min_hits=1, oru=oru)
        for f in range(4):
            step(trk, [box(100 + 2 * f, 100 + f)], [0.9])
        for _ in range(g - 1):
            step(trk, [], [])
        return trk
    trk = run(True)
    t = trk.trackers[0]
    assert (t.kstate == FROZEN) == (g > 1)
    if g == 1:
        return
    fx, fP = t.saved[0].copy(), t.saved[1].copy()
    last = t.last_observation.copy()
    new = box(100 + 2 * (3 + g) + 5, 100 + (3 + g) - 3, 44, 96)
    step(trk, [new], [0.9])
    assert t.kstate == OBSERVED and trk.stats["n_oru"] == 1 and trk.stats["max_gap"] == g
    # by hand: g interpolated boxes into a copy of the frozen filter, then the ordinary update
    z1, z2 = O.bbox_to_z(last), O.bbox_to_z(new)
    w1, h1, w2, h2 = np.sqrt(z1[2] * z1[3]), np.sqrt(z1[2] / z1[3]), np.sqrt(z2[2] * z2[3]), np.sqrt(z2[2] / z2[3])
    x, P = fx, fP
    for i in range(g):
        k = F32(i + 1)
        bx = z1[0] + k * ((z2[0] - z1[0]) / F32(g))
        by = z1[1] + k * ((z2[1] - z1[1]) / F32(g))
        bw = w1 + k * ((w2 - w1) / F32(g))
        bh = h1 + k * ((h2 - h1) / F32(g))
        x, P = O.kf7_update(x, P, np.array([bx, by, bw * bh, bw / bh], F32))
        if i != g - 1:
            x, P = O.kf7_predict(x, P)
    x, P = O.kf7_update(x, P, z2)
    assert np.array_equal(t.x, x) and np.array_equal(t.P, P)
    trk2 = run(False)
    step(trk2, [new], [0.9])
    assert not np.allclose(trk2.trackers[0].x, t.x, rtol=1e-3)    # without ORU the filter is somewhere else


def test_removed_exactly_after_max_age():
    trk = OCSort(max_age=5)
    step(trk, [box(10, 10)], [0.9])
    step(trk, [box(10, 10)], [0.9])
    for k in range(5):
        step(trk, [], [])
        assert len(trk.trackers) == 1 and trk.trackers[0].time_since_update == k + 1
    step(trk, [], [])
    assert trk.trackers == []                                     # time_since_update 6 > max_age
    trk = OCSort(max_age=5)
    step(trk, [box(10, 10)], [0.9])
    step(trk, [box(10, 10)], [0.9])
    for k in range(5):
        step(trk, [], [])
    step(trk, [box(10, 10)], [0.9])                               # refound with a gap of max_age + 1, the longest there is
    assert ids(trk.trackers) == [1] and trk.stats["max_gap"] == 6


def test_non_finite_prediction_drops_the_track():
    trk = OCSort()
    step(trk, [np.array([10, 10, 10, 90], F32), box(300, 10)], [0.9, 0.9])     # a zero-width box: s = 0, h = 0 / 0 at the predict
    assert ids(trk.trackers) == [1, 2]
    out = step(trk, [box(300, 10)], [0.9])
    assert ids(trk.trackers) == [2] and ids(out) == [2]


def test_read_off_and_lsap_agree_where_nothing_outweighs_a_pair():
    """Matrices where the read-off applies and every other entry is zero (boxes that do not overlap): the LSAP has one optimum
    in the pairs above the threshold, so both give the same pairs."""
    rng = np.random.default_rng(0)
    thr = F32(0.3)
    for _ in range(200):
        n, t = rng.integers(1, 9, 2)
        iou = np.zeros((n, t), F32)
        k = rng.integers(1, min(n, t) + 1)
        for r, c in zip(rng.permutation(n)[:k], rng.permutation(t)[:k]):
            iou[r, c] = F32(rng.uniform(0.31, 1.0))
        pairs = O.read_off(iou, thr)
        assert pairs is not None
        got = [(r, c) for r, c in O.linear_assignment(-iou) if not iou[r, c] < thr]
        assert sorted(got) == sorted(pairs)


def test_read_off_and_lsap_can_differ():
    """Change 10 of the oracle: the shortcut is upstream's behaviour, not an identity."""
    iou = np.array([[0.35, 0.29], [0.29, 0.0]], F32)
    assert O.read_off(iou, F32(0.3)) == [(0, 0)]
    assert [(r, c) for r, c in O.linear_assignment(-iou) if not iou[r, c] < F32(0.3)] == []


def test_read_off_needs_one_entry_per_row_and_column():
    thr = F32(0.3)
    assert O.read_off(np.array([[0.5, 0.4]], F32), thr) is None
    assert O.read_off(np.array([[0.5], [0.4]], F32), thr) is None
    assert O.read_off(np.zeros((2, 2), F32), thr) is None         # nothing above the threshold: upstream goes to the LSAP
    assert O.read_off(np.array([[0.3, 0.0], [0.0, 0.31]], F32), thr) == [(1, 1)]


def test_lsap_equals_brute_force_on_small_rectangles():
    rng = np.random.default_rng(1)
    for _ in range(150):
        n, t = (int(v) for v in rng.integers(1, 6, 2))
        cost = rng.uniform(-1.2, 0.0, (n, t)).astype(F32)
        pairs = O.linear_assignment(cost)
        assert len(pairs) == min(n, t)
        got = sum(float(cost[r, c]) for r, c in pairs)
        if n <= t:
            best = min(sum(float(cost[i, p[i]]) for i in range(n)) for p in itertools.permutations(range(t), n))
        else:
            best = min(sum(float(cost[p[j], j]) for j in range(t)) for p in itertools.permutations(range(n), t))
        assert abs(got - best) < 1e-9


def test_asin32_error_monotonic_odd():
    g = np.linspace(-1.0, 1.0, 2 ** 21 + 1).astype(F32)
    assert g[0] == -1 and g[-1] == 1
    a = O.asin32(g)
    assert a.dtype == F32
    err = float(np.abs(a.astype(np.float64) - np.arcsin(g.astype(np.float64))).max())
    print("asin32 max error", err)
    assert err <= 2 * 1.64e-7                                     # measured 1.64e-7 (oracle docstring, change 5)
    assert (np.diff(a) >= 0).all()
    assert np.array_equal(a, -a[::-1])
    assert a[-1] == O.PIO2 and a[len(g) // 2] == 0


def test_ocm_term_matches_upstream_formula():
    rng = np.random.default_rng(2)
    dets = np.array([box(*rng.uniform(0, 500, 2)) for _ in range(6)])
    prev = np.array([box(*rng.uniform(0, 500, 2)) for _ in range(4)])
    vel = rng.normal(size=(4, 2))
    vel = (vel / np.linalg.norm(vel, axis=1, keepdims=True)).astype(F32)
    sc = rng.uniform(0.6, 1, 6).astype(F32)
    valid = np.array([1, 1, 0, 1], bool)
    got = O.ocm_term(dets, sc, prev, valid, vel, 0.2)
    cd, cp = (dets[:, :2] + dets[:, 2:]) / 2, (prev[:, :2] + prev[:, 2:]) / 2
    d = cd[:, None, :].astype(np.float64) - cp[None, :, :]
    n = np.linalg.norm(d, axis=2) + 1e-6
    c = np.clip(vel[None, :, 1] * d[..., 0] / n + vel[None, :, 0] * d[..., 1] / n, -1, 1)
    want = 0.2 * valid[None, :] * (np.pi / 2 - np.abs(np.arccos(c))) / np.pi * sc[:, None]
    assert got.shape == (6, 4) and np.abs(got - want).max() < 1e-6 and (got[:, 2] == 0).all()


def test_filter_matches_textbook_fp64():
    rng = np.random.default_rng(3)
    x = np.array([100, 200, 4000, 0.4, 1, -2, 10], F32)
    P = np.diag(O.P0_DIAG).astype(F32)
    F = np.eye(7)
    F[0, 4] = F[1, 5] = F[2, 6] = 1
    H = np.eye(4, 7)
    x64, P64 = x.astype(np.float64), P.astype(np.float64)
    for k in range(20):
        x, P = O.kf7_predict(x, P)
        x64, P64 = F @ x64, F @ P64 @ F.T + np.diag(O.Q_DIAG.astype(np.float64))
        if k % 3 != 2:
            z = (x[:4] + rng.normal(size=4).astype(F32) * np.array([2, 2, 50, 0.01], F32)).astype(F32)
            x, P = O.kf7_update(x, P, z)
            S = H @ P64 @ H.T + np.diag(O.R_DIAG.astype(np.float64))
            K = P64 @ H.T @ np.linalg.inv(S)
            x64 = x64 + K @ (z - H @ x64)
            A = np.eye(7) - K @ H
            P64 = A @ P64 @ A.T + K @ np.diag(O.R_DIAG.astype(np.float64)) @ K.T
    assert np.allclose(x, x64, rtol=1e-4, atol=1e-2) and np.allclose(P, P64, rtol=1e-3, atol=1e-2)


def test_velocity_uses_the_observation_delta_t_back():
    trk = OCSort(delta_t=3)
    xs = [100, 110, 120, 130, 100]
    for x in xs[:4]:
        step(trk, [box(x, 100)], [0.9])
    t = trk.trackers[0]
    # observations at ages 1, 2, 3 (the first box is the filter's seed, not an observation): at age 4 the one delta_t back is x = 110
    step(trk, [box(118, 130)], [0.9])
    want = O.speed_direction(box(110, 100), box(118, 130))
    assert np.array_equal(t.velocity, want) and t.has_vel and sorted(t.observations) == [2, 3, 4]


def test_rows_format_and_class_follows_last_detection():
    trk = OCSort()
    out = step(trk, [np.array([10.5, 11.5, 50.4, 111.6], F32)], [0.9], np.array([2], np.int32))
    rows, conf = OCSort.rows(out)
    assert rows.dtype == np.int32 and rows.shape == (1, 6) and conf.dtype == F32
    b = O.x_to_bbox(trk.trackers[0].x)                            # no observation yet: the filter's box
    assert rows[0].tolist() == [int(np.rint(v)) for v in b] + [1, 2]
    out = step(trk, [np.array([10.5, 11.5, 50.5, 112.5], F32)], [0.8], np.array([1], np.int32))
    rows, conf = OCSort.rows(out)
    assert rows[0].tolist() == [10, 12, 50, 112, 1, 1] and conf[0] == F32(0.8)      # the observation itself, half to even
    assert OCSort.rows([])[0].shape == (0, 6)
    e = trk.export()
    assert e["mean"].shape == (1, 7) and e["cov"].shape == (1, 7, 7) and e["track_id"].tolist() == [1] and e["hits"].tolist() == [1]
    assert OCSort(first_track_id=7).next_id == 7


def test_scene_reaches_every_path():
    """The scene tests/test_gpu_ocsort.py holds the device to: the oracle alone must reach ORU (a gap above delta_t), OCR, the
    read-off and the LSAP, and with use_byte the BYTE stage."""
    from conftest import pkg
    syn = pkg("synthetic")
    n, frames, seed = 30, 300, 4
    rng = np.random.default_rng(seed)
    gaps = [(int(t), int(a), int(a + rng.integers(3, 40))) for t, a in zip(rng.integers(0, n, n // 2), rng.integers(5, frames - 50, n // 2))]
    births = {int(t): int(f) for t, f in zip(rng.choice(n, n // 5, replace=False), rng.integers(1, frames // 2, n // 5))}
    sc = syn.Scene(seed=seed, n_targets=n, gaps=gaps, births=births, conf_range=(0.05, 0.95), jitter=1.5, shuffle=True)
    a, b = OCSort(), OCSort(use_byte=True)
    for f in range(frames):
        bx, c, k, _ = sc.detections(f)
        a.update_xyxy(bx, c, k)
        b.update_xyxy(bx, c, k)
    s = a.stats
    assert s["n_oru"] > 0 and s["max_gap"] > 3 and s["n_ocr"] > 0 and s["n_fast"] > 0 and s["n_lsap"] > 0, s
    assert b.stats["n_byte"] > 0 and b.stats["n_oru"] > 0 and b.stats["max_gap"] > 3, b.stats
