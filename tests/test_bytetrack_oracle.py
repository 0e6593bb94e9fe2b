"""The ByteTrack oracle (tests/bytetrack_oracle.py) on hand-built scenes: each test pins one rule of BYTETracker.update()."""
import itertools

import numpy as np
import pytest

from bytetrack_oracle import BYTETracker, LOST, TRACKED, extended_matrix, linear_assignment


def box(x, y, w=40.0, h=100.0):
    return np.array([x, y, x + w, y + h], np.float32)


def step(trk, boxes, scores):
    b = np.array(boxes, np.float32).reshape(-1, 4)
    return trk.update_xyxy(b, np.array(scores, np.float32), np.zeros(len(b), np.int32))


def ids(out):
    return [t.track_id for t in out]


def test_first_frame_tracks_are_output_at_once():
    trk = BYTETracker()
    out = step(trk, [box(10, 10), box(300, 10)], [0.9, 0.8])
    assert ids(out) == [1, 2]
    assert all(t.is_activated for t in out)


def test_low_score_keeps_track_through_second_stage():
    trk = BYTETracker()
    step(trk, [box(10, 10)], [0.9])
    for f in range(3):
        out = step(trk, [box(11 + f, 10)], [0.3])        # second band (0.1, 0.5)
        assert ids(out) == [1]
        assert out[0].score == np.float32(0.3)
    # with low_thresh = track_thresh the second band is empty: the track goes Lost
    trk = BYTETracker(low_thresh=0.5)
    step(trk, [box(10, 10)], [0.9])
    assert step(trk, [box(11, 10)], [0.3]) == []
    assert [t.state for t in trk.lost_stracks] == [LOST]


def test_lost_track_refound_within_buffer_and_removed_after():
    trk = BYTETracker()
    step(trk, [box(100, 100)], [0.9])
    step(trk, [box(100, 100)], [0.9])
    for _ in range(30):
        assert step(trk, [], []) == []
    out = step(trk, [box(100, 100)], [0.9])                # lost 30 frames: refound, same id
    assert ids(out) == [1]
    trk = BYTETracker()
    step(trk, [box(100, 100)], [0.9])
    step(trk, [box(100, 100)], [0.9])
    for _ in range(31):
        step(trk, [], [])
    assert trk.lost_stracks == [] and trk.tracked_stracks == []
    out = step(trk, [box(100, 100)], [0.9])                # a new, unconfirmed track
    assert out == [] and [t.track_id for t in trk.tracked_stracks] == [2]


def test_late_detection_needs_a_second_match_and_unmatched_unconfirmed_is_removed():
    trk = BYTETracker()
    step(trk, [box(10, 10)], [0.9])
    out = step(trk, [box(10, 10), box(500, 10)], [0.9, 0.9])
    assert ids(out) == [1]                                 # frame >= 2: born unconfirmed
    assert [t.track_id for t in trk.tracked_stracks] == [1, 2]
    out = step(trk, [box(10, 10), box(501, 10)], [0.9, 0.9])
    assert ids(out) == [1, 2]
    # an unconfirmed track that finds nothing is removed
    step(trk, [box(10, 10), box(501, 10), box(900, 10)], [0.9, 0.9, 0.9])
    assert [t.track_id for t in trk.tracked_stracks] == [1, 2, 3]
    step(trk, [box(10, 10), box(501, 10)], [0.9, 0.9])
    assert [t.track_id for t in trk.tracked_stracks] == [1, 2]
    assert 3 not in [t.track_id for t in trk.lost_stracks]


def test_new_track_needs_new_track_thresh():
    trk = BYTETracker()
    assert step(trk, [box(10, 10)], [0.55]) == []           # > track_thresh, < track_thresh + 0.1
    assert trk.tracked_stracks == []


def test_duplicate_between_tracked_and_lost_drops_the_younger():
    from bytetrack_oracle import STrack, remove_duplicate_stracks
    from oracle.deepsort_oracle import kf_initiate, tlwh_to_xyah
    a, b = STrack(np.zeros(4), 0.9, 0), STrack(np.zeros(4), 0.9, 0)
    for t, tid in ((a, 1), (b, 2)):
        t.track_id = tid
        t.mean, t.covariance = kf_initiate(tlwh_to_xyah(np.array([10, 10, 40, 100], np.float32)))
    a.start_frame, a.frame_id = 1, 10                      # tracked, age 9
    b.start_frame, b.frame_id = 5, 8                       # lost, age 3: the younger, dropped
    ra, rb = remove_duplicate_stracks([a], [b])
    assert ra == [a] and rb == []
    a.start_frame = 8                                      # now the tracked one is the younger (ties drop the tracked one too)
    ra, rb = remove_duplicate_stracks([a], [b])
    assert ra == [] and rb == [b]
    b.mean = b.mean.copy()
    b.mean[0] += 30                                        # far apart: no duplicate
    ra, rb = remove_duplicate_stracks([a], [b])
    assert ra == [a] and rb == [b]


def _brute(cost, thresh):
    t, n = cost.shape
    best = 0.0
    for k in range(1, min(t, n) + 1):
        for rows in itertools.combinations(range(t), k):
            for cols in itertools.permutations(range(n), k):
                best = min(best, sum(float(cost[r, c]) - float(np.float32(thresh)) for r, c in zip(rows, cols)))
    return best


@pytest.mark.parametrize("seed", range(12))
def test_extended_assignment_is_the_brute_force_minimum(seed):
    rng = np.random.default_rng(seed)
    t, n = rng.integers(1, 5), rng.integers(1, 5)
    cost = rng.uniform(0, 1, (t, n)).astype(np.float32)
    thresh = 0.8
    matches, _, _ = linear_assignment(cost, thresh)
    got = sum(float(cost[r, c]) - float(np.float32(thresh)) for r, c in matches)
    assert got == pytest.approx(_brute(cost, thresh), abs=1e-6)
    ext = extended_matrix(cost, thresh)
    assert ext.dtype == np.float32 and ext.shape == (t + n, t + n)
    assert (ext[t:, n:] == 0).all() and (ext[:t, n:] == np.float32(0.4)).all()


def test_output_rows_format():
    trk = BYTETracker()
    out = step(trk, [box(10.4, 10.6, 40, 100)], [0.9])
    rows, conf = BYTETracker.rows(out)
    assert rows.tolist() == [[10, 11, 50, 111, 1, 0]] and conf.tolist() == [np.float32(0.9)]
    assert out[0].state == TRACKED
