"""The best-shot specification (tests/bestshot_oracle.py) on its own, without a GPU: the seeded cases of
tests/bestshot_cases.py reach every branch the device is later compared on, the score prefers the shot an operator would, and the
window arithmetic is what the specification says at its edges."""
import numpy as np
import pytest

import bestshot_cases as BC
import bestshot_oracle as BO


@pytest.fixture(scope="module")
def runs():
    return [(case,) + BC.run_oracle(case) for case in BC.CASES]


def test_seeded_cases_are_not_vacuous(runs):
    log = dict(replaced=0, tie_kept=0, reused_in_call=0)
    expired_shot = expired_bare = deferred = stops = 0
    for case, results, oracles in runs:
        for o in oracles:
            for k in log:
                log[k] += o.log[k]
        for n_final, events, thumbs, pending, status in results:
            deferred += int((pending > 0).sum())
            for s in range(case["streams"]):
                ev = events[s, :n_final[s]]
                expired_shot += int(((ev[:, 0] == BO.EXPIRED) & (ev[:, 7] == 1)).sum())
                expired_bare += int(((ev[:, 0] == BO.EXPIRED) & (ev[:, 7] == 0)).sum())
                for e, t in zip(ev, thumbs[s]):
                    assert e[7] == 1 or (not t.any() and not e[8:14].any())           # no shot: zero thumbnail, zero shot fields
        stops += int((results[-1][4] == BO.ERR_CAPACITY).sum())
    assert log["replaced"] >= 1 and log["tie_kept"] >= 1 and log["reused_in_call"] >= 1, log
    assert expired_shot >= 1 and expired_bare >= 1 and deferred >= 1 and stops >= 1, (expired_shot, expired_bare, deferred, stops)


def test_deferred_finals_all_arrive(runs):
    case, results, oracles = next(r for r in runs if r[0]["name"].startswith("deferral"))
    n_final, events, _, pending, _ = results[0]
    assert n_final.tolist() == [1] and pending.tolist() == [3]               # four ended at tick 1, one fitted
    got = [events[0, 0, 2]]
    while oracles[0].pending():
        out, pend, _ = oracles[0].update([], [], 1)
        assert len(out) == 1
        got.append(out[0][0][2])
    assert got == [10, 11, 12, 13]                                            # slot order, nothing dropped


def test_capacity_stop_keeps_the_shots_for_export_and_flush(runs):
    case, results, oracles = next(r for r in runs if r[0]["name"] == "capacity stop")
    assert results[0][4].tolist() == [BO.ERR_CAPACITY, 0]
    o = oracles[0]
    assert o.frame == 1 and [e[2] for e, _ in o.export()] == [1, 2]          # tick 1 was not committed
    out, pend, status = o.flush(8)
    assert [int(e[0]) for e, _ in out] == [BO.FLUSHED] * 2 and pend == 0 and status == BO.ERR_CAPACITY
    o.reset()
    assert o.status == 0 and o.export() == []


def test_the_planted_frame_wins():
    """One track over six frames: sharp and free at frame 2; blurred, half covered by a box standing in front, clipped by the frame's
    edge, or half the size elsewhere."""
    H, W = 160, 200
    rng = np.random.default_rng(7)
    sharp = BC.texture(rng, H, W)
    blurred = BC.texture(np.random.default_rng(7), H, W, blur=2)
    me = BC.row(40, 20, 64, 128, 5)
    front = BC.row(40, 84, 64, 70, 6)                                         # covers the lower half, its feet are lower
    o = BO.BestShotOracle((H, W), max_tracks=4, min_w=8, min_h=16)
    scenes = [(blurred, [me]), (sharp, [me, front]), (sharp, [me]), (sharp, [BC.row(170, 20, 64, 128, 5)]), (sharp, [BC.row(40, 20, 32, 64, 5)]),
              (blurred, [me])]
    scores = []
    for frame, rows in scenes:
        o.step(frame, BC.rows_of(*rows), [], 0)
        scores.append([c[6] for c in o.measure(frame, BC.rows_of(*rows)) if c[1] == 5][0])
    ev, thumb = [e for e in o.export() if e[0][2] == 5][0]
    assert ev[8] == 2 and ev[9] == scores[2] == max(scores) and ev[10:14].tolist() == [40, 20, 103, 147]
    assert all(scores[2] > 1.5 * s for i, s in enumerate(scores) if i != 2), scores
    assert np.array_equal(thumb, sharp[20:148, 40:104])                      # a native-size crop is copied pixel by pixel


@pytest.mark.parametrize("cn,tn", [(5, 16), (16, 16), (17, 16), (1, 16), (16384, 16), (16384, 128), (127, 128), (129, 128), (300, 256)])
def test_window_arithmetic(cn, tn):
    w = BO.windows(3, cn, tn)
    assert len(w) == tn and all(b > a for a, b in w) and w[0][0] == 3 and w[-1][1] <= 3 + cn and all(3 <= a and b <= 3 + cn for a, b in w)
    if cn >= tn:                                                             # a partition of the crop: every source column once
        assert all(w[u][1] == w[u + 1][0] for u in range(tn - 1)) and w[-1][1] == 3 + cn
        assert max(b - a for a, b in w) - min(b - a for a, b in w) <= 1
    else:                                                                    # narrower than the thumbnail: single columns, repeated in order
        assert all(b == a + 1 for a, b in w) and [a for a, _ in w] == sorted(a for a, _ in w) and {a for a, _ in w} == set(range(3, 3 + cn))
    if cn == tn:
        assert w == [(3 + u, 4 + u) for u in range(tn)]
    if cn == tn + 1:
        assert sorted(b - a for a, b in w) == [1] * (tn - 1) + [2]


def test_thumbnail_average_and_upsampling():
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (40, 50, 3)).astype(np.uint8)
    t = BO.thumbnail(frame, (4, 2, 8, 33), 16, 16)                           # 5 x 32 -> 16 x 16: columns repeat, rows average pairs
    for u, (xa, xb) in enumerate(BO.windows(4, 5, 16)):
        for v in range(16):
            win = frame[2 + 2 * v:4 + 2 * v, xa:xb].astype(np.int64).reshape(-1, 3)
            assert np.array_equal(t[v, u], (win.sum(0) + len(win) // 2) // len(win))
    flat = np.full((64, 64, 3), 200, np.uint8)
    assert BO.sharpness(BO.thumbnail(flat, (0, 0, 63, 63), 16, 16)) == 0     # no texture, no score


def test_score_terms():
    """fill: a crop smaller than the thumbnail counts for less; the occluder rule: lower feet stand in front, equal feet by row order;
    trunc halves."""
    H, W = 100, 100
    frame = BC.texture(np.random.default_rng(1), H, W)
    o = BO.BestShotOracle((H, W), thumb=(16, 16), min_w=1, min_h=1)
    a, b = BC.row(10, 10, 16, 16, 1), BC.row(10, 10, 16, 16, 2)              # the same box twice, equal feet
    m = {c[1]: c for c in o.measure(frame, BC.rows_of(a, b))}
    assert m[1][6] > 0 and m[2][6] == 0                                      # row 0 stands in front of row 1, never the reverse
    lower = BC.row(10, 18, 16, 16, 2)                                        # feet lower: covers half of a
    m = {c[1]: c for c in o.measure(frame, BC.rows_of(a, lower))}
    free = o.measure(frame, BC.rows_of(a))[0][6]
    assert m[1][6] == free * 128 >> 8 or abs(m[1][6] - free // 2) <= 1
    small = o.measure(frame, BC.rows_of(BC.row(10, 10, 8, 8, 1)))[0]
    th = BO.thumbnail(frame, small[3], 16, 16)
    assert small[6] == (BO.sharpness(th) * 64 * 256) >> 16                   # fill_q8 = 8 * 8 * 256 // (16 * 16) = 64
    edge = o.measure(frame, BC.rows_of(BC.row(-4, 10, 16, 16, 1)))[0]
    assert edge[5] == 1 and edge[3] == (0, 10, 11, 25)
    head = BO.region_of([10, 20, 30, 120, 1, 0], "head", 64, 3)
    assert head == (7, 17, 33, 45)
