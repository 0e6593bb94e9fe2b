"""The left-objects specification alone (tests/left_oracle.py; no GPU): what the planted scenes of
tests/left_cases.py do, the exact edges of the cell model recomputed by scalar loops, and the component labels against
scipy.ndimage.label.  tests/test_gpu_left.py holds the device to the same oracle bit for bit."""

import numpy as np
import pytest

import left_cases as LC
import left_oracle as LO
import scene_cases as SC

_RUN = {}


def run(cs):
    """(records, objects, events, cand, labels, oracles) of a case, once per name."""
    if cs["name"] not in _RUN:
        o = LC.oracles_for(cs)
        _RUN[cs["name"]] = LO.run(o, cs["frames"], cs["rows"]) + (o,)
    return _RUN[cs["name"]]


def events_of(ev, kind):
    return ev[ev[:, 2] == kind]


# ---- quiet scenes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (2, 6, 12))
def test_noise_and_a_mover_raise_no_candidate(sigma):
    cs = SC.noise_mover(sigma)
    o = LO.LeftOracle(cs["hw"], cs["cell"])
    top = 0
    for t, f in enumerate(cs["frames"][:, 0]):
        rec, obj, ev, cand, labels = o.tick(f)
        assert not cand.any() and rec[2] == 0 and not len(ev) and not obj.any(), t
        top = max(top, int(o.still.max()))
    assert top <= 8                                                          # the 3 px per tick mover never rests long enough


# ---- a bag, its mirror and its owner ------------------------------------------------------------------------------------------------------
def test_a_bag_is_one_object_left_and_ended():
    cs = LC.bag()
    rec, obj, ev, cand, labels, _ = run(cs)
    o = LO.OPTIONS
    assert [int(e[2]) for e in ev] == [LO.APPEARED, LO.RAISED, LO.ENDED] and set(ev[:, 3]) == {1}           # one uid, although the blob grows
    uids = obj[..., 0]
    assert set(np.unique(uids)) == {0, 1} and (ev[:, 1] == 0).all()
    app, rai, end = ev
    assert app[0] < rai[0] < end[0]
    assert rai[4] == LO.LEFT and rai[5:9].tolist() == cs["box"] and app[10] < rai[10] == 12                   # it appeared smaller
    assert rai[0] >= cs["rest_from"] + o["min_ticks"][0] + o["alarm_hold"][0] - 1
    n_cand = rec[:, 0, 2]
    last = int(np.nonzero(n_cand)[0][-1])
    assert last > cs["taken_at"] and end[0] == last + o["gone_ticks"][0] + 1
    assert n_cand[:cs["rest_from"] + o["min_ticks"][0]].max() == 0           # nothing while it slid in
    # the oracle's own ticks, as DESIGN.md section 44 records them
    assert (int(np.nonzero(n_cand)[0][0]), int(np.nonzero(n_cand == 12)[0][0]), last, int(n_cand[278]), app[0], rai[0], end[0]) == \
        (119, 127, 278, 8, 119, 143, 294)
    assert (n_cand[260:263] == 12).all()
    live = rec[:, 0, 4]
    assert live[:119].max() == 0 and (live[119:294] == 1).all() and live[294:].max() == 0
    assert rec[143:294, 0, 5].min() == 1 and rec[:143, 0, 5].max() == 0


def test_the_mirror_is_removed():
    cs = LC.mirror()
    rec, obj, ev, cand, labels, _ = run(cs)
    assert [int(e[2]) for e in ev] == [LO.APPEARED, LO.RAISED] and set(ev[:, 3]) == {1}
    assert ev[1, 4] == LO.REMOVED and ev[1, 5:9].tolist() == cs["box"] and ev[1, 0] >= 60 + 50 + 25 - 1
    assert obj[-1, 0, 0, :3].tolist() == [1, LO.REMOVED, 1]


def test_owner_is_who_carried_it():
    rec, obj, ev, *_ = run(LC.owner_carried())
    assert [int(e[2]) for e in ev] == [LO.APPEARED, LO.RAISED] and (ev[:, 9] == 12).all() and obj[-1, 0, 0, 7] == 12
    rec0, obj0, ev0, *_ = run(LC.owner_carried(0))                           # the row left 50 ticks before the first candidate
    assert [int(e[2]) for e in ev0] == [LO.APPEARED, LO.RAISED] and (ev0[:, 9] == -1).all()
    assert np.array_equal(ev[:, :9], ev0[:, :9])


def test_no_candidate_under_a_standing_person():
    """The reading pinned here (left_oracle.py): an occupied cell's `still` stays, so under the row of id 5 (and its pad of one cell) no
    cell of the resting block becomes a candidate for the 400 ticks; when the person leaves, min_ticks later the object appears, owned
    by 5.  Cells that WERE candidates when a row steps on them stay candidates: `missing` never advances because of occupancy."""
    cs = LC.owner_standing()
    rec, obj, ev, cand, labels, _ = run(cs)
    assert rec[:460 + 49, 0, 2].max() == 0                                   # still is 1 at tick 460 (fast settled under the row), 50 at 509
    assert [int(e[2]) for e in ev] == [LO.APPEARED, LO.RAISED] and (ev[:, 9] == 5).all() and ev[0, 0] == 460 + 49
    assert ev[1, 4] == LO.LEFT and ev[1, 5:9].tolist() == cs["box"]
    # the second half: an alarmed object is stepped on for 40 ticks (longer than gone_ticks) and stays as it is
    bag = LC.bag(ticks=230, taken_at=10 ** 6)
    o = LC.oracles_for(bag)[0]
    x0, y0, x1, y1 = bag["box"]
    cover = np.array([[x0, y0, x1 - 1, y1 - 1, 9, 0]], np.int32)
    for t, f in enumerate(bag["frames"][:, 0]):
        r, ob, e, cd, _ = o.tick(f, cover if 180 <= t < 220 else None, t)
        if t >= 180:
            assert r[2] == 12 and ob[0, 0] == 1 and ob[0, 11] == 0 and not len(e), t


# ---- exact scenes ------------------------------------------------------------------------------------------------------------------------
def stills(cs):
    """still [ticks, Hc, Wc] and the oracle after the last tick."""
    o = LC.oracles_for(cs)[0]
    out = []
    for t, f in enumerate(cs["frames"][:, 0]):
        o.tick(f, None if cs["rows"] is None else cs["rows"][t][0], t)
        out.append((o.still.copy(), o.fast.copy(), o.slow.copy()))
    return out, o


def test_df_at_the_threshold_is_stable_and_one_more_is_not():
    cs = LC.df_edge()
    hist, o = stills(cs)
    t = cs["test_tick"]
    still0, fast0, _ = hist[t - 1]
    assert fast0[1, 1] == 25600 and fast0[1, 3] == 25599 and still0[1, 1] > 2 and still0[1, 3] > 2
    still1 = hist[t][0]
    assert still1[1, 1] == still0[1, 1] + 1                                  # df = 28160 - 25600 = thresh << 8: stable (and it differs from slow)
    assert still1[1, 3] == still0[1, 3] - 2                                  # df = 2561: not stable, decay


def test_ds_at_the_threshold_does_not_differ_and_one_more_does():
    cs = LC.ds_edge()
    hist, o = stills(cs)
    t = cs["test_tick"]
    still0, fast0, slow0 = hist[t - 1]
    assert fast0[1, 1] == fast0[1, 3] == 23040 and slow0[1, 1] == 25600 and slow0[1, 3] == 25601 and not still0.any()
    still1, _, slow1 = hist[t]
    assert still1[1, 1] == 0 and still1[1, 3] == 1                           # ds = 2560 / 2561
    assert slow1[1, 1] == 25600 + ((23040 - 25600) >> 8) and slow1[1, 3] == 25601    # the one that does not differ learns, the other is held
    assert run(cs)[3][t, 0].tolist() == [[0] * 5, [0, 0, 0, 1, 0], [0] * 5]


def test_settle_tick_of_a_jump_by_a_scalar_loop():
    cs = LC.jump()
    rec, obj, ev, cand, labels, _ = run(cs)
    fast = slow = 100 * 256
    still, first = 0, None
    for t in range(1, 40):                                                   # tick 0 is age 0
        g256 = (200 if t >= cs["jump_at"] else 100) * 256
        df, ds = abs(g256 - fast), abs(g256 - slow)
        fast += (g256 - fast) >> 1
        if df <= 2560:
            still = min(still + 1, 65535) if ds > 2560 else 0
        else:
            still = max(still - 2, 0)
        if still == 0:
            slow += (g256 - slow) >> 8
        if still >= 1 and first is None:
            first = t
    assert first == cs["jump_at"] + 4                                        # df: 25600, 12800, 6400, 3200, 1600
    assert cand[:first, 0].max() == 0 and cand[first:, 0, 1, 1:3].all() and cand[first:, 0].sum() == 2 * (40 - first)
    assert ev[0, 0] == first and ev[0, 5:9].tolist() == [4, 4, 12, 8] and run(cs)[5][0].still[1, 1] == still


def test_still_saturates_and_absorb_relearns():
    o = LO.LeftOracle((12, 20), 4, **dict(LC.EXACT, absorb_ticks=65535))
    g = np.full((3, 5), 100, np.uint8)
    o.tick(SC.paint(g, 4))
    o.tick(SC.paint(g, 4))
    o.still[1, 1], o.slow[1, 1] = 65533, 50 * 256                            # a cell that has differed from its background for ages
    o.tick(SC.paint(g, 4))
    assert o.still[1, 1] == 65534
    o.set_option("min_ticks", 65534)
    rec, *_ = o.tick(SC.paint(g, 4))
    assert o.still[1, 1] == 0 and o.slow[1, 1] == o.fast[1, 1] == 25600 and rec[2] == 0     # 65535 = absorb_ticks: re-learned at the cap
    cs = LC.absorb()
    rec, obj, ev, cand, labels, oracles = run(cs)
    first = cs["jump_at"] + 4
    assert cand[first + 6, 0].sum() == 2 and not cand[first + 7:, 0].any()   # still 1..7 are candidates, 8 = absorb_ticks is absorbed
    assert [int(e[2]) for e in ev] == [LO.APPEARED, LO.RAISED, LO.ENDED] and ev[2, 0] == first + 6 + 2
    assert oracles[0].slow[1, 1] == oracles[0].fast[1, 1] == 200 * 256 and not obj[-1].any()


def test_decay_zero_holds_still():
    held, _ = stills(LC.no_decay(0))
    lost, _ = stills(LC.no_decay(2))
    f = 16
    assert held[f - 1][0][1, 1] == lost[f - 1][0][1, 1] > 0
    assert all(h[0][1, 1] == held[f - 1][0][1, 1] for h in held[f:])         # unstable on every tick, decay 0: held
    assert [int(h[0][1, 1]) for h in lost[f:f + 5]] == [max(int(lost[f - 1][0][1, 1]) - 2 * k, 0) for k in range(1, 6)]


# ---- components -------------------------------------------------------------------------------------------------------------------------
def scipy_labels(cand):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, n = ndi.label(cand, structure=np.ones((3, 3), int))
    out = np.full(cand.shape, -1, np.int32)
    for k in range(1, n + 1):
        out[lab == k] = np.flatnonzero(lab == k)[0]
    return out


CASES = {cs["name"]: cs for cs in LC.component_cases(4)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_component_labels_against_scipy(name):
    cs = CASES[name]
    rec, obj, ev, cand, labels, _ = run(cs)
    assert cand[-1, 0].any()
    for t in range(len(cand)):
        assert np.array_equal(labels[t, 0], scipy_labels(cand[t, 0])), t
    if "mask" in cs:
        assert np.array_equal(cand[-1, 0].astype(bool), cs["mask"])


def test_random_grids_against_scipy():
    rng = np.random.default_rng(0)
    for p in (0.2, 0.45, 0.6):
        m = rng.random((33, 65)) < p
        assert np.array_equal(LO.label(m), scipy_labels(m))


def test_components_counts_flags_and_sizes():
    last = lambda name: [x[-1, 0] if x.ndim > 2 else x for x in run(CASES[name])[:5]]
    rec, obj, ev, cand, labels = last("corner c4")
    assert rec[3] == 1 and len(np.unique(labels[labels >= 0])) == 1
    rec, obj, ev, cand, labels = last("apart c4")
    assert rec[3] == 2 and len(np.unique(labels[labels >= 0])) == 2
    for name, n in (("spiral c4", 161), ("comb c4", 89)):
        rec, obj, ev, cand, labels = last(name)
        assert rec[2] == n and rec[3] == 1 and set(np.unique(labels)) == {-1, 0} and obj[0, 9] == n
    rec, obj, ev, cand, labels = last("70 isolated c4")
    assert rec[2] == 70 and rec[3] == 64 and rec[6] == 1 and rec[4] == 64 and rec[7] == 0 and len(np.unique(labels)) == 71
    rec, obj, ev, cand, labels = last("40 on 32 c4")
    assert rec[3] == 40 and rec[4] == 32 and rec[7] == 8 and rec[6] == 2
    assert sorted(ev[:, 3]) == list(range(1, 33)) and (ev[:, 2] == LO.APPEARED).sum() == 32     # once: the same 32 keep their slots
    rec, obj, ev, cand, labels = last("sizes 3..3 c4")
    assert rec[3] == 1 and obj[0, 9] == 3 and obj[0, 3:7].tolist() == [20, 4, 32, 8] and len(np.unique(labels)) == 4   # discarded blobs keep labels
    rec, obj, ev, cand, labels = last("sizes 2..4 c4")
    assert rec[3] == 3 and obj[:3, 9].tolist() == [2, 3, 4]


def test_split_and_merge_label_order_and_lowest_slot_decide():
    cs = CASES["split and merge c4"]
    rec, obj, ev, cand, labels, _ = run(cs)
    a, b = cs["phases"]
    assert obj[a - 1, 0, 0, [0, 3, 5]].tolist() == [1, 4, 24] and not obj[a - 1, 0, 1:].any()
    two = int(np.nonzero(rec[:, 0, 3] == 2)[0][0])
    assert obj[two, 0, 0, [0, 3, 5]].tolist() == [1, 4, 12]                  # both blobs meet slot 0's old box: the first in label order has it
    assert obj[two, 0, 1, [0, 3, 5]].tolist() == [2, 16, 24]                 # the other opens the lowest free slot
    one = two + int(np.nonzero(rec[two:, 0, 3] == 1)[0][0])
    assert obj[one, 0, 0, [0, 3, 5, 9]].tolist() == [1, 4, 24, 5]            # 2 cells with either slot: the lowest slot has it
    assert obj[one, 0, 1, [0, 11]].tolist() == [2, 1]
    end = events_of(ev, LO.ENDED)
    assert len(end) == 1 and end[0, 3] == 2 and end[0, 0] == one + 2 and end[0, 5:9].tolist() == [16, 4, 24, 8]
    assert set(ev[:, 3]) == {1, 2}
