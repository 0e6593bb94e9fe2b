"""The planted scenes of tests/byte_edge_cases.py through the NumPy oracles alone: every scene reaches the edge it is named for, for
both trackers, and every ByteTrack scene keeps to its class (exact: the tracks of the edge decision have never been updated; margin:
every float decision behind a first update stays MARGIN_* away from its threshold).  This is what entitles
tests/test_gpu_byte_edges.py to compare the device with the oracles exactly on these scenes."""
import numpy as np
import pytest

import byte_edge_cases as E

F32 = np.float32
_TRACES = {}


def trace(kind, sid):
    if (kind, sid) not in _TRACES:
        _TRACES[kind, sid] = E.oracle_trace(kind, sid)[0]
    return _TRACES[kind, sid]


def frame(kind, sid, f):
    rec = trace(kind, sid)[f - 1]
    assert rec["frame"] == f
    return rec


def problem(kind, sid, f, stage):
    ps = [p for p in frame(kind, sid, f)["problems"] if p["stage"] == stage]
    assert len(ps) == 1, (sid, f, stage)
    return ps[0]


# ------------------------------------------------------------------------------------------------------------------ the scenes' shape
def test_scenes_are_small_and_their_edges_lie_inside_a_call():
    assert len({sc.id for sc in E.SCENES}) == len(E.SCENES) and set(E.EDGE_FRAMES) == {sc.id for sc in E.SCENES}
    for sc in E.SCENES:
        for kind in E.KINDS:
            frames = E.frames_of(sc.id, kind)
            assert len(frames) <= 20 and max(len(fr[0]) for fr in frames) <= 10, sc.id
            assert sum(sc.chunks) == len(frames) and (len(set(sc.chunks)) > 1 or len(sc.chunks) == 1), sc.id
            if kind == "botsort":
                assert all(fr[3].shape == (len(fr[0]), E.DIM) and fr[3].dtype == F32 for fr in frames), sc.id
            h = np.concatenate([fr[0][:, 3] - fr[0][:, 1] for fr in frames])
            assert (h > 0).all() and all(np.isfinite(fr[0]).all() and np.isfinite(fr[1]).all() for fr in frames), sc.id
        firsts = np.cumsum((0,) + sc.chunks[:-1]) + 1            # first frame of every call
        assert not set(E.EDGE_FRAMES[sc.id]) & set(firsts.tolist()), (sc.id, firsts)
    assert sum(sc.params("botsort")["with_reid"] is False for sc in E.SCENES) == 1
    lengths = [len(E.frames_of(sc.id, "bytetrack")) for sc in E.SCENES]
    plan = E.bank_plan(lengths)
    assert [sum(c[s] for c in plan) for s in range(len(lengths))] == lengths
    assert all(any(c[s] == 0 and sum(d[s] for d in plan[:i]) < lengths[s] for i, c in enumerate(plan)) for s in range(len(lengths)))


def test_read_off_is_the_unique_optimum_condition():
    th = F32(0.5)
    assert E.read_off([[0.1, 0.9], [0.9, 0.2]], th) and E.read_off([[0.9, 0.9]], th) and E.read_off([[0.9, 0.1], [0.2, 0.9]], th)
    assert not E.read_off([[0.1, 0.2], [0.9, 0.9]], th)           # two entries below in a row
    assert not E.read_off([[0.1, 0.9], [0.2, 0.9]], th)           # two in a column
    assert not E.read_off([[0.1, 0.9], [0.9, 0.5]], th)           # an entry on the threshold
    assert E.read_off([[0.1, E.up(th)], [E.down(th), 0.9]], th) is False and E.read_off([[0.1, E.up(th)], [E.up(th), E.down(th)]], th)


# ------------------------------------------------------------------------------------------------------------------ duplicates
DUP_OUTCOMES = {"dup_drop_tracked": (13, [(3, 2, 3, 7)], [3], []),    # frame, (tracked id, lost id, age, age), dropped tracked, dropped lost
                "dup_drop_lost": (12, [(3, 2, 8, 2)], [], [2]),
                "dup_tie": (12, [(3, 2, 5, 5)], [3], []),
                "dup_many": (13, [(4, 2, 12, 7), (6, 3, 7, 7), (6, 5, 7, 6), (7, 2, 3, 7)], [6, 7], [2, 5])}


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("sid", sorted(DUP_OUTCOMES))
def test_duplicate_scenes_drop_what_they_claim(kind, sid):
    f, pairs, dt, dl = DUP_OUTCOMES[sid]
    assert (f,) == E.EDGE_FRAMES[sid]
    for rec in trace(kind, sid):
        d = rec["dup"]
        if rec["frame"] == f:
            assert sorted(d["pairs"]) == pairs and sorted(d["dropped_tracked"]) == dt and sorted(d["dropped_lost"]) == dl
            assert rec["frame"] not in (1,) and d["dist"].shape[0] >= 2           # a bystander shares the tracked list
        else:
            assert not d["pairs"], (rec["frame"], d["pairs"])
    if sid == "dup_tie":
        assert pairs[0][2] == pairs[0][3]                        # equal end - start: the tracked one goes
    if sid == "dup_many":                                        # the lost B and the tracked D each stand in two pairs, one that drops them and one
        b, d = [p for p in pairs if p[1] == 2], [p for p in pairs if p[0] == 6]      # that drops the other: both flag arrays take two writes
        assert len(b) == len(d) == 2 and sorted(p[2] > p[3] for p in b) == sorted(p[2] > p[3] for p in d) == [False, True]
        assert any(p[2] == p[3] for p in d)                      # one of them a tie


# ------------------------------------------------------------------------------------------------------------------ cost == threshold
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("stage", (1, 2, 3))
def test_cost_scenes_sit_on_below_and_above_their_threshold(kind, stage):
    th, f = E.STAGE_THRESH[stage], 3 if stage == 3 else 2
    got = {}
    for sfx in ("", "_below", "_above"):
        sid = f"cost_eq_stage{stage}{sfx}"
        assert E.EDGE_FRAMES[sid] == (f,)
        p = problem(kind, sid, f, stage)
        near = p["cost"][np.abs(p["cost"].astype(np.float64) - float(th)) < 1e-6]
        assert near.size == 1 and near.dtype == F32, (sid, p["cost"])
        got[sfx] = (near[0], p)
        assert not set(p["ids"]) & frame(kind, sid, f)["updated"], sid         # exact class: the track has only been predicted
    eq, lo, hi = got[""], got["_below"], got["_above"]
    assert eq[0] == th and lo[0] < th < hi[0]
    assert th - lo[0] <= 2 * np.spacing(th) and hi[0] - th <= 2 * np.spacing(th)       # one step of the score or of the box edge
    assert not E.read_off(eq[1]["cost"], th) and E.read_off(lo[1]["cost"], th) and E.read_off(hi[1]["cost"], th)
    # what SciPy makes of them: at the threshold and above it the pair is left apart, below it is matched
    n = [len(x[1]["matches"]) for x in (lo, eq, hi)]
    assert n[0] == n[1] + 1 == n[2] + 1


def test_stage3_score_is_a_high_band_score_of_both_trackers():
    assert E.fused(F32(0.625), E.STAGE3_SCORE) == E.UNCONF and E.fused(F32(0.75), F32(0.8)) == E.MATCH
    assert E.iou_cost((0, 0, 64, 128), (0, 0, 32, 128)) == E.SECOND
    for kind in E.KINDS:
        high, _, new = E.BANDS["default"][kind]
        assert E.STAGE3_SCORE > high and E.STAGE3_SCORE >= new


# ------------------------------------------------------------------------------------------------------------------ tied optima
def tie_patterns(cost, th):
    """(a row with two equal entries below th, a column with two, a 2 x 2 block of four) in a cost matrix."""
    c = np.asarray(cost, F32)
    below = c < th
    row = any(below[r, a] and below[r, b] and c[r, a] == c[r, b] and below[:, a].sum() == below[:, b].sum() == 1
              for r in range(c.shape[0]) for a in range(c.shape[1]) for b in range(a + 1, c.shape[1]))
    col = any(below[a, k] and below[b, k] and c[a, k] == c[b, k] and below[a].sum() == below[b].sum() == 1
              for k in range(c.shape[1]) for a in range(c.shape[0]) for b in range(a + 1, c.shape[0]))
    blk = any(below[np.ix_((r, s), (a, b))].all() and len({c[r, a], c[r, b], c[s, a], c[s, b]}) == 1
              for r in range(c.shape[0]) for s in range(r + 1, c.shape[0]) for a in range(c.shape[1]) for b in range(a + 1, c.shape[1]))
    return row, col, blk


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("sid,f,stage", [("ties", 2, 1), ("ties", 2, 2), ("ties_unconfirmed", 3, 3)])
def test_tie_scenes_hold_the_three_tied_problems(kind, sid, f, stage):
    assert f in E.EDGE_FRAMES[sid]
    p = problem(kind, sid, f, stage)
    assert tie_patterns(p["cost"], p["th"]) == (True, True, True), p["cost"]
    assert not E.read_off(p["cost"], p["th"]) and not (p["cost"] == p["th"]).any()
    assert not set(p["ids"]) & frame(kind, sid, f)["updated"]    # exact class


# ------------------------------------------------------------------------------------------------------------------ score edges
@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("sid,bands", [("score_edges", "default"), ("score_edges_alt", "alt")])
def test_score_scenes_put_a_detection_on_every_band_edge(kind, sid, bands):
    high, low, new = E.BANDS[bands][kind]
    ora = E.scene_of(sid).oracle(kind)
    o_high, o_low, o_new = (ora.track_thresh, ora.low_thresh, ora.det_thresh) if kind == "bytetrack" else (ora.high, ora.low, ora.new_thresh)
    assert (high, low, new) == (o_high, o_low, o_new) and all(x.dtype == F32 for x in (o_high, o_low, o_new))
    if bands == "alt":
        assert (high, low, new) != E.BANDS["default"][kind] and (kind != "bytetrack" or new == F32(0.3 + 0.1))
    s = E.frames_of(sid, kind)[1][1]
    want = np.array([E.down(high), high, E.up(high), E.down(low), low, E.up(low), E.down(new), new, E.up(new)], F32)
    assert s.dtype == F32 and np.array_equal(s.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.nextafter(s[[0, 3, 6]], F32(1)), s[[1, 4, 7]]) and np.array_equal(np.nextafter(s[[1, 4, 7]], F32(1)), s[[2, 5, 8]])
    # frame 2: the high band is high+ and the three around new; the second band is high- and low+; the scores ON high and ON low are in no band
    rec = frame(kind, sid, 2)
    assert problem(kind, sid, 2, 1)["cost"].shape == (6, 4) and problem(kind, sid, 2, 2)["cost"].shape == (5, 2)
    assert rec["tracked"] == [1, 3, 6, 7, 8] and rec["lost"] == [2, 4, 5] and rec["unconfirmed"] == [7, 8]      # born: new and new+, not new-
    assert not rec["updated"]                                    # exact class
    out = dict(zip(rec["out_ids"], rec["conf"]))
    assert (out[1], out[3], out[6]) == (s[0], s[2], s[5])
    assert frame(kind, sid, 3)["unconfirmed"] == [9]             # the place of new- gets its track once the score allows it


# ------------------------------------------------------------------------------------------------------------------ slots and empties
@pytest.mark.parametrize("kind", E.KINDS)
def test_slot_scene_reuses_frees_times_out_and_fills_the_table(kind):
    sid = "slots_and_empties"
    sc = E.scene_of(sid)
    cap, buf = sc.kw["max_tracks"], sc.kw["track_buffer"]
    assert (cap, buf) == (8, 3) and sc.oracle(kind).max_time_lost == 3
    tr = trace(kind, sid)
    live = lambda f: len(tr[f - 1]["tracked"]) + len(tr[f - 1]["lost"])
    born = lambda f: sorted(set(tr[f - 1]["tracked"]) - set(tr[f - 2]["tracked"]) - set(tr[f - 2]["lost"]))
    # frame 3: an unconfirmed track is removed and a track is born: six slots in use before and after, so the new one has the old one's
    assert tr[1]["unconfirmed"] == [6] and tr[2]["removed"] == [6] and born(3) == [7] and live(2) == live(3) == 6
    # frame 4: low-band detections only; frame 5: none at all
    s4 = E.frames_of(sid, kind)[3][1]
    high, low, _ = E.BANDS["default"][kind]
    assert len(s4) == 3 and ((s4 > low) & (s4 < high)).all() and [p["stage"] for p in tr[3]["problems"]] == [2]
    assert tr[3]["lost"] == [4, 5] and tr[3]["removed"] == [7]
    assert tr[4]["n_dets"] == 0 and not tr[4]["problems"] and tr[4]["tracked"] == [] and tr[4]["lost"] == [4, 5, 1, 2, 3]
    # frame 6: T1 is refound; the low box over the lost T2 meets nothing (stage 2 takes Tracked tracks only)
    s6 = E.frames_of(sid, kind)[5][1]
    assert tr[5]["tracked"] == [1] and 1 in tr[4]["lost"] and (s6 < high).sum() == 1 and [p["stage"] for p in tr[5]["problems"]] == [1]
    # T4, T5: lost since frame 3, max_time_lost old on frame 6 and still there: frame 7 refinds T4, and only then is T5 removed.
    # T2, T3: the same a frame later.  A timeout by >= would have removed T4 and T2 before their boxes came.
    assert 6 - 3 == buf and tr[5]["lost"] == [4, 5, 2, 3] and tr[5]["removed"] == []
    assert tr[6]["tracked"] == [1, 4] and tr[6]["removed"] == [5] and tr[6]["lost"] == [2, 3]
    assert tr[7]["tracked"] == [1, 4, 2] and tr[7]["removed"] == [3] and tr[7]["lost"] == []
    # frames 9 and 10: one slot is left; two births with one slot freed by a removal in the same frame fill the table exactly
    assert live(9) == cap - 1 and len(tr[9]["removed"]) == 1 and len(born(10)) == 2 and live(10) == cap
    assert 10 in E.EDGE_FRAMES[sid] and 3 in E.EDGE_FRAMES[sid] and 5 in E.EDGE_FRAMES[sid]
    # the frame behind the scene: two slots are freed, three are needed
    more, _ = E.oracle_trace(kind, sid, extra=[E.overflow_of(sid, kind)])
    last = more[-1]
    births = sorted(set(last["tracked"]) - set(tr[-1]["tracked"]))
    assert len(last["removed"]) == 2 and len(births) == 3 and cap - live(10) + len(last["removed"]) == len(births) - 1


# ------------------------------------------------------------------------------------------------------------------ ByteTrack's classes
def stable(p, rng):
    """The oracle's assignment of a problem survives every cost moving by up to MARGIN_COST / 10 (ten times what a 1e-3 px shift of a mean
    does to the IoU of these boxes)."""
    import bytetrack_oracle
    for _ in range(4):
        c = (p["cost"] + rng.uniform(-E.MARGIN_COST / 10, E.MARGIN_COST / 10, p["cost"].shape)).astype(F32)
        if bytetrack_oracle.linear_assignment(c, p["th"])[0] != p["matches"]:
            return False
    return True


@pytest.mark.parametrize("sid", [sc.id for sc in E.SCENES])
def test_bytetrack_scenes_keep_to_their_class(sid):
    """A decision among tracks that have only been initiated and predicted is bit-comparable; any other keeps its margins."""
    sc, rng = E.scene_of(sid), np.random.default_rng(5)
    n_exact_edges = 0
    for rec in trace("bytetrack", sid):
        upd = rec["updated"]
        for p in rec["problems"]:
            if not set(p["ids"]) & upd:
                n_exact_edges += not E.read_off(p["cost"], p["th"])
                continue
            gap = np.abs(p["cost"].astype(np.float64) - float(p["th"])).min()
            assert gap >= E.MARGIN_COST, (rec["frame"], p["stage"], gap)
            assert stable(p, rng), (rec["frame"], p["stage"])
        d = rec["dup"]
        if d["dist"].size:
            touched = np.array([[a in upd or b in upd for b in d["ids"][1]] for a in d["ids"][0]]).reshape(d["dist"].shape)
            gap = np.abs(d["dist"].astype(np.float64) - float(E.DUP))[touched]
            assert gap.size == 0 or gap.min() >= E.MARGIN_COST, (rec["frame"], gap.min())
        moved = np.array([i in rec["updated_after"] for i in rec["out_ids"]], bool)
        raw = rec["raw"][moved].astype(np.float64)
        off = np.abs(raw - np.floor(raw) - 0.5)
        assert off.size == 0 or off.min() >= E.MARGIN_PIXEL, (rec["frame"], off.min())
    if sc.cls == "exact":
        assert n_exact_edges >= 1 or sid.startswith("score_edges") or sid.endswith(("_below", "_above"))
    else:                                                        # an integer edge: no float decision of the scene is an exact-class one
        assert n_exact_edges == 0 or sid == "dup_many"
