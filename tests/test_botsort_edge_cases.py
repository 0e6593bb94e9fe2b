"""The planted scenes of tests/botsort_edge_cases.py through the NumPy oracle alone: the exact-feature recipe holds, and every scene
reaches the edge it is named for on the frame it names -- the planted cost is the threshold or its fp32 neighbour, the match flips
between the _below / _eq / _above twins, n_appearance moves by the stated amount, the planted pair has the stated pair index, the planted
self-dot is above 1, and a feature that does not normalise to finite values is no feature.  A scene that misses its edge fails here, not
on the GPU; tests/test_gpu_botsort_edges.py then holds the device to the oracle bit for bit."""
import numpy as np
import pytest

import botsort_edge_cases as B
import botsort_oracle as O

F32 = np.float32
LOST, TRACKED = O.LOST, O.TRACKED


def rec(sid, f):
    r = B.oracle_trace(sid)[0][f - 1]
    assert r["frame"] == f
    return r


def n_app_moved(sid, f):
    return rec(sid, f)["n_app"] - (rec(sid, f - 1)["n_app"] if f > 1 else 0)


def pair(stage, track_id, col):
    """(fused IoU distance, gated appearance distance, cost, IoU distance, needs a dot product, matched) of one pair of a problem."""
    r = stage["ids"].index(track_id)
    return (stage["d_iou"][r, col], stage["d_emb"][r, col], stage["cost"][r, col], stage["plain"][r, col], bool(stage["need"][r, col]),
            (r, col) in stage["matches"])


# ------------------------------------------------------------------------------------------------------------------ the scenes' shape
def test_scenes_are_small_and_their_edges_lie_inside_a_call():
    ids = [sc.id for sc in B.SCENES]
    assert len(set(ids)) == len(ids)
    for sc in B.SCENES:
        frames = B.frames_of(sc.id)
        assert len(frames) <= 10 and max(len(fr[0]) for fr in frames) <= 70, sc.id
        assert sum(sc.chunks) == len(frames) and (len(set(sc.chunks)) > 1 or len(sc.chunks) == 1), sc.id
        assert all(fr[3].shape == (len(fr[0]), B.DIM) and fr[3].dtype == F32 for fr in frames), sc.id
        firsts = np.cumsum((0,) + sc.chunks[:-1]) + 1            # first frame of every call
        assert sc.edge and not set(sc.edge) & set(firsts.tolist()) and max(sc.edge) <= len(frames), (sc.id, firsts)
        p = sc.params()
        assert all(0.0 < p.get(k, 0.5) <= 1.0 and float(F32(p.get(k, 0.5))) == p.get(k, 0.5) for k in ("proximity_thresh", "appearance_thresh")), sc.id
    for g in B.groups():
        lengths = [len(B.frames_of(sid)) for sid in g]
        plan = B.bank_plan(lengths)
        assert [sum(c[s] for c in plan) for s in range(len(g))] == lengths and any(0 in call for call in plan)
    assert sorted(sid for g in B.groups() for sid in set(g)) == sorted(ids) and max(len(g) for g in B.groups()) >= 10


def test_exact_feature_recipe():
    for k in (1, 9, 40):
        u = O.normalise(B.feat(k))
        assert np.array_equal(np.abs(u), np.full(B.DIM, F32(0.125)))
        for m in (0, 4, 15, 16, 40, 64):
            dot = O.wave_sum(u * O.normalise(B.feat(k, m)))
            assert dot == F32((64 - 2 * m) / 64) and np.maximum(F32(0), F32(1) - dot) / F32(2) == F32(m / 64), (k, m)
        assert O.wave_sum(u * O.normalise(B.feat(k + 1))) == 0
    # negating every feature negates every smoothed feature and leaves every product of two of them alone
    a, b = B.blend(B.feat(3), B.feat(3, 8)), B.blend(-B.feat(3), -B.feat(3, 8))
    assert np.array_equal(a, -b) and O.wave_sum(a * O.normalise(B.feat(3, 12))) == O.wave_sum(b * O.normalise(-B.feat(3, 12)))
    # a slot that has taken one feature holds it verbatim
    assert np.array_equal(rec("app_eq", 1)["tracks"][2]["smooth"], O.normalise(B.feat(2)))


def test_negated_features_negate_the_smoothed_ones():
    """What entitles the bank test to give neighbouring streams opposite features: the two runs differ in the sign of smooth_feat alone."""
    for sid in ("app_smooth_eq", "feature_presence", "nonfinite_inf"):
        (ta, a), (tb, b) = B.oracle_trace(sid, 1), B.oracle_trace(sid, -1)
        ea, eb = a.export(B.DIM), b.export(B.DIM)
        assert all(np.array_equal(ea[k], eb[k]) for k in ea if k != "smooth_feat") and np.array_equal(ea["smooth_feat"], -eb["smooth_feat"])
        assert ea["smooth_feat"].any() and a.n_appearance == b.n_appearance > 0
        assert all(np.array_equal(x["rows"], y["rows"]) and np.array_equal(x["conf"], y["conf"]) for x, y in zip(ta, tb))


# ------------------------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("sfx,side", B.SIDES)
def test_proximity_veto_on_its_threshold(sfx, side):
    sid = "prox" + sfx
    th = F32(B.scene_of(sid).params()["proximity_thresh"])
    assert th == (B.down, F32, B.up)[side + 1](F32(0.75))
    d_iou, d_emb, cost, plain, need, matched = pair(rec(sid, 2)["stages"][1], 2, 1)
    assert plain == F32(0.75) and d_iou == B.fused(0.75, B.RESCUE_S) and d_iou > B.MATCH     # IoU alone does not match
    near = side >= 0                                             # equality is near: far = d > proximity
    assert need == near and matched == near and d_emb == (F32(4 / 64) if near else F32(1)) and cost == min(d_iou, d_emb)
    assert n_app_moved(sid, 2) == 1 + near                       # the bystander's pair, and the planted one
    assert (2 in rec(sid, 2)["tracks"] and rec(sid, 2)["tracks"][2]["state"] == TRACKED) == near


@pytest.mark.parametrize("sfx,side", B.SIDES)
def test_appearance_gate_on_its_threshold(sfx, side):
    sid = "app" + sfx
    th = F32(B.scene_of(sid).params()["appearance_thresh"])
    assert th == (B.down, F32, B.up)[side + 1](F32(0.25))
    d_iou, d_emb, cost, plain, need, matched = pair(rec(sid, 2)["stages"][1], 2, 1)
    admitted = side >= 0                                         # e <= appearance admits equality
    assert need and plain == F32(0.75) and d_iou > B.MATCH
    assert d_emb == (F32(16 / 64) if admitted else F32(1)) and matched == admitted and n_app_moved(sid, 2) == 1 + admitted


@pytest.mark.parametrize("sfx,side", B.SIDES)
def test_appearance_gate_on_a_smoothed_feature(sfx, side):
    sid, f = "app_smooth" + sfx, B.SMOOTH_EDGE
    e = B.smooth_e()
    assert F32(B.scene_of(sid).params()["appearance_thresh"]) == (B.down, F32, B.up)[side + 1](e)
    # the first pass, at the default appearance_thresh, is this pass up to the edge frame
    first = B.run_oracle(O.BoTSORT(proximity_thresh=B.NEAR), B.frames_of(sid))
    for a, b in zip(first[:f - 1], B.oracle_trace(sid)[0][:f - 1]):
        assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["conf"], b["conf"]) and a["n_app"] == b["n_app"]
        assert a["tracks"].keys() == b["tracks"].keys()
        for i in a["tracks"]:
            assert all(np.array_equal(a["tracks"][i][key], b["tracks"][i][key]) for key in ("mean", "smooth", "state"))
    smooth = rec(sid, f - 1)["tracks"][2]["smooth"]
    assert len(set(np.abs(smooth).tolist())) == 2                # a blend of two features: no longer +-1/8
    assert np.maximum(F32(0), F32(1) - O.wave_sum(smooth * O.normalise(B.feat(3, 12)))) / F32(2) == e
    d_iou, d_emb, cost, plain, need, matched = pair(rec(sid, f)["stages"][1], 2, 1)
    admitted = side >= 0
    assert need and d_iou > B.MATCH and d_emb == (e if admitted else F32(1)) and matched == admitted
    assert n_app_moved(sid, f) == 1 + admitted


def test_appearance_distance_equal_to_the_iou_distance_is_not_counted():
    for sid, e, counted in (("app_ties_iou", F32(16 / 64), 0), ("app_under_iou", F32(15 / 64), 1)):
        assert B.scene_of(sid).params()["fuse_score"] is False
        d_iou, d_emb, cost, plain, need, matched = pair(rec(sid, 2)["stages"][1], 2, 1)
        assert need and matched and d_iou == plain == F32(0.25) and d_emb == e and cost == e
        assert n_app_moved(sid, 2) == counted                    # the planted pair if e < d_iou (the bystander's is 0 against 0 without fusion)


def test_clamp_and_range():
    sid, f = "clamp_and_range", 3
    assert B.scene_of(sid).params()["appearance_thresh"] == 1.0
    st, before = rec(sid, f)["stages"][1], rec(sid, f - 1)["tracks"]
    dets = B.oracle_args(B.frames_of(sid)[f - 1])[3]
    dot = {i: O.wave_sum(before[i]["smooth"] * O.normalise(dets[i - 1])) for i in (2, 3, 4)}     # track i meets detection i - 1
    assert dot[2] == 1 and np.array_equal(before[2]["smooth"], O.normalise(B.feat(5)))            # an identical first feature
    assert dot[3] > 1 and F32(1) - dot[3] < 0                                                    # the planted self-dot: the clamp is taken
    assert np.array_equal(before[3]["smooth"], B.blend(B.feat(B.CLAMP_K), B.feat(B.CLAMP_K, B.CLAMP_M)))
    assert dot[4] == -1                                                                          # the opposite feature
    for i, e in ((2, 0), (3, 0), (4, 1)):
        d_iou, d_emb, cost, plain, need, matched = pair(st, i, i - 1)
        assert need and matched and d_iou == 0 and d_emb == e and cost == 0, i                   # e = 1 is admitted (and is no gain)
    assert n_app_moved(sid, f) == 1                              # the bystander alone: 0 < 0 counts nothing, a negative e would


def test_feature_presence():
    sid = "feature_presence"
    t = lambda f: rec(sid, f)["tracks"]
    unit = lambda k, m=0: O.normalise(B.feat(k, m))
    assert {i: t(1)[i]["has_feat"] for i in range(1, 8)} == {1: True, 2: True, 3: False, 4: False, 5: True, 6: False, 7: True}
    # stage 1 on frame 2: blend / keep byte for byte / first feature copied / still none
    assert np.array_equal(t(2)[1]["smooth"], B.blend(B.feat(10), B.feat(10, 6))) and np.array_equal(t(2)[2]["smooth"], t(1)[2]["smooth"])
    assert np.array_equal(t(2)[3]["smooth"], unit(12, 6)) and not t(2)[4]["has_feat"]
    assert all((i, i) in rec(sid, 2)["stages"][1]["matches"] for i in range(4))
    # stage 3 on frame 3 (tracks 11..14 were born on frame 2): the same four
    st3 = rec(sid, 3)["stages"][3]
    assert st3["ids"] == [9, 10, 11, 12, 13, 14] and sorted(st3["ids"][r] for r, _ in st3["matches"]) == [11, 12, 13, 14]
    assert np.array_equal(t(3)[11]["smooth"], B.blend(B.feat(14), B.feat(14, 5))) and np.array_equal(t(3)[12]["smooth"], t(2)[12]["smooth"])
    assert np.array_equal(t(3)[13]["smooth"], unit(16, 5)) and not t(3)[14]["has_feat"]
    # stage 2 on frame 3: tracks 5 and 6 meet low-band rows that carry a feature; nothing is read or written
    assert 5 not in [st3["ids"][r] for r, _ in st3["matches"]] and len(rec(sid, 3)["problems"]) == 3
    assert t(3)[5]["state"] == TRACKED and np.array_equal(t(3)[5]["smooth"], t(2)[5]["smooth"])
    assert t(3)[6]["state"] == TRACKED and not t(3)[6]["has_feat"] and np.array_equal(t(4)[6]["smooth"], unit(21, 1))
    # a lost track found again in stage 1 blends
    assert t(2)[7]["state"] == t(3)[7]["state"] == LOST and t(4)[7]["state"] == TRACKED
    assert np.array_equal(t(4)[7]["smooth"], B.blend(B.feat(22), B.feat(22, 10)))
    # X (9, with a feature) and X0 (10, without) leave on frame 3; Y (15) is born without a feature and Z (16) with one on that frame,
    # on the device in the slots of X and X0; Y's first feature on frame 4 is a copy
    assert t(2)[9]["has_feat"] and not t(2)[10]["has_feat"] and not {9, 10} & set(t(3)) and not t(3)[15]["has_feat"]
    assert np.array_equal(t(3)[16]["smooth"], unit(25)) and np.array_equal(t(4)[15]["smooth"], unit(24))


@pytest.mark.parametrize("nr,nc,p", [(nr, nc, p) for nr, nc in B.PAIR_PROBLEMS for p in B.PAIR_INDEX[nr, nc]])
def test_one_pair_needs_a_dot_product_at_the_stated_index(nr, nc, p):
    st = rec(f"pair_groups_{nr}x{nc}_{p}", 2)["stages"][1]
    assert st["cost"].shape == (nr, nc) and st["ids"] == list(range(1, nr + 1)) and st["need"].sum() == 1
    r, c = map(int, np.argwhere(st["need"])[0])
    assert r * nc + c == p and st["d_iou"][r, c] > B.MATCH and st["d_emb"][r, c] == F32(4 / 64) and (r, c) in st["matches"]
    assert (st["d_emb"] < 1).sum() == 1 and len(st["matches"]) == nr


def test_pair_indices_cover_the_group_boundaries():
    assert B.PAIR_INDEX == {(8, 8): (0, 63), (5, 13): (0, 63, 64), (23, 23): (0, 63, 64, 511, 512, 528)}


def test_warp_is_applied_before_the_costs():
    sid, f = "warp_first", B.WARP_EDGE
    frames = B.frames_of(sid)
    assert frames[f - 1][4] is not None and frames[f - 2][4] is None and np.array_equal(frames[f - 1][4], [[1, 0, 1000], [0, 1, 500]])
    before, r = rec(sid, f - 1), rec(sid, f)
    # A (2) is tracked and moving, C (3) lost with a velocity, B (4) unconfirmed
    assert before["tracks"][2]["state"] == TRACKED and before["tracks"][2]["mean"][4] != 0
    assert before["tracks"][3]["state"] == LOST and before["tracks"][3]["mean"][4] != 0
    assert r["stages"][3]["ids"] == [4] and r["stages"][1]["ids"] == [1, 2, 3]
    for st, i, col in ((1, 2, 1), (1, 3, 3), (3, 4, 0)):
        d_iou, d_emb, cost, plain, need, matched = pair(r["stages"][st], i, col)
        assert need and matched and d_iou > r["stages"][st]["th"] and d_emb < F32(0.25) and plain <= F32(B.NEAR), i
    # without the warp of that frame every one of the three is far and unmet
    ora = B.scene_of(sid).oracle()
    unwarped = B.run_oracle(ora, frames[:f - 1] + [frames[f - 1][:4] + (None,) + frames[f - 1][5:]])[-1]
    assert not unwarped["stages"][1]["need"][1:].any() and not unwarped["stages"][3]["need"].any()
    assert unwarped["stages"][1]["matches"] == [] and unwarped["stages"][3]["matches"] == []


# ------------------------------------------------------------------------------------------------------------------ non-finite features
class FmaxOracle(O.BoTSORT):
    """The arithmetic this policy replaces: max(0, 1 - dot) as C's fmaxf, which returns the operand that is not a NaN."""

    def fused_cost(self, tracks, dets):
        d_iou, d_emb, _ = super().fused_cost(tracks, dets)
        far = O.iou_distance(tracks, dets) > self.proximity
        for i, t in enumerate(tracks):
            for j, d in enumerate(dets):
                if d_iou.size and not far[i, j] and t.smooth_feat is not None and d.curr_feat is not None:
                    e = np.fmax(F32(0), F32(1) - O.wave_sum(t.smooth_feat * d.curr_feat)) / F32(2)
                    d_emb[i, j] = e if e <= self.appearance else F32(1)
        return d_iou, d_emb, np.minimum(d_iou, d_emb).astype(F32)


@pytest.mark.parametrize("kind", ["zero", "inf", "nan"])
def test_a_feature_that_is_not_finite_is_no_feature(kind, monkeypatch):
    sid = "nonfinite_" + kind
    assert B.scene_of(sid).edge == B.NONFINITE_EDGE == (3, 5) and len(B.frames_of(sid)) == 5 + 3
    u = O.normalise(B.bad_feature(kind, 40))
    assert not O.has_feature(u) and O.has_feature(O.normalise(B.feat(40, 2)))
    if kind == "inf":                                            # inf / inf in one element, 0 in all the others
        assert np.isnan(u[7]) and not np.delete(u, 7).any()
    else:
        assert np.isnan(u).all()
    trace = B.oracle_trace(sid)[0]
    assert all(fr[5] is None for fr in B.frames_of(sid))         # every row is valid = 1
    # frame 3: the bad row (column 1) is never compared and is left over; the ordinary one (column 2) takes the track
    st = rec(sid, 3)["stages"][1]
    assert not st["need"][:, 1].any() and (st["d_emb"][:, 1] == 1).all() and st["plain"][1, 1] < F32(0.5)
    assert pair(st, 2, 2)[4:] == (True, True) and 1 not in [c for _, c in st["matches"]]
    assert not rec(sid, 3)["tracks"][3]["has_feat"] and rec(sid, 3)["tracks"][3]["smooth"] is None          # born from it, without a feature
    assert np.array_equal(rec(sid, 4)["tracks"][3]["smooth"], O.normalise(B.feat(41)))                     # its first feature, a frame later
    # frame 5: a bad row alone on the track matches by IoU and leaves the smoothed feature as it was
    st = rec(sid, 5)["stages"][1]
    assert pair(st, 2, 1)[4:] == (False, True) and pair(st, 2, 1)[0] == st["cost"][st["ids"].index(2), 1] < B.MATCH
    assert np.array_equal(rec(sid, 5)["tracks"][2]["smooth"], rec(sid, 4)["tracks"][2]["smooth"])
    for r in trace:
        assert all(np.isfinite(t["smooth"]).all() for t in r["tracks"].values() if t["has_feat"]), r["frame"]
        assert all(np.isfinite(s["cost"]).all() for s in r["stages"].values())
    # taken as a feature, with fmaxf's reading of a NaN, the bad row is at distance 0 from the track and wins it on frame 3
    monkeypatch.setattr(O, "has_feature", lambda unit: True)
    old = B.run_oracle(FmaxOracle(proximity_thresh=B.NEAR), B.frames_of(sid))
    st = old[2]["stages"][1]
    assert pair(st, 2, 1)[1] == 0 and pair(st, 2, 1)[5] and not np.array_equal(old[2]["rows"], trace[2]["rows"])
    assert not np.isfinite(old[2]["tracks"][2]["smooth"]).all()
