"""The planted scenes of tests/ocsort_edge_cases.py against the OC-SORT oracle alone (CPU): every scene must reach the edge it is named
for, or tests/test_gpu_ocsort_edges.py proves nothing.  The figures come from the oracle's recording hook (one record per association
problem: stage, IoU matrix, OCM term, cost, threshold, read-off or LSAP) and from the trace of ocsort_edge_cases.oracle_trace."""
import numpy as np
import pytest

import ocsort_edge_cases as E
import ocsort_oracle as O
from ocsort_edge_cases import down, up

F32 = np.float32
CHECKS = {}


def check(*prefixes):
    """Registers the assertion of every scene whose id starts with one of `prefixes`."""
    def deco(fn):
        for sc in E.SCENES:
            if sc.id.startswith(prefixes):
                assert sc.id not in CHECKS, sc.id
                CHECKS[sc.id] = fn
        return fn
    return deco


def recs(sid, lsap_fast=True):
    return E.oracle_trace(sid, lsap_fast)[0]


def edge_rec(sc, lsap_fast=True):
    return recs(sc.id, lsap_fast)[sc.edge - 1]


def track(rec, tid, key):
    return rec["export"][key][rec["ids"].index(tid)]


def same_before_edge(sids, edge):
    """The variants of one threshold scene agree frame by frame before the edge frame: outputs, state and every association problem."""
    first = recs(sids[0])
    for sid in sids[1:]:
        for a, b in zip(first[:edge - 1], recs(sid)[:edge - 1]):
            assert np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["conf"], b["conf"]) and a["ids"] == b["ids"], (sid, a["frame"])
            assert a["export"].keys() == b["export"].keys() and all(np.array_equal(a["export"][k], b["export"][k]) for k in a["export"]), (sid, a["frame"])
            assert [(p["stage"], p["solved"]) for p in a["problems"]] == [(p["stage"], p["solved"]) for p in b["problems"]], (sid, a["frame"])
            assert all(np.array_equal(p["iou"], q["iou"]) for p, q in zip(a["problems"], b["problems"])), (sid, a["frame"])


def planted(sc, rec):
    p = E.stage_problem(rec, sc.facts["stage"])
    assert p is not None, sc.id
    v = p["iou"][list(p["dets"]).index(sc.facts["det"]), p["tracks"].index(sc.facts["track"])]
    assert v == sc.facts["iou"] and v.dtype == F32 and p["th"] == F32(sc.params["iou_threshold"]), (sc.id, v, p["th"])
    assert {"eq": v == p["th"], "below": up(v) == p["th"] and v < p["th"], "above": down(v) == p["th"] and v > p["th"]}[sc.facts["side"]], sc.id
    return p, v


@check("th_stage1_")
def check_threshold_stage1(sc):
    same_before_edge(["th_stage1_eq", "th_stage1_below", "th_stage1_above"], sc.edge)
    for lsap_fast in (True, False):
        rec, before = edge_rec(sc, lsap_fast), recs(sc.id, lsap_fast)[sc.edge - 2]
        p, v = planted(sc, rec)
        assert p["iou"].shape == (1, 1) and before["ids"] == [1]
        d = {k: rec["stats"][k] - before["stats"][k] for k in ("n_fast", "n_lsap", "n_ocr")}
        side = sc.facts["side"]
        # on the threshold the read-off does not count the pair (iou > th) and the LSAP's pair stands (not iou < th); one ulp below it is dropped
        assert p["solved"] == ("read_off" if side == "above" and lsap_fast else "lsap"), (sc.id, lsap_fast)
        assert d == dict(n_fast=int(side == "above" and lsap_fast), n_lsap=int(not (side == "above" and lsap_fast)), n_ocr=0), (sc.id, d)
        if side == "below":                                       # OCR cannot rescue it: the last observation is further away still
            q = E.stage_problem(rec, "ocr")
            assert q["solved"] == "gate_shut" and q["iou"].max() < p["th"]
            assert rec["ids"] == [1, 2] and track(rec, 1, "time_since_update") == 1
        else:
            assert rec["ids"] == [1] and track(rec, 1, "time_since_update") == 0 and E.stage_problem(rec, "ocr") is None


@check("th_ocr_", "th_byte_")
def check_threshold_second_stages(sc):
    stage = sc.facts["stage"]
    same_before_edge([f"th_{stage}_eq_companion", f"th_{stage}_below_companion"], sc.edge)
    counter = "n_" + stage
    for lsap_fast in (True, False):
        rec, before = edge_rec(sc, lsap_fast), recs(sc.id, lsap_fast)[sc.edge - 2]
        p, v = planted(sc, rec)
        made = rec["stats"][counter] - before["stats"][counter]
        if not sc.facts["companion"]:                             # the equality pair alone: max > th is false, nothing is solved
            assert p["iou"].shape == (1, 1) and p["solved"] == "gate_shut" and made == 0
            assert track(rec, 1, "time_since_update") > 0 and rec["ids"] == ([1, 2] if stage == "ocr" else [1])
            continue
        assert p["iou"].shape == (2, 2) and p["solved"] == "lsap" and p["iou"].max() > p["th"]
        assert track(rec, 2, "time_since_update") == 0
        if sc.facts["side"] == "eq":
            assert made == 2 and track(rec, 1, "time_since_update") == 0 and rec["ids"] == [1, 2]
        else:
            assert made == 1 and track(rec, 1, "time_since_update") > 0 and rec["ids"] == ([1, 2, 3] if stage == "ocr" else [1, 2])


@check("ocr_no_observation")
def check_ocr_no_observation(sc):
    rec, before = edge_rec(sc), recs(sc.id)[sc.edge - 2]
    assert before["ids"] == [1] and before["export"]["has_obs"].tolist() == [0] and (before["export"]["last_observation"] == -1).all()
    p, q = E.stage_problem(rec, "stage1"), E.stage_problem(rec, "ocr")
    assert p["solved"] == "lsap" and 0 < p["iou"][0, 0] < p["th"]
    assert q["solved"] == "gate_shut" and q["iou"].shape == (1, 1) and q["iou"][0, 0] == 0
    assert rec["ids"] == [1, 2] and rec["stats"]["n_ocr"] == 0


def constant_blocks(p):
    """The four tie groups as blocks of one value each in the problem's IoU matrix (rows and columns in group order)."""
    r0 = c0 = 0
    tracks = [t for t in p["tracks"]]
    for nd, nt in zip(E.DETS_PER_GROUP, E.TRACKS_PER_GROUP):
        blk = p["iou"][r0:r0 + nd, c0:c0 + nt]
        assert blk.shape == (nd, nt) and (blk == blk[0, 0]).all() and blk[0, 0] > p["th"], (blk, tracks)
        rest = np.delete(p["iou"][r0:r0 + nd], np.s_[c0:c0 + nt], axis=1)
        assert (rest == 0).all()
        r0, c0 = r0 + nd, c0 + nt


@check("ties_")
def check_ties(sc):
    for lsap_fast in (True, False):
        rec = edge_rec(sc, lsap_fast)
        p = E.stage_problem(rec, sc.facts["stage"])
        assert p["solved"] == "lsap" and p["iou"].shape == (sum(E.DETS_PER_GROUP), sum(E.TRACKS_PER_GROUP)), sc.id
        constant_blocks(p)
        assert E.optimal_assignments_at_least_two(p["cost"]), sc.id
        assert len(rec["ids"]) == 8 + (0 if sc.facts["stage"] == "byte" else 2)        # the two boxes that lose are born (high band only)
    if sc.id == "ties_stage1_inertia":                            # with a velocity: the OCM term is in the cost and identical boxes still tie
        later = [E.stage_problem(r, "stage1") for r in recs(sc.id)[sc.edge:]]
        assert any(np.any(p["ocm"] != 0) and E.optimal_assignments_at_least_two(p["cost"]) for p in later)
    if sc.id == "ties_stage1":
        assert all(not np.any(E.stage_problem(r, "stage1")["ocm"]) for r in recs(sc.id)[1:])


@check("score_edges")
def check_score_edges(sc):
    t, use_byte = F32(sc.params["det_thresh"]), sc.params["use_byte"]
    tr = recs(sc.id)
    rec = edge_rec(sc)
    s = sc.frames[sc.edge - 1][1]
    assert s[:5].tolist() == [t, up(t), down(t), F32(0.1), up(F32(0.1))] and s[5:].tolist() == [t, up(t), down(t)] and s.dtype == F32
    assert list(E.stage_problem(rec, "stage1")["dets"]) == [1, 6]                      # the high band: s > det_thresh only
    b = E.stage_problem(rec, "byte")
    assert (list(b["dets"]) == [2, 4, 7] and len(b["tracks"]) == 4) if use_byte else b is None      # 0.1 < s < det_thresh
    assert [track(rec, i, "time_since_update") for i in range(1, 6)] == ([1, 0, 0, 1, 0] if use_byte else [1, 0, 1, 1, 1])
    assert rec["ids"] == [1, 2, 3, 4, 5, 6] and rec["stats"]["n_byte"] == (2 if use_byte else 0)
    # the frames around it: empty first frame, boxes and no tracks, an empty frame in the middle, a low-only frame
    assert tr[0]["n_dets"] == 0 and tr[0]["ids"] == [] and tr[1]["problems"] == [] and tr[1]["ids"] == [1, 2, 3, 4, 5]
    assert tr[3]["n_dets"] == 0 and len(tr[3]["ids"]) == 6 and tr[3]["problems"] == []
    assert tr[4]["n_dets"] == 5 and E.stage_problem(tr[4], "stage1") is None and (E.stage_problem(tr[4], "byte") is not None) == use_byte


def ocm_end_point(score=0.9, inertia=0.2):
    """The term at cosine +1, in ocm_term's order: ((asin32(1) / pi) * inertia) * score."""
    return F32(F32(F32(O.asin32(F32(1)) / O.PI) * F32(inertia)) * F32(score))


@check("ocm_")
def check_ocm(sc):
    rec, before = edge_rec(sc), recs(sc.id)[sc.edge - 2]
    p = E.stage_problem(rec, "stage1")
    assert p["solved"] == "lsap" and before["export"]["has_obs"].tolist() == [1] and p["iou"].shape[1] == 1
    iou, ocm, vel = p["iou"][:, 0], p["ocm"][:, 0], before["export"]["velocity"][0]
    assert abs(float(iou[0]) - float(iou[1])) < 2e-6 and iou[0] > p["th"] and iou[1] > p["th"]       # left and right of the prediction
    if sc.id == "ocm_zero_velocity":
        assert (vel == 0).all() and (ocm == 0).all() and before["export"]["hits"].tolist() == [1]
        return
    if sc.id == "ocm_same_centre":
        d, q = sc.frames[sc.edge - 1][0][sc.facts["det"]], rec["lookup"][1][2]
        assert rec["lookup"][1][:2] == (4, 1)
        assert (d[0] + d[2]) / F32(2) == (q[0] + q[2]) / F32(2) and (d[1] + d[3]) / F32(2) == (q[1] + q[3]) / F32(2)
        assert ocm[2] == 0 and iou[2] > p["th"] and np.any(vel != 0) and ocm[0] > 0.01 and ocm[1] > 0.01     # norm = 1e-6: a cosine of exactly 0, not 0 / 0
        return
    right = sc.frames[sc.edge - 1][0][1]
    assert ocm[0] < -0.01 and ocm[1] > 0.01 and np.array_equal(track(rec, 1, "last_observation"), right)     # the direction of motion decides
    assert rec["lookup"][1][1] == 1 and sc.params["delta_t"] == 1
    if sc.id == "ocm_axis":
        assert vel.tolist() == [0.0, 1.0] and ocm[1] == ocm_end_point() and ocm[0] == -ocm_end_point()


@check("ring_dt")
def check_ring(sc):
    tr = recs(sc.id)
    dt = sc.params["delta_t"]
    assert dt == (E.DTMAX if sc.id == "ring_dt8" else 1)
    exits = set()
    for f, rec in enumerate(tr):
        assert rec["ids"] == [1]
        seen = f in sc.facts["ages"]
        assert (track(rec, 1, "time_since_update") == 0) == (seen or f == 0), f
        if seen and rec["lookup"][1][1]:                          # the velocity exported after the frame carries the lookup's result
            age, ex, box = rec["lookup"][1]
            assert age == f
            exits.add(ex)
            assert np.array_equal(track(rec, 1, "velocity"), O.speed_direction(box, sc.frames[f][0][0])), f
    assert exits == ({1, 2, 3} if dt > 1 else {1, 3}), exits
    assert tr[sc.edge - 1]["lookup"][1][1] == (3 if dt > 1 else 1)


@check("slot_reuse_stale_ring")
def check_slot_reuse(sc):
    tr = recs(sc.id)
    assert all(len(r["ids"]) <= 1 for r in tr)                   # one track at a time: the second is born on the slot of the first
    assert [r["ids"] for r in tr[:5]] == [[1]] * 5 and tr[5]["ids"] == [] and [r["ids"] for r in tr[6:]] == [[2]] * 5
    assert [track(r, 1, "time_since_update") for r in tr[1:4]] == [0, 0, 0] and tr[3]["export"]["age"].tolist() == [3]   # ages 1, 2, 3 observed
    assert track(tr[7], 2, "time_since_update") == 1 and track(tr[7], 2, "age") == 1      # the new track has no observation at age 1
    rec = edge_rec(sc)
    age, ex, box = rec["lookup"][2]
    assert (age, ex) == (3, 2) and np.array_equal(box, sc.frames[8][0][0])               # key 1 (delta_t - 1 back) misses, key 2 is its own
    assert np.array_equal(track(rec, 2, "velocity"), O.speed_direction(sc.frames[8][0][0], sc.frames[9][0][0]))
    stale = O.speed_direction(sc.frames[1][0][0], sc.frames[9][0][0])                    # what the previous occupant's age-1 box would give
    assert not np.array_equal(stale, track(rec, 2, "velocity"))


@check("pred_zero_width")
def check_zero_width(sc):
    rec, before = edge_rec(sc), recs(sc.id)[sc.edge - 2]
    assert before["ids"] == [1, 2, 3] and before["out_ids"] == [2, 1] and rec["dropped"] == [3] and rec["ids"] == [1, 2, 4]
    assert [track(rec, i, "time_since_update") for i in (1, 2)] == [0, 0] and rec["out_ids"] == [2, 1]


@check("pred_shrinking")
def check_shrinking(sc):
    tr = recs(sc.id)
    assert [r["zeroed"] for r in tr] == [[]] * 5 + [[1], [], [1], []]      # the branch of the predict: frame 6, and frame 8 with a negative area
    assert [r["dropped"] for r in tr] == [[]] * 7 + [[1], []] and [r["ids"] for r in tr] == [[1, 2]] * 7 + [[2]] * 2
    area = [float(track(r, 1, "mean")[2]) for r in tr[:7]]
    rate = [float(track(r, 1, "mean")[6]) for r in tr[:7]]
    assert all(a > 0 for a in area[:6]) and area[4] < area[3] and rate[4] == rate[3] < 0 and area[5] == area[4] and rate[5] == 0
    rec = tr[6]                                                   # refound: ORU over a gap of 3, observed, output from the observation
    assert rec["stats"]["n_oru"] == 1 and rec["stats"]["max_gap"] == 3 and track(rec, 1, "time_since_update") == 0 and rec["out_ids"] == [2, 1]
    assert track(rec, 1, "has_obs") == 1 and track(rec, 1, "frozen") == 0 and np.isfinite(rec["raw"]).all()
    assert area[6] < -1000 and rate[6] < 0                        # the area after the closing updates is far below zero
    assert all(track(r, 2, "time_since_update") == 0 for r in tr) and tr[7]["out_ids"] == [2]      # the other track carries on


@check("life_refind_last", "life_max_age_1")
def check_refind(sc):
    rec, before = edge_rec(sc), recs(sc.id)[sc.edge - 2]
    max_age = sc.params["max_age"]
    assert before["ids"] == [1, 2] and before["export"]["time_since_update"].tolist() == [max_age, max_age]
    assert rec["ids"] == [1] and track(rec, 1, "time_since_update") == 0               # refound at max_age + 1; the other is removed
    assert rec["stats"]["n_oru"] == 1 and rec["stats"]["max_gap"] == max_age + 1


@check("life_min_hits")
def check_min_hits(sc):
    tr = recs(sc.id)
    assert "min_hits" not in sc.params and sc.edge == 3 + 1
    assert [r["out_ids"] for r in tr] == [[1], [2, 1], [2, 1], [1], [2], [2], [2], [2, 1]]
    assert [track(r, 1, "hit_streak") for r in tr] == [0, 1, 2, 3, 3, 1, 2, 3] and [track(r, 2, "hit_streak") for r in tr[1:]] == [0, 1, 2, 3, 4, 5, 6]
    assert tr[0]["export"]["has_obs"].tolist() == [0] and np.array_equal(tr[0]["raw"][0], O.x_to_bbox(tr[0]["export"]["mean"][0]))


@check("out_rounding")
def check_rounding(sc):
    tr = recs(sc.id)
    floors = set()
    for rec in tr[1:]:
        raw = rec["raw"].astype(np.float64)
        assert rec["export"]["has_obs"].all() and (raw - np.floor(raw) == 0.5).all()     # every coordinate is exactly k + 0.5
        floors |= {int(v) for v in np.floor(raw).ravel()}
        assert np.array_equal(rec["rows"][:, :4], np.rint(raw).astype(np.int32))
        assert (rec["rows"][:, :4] % 2 == 0).all()                # half to even
    assert any(k % 2 == 0 and k >= 0 for k in floors) and any(k % 2 and k >= 0 for k in floors)
    assert any(k % 2 == 0 and k < 0 for k in floors) and any(k % 2 and k < 0 for k in floors)


@check("capacity_boundary")
def check_capacity(sc):
    tr = recs(sc.id)
    cap = sc.params["max_tracks"]
    assert len(tr[0]["ids"]) == 5 and len(tr[1]["ids"]) == cap       # the births of frame 2 fill the table exactly
    assert tr[2]["n_dets"] == E.NMAX and E.stage_problem(tr[2], "stage1")["iou"].shape == (cap, cap) and len(tr[2]["ids"]) == cap
    more, _ = E.oracle_trace(sc.id, True, extra=(sc.overflow,))
    assert len(more[-1]["ids"]) == cap + 1                        # the overflow frame needs one slot more


@check("regime_")
def check_regime(sc):
    nd, nt = sc.facts["shape"]
    for lsap_fast in (True, False):
        rec = edge_rec(sc, lsap_fast)
        p = E.stage_problem(rec, "stage1")
        assert p["iou"].shape == (nd, nt) and p["solved"] == "lsap" and rec["stats"]["max_side"] == max(nd, nt) and rec["stats"]["n_lsap"] == 1
        above = p["iou"] > p["th"]
        assert above.sum(1).max() >= 2 and len(np.unique(np.round(p["iou"][above], 4))) <= 8      # each box over several tracks, IoU values repeat
    assert (nd, nt) in E.REGIMES
    if (nd, nt) == (86, 98):
        assert nd * nt == E.LDS_ARENA_FLOATS                     # the last matrix that fits the LDS arena
    if (nd, nt) == (87, 97):
        assert nd * nt > E.LDS_ARENA_FLOATS and max(nd, nt) < 98  # the first that goes to HBM, and a smaller side


@pytest.mark.parametrize("sid", [sc.id for sc in E.SCENES])
def test_scene_reaches_its_edge(sid):
    sc = E.scene_of(sid)
    assert 1 <= sc.edge <= len(sc.frames) and sum(sc.chunks) == len(sc.frames)
    calls = np.cumsum((0,) + sc.chunks)
    assert sc.edge == 1 or sc.edge - 1 not in calls.tolist() or len(sc.chunks) == 1, (sid, sc.chunks)     # the edge frame does not open a call
    CHECKS[sid](sc)


def test_every_scene_is_asserted():
    assert set(CHECKS) == {sc.id for sc in E.SCENES} and len(E.SCENES) == len(CHECKS)
    assert {sc.id[7:] for sc in E.SCENES if sc.id.startswith("regime_")} == {f"{a}x{b}" for a, b in E.REGIMES}


def test_recording_hook_changes_nothing():
    """The oracle with and without the hook: same outputs, state and counters."""
    for sid in ("ties_ocr_inertia", "score_edges_byte", "th_stage1_eq"):
        sc = E.scene_of(sid)
        a, b = sc.oracle(record=None), sc.oracle(record=[])
        for fr in sc.frames:
            ra, rb = O.OCSort.rows(a.update_xyxy(*fr)), O.OCSort.rows(b.update_xyxy(*fr))
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
        ea, eb = a.export(), b.export()
        assert all(np.array_equal(ea[k], eb[k]) for k in ea) and a.stats == b.stats and len(b.record) > 0
