"""The proximity oracle (tests/prox_oracle.py) on its own, without a GPU: its arithmetic against Python's own (math.isqrt,
Fraction, floor division), the derived bound of proximity.homography on two synthetic cameras, and branch counters that show that the
seeded cases of tests/prox_cases.py -- the ones tests/test_gpu_prox.py holds the device to -- reach every branch."""
import math
from fractions import Fraction

import numpy as np
import pytest

import prox_cases as PC
import prox_oracle as PO
from conftest import pkg


def test_isqrt_against_math_isqrt_up_to_2_61():
    vs = {0, 1, 2, 3}
    for b in range(1, 31):
        for k in ((1 << b) - 1, 1 << b, (1 << b) + 1, 3 << (b - 1), 1518500249 >> (30 - b)):
            vs |= {k * k - 1, k * k, k * k + 1}
    for b in range(2, 62):
        vs |= {(1 << b) - 1, 1 << b, (1 << b) + 1}
    vs = sorted(v for v in vs if 0 <= v <= (1 << 61) + 1)
    assert vs[-1] == (1 << 61) + 1 and len(vs) > 500
    for v in vs:
        r = PO.isqrt(v)
        assert r == math.isqrt(v) and r * r <= v < (r + 1) * (r + 1), v


def test_near_rule_of_both_metrics_against_fractions():
    # metric 0: a lattice that includes d2 == near^2 and near^2 + 1
    near = 13
    seen = set()
    for dx in range(-15, 16):
        for dy in range(-15, 16):
            d2 = dx * dx + dy * dy
            got = PO.near_rule(PO.GROUND, near, 384, (5, -7, 20), (5 + dx, -7 + dy, 31))
            assert got == (Fraction(d2) <= Fraction(near) ** 2), (dx, dy)
            seen.add(d2 - near * near)
            assert PO.distance(PO.GROUND, (0, 0, 1), (dx, dy, 1)) == math.isqrt(d2)
    assert {0, 1} <= seen                                                    # 5, 12 -> 169 exactly; 7, 11 -> 170 = 169 + 1 (168 is no sum of two squares)
    # metric 1: the distance in units of the mean height, and the height-ratio boundary with its neighbour
    hits = dict(on_radius=0, past_radius=0, on_ratio=0, past_ratio=0)
    for ha, hb in ((20, 20), (20, 30), (30, 20), (20, 31), (10, 15), (10, 16), (256, 384), (256, 385), (1, 1), (32767, 32767)):
        for near_pm in (700, 1000, 4096):
            for dx in range(-60, 61, 1 if ha <= 31 else 13):
                for dy in (0, 2, 14, 28, 56):
                    D2 = dx * dx + dy * dy
                    ratio_ok = Fraction(max(ha, hb), min(ha, hb)) <= Fraction(384, 256)
                    # doubled pixels over twice the mean height (ha + hb) is pixels over the mean height: the rule compares it with near / 1000
                    dist_ok = Fraction(D2, (ha + hb) ** 2) <= Fraction(near_pm, 1000) ** 2
                    assert PO.near_rule(PO.BODY, near_pm, 384, (0, 0, ha), (dx, dy, hb)) == (ratio_ok and dist_ok), (ha, hb, near_pm, dx, dy)
                    hits["on_radius"] += Fraction(D2, (ha + hb) ** 2) == Fraction(near_pm, 1000) ** 2
                    hits["past_radius"] += not dist_ok and Fraction((abs(dx) - 1) ** 2 + dy * dy, (ha + hb) ** 2) <= Fraction(near_pm, 1000) ** 2
                    hits["on_ratio"] += 256 * max(ha, hb) == 384 * min(ha, hb)
                    hits["past_ratio"] += 0 < 256 * max(ha, hb) - 384 * min(ha, hb) <= 256
                    want = math.isqrt(1000000 * D2) // (ha + hb)
                    assert PO.distance(PO.BODY, (0, 0, ha), (dx, dy, hb)) == want
    assert all(hits.values()), hits


def test_floor_division_with_negative_numerators():
    H = (3, -5, 7, -2, 1, -9, 0, 1, 2)                                       # den = fy + 4
    for shift in (0, 3, 14):
        for fx in range(0, 128, 7):
            for fy in range(0, 96, 5):
                ok, gx, gy = PO.place(PO.GROUND, H, shift, fx, fy)
                nx, ny, den = 3 * fx - 5 * fy + 14, -2 * fx + fy - 18, fy + 4
                assert ok and gx == math.floor(Fraction(nx << shift, den)) and gy == math.floor(Fraction(ny << shift, den))
    assert PO.place(PO.GROUND, H, 0, 0, 10)[1:] == (-3, -1)                  # -36 / 14 and -8 / 14 round DOWN
    assert PO.place(PO.GROUND, (1, 0, 0, 0, 1, 0, 0, -1, 5), 0, 3, 10) == (False, 0, 0)          # den = 0
    assert PO.place(PO.GROUND, (1, 0, 0, 0, 1, 0, 0, -1, 4), 0, 3, 10) == (False, 0, 0)          # den < 0
    big = (1 << 30, 0, 0, 0, 1, 0, 0, 0, 1)
    assert PO.place(PO.GROUND, big, 0, 1, 0) == (False, 0, 0) and PO.place(PO.GROUND, big, 0, 0, 7)[0]      # 2^29 is beyond 2^24
    edge = (1 << 24, 0, 0, 0, 1, 0, 0, 0, 1)
    assert PO.place(PO.GROUND, edge, 0, 2, 0) == (True, 1 << 24, 0) and PO.place(PO.GROUND, edge, 0, 3, 0) == (False, 0, 0)


# ---------------------------------------------------------------------------------------------------- homography
def camera(tilt_deg, height, f, hw):
    """The 3 x 3 map pixel -> ground of a pinhole camera `height` above the plane, looking along +Y, tilted down by tilt_deg from the
    horizontal (90: straight down): (x, y, 1) -> (X w, Y w, w)."""
    H, W = hw
    t = math.radians(tilt_deg)
    K_inv = np.array([[1 / f, 0, -W / (2 * f)], [0, 1 / f, -H / (2 * f)], [0, 0, 1]])
    # a ray d = (u, v, 1) in camera axes (x right, y down, z forward) -> world (X right, Y forward, Z up)
    R = np.array([[1, 0, 0], [0, -math.sin(t), math.cos(t)], [0, -math.cos(t), -math.sin(t)]])
    D = R @ K_inv                                                            # the ray's world direction per pixel
    # the ground point is height * (dX, dY) / (-dZ): numerators height * D[0], height * D[1], denominator -D[2]
    return np.stack([height * D[0], height * D[1], -D[2]])


@pytest.mark.parametrize("name,tilt,height,f", [("looking down", 90.0, 3000.0, 900.0), ("oblique, the horizon inside the frame", 12.0, 2500.0, 700.0)])
def test_homography_keeps_its_derived_bound(name, tilt, height, f):
    M = pkg("proximity")
    hw = (720, 1280)
    true = camera(tilt, height, f, hw)
    # four-plus correspondences well below the horizon
    px = np.array([[100, 700], [1200, 690], [640, 500], [300, 600], [900, 650], [500, 560]], np.float64)
    hom = (true @ np.c_[px, np.ones(len(px))].T).T
    assert (hom[:, 2] > 0).all()
    ground = hom[:, :2] / hom[:, 2:]
    H, shift = M.homography(px, ground)
    assert H.dtype == np.int32 and H.shape == (9,) and np.abs(H.astype(np.int64)).max() <= 1 << 30 and 0 <= shift <= 14
    assert max(np.abs(H[:6].astype(np.int64)).max(), np.abs(H[6:].astype(np.int64)).max()) > 1 << 28       # the int32 range is used
    # The correspondences are exact, so the fit IS the camera's map up to a factor: `true` stands for the float64 fit, and lam is the
    # factor b of the denominator row (its largest entry became the largest integer, to 2^-29).
    Hi = [int(v) for v in H]
    lam = max(abs(v) for v in Hi[6:]) / np.abs(true[2]).max()
    placed = unplaced = horizon = 0
    for y in range(0, 720, 24):
        for x in range(0, 1280, 40):
            fx, fy = 2 * x + 1, 2 * y                                        # an anchor as a box gives it
            den = Hi[6] * fx + Hi[7] * fy + 2 * Hi[8]
            ok, gx, gy = PO.place(PO.GROUND, Hi, shift, fx, fy)
            E = (fx + fy + 2) / 2
            t = true @ np.array([fx, fy, 2.0])
            if lam * t[2] < -E - 1:                                          # above the horizon by more than the rounding: den <= 0
                assert den <= 0 and not ok, (name, x, y, den)
                horizon += 1
            if not ok:
                unplaced += 1
                continue
            assert den > 0
            g = t[:2] / t[2]                                                 # the float64 evaluation of the fit
            bound = 1 + ((1 << shift) + np.abs(g)) * E / den + 1e-6 * (1 + np.abs(g))
            assert (np.abs(np.array([gx, gy]) - g) <= bound).all(), (name, x, y, gx, gy, g, bound)
            placed += 1
    assert placed > 300
    if tilt < 45:
        assert horizon > 100 and unplaced >= horizon                         # the rows above the horizon come out unplaced
    else:
        assert unplaced == 0


def test_homography_and_event_dicts_reject_and_name():
    M = pkg("proximity")
    with pytest.raises(ValueError):
        M.homography([[0, 0], [1, 0], [0, 1]], [[0, 0], [1, 0], [0, 1]])
    with pytest.raises(ValueError):
        M.homography([[0, 0], [1, 0], [0, 1], [1, 1]], [[0, 0], [1, 0], [0, 1]])
    H, shift = M.scale_map(np.array([[2.0, 0, 0], [0, 2.0, 0], [0, 0, 1.0]]))
    assert shift == 1 and H.tolist() == [1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0, 1 << 30]
    d = M.event_dict(np.array([M.EXPIRED, 1, 7, 0, 3, 40, 30, 2, 900, 5120, 256, 12, 3, 100, 90, 2], np.int32))
    assert (d["why"], d["gait_name"], d["speed"], d["max_speed"], d["links"], d["max_party"]) == ("expired", "moving", 1.0, 20.0, 2, 3)
    e = M.pair_event_dict(np.array([M.UNLINK, 9, 4, 11, 5, 1300, 2, 0], np.int32), stream=1)
    assert e == dict(kind="unlink", frame=9, ids=(4, 11), duration=5, distance=1300, ticks=2, stream=1)
    assert (M.EVENT_FIELDS, M.RECORD_FIELDS, M.TAG_FIELDS, M.PAIR_EVENT_FIELDS) == (PO.EVENT_FIELDS, PO.RECORD_FIELDS, PO.TAG_FIELDS, PO.PAIR_EVENT_FIELDS)
    assert (M.F_VALID, M.F_FIRST, M.F_NONEMPTY, M.F_PLACED, M.F_NEW) == (PO.F_VALID, PO.F_FIRST, PO.F_NONEMPTY, PO.F_PLACED, PO.F_NEW)


# ---------------------------------------------------------------------------------------------------- the seeded cases reach every branch
@pytest.fixture(scope="module")
def logs():
    """Every seeded case through the oracle once: {case name: (summed log, results per update)}."""
    out = {}
    for case in PC.seeded_cases():
        oracles, res = PC.oracles_for(case), []
        for op in case["ops"]:
            r = PC.run_op(oracles, op, case["cap"], case["cap_pairs"])
            if r is not None:
                res.append((op[0], r))
        log = {}
        for o in oracles:
            for k, v in o.log.items():
                log[k] = [a + b for a, b in zip(log.get(k, [0] * 4), v)] if k == "gait" else log.get(k, 0) + v
        out[case["name"]] = (log, res, oracles)
    return out


def test_the_planted_pair_links_and_unlinks_exactly_on_time(logs):
    log, res, oracles = logs["pair"]
    assert log["link_at"] == 2 and log["link_before"] == 2 and log["unlink_at"] == 1      # A-B at tick 2, A-D at tick 11; never a tick early
    events = [e.tolist() for _, r in res for f in r[7] for e in f if e[0]]
    assert [e[:4] for e in events] == [[PO.LINK, 2, 1, 2], [PO.UNLINK, 6, 1, 2], [PO.LINK, 11, 1, 4]]
    assert events[0][4:7] == [0, 300, 3] and events[1][4:7] == [4, 1250, 2] and events[2][6] == 3
    recs = np.concatenate([r[4] for _, r in res if len(r[4])])
    assert recs[1, 12] == 0 and recs[2, 12] == 1 and recs[5, 13] == 0 and recs[6, 13] == 1 and recs[10, 12] == 0 and recs[11, 12] == 1
    assert log["frozen"] >= 1 and log["frozen_back"] >= 1                    # B misses tick 3 and comes back with the counters as left
    assert log["reused_with_partner"] >= 1 and log["duplicate"] == 1 and log["dt_gt_1"] >= 1
    assert all(log["gait"]), log["gait"]                                     # 0 none yet, 1 still (A), 2 moving (B), 3 running (C)
    tags = np.concatenate([t for _, r in res for t in [r[5]] if len(t)])
    assert {0, 1, 2, 3} <= set(tags[:, 3].tolist())


def test_the_other_branches_are_reached(logs):
    ground = logs["ground"][0]
    assert ground["den_le_0"] > 0 and ground["beyond"] > 0 and ground["unplaced_then_placed"] > 0
    assert logs["crowd1-S3"][0]["capacity_stop"] == 1 and logs["crowd2-S3"][0]["capacity_stop"] == 1
    assert logs["crowd1-S3"][0]["pending_over_cap"] > 0 and logs["crowd1-S3"][0]["expired"] > 0 and logs["crowd1-S3"][0]["flushed"] > 0
    assert logs["crowd1-S3"][0]["reused_with_partner"] > 0 and logs["crowd1-S3"][0]["frozen"] > 0
    trunc = logs["truncation"]
    assert trunc[0]["truncated"] == 1
    n_pe, pe = trunc[1][0][1][6], trunc[1][0][1][7]
    assert n_pe.tolist() == [15, 0, 0, 0] and pe.shape == (4, 4, 8) and (pe[0, :, 0] == PO.LINK).all() and not pe[1:].any()
    assert trunc[0]["pending_over_cap"] > 0
    long = logs["long"]
    assert long[0]["on_saturated"] == 3 and long[2][0].export_pairs().tolist() == [[1, 2, 1, 32767, 0, 1]]
    path = logs["path"][1][0][1][4]
    assert path[0, 4] == 512 and path[0, 8] == 512 and path[1, 4] == 256 and path[1, 6] == 2
    cl = np.concatenate([r[4] for _, r in logs["cliques"][1] if len(r[4])])
    assert cl[1, 8] == 8 and cl[4, 13] == 1 and cl[4, 8] == 4 and cl[4, 6] == 2
    sizes = np.concatenate([r[4] for _, r in logs["sizes"][1] if len(r[4])])
    assert sizes[:, 1].tolist() == [0, 0, 1, 1, 2, 2, 63, 63, 64, 64, 65, 65, 512, 512]


def test_state_and_records_do_not_depend_on_cap_pairs():
    a, b = PC.crowd_case(3, 1, (4,), cap=16, cap_pairs=64), PC.crowd_case(3, 1, (4,), cap=16, cap_pairs=0)
    oa, ob = PC.oracles_for(a), PC.oracles_for(b)
    for op in a["ops"]:
        ra, rb = PC.run_op(oa, op, 16, 64), PC.run_op(ob, op, 16, 0)
        if ra is not None:
            for k in (0, 1, 2, 3, 4, 5, 6):
                assert np.array_equal(ra[k], rb[k])
        assert np.array_equal(oa[0].export_pairs(), ob[0].export_pairs())
