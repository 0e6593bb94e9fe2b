"""tests/trk_ref.py on the CPU: the float64 reference against the fixtures the real reference wrote, and the conditions a device test of
the association kernels relies on, asserted on the builders' own output -- a change of seed, noise or layout that removed such a
test's sensitivity fails here, without a GPU."""
import numpy as np
import pytest

import trk_ref as R
from conftest import pkg
from oracle import deepsort_oracle as O

DIMS_PLANTED = (30, 68, 70, 128, 512)        # dims at which random rows are far from every detection
SCENE = R.SCENE


def oracle_seed_state():
    """The seed run (five featureless frames of the scene) through the NumPy oracle: fifteen confirmed tracks."""
    trk = O.OracleTracker(nn_budget=R.BUDGET)
    for tlwh, conf, cls in R.seed_frames(pkg("synthetic").Scene(**SCENE)):
        trk.predict()
        trk.update(list(tlwh), list(conf), ["person"] * len(tlwh), [None] * len(tlwh))
    assert len(trk.tracks) == len(R.GLENS) and all(t.state == O.CONFIRMED for t in trk.tracks)
    return np.stack([t.mean for t in trk.tracks]).astype(np.float32), np.stack([t.covariance for t in trk.tracks]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def test_costs_fixture(golden):
    g = golden("costs")
    gal = [g["gallery"][i, :g["gallery_len"][i]] for i in range(len(g["mean"]))]
    app, arg, gap = R.app64(gal, g["det_feat"], g["has_feat"])
    assert np.allclose(app, g["app_cost"], rtol=0, atol=2e-6)                              # test_cost_kernels_vs_reference_fixture
    assert (app[:, ~g["has_feat"]] == 1e5).all() and (app[g["gallery_len"] == 0] == 1e5).all()
    assert (arg[app == 1e5] == -1).all() and (arg[app < 1e5] >= 0).all() and (gap >= 0).all()
    assert np.allclose(R.tlwh_to_xyah64(g["det_tlwh"]), g["det_xyah"], rtol=1e-6, atol=0)
    assert np.allclose(R.mean_to_tlwh64(g["mean"]), g["track_tlwh"], rtol=1e-6, atol=1e-5)
    # the fixture's 1 - IoU is fp32 arithmetic on fp32 boxes (the kernels match it bit for bit), so float64 cannot equal it: it sits
    # within R.iou_fp32_bound per cell, the roundings of the corners x + w, y + h carried through intersection and union (derived
    # there; the error found is 1.8e-6 at its largest and never above 0.19 of its cell's bound)
    err = np.abs(R.iou_cost64(g["track_tlwh"], g["det_tlwh"]) - g["iou_cost"])
    bound = R.iou_fp32_bound(g["track_tlwh"], g["det_tlwh"])
    assert (err <= bound).all(), (err.max(), bound.max())
    d2 = R.maha64(g["mean"], g["cov"], g["det_xyah"])
    assert np.allclose(d2, g["maha_d2"], rtol=2e-5, atol=1e-5)
    sure = np.abs(d2 - R.CHI2_4) > 1e-3
    gated = np.where(d2 > R.CHI2_4, 1e5, app)
    assert sure.mean() > 0.99 and np.array_equal((gated == 1e5)[sure], (g["gated_cost"] == 1e5)[sure])


def test_kalman_fixture(golden):
    g = golden("kf")
    idx = 0
    for step in range(6):
        pm, pc = (g["chain_mean"][idx - 1], g["chain_cov"][idx - 1]) if idx else (g["init_mean"], g["init_cov"])
        for _ in range(1 + step % 3):
            pm, pc = R.predict64(pm, pc)
        assert np.allclose(pm, g["chain_mean"][idx], rtol=3e-7, atol=0) and np.allclose(pc, g["chain_cov"][idx], rtol=1e-6, atol=1e-9)
        sm, sc = g["chain_mean"][idx], g["chain_cov"][idx]
        idx += 1
        jm, js = R.project64(sm, sc)
        assert np.allclose(jm, g["proj_mean"][step], rtol=0, atol=0) and np.allclose(js, g["proj_cov"][step], rtol=1e-6, atol=1e-9)
        for k in range(len(sm)):
            assert np.allclose(R.maha64(sm[k:k + 1], sc[k:k + 1], g["gate_z"][step, k])[0], g["gate_d2"][step, k], rtol=2e-5, atol=1e-5)
            assert np.allclose(R.maha64(sm[k:k + 1], sc[k:k + 1], g["gate_z"][step, k], only_position=True)[0], g["gate_d2_pos"][step, k],
                               rtol=2e-5, atol=1e-5)
            um, uc = R.update64(sm[k], sc[k], g["chain_z"][step, k])
            assert np.allclose(um, g["chain_mean"][idx, k], rtol=1e-5, atol=1e-3) and np.allclose(uc, g["chain_cov"][idx, k], rtol=1e-4, atol=1e-4)
        idx += 1


def test_kalman_time_step_fixture(golden):
    g = golden("kf_dt")
    for di, dt in enumerate(g["dts"]):
        pm, pc = g[f"start_mean_{di}"], g[f"start_cov_{di}"]
        for step in range(6):
            em, ec = g[f"chain_mean_{di}"][step], g[f"chain_cov_{di}"][step]
            if step == 3:
                for k in range(len(pm)):
                    m, c = R.update64(pm[k], pc[k], g[f"upd_z_{di}"][k])
                    assert np.allclose(m, em[k], rtol=1e-5, atol=1e-3) and np.allclose(c, ec[k], rtol=1e-4, atol=1e-4)
            else:
                m, c = R.predict64(pm, pc, dt=float(dt))
                assert np.allclose(m, em, rtol=3e-7, atol=0) and np.allclose(c, ec, rtol=1e-6, atol=1e-9), (dt, step)
            pm, pc = em, ec


# ------------------------------------------------------------------------------------------------------------------ builders
def test_gallery_lengths_sit_on_every_tile_edge():
    g = set(R.GLENS)
    for edge in (16, 64, 7 * 16, 128):                              # MFMA tile, grid.y block, prep batch, fused kernel's gallery step
        assert {edge - 1, edge, edge + 1} <= g
    assert {0, 1, R.BUDGET} <= g and max(g) == R.BUDGET and len(R.GLENS) <= 16
    assert R.N_FULL == 5 * 32 + 1 and R.N_FULL >= R.BUDGET


@pytest.mark.parametrize("n", [R.N_FULL, 1, 32, 33])
@pytest.mark.parametrize("dim", DIMS_PLANTED)
def test_planted_rows_are_strict_minimisers(dim, n):
    c = R.plant(dim, n)
    cost, arg, gap = R.app64(c.galleries, c.det_feat, c.has_feat)
    assert [len(g) for g in c.galleries] == list(R.GLENS) and c.det_feat.dtype == np.float32 and c.galleries[-1].dtype == np.float32
    pl = c.planted
    assert pl.any() and (cost[pl] <= R.PLANT_MAX).all() and (gap[pl] >= R.PLANT_GAP).all(), (cost[pl].max(), gap[pl].min())
    assert (cost[pl] >= 5e-3).all()                                 # and well above the tolerance: a stale copy (distance 0) shows
    for t, g in enumerate(c.glen):
        j = np.nonzero(pl[t])[0]
        assert np.array_equal(arg[t, j], (j + 7 * t) % max(g, 1)), t  # the minimiser is the row the detection was planted at
        if n == R.N_FULL:                                           # every live row is some detection's strict minimiser
            exempt = {R.ZERO_ROW[1]} if t == R.ZERO_ROW[0] else set()
            assert set(arg[t, j].tolist()) == set(range(g)) - exempt, t
    # the exceptions are present
    assert (cost[0] == 1e5).all() and c.glen[0] == 0
    for j in R.FEATURELESS:
        if j < n:
            assert not c.has_feat[j] and (cost[:, j] == 1e5).all()
    if R.ZERO_DET < n:
        assert not c.det_feat[R.ZERO_DET].any() and (cost[1:, R.ZERO_DET] == 1.0).all()
    zt, zr = R.ZERO_ROW
    assert c.glen[zt] == zr + 1 and not c.galleries[zt][zr].any()
    # normalisation matters: norms spread over more than a decade on both sides
    nd = np.linalg.norm(c.det_feat[c.det_feat.any(1)], axis=1)
    ng = np.linalg.norm(c.galleries[-1], axis=1)
    if n >= 32:
        assert nd.max() / nd.min() > 10 and ng.max() / ng.min() > 10


@pytest.mark.parametrize("dim", DIMS_PLANTED)
def test_poison_rows_would_show(dim):
    """Rows left behind past glen by the all-full poison state are exact copies of detection features: read by mistake they give 0
    in a cell whose true value is at least 5e-3, some 1200 tolerances away at dim 30 and 80 at dim 512."""
    c = R.plant(dim)
    cost, _, _ = R.app64(c.galleries, c.det_feat, c.has_feat)
    p = R.poison_rows(c)
    assert p.shape == (R.BUDGET, dim)
    dist = np.maximum(0.0, 1.0 - R.unit64(p) @ R.unit64(c.det_feat).T)        # [BUDGET, n]
    live = cost[1:] < 1e5
    assert (cost[1:][live] >= 5e-3).all() and 5e-3 > 80 * R.app_bound(dim)
    for r in range(R.BUDGET):
        j = int(np.argmin(dist[r]))
        assert dist[r, j] < 1e-12 and c.has_feat[j] and (cost[1:, j] >= 5e-3).all()
    # ... and every track but the full one has poison behind its live rows
    assert (c.glen < R.BUDGET).sum() == len(R.GLENS) - 1


@pytest.mark.parametrize("n", [R.N_FULL, 33])
def test_boxes_reach_both_sides_of_the_gate(n):
    mean, cov = oracle_seed_state()
    det = R.boxes(mean, cov, n)
    assert det.dtype == np.float32 and det.shape == (n, 4) and (det[:, 2:] > 0).all()
    ref = R.frame64(mean, cov, [np.zeros((0, 4))] * len(mean), det, np.zeros((n, 4)), np.zeros(n))
    inside = ref["maha"] <= R.CHI2_4
    assert inside[np.arange(len(mean)), np.arange(len(mean))].all()              # ring 0 sits on its track
    assert 0.02 < inside.mean() < 0.5
    assert ((ref["iou"] < 1.0).mean() > 0.1) and ((ref["iou"] == 1.0).mean() > 0.1)
    # 1 - IoU in exact fp32 arithmetic stays within 1e-6 of float64 on these boxes (coordinates below 512: see R.SCENE)
    iou32 = O.iou_cost_matrix([O.mean_to_tlwh(O.kf_predict(mean[t], cov[t])[0]) for t in range(len(mean))], det)
    assert np.abs(iou32 - ref["iou"]).max() <= 1e-6
    if n == R.N_FULL:
        own = np.arange(n) % len(mean)
        d2 = ref["maha"][own, np.arange(n)]
        assert (d2 <= R.CHI2_4).sum() >= 2 * len(mean) and (d2 > R.CHI2_4).sum() >= 2 * len(mean)   # each side on a track's own rings


def test_oracle_mahalanobis_deviation_is_a_usable_yardstick():
    """The yardstick for a kernel's squared Mahalanobis distance: the fp32 oracle's own deviation from float64 on the planted boxes, metric
    |x - x64| / max(1, x64).  It must be a small number (else a multiple of it would admit anything) and not zero."""
    mean, cov = oracle_seed_state()
    det = R.boxes(mean, cov, R.N_FULL)
    ref = R.frame64(mean, cov, [np.zeros((0, 4))] * len(mean), det, np.zeros((R.N_FULL, 4)), np.zeros(R.N_FULL))
    xyah = np.stack([O.tlwh_to_xyah(b) for b in det])
    dev = 0.0
    for t in range(len(mean)):
        m, p = O.kf_predict(mean[t], cov[t])
        assert m.dtype == np.float32 and p.dtype == np.float32
        d2 = O.kf_gating_distance(m, p, xyah)
        dev = max(dev, float((np.abs(d2 - ref["maha"][t]) / np.maximum(1.0, ref["maha"][t])).max()))
    assert 1e-8 < dev < 1e-4, dev


@pytest.mark.parametrize("dim", (68, 128))
def test_follow_up_and_identity_rows(dim):
    """The later-frame builder aims at the newest, the oldest and other rows of whatever galleries it is given; own_rows() puts one
    identity row in the middle of every gallery; state_dict() carries either the planted or the all-full poison galleries."""
    c = R.plant(dim)
    t = len(c.glen)
    feat, has = R.follow_up(c.galleries, 33, 1, dim)
    cost, arg, gap = R.app64(c.galleries, feat, has)
    assert feat.dtype == np.float32 and not has[5] and has.sum() == 32 and (cost[:, 5] == 1e5).all()
    for j in range(33):
        i, g = j % t, int(c.glen[j % t])
        if g == 0 or not has[j]:
            continue
        want = g - 1 if j < t else 0 if j < 2 * t else (37 * j + 11) % g
        if (i, want) == R.ZERO_ROW:
            continue
        assert arg[i, j] == want and cost[i, j] <= R.PLANT_MAX and gap[i, j] >= R.PLANT_GAP, (j, i, want)
    ident = np.random.default_rng(3).standard_normal((t, dim)).astype(np.float32)
    o = R.own_rows(c, ident)
    oc, oa, _ = R.app64(o.galleries, ident, np.ones(t))
    for i in range(1, t):
        assert oa[i, i] == c.glen[i] // 2 and oc[i, i] < 1e-6
    exported = dict(track_id=np.arange(1, t + 1, dtype=np.int32), mean=np.zeros((t, 8), np.float32), gallery_len=np.zeros(t, np.int32))
    st, sp = R.state_dict(exported, c), R.state_dict(exported, c, galleries=np.tile(R.poison_rows(c), (t, 1)))
    assert st["galleries"].shape == (int(c.glen.sum()), dim) and st["gallery_len"].tolist() == list(R.GLENS) and st["next_track_id"] == t + 1
    assert sp["galleries"].shape == (t * R.BUDGET, dim) and (sp["gallery_len"] == R.BUDGET).all() and st["dim"] == sp["dim"] == dim
