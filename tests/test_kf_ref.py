"""tests/kf_ref.py on the CPU: the float64 Kalman reference against the states the real reference wrote (tests/golden/kf.npz, kf_dt.npz),
the fp32 NumPy restatement (oracle.deepsort_oracle.kf_*) measured against it on every case in the metrics of kf_ref -- these figures are
what the device tests' allowances are made of -- and the conditions those tests lean on, asserted on the builders' own output so that a
change of seed, grid or layout cannot quietly remove them."""
import dataclasses
import functools

import numpy as np
import pytest

import kf_ref as K
from oracle import deepsort_oracle as O


class OracleKF:
    """oracle.deepsort_oracle.kf_* on fp32 batches: the interface kf_ref.measure takes."""

    def initiate(self, z):
        r = [O.kf_initiate(x) for x in z]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def predict(self, mean, cov, dt=1.0):
        r = [O.kf_predict(m, p, np.float32(dt)) for m, p in zip(mean, cov)]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def project(self, mean, cov):
        r = [O.kf_project(m, p) for m, p in zip(mean, cov)]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def update(self, mean, cov, z):
        r = [O.kf_update(m, p, x) for m, p, x in zip(mean, cov, z)]
        return np.stack([a for a, _ in r]), np.stack([b for _, b in r])

    def gating(self, mean, cov, zs, shared_z, only_position):
        return np.stack([O.kf_gating_distance(m, p, zs if shared_z else zs[t], bool(only_position)) for t, (m, p) in enumerate(zip(mean, cov))])


def oracle_step(p):
    """The restatement's predict + update of every planned pair: {list position: (mean, cov)} fp32."""
    z = K.xyah32(p.det)
    out = {}
    for t, j in p.pair.items():
        pm, pp = O.kf_predict(p.mean[t], p.cov[t])
        out[t] = O.kf_update(pm, pp, z[j])
    return out


def step_figures(p, got):
    """`got` ({list position: (mean, cov)}) on the plan's pairs, twice:
      (covariance, mean) against float64 update(predict(state), z) in one piece.  The innovation z - H x is then taken from a float64
          predicted mean, while every fp32 copy rounds x + v first: at a centre of 30 000 px that rounding (1e-3 px) is a tenth of the
          innovation of a 0.5 px box, so the mean figure of the RESTATEMENT is 1e-2 here and the check is a loose one;
      (covariance, mean) against float64 update restarted from the fp32 predicted state -- the restatement's predict, which every
          device copy is held to bit for bit (dt = 1) -- where the update's metrics apply as they stand.  This is the tight one."""
    z = K.xyah32(p.det)
    e = [K.step_errs(got[t][0], got[t][1], p.mean[t], p.cov[t], z[j]) for t, j in p.pair.items()]
    r = [K.update_errs(got[t][0], got[t][1], *O.kf_predict(p.mean[t], p.cov[t]), z[j]) for t, j in p.pair.items()]
    return max(a for a, _ in e), max(b for _, b in e), max(a for a, _ in r), max(b for _, b in r)


@functools.lru_cache(maxsize=None)
def oracle_figures():
    """{operation: (covariance figure, mean figure)} of the restatement on every case, "gating": its figure over every gating run, and
    the gating records themselves.  The device tests take their allowances from here."""
    fig = K.measure(OracleKF())
    recs = K.gate_runs(OracleKF().gating)
    fig["gating"] = K.gate_figure(recs)
    return fig, recs


@functools.lru_cache(maxsize=None)
def base_plan():
    return K.plan(K.track_case_ids())


FALLBACK_T = K.first_fallback_tracks()


def far_ids(n):
    """n case states for the two big frames: the trackable cases in turn, without those whose predicted position is uncertain by more
    than 300 px (h = 179.3 and 2000 after seventy predicts; the planted frame of 28 tracks has them), so that tracks 3000 px apart are
    far outside each other's gates."""
    ok = []
    for i, c in enumerate(K.CASES):
        if c.trackable:
            _, pp = K.predict(c.mean, c.cov)
            if max(pp[0, 0], pp[1, 1]) <= 300.0 ** 2:
                ok.append(i)
    return [ok[k % len(ok)] for k in range(n)]


@functools.lru_cache(maxsize=None)
def big_plan(n_tracks):
    """The FIRST of the two frames of test_epoch_kernel_both_update_forms: n_tracks confirmed tracks with a tentative decoy after every
    third (the frame prunes them; no new tracks), the states of far_ids, track k moved to cell (k mod 16, k div 16) of a 1500 px lattice (the case's own
    centre taken off: every coordinate stays below 2^15, where fp32 still resolves 2e-3 px, the rounding edge of the output rows).  The 32
    features repeat every two lattice rows; what tells two tracks of one feature apart is the gate."""
    ids = far_ids(n_tracks)
    off = [(1500.0 * (k % 16) - float(K.CASES[ci].mean[0]) + 10 * (k // 16), 1500.0 * (k // 16) - float(K.CASES[ci].mean[1]) + 7 * (k % 16))
           for k, ci in enumerate(ids)]
    return K.plan(ids, offsets=off, decoy_every=3, seed=n_tracks, new=False)


def through_xyxy(tlwh):
    """A pipeline is handed corners and takes w = x2 - x1, h = y2 - y1 in fp32: (the corners to inject, the tlwh the tracker then gets)."""
    b = np.asarray(tlwh, np.float32)
    xyxy = np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1).astype(np.float32)
    return xyxy, np.stack([xyxy[:, 0], xyxy[:, 1], xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1]], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pipeline_plan(frames=4):
    """(the plan, the frames' corner boxes, the frames' tlwh) of the test that reaches the commit in front of trk_assoc_all_kernel, which
    only a pipeline does.  A pipeline embeds what it crops, so every box lies LEFT of the image (x2 < 0): the crops are empty, no
    detection has a feature, the galleries stay empty and the match is the IoU stage's.  That stage must then be unambiguous without
    features: the planted frame's 28 states on a 1500 px lattice, x mirrored."""
    ids = K.track_case_ids()
    off = [(-1700.0 - 1500.0 * (k % 8) - float(K.CASES[ci].mean[0]), 800.0 + 1500.0 * (k // 8) - float(K.CASES[ci].mean[1])) for k, ci in enumerate(ids)]
    p = K.plan(ids, offsets=off, seed=3)
    boxes = [through_xyxy(d) for d in K.drift_frames(p, frames)]
    return dataclasses.replace(p, det=boxes[0][1]), [b[0] for b in boxes], [b[1] for b in boxes]


# ------------------------------------------------------------------------------------------------------------------ fixtures
def test_reference_reproduces_kf_fixture(golden):
    g = golden("kf")
    m, p = zip(*(K.initiate(z) for z in g["z0"]))
    assert np.allclose(m, g["init_mean"], rtol=3e-7, atol=0) and np.allclose(p, g["init_cov"], rtol=1e-6, atol=1e-12)
    idx = 0
    for step in range(6):
        pm, pc = (g["chain_mean"][idx - 1], g["chain_cov"][idx - 1]) if idx else (g["init_mean"], g["init_cov"])
        for _ in range(1 + step % 3):
            pm, pc = zip(*(K.predict(a, b) for a, b in zip(pm, pc)))
        assert np.allclose(pm, g["chain_mean"][idx], rtol=3e-7, atol=0) and np.allclose(pc, g["chain_cov"][idx], rtol=1e-6, atol=1e-9)
        sm, sc = g["chain_mean"][idx], g["chain_cov"][idx]
        idx += 1
        for k in range(len(sm)):
            jm, js = K.project(sm[k], sc[k])
            assert np.array_equal(jm, g["proj_mean"][step, k]) and np.allclose(js, g["proj_cov"][step, k], rtol=1e-6, atol=1e-9)
            assert np.allclose(K.gating(sm[k], sc[k], g["gate_z"][step, k]), g["gate_d2"][step, k], rtol=2e-5, atol=1e-5)
            assert np.allclose(K.gating(sm[k], sc[k], g["gate_z"][step, k], True), g["gate_d2_pos"][step, k], rtol=2e-5, atol=1e-5)
            um, uc = K.update(sm[k], sc[k], g["chain_z"][step, k])
            assert np.allclose(um, g["chain_mean"][idx, k], rtol=1e-5, atol=1e-3) and np.allclose(uc, g["chain_cov"][idx, k], rtol=1e-4, atol=1e-4)
        idx += 1


def test_reference_reproduces_kf_dt_fixture(golden):
    g = golden("kf_dt")
    for di, dt in enumerate(g["dts"]):
        pm, pc = g[f"start_mean_{di}"], g[f"start_cov_{di}"]
        for step in range(6):
            em, ec = g[f"chain_mean_{di}"][step], g[f"chain_cov_{di}"][step]
            for k in range(len(pm)):
                if step == 3:
                    m, c = K.update(pm[k], pc[k], g[f"upd_z_{di}"][k])
                    assert np.allclose(m, em[k], rtol=1e-5, atol=1e-3) and np.allclose(c, ec[k], rtol=1e-4, atol=1e-4)
                else:
                    m, c = K.predict(pm[k], pc[k], float(dt))
                    assert np.allclose(m, em[k], rtol=3e-7, atol=0) and np.allclose(c, ec[k], rtol=1e-6, atol=1e-9), (dt, step)
            pm, pc = em, ec


# ------------------------------------------------------------------------------------------------------------------ the restatement, measured
def test_restatement_against_float64_on_every_case():
    """Measured here: covariance figure / mean figure
         initiate 1.2e-7 / 0      project 9.4e-8 / 0      update 3.2e-7 / 1.9e-7      predict dt 1 9.1e-8 / 5.5e-8, other dt 1.0e-7 .. 1.1e-7 / 5.9e-8
         gating 4.4e-7            predict + update of the planted frame 3.3e-7 / 1.0e-2 in one piece, 3.3e-7 / 1.6e-7 from the fp32 predicted state
    The asserts only keep the figures in the range where 4 x them is a check (a case that made the restatement itself ill-conditioned
    would widen every device allowance): 1e-6 for the filter's steps, 1e-5 for the gate's solves at cond(S) up to 1e10."""
    fig, recs = oracle_figures()
    for k in sorted(fig):
        print(f"restatement vs float64, {k}: " + (f"{fig[k]:.2e}" if k == "gating" else f"covariance {fig[k][0]:.2e}, mean {fig[k][1]:.2e}"))
    for k, v in fig.items():
        if k == "gating":
            assert v <= 1e-5, v
        else:
            assert v[0] <= 1e-6 and v[1] <= 1e-6, (k, v)
    assert fig["update"][0] >= 1e-8                                  # the measure does see fp32 rounding
    p = base_plan()
    c, m, c2, m2 = step_figures(p, oracle_step(p))
    print(f"restatement vs float64, predict + update of the planted frame: covariance {c:.2e}, mean {m:.2e} in one piece; "
          f"covariance {c2:.2e}, mean {m2:.2e} restarted from the fp32 predicted state")
    assert 1e-8 <= c <= 1e-6 and 1e-8 <= c2 <= 1e-6 and m2 <= 1e-6


def test_every_update_case_is_positive_definite():
    for c in K.CASES:
        _, s = K.project(c.mean, c.cov)
        assert K.is_pd(s), c.name
        assert np.array_equal(s, s.T), c.name                       # the measured block is symmetric in every case, the dense ones included
        if c.trackable:
            _, s = K.project(*K.predict(c.mean, c.cov))
            assert K.is_pd(s) and np.allclose(s, s.T, rtol=1e-12, atol=0), c.name
    names = [c.name for c in K.CASES]
    assert len(K.CASES) == K.GRID + 7 and len(set(names)) == len(names)
    m, p = K.predict(K.CASES[K.GRID + 1].mean, K.CASES[K.GRID + 1].cov)
    assert m[3] <= 0 and K.CASES[K.GRID + 2].mean[3] < 0             # the predicted h <= 0, and the state that enters with h < 0
    q = K.CASES[-1].cov.astype(np.float64)
    assert np.abs(q - q.T).max() > 0 and np.array_equal(q[:4, :4], q[:4, :4].T)
    _, pq = K.predict(K.CASES[-1].mean, q)
    assert np.abs(pq[:4, 4:] - pq[4:, :4].T).max() > 1e-3 * np.abs(pq[:4, 4:]).max()   # still no transposes after a predict


def check_plan(p, gate_tells_apart):
    z = K.xyah32(p.det).astype(np.float64)
    conf = [t for t in range(len(p.mean)) if p.state[t] == 2]
    assert sorted(p.pair) == conf and len(set(p.pair.values())) == len(conf)
    pred = {t: K.predict(p.mean[t], p.cov[t]) for t in range(len(p.mean))}
    for t in conf:
        j = p.pair[t]
        assert K.iou(K.mean_to_tlwh(pred[t][0]), p.det[j].astype(np.float64)) > 0.5, t
        d2 = K.gating(*pred[t], z)
        assert d2[j] < K.CHI2_4 / 2, (t, d2[j])
        app = np.maximum(0.0, 1.0 - p.det_feat.astype(np.float64) @ p.feat[t].astype(np.float64))      # unit vectors
        assert app[j] == 0.0
        others = np.delete(np.arange(len(p.det)), j)
        if gate_tells_apart:
            assert ((app[others] >= 0.9) | (d2[others] > 2 * K.CHI2_4)).all(), t
        else:
            assert (app[others] >= 0.9).all(), t
    for t in range(len(p.mean)):
        if p.state[t] != 2:                                          # a decoy overlaps no detection and holds no gallery
            assert all(K.iou(K.mean_to_tlwh(pred[t][0]), d.astype(np.float64)) == 0 for d in p.det)
    for j in p.new:                                                  # a detection of nobody overlaps no track
        assert all(K.iou(K.mean_to_tlwh(pred[t][0]), p.det[j].astype(np.float64)) == 0 for t in range(len(p.mean)))
    assert not p.new or [round(float(h), 6) for h in sorted(p.det[p.new, 3])] == [round(float(np.float32(h)), 6) for h in sorted(K.NEW_H)]


def test_planted_frame_conditions():
    p = base_plan()
    check_plan(p, gate_tells_apart=False)
    assert len(p.pair) == 28 and (p.state == 1).sum() == 9 and len(p.new) == 3
    assert sum(1 for t in p.pair if t != sorted(p.pair).index(t)) >= 20      # list position != position among the matched for most tracks
    assert [p.pair[t] for t in sorted(p.pair)] != sorted(p.pair.values())    # the detection rows are shuffled


def test_sixteen_drifting_frames_stay_inside_the_gate():
    """The float64 filter fed kf_ref.drift_frames: every planted track finds its detection at less than half the gate in every frame."""
    p = base_plan()
    frames = K.drift_frames(p, 16)
    state = {t: (p.mean[t].astype(np.float64), p.cov[t].astype(np.float64)) for t in p.pair}
    worst = 0.0
    for det in frames:
        z = K.xyah32(det).astype(np.float64)
        for t, j in p.pair.items():
            pm, pp = K.predict(*state[t])
            d2 = float(K.gating(pm, pp, z[j:j + 1])[0])
            worst = max(worst, d2)
            assert d2 < K.CHI2_4 / 2 and det[j, 3] > 0, (t, d2)
            state[t] = K.update(pm, pp, z[j])
    print(f"sixteen drifting frames: largest squared Mahalanobis distance of a planned pair {worst:.2f}")


def test_pipeline_plan_conditions():
    p, xyxy, tlwh = pipeline_plan()
    check_plan(p, gate_tells_apart=True)
    assert all((b[:, 2] < 0).all() and (t[:, 2:] > 0).all() for b, t in zip(xyxy, tlwh))      # left of the image, and still boxes
    pred = [K.mean_to_tlwh(K.predict(p.mean[t], p.cov[t])[0]) for t in range(len(p.mean))]
    for t in range(len(p.mean)):                                     # IoU alone decides: own cost <= 0.25, any other >= 0.5, so swapping k pairs costs k / 4 more at least
        for j in range(len(p.det)):
            cost = 1 - K.iou(pred[t], p.det[j].astype(np.float64))
            assert cost <= 0.25 if p.pair.get(t) == j else cost >= 0.5, (t, j, cost)


def test_bytetrack_lost_track_has_a_height_velocity():
    """kf_ref.bt_boxes through the float64 filter: when object 2 goes missing after frame 4 its track's height velocity is far from 0, so
    zeroing it before the predicts of frames 6 .. 9 (multi_predict on a lost track) moves the predicted height; and every component of
    every update of every object has an innovation."""
    state = {}
    for f in range(1, 13):
        xyxy, who = K.bt_boxes(f)
        z = K.xyah32(np.stack([xyxy[:, 0], xyxy[:, 1], xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1]], 1)).astype(np.float64)
        for k in range(len(K.BT_OBJECTS)):
            if f == 1:
                state[k] = K.initiate(z[who.index(k)])
                continue
            m, p = state[k]
            if k == K.BT_ABSENT and f - 1 in K.BT_GONE:              # lost in the frame before: the height velocity goes
                if f == K.BT_GONE[0] + 1:                            # (from then on it is 0 already)
                    assert abs(m[7]) > 5e-3 * m[3], (f, m[7])
                    assert abs(K.predict(m, p)[0][3] - K.predict(np.append(m[:7], 0.0), p)[0][3]) > 5e-3 * m[3]
                m = np.append(m[:7], 0.0)
            m, p = K.predict(m, p)
            if k in who:
                zz = z[who.index(k)]
                s = np.sqrt(np.diag(K.project(m, p)[1]))
                assert (np.abs(zz - m[:4]) > 1e-3 * s).all(), (f, k)
                assert K.gating(m, p, zz[None])[0] < K.CHI2_4 and K.iou(K.mean_to_tlwh(m), [xyxy[who.index(k)][0], xyxy[who.index(k)][1], *(xyxy[who.index(k)][2:] - xyxy[who.index(k)][:2])]) > 0.5
                m, p = K.update(m, p, zz)
            state[k] = (m, p)


def test_epoch_kernel_fallback_threshold():
    """The derivation beside kf_ref.epoch_arena_floats: at the default capacity of 512 slots and one frame per launch, 193 tracks with
    196 detections leave 13 880 floats of arena, 72 x 193 = 13 896 do not fit; 192 tracks with 195 detections leave 13 888 >= 13 824.
    The device test cannot observe which form a launch took; it stands on this restatement of lds_carve (kernels_trk_dev.hip).  A change
    of the carve -- a new table, another KF_SLOTS, another launch size -- moves the threshold without failing anything: whoever makes one
    has to carry it into kf_ref.epoch_arena_floats, or both device runs take the same form and the fallback goes untested again."""
    assert FALLBACK_T == 193
    assert K.epoch_arena_floats(512, 196, 1) == 13880 and K.epoch_arena_floats(512, 195, 1) == 13888
    for n in (FALLBACK_T - 1, FALLBACK_T):
        p = big_plan(n)
        assert len(p.pair) == len(p.det) == n and len(p.mean) == n + n // 3 <= 512 and np.abs(p.mean[p.state == 2, :2]).max() < 2 ** 15
        check_plan(p, gate_tells_apart=True)
    a, b = big_plan(FALLBACK_T - 1), big_plan(FALLBACK_T)
    assert np.array_equal(a.mean, b.mean[:len(a.mean)]) and np.array_equal(a.cov, b.cov[:len(a.mean)])      # the tracks the two runs share


def test_gating_cells_are_sure():
    fig, recs = oracle_figures()
    sure = K.gate_sure(recs, fig["gating"])
    cells = sum(s.size for s in sure)
    unsure = sum(int((~s).sum()) for s in sure)
    print(f"gating: {cells} cells in {len(recs)} runs, {unsure} within 4 x {fig['gating']:.2e} of CHI2_4")
    assert unsure <= 0.01 * cells
    finite = np.concatenate([r[5][np.isfinite(r[5])] for r in recs])
    assert (finite < K.CHI2_4).mean() > 0.1 and (finite > K.CHI2_4).mean() > 0.1
    near = np.abs(finite / K.CHI2_4 - 1)
    assert ((near < 2e-3) & (finite < K.CHI2_4)).any() and ((near < 2e-3) & (finite > K.CHI2_4)).any()     # (d) the gate is straddled closely
    # (a), (b): +inf whatever is asked; (c): finite on the position block alone
    by = {(r[0], r[1], r[4]): r[5] for r in recs if r[2] == 65 and r[3] == 0}
    assert np.isinf(by[(0, 5, 0)][1]).all() and np.isinf(by[(0, 5, 1)][1]).all()
    assert np.isinf(by[(1, 5, 0)][3]).all() and np.isinf(by[(1, 5, 1)][3]).all()
    assert np.isinf(by[(2, 5, 0)][4]).all() and np.isfinite(by[(2, 5, 1)][4]).all()
    last = len(K.gate_groups()) - 1
    assert np.isinf(by[(last, 1, 0)]).all() and np.isfinite(by[(last, 1, 1)]).all()
    for r, s in zip(recs, sure):                                     # the restatement itself is on the right side of every sure cell
        inf = np.isinf(r[5])
        assert np.array_equal(np.isposinf(r[6]), inf)
        assert np.array_equal((r[6] > K.CHI2_4)[s], (r[5] > K.CHI2_4)[s])


# ------------------------------------------------------------------------------------------------------------------ would a slip show?
class SlippedKF(OracleKF):
    """The restatement's update with one of the slips a hand-copied device update could have, in fp32:
      "ki twice"     row j of the gain replaced by row i in K S K^T (the element (i, j) gets (K S K^T)[i][i])
      "no r33"       the measurement noise missing from S[3][3]
      "transposed"   row j of P H^T read down a column of P (P[a][j] for P[j][a])"""

    def __init__(self, slip):
        self.slip = slip

    def update(self, mean, cov, z):
        out = []
        for m, p, x in zip(mean, cov, z):
            pm, s = O.kf_project(m, p)
            if self.slip == "no r33":
                s = s.copy()
                s[3, 3] = p[3, 3]
            k = np.linalg.solve(s, p[:, :4].T).T.astype(np.float32)
            kj = np.linalg.solve(s, p[:4, :]).T.astype(np.float32) if self.slip == "transposed" else k
            ksk = k @ s @ kj.T
            if self.slip == "ki twice":
                ksk = np.repeat(np.diag(ksk)[:, None], 8, axis=1)
            out.append((m + k @ (x - pm), (p - ksk).astype(np.float32)))
        return np.stack([a for a, _ in out]), np.stack([b for _, b in out])


@pytest.mark.parametrize("slip", ["ki twice", "no r33", "transposed"])
def test_a_slipped_update_is_far_outside_the_allowance(slip):
    """On the form-1 cases and on the planted frame's pairs (what every tracker path is held to).  Without a slip the same code is inside."""
    fig, _ = oracle_figures()
    p = base_plan()
    z = K.xyah32(p.det)

    def figures(kf):
        mean, cov, zz = K.batch(range(len(K.CASES)))
        um, uc = kf.update(mean, cov, zz)
        form1 = max(K.update_errs(um[k], uc[k], mean[k], cov[k], zz[k])[0] for k in range(len(mean)))
        ts = sorted(p.pair)
        pm, pp = OracleKF().predict(p.mean[ts], p.cov[ts])
        um, uc = kf.update(pm, pp, z[[p.pair[t] for t in ts]])
        return form1, step_figures(p, {t: (um[i], uc[i]) for i, t in enumerate(ts)})[2]
    allow_step = K.allow(step_figures(p, oracle_step(p))[2])
    clean = figures(SlippedKF(None))
    assert clean[0] <= K.allow(fig["update"][0]) and clean[1] <= allow_step, clean
    bad = figures(SlippedKF(slip))
    print(f"{slip}: covariance figure {bad[0]:.2e} on the cases (allowed {K.allow(fig['update'][0]):.2e}), {bad[1]:.2e} on the planted frame (allowed {allow_step:.2e})")
    assert bad[0] > 100 * K.allow(fig["update"][0]) and bad[1] > 100 * allow_step
