"""The DeepSORT association kernels cell by cell against float64 (tests/trk_ref.py), at the edges of their tiling: the fused per-frame
kernel (trk_assoc_all_kernel, host path), cosine_min_mfma_kernel (aic_appearance_cost) and the epoch prep kernel with the pair loop of
the epoch kernel (device path).  Galleries of 0 .. 130 rows on every boundary of the 16-row tile, the 64-row grid.y block, the 7 x 16
row batch and the 128-row step; 161, 33, 32 and 1 detections; feature dims with a K tail (4, 30, 68, 70) and without; every gallery
row the strict minimiser of some detection (asserted on the CPU in tests/test_trk_ref.py), and exact copies of detection features
left behind every gallery's live rows, so that a row dropped, misindexed or read past the end moves a cell by far more than the
tolerance."""
import numpy as np
import pytest

import trk_ref as R
from conftest import pkg
from oracle import deepsort_oracle as O

pytestmark = pytest.mark.gpu

DIMS_BOTH = (4, 16, 68, 128, 512)            # 4: only the lane quartet q = 0 has live elements; 68: one vector slice + a 4-element tail
DIMS_HOST = (30, 70)                         # dim % 4 != 0: host path and aic_appearance_cost only (element-guarded loop over all of K)
T = len(R.GLENS)


@pytest.fixture(scope="module")
def seed(gpu):
    """export_arrays() of the host tracker after five featureless frames of the scene: fifteen confirmed tracks with real Kalman states."""
    trk = pkg("core.tracker_core").TrackerCore(nn_budget=R.BUDGET)
    for tlwh, conf, cls in R.seed_frames(pkg("synthetic").Scene(**R.SCENE)):
        trk.predict()
        trk.update_arrays(tlwh, conf, cls, None)
    a = trk.export_arrays()
    assert a["track_id"].tolist() == list(range(1, T + 1)) and (a["state"] == 2).all() and (a["time_since_update"] == 0).all()
    return a


def planted_tracker(seed, case, device=False):
    """A tracker holding the planted state.  First the poison: the same slots with FULL galleries of exact copies of detection features;
    the second import reuses the slots and leaves the rows past glen in place."""
    trk = pkg("core.tracker_core").TrackerCore(nn_budget=R.BUDGET)
    trk.import_state(R.state_dict(seed, case, galleries=np.tile(R.poison_rows(case), (T, 1))))
    trk.import_state(R.state_dict(seed, case))
    if device:
        trk.option("device_assoc", 1)
    return trk


def check_costs(got, ref, mean32, cov32, det, dim, where):
    """The three [T, n] matrices of one frame against float64 (`ref`: R.frame64 of the state before the frame).  Returns the measured
    maxima (appearance error, kernel Mahalanobis deviation, oracle Mahalanobis deviation)."""
    app, maha, iou = got
    nt, n = ref["app"].shape
    assert app.shape == maha.shape == iou.shape == (nt, n), where
    # ---- appearance: (2 dim + 8) * 2^-24, derived in R.app_bound; 1e5 cells exact
    inf = ref["app"] == R.INFTY
    assert np.array_equal(app == np.float32(1e5), inf), where
    err_app = float(np.abs(app.astype(np.float64) - ref["app"])[~inf].max()) if (~inf).any() else 0.0
    # measured on MI355X at 15 x 161 (host path, device path and aic_appearance_cost give the same figure):
    #   dim 4: 1.8e-7 of 9.5e-7   16: 2.3e-7 of 2.4e-6   30: 2.6e-7 of 4.1e-6   68: 3.8e-7 of 8.6e-6   70: 3.7e-7 of 8.8e-6
    #   128: 5.3e-7 of 1.6e-5   512: 1.1e-6 of 6.2e-5
    assert err_app <= R.app_bound(dim), (where, err_app, R.app_bound(dim))
    # ---- 1 - IoU: exact fp32 arithmetic (the NumPy restatement on the fp32-predicted means), and within 1e-6 of float64
    pred = [O.kf_predict(mean32[t], cov32[t]) for t in range(nt)]
    iou32 = O.iou_cost_matrix([O.mean_to_tlwh(m) for m, _ in pred], det)
    assert np.array_equal(iou, iou32), (where, np.abs(iou - iou32).max())
    # (the seed scene is 320 x 320, R.SCENE: at the project's 1280 x 720 coordinates exact fp32 arithmetic is itself 2.3e-6 from float64,
    # so this absolute bound is not exercised there; the bit-equality above is)
    assert np.abs(iou.astype(np.float64) - ref["iou"]).max() <= 1e-6, where
    # ---- squared Mahalanobis distance: within 4 x the fp32 oracle's own deviation from float64 on the same inputs (the kernel's Cholesky
    # and forward solve round in another order than LAPACK's, the two errors may add); metric |x - x64| / max(1, x64)
    xyah = np.stack([O.tlwh_to_xyah(b) for b in det])
    d32 = np.stack([O.kf_gating_distance(m, p, xyah) for m, p in pred])
    scale = np.maximum(1.0, ref["maha"])
    dev_oracle = float((np.abs(d32 - ref["maha"]) / scale).max())
    dev_kernel = float((np.abs(maha.astype(np.float64) - ref["maha"]) / scale).max())
    # measured on MI355X: 15 x 161 planted frame oracle 1.15e-6, kernel 1.34e-6 (allowed 4.6e-6); 15 x 1: 3.5e-7 both; device frames 1 and 2
    # (161 x 33, 33 x 33): oracle 1.5e-6 / 1.8e-6, kernel the same to three digits -- both are led by the fp32 rounding of the shared inputs
    assert dev_kernel <= 4 * dev_oracle, (where, dev_kernel, dev_oracle)
    sure = np.abs(ref["maha"] - R.CHI2_4) > 4 * dev_oracle * scale
    assert (~sure).mean() <= 0.01, where
    assert np.array_equal((maha > np.float32(R.CHI2_4))[sure], (ref["maha"] > R.CHI2_4)[sure]), where
    return err_app, dev_kernel, dev_oracle


@pytest.mark.parametrize("n", [R.N_FULL, 1, 32, 33])
@pytest.mark.parametrize("dim", DIMS_BOTH + DIMS_HOST)
def test_host_costs_against_fp64(seed, dim, n):
    case = R.plant(dim, n)
    det = R.boxes(seed["mean"], seed["cov"], n)
    trk = planted_tracker(seed, case)
    trk.predict()
    trk.update_arrays(det, np.full(n, 0.9, np.float32), np.zeros(n, np.int32), case.det_feat, case.has_feat)
    ref = R.frame64(seed["mean"], seed["cov"], case.galleries, det, case.det_feat, case.has_feat)
    m = check_costs(trk.last_costs(), ref, seed["mean"], seed["cov"], det, dim, (dim, n))
    print(f"host dim {dim} n {n}: appearance {m[0]:.2e} of {R.app_bound(dim):.2e}; Mahalanobis kernel {m[1]:.2e}, oracle {m[2]:.2e}")
    gate_in = ref["maha"] <= R.CHI2_4
    assert n == 1 or (gate_in.any() and (~gate_in).any())
    # ---- state after the frame: unmatched tracks hold the predict bit for bit, matched ones the update within the tolerances of
    # test_kalman_vs_reference_fixture, against float64 predict + update with the match the tracker reported
    after = trk.export_arrays()
    match = dict(trk.last_matches())
    row = {int(tid): k for k, tid in enumerate(after["track_id"])}
    z = R.tlwh_to_xyah64(det)
    assert match and (n > 1 or len(match) < T)
    for i, tid in enumerate(seed["track_id"].tolist()):
        k = row[tid]
        if tid in match:
            m64, p64 = R.update64(ref["mean"][i], ref["cov"][i], z[match[tid]])
            assert np.allclose(after["mean"][k], m64, rtol=1e-5, atol=1e-3), (dim, n, tid)
            assert np.allclose(after["cov"][k], p64, rtol=1e-4, atol=1e-4), (dim, n, tid)
        else:
            pm, pc = O.kf_predict(seed["mean"][i], seed["cov"][i])
            assert np.array_equal(after["mean"][k], pm) and np.array_equal(after["cov"][k], pc), (dim, n, tid)


@pytest.mark.parametrize("dim", DIMS_BOTH + DIMS_HOST)
def test_appearance_cost_entry_against_fp64(gpu, lib, dim):
    """cosine_min_mfma_kernel through aic_appearance_cost at gmax = 130: grid.y = 3, the blocks of a track meet through atomicMin."""
    case = R.plant(dim)
    ref, _, _ = R.app64(case.galleries, case.det_feat, case.has_feat)
    inf = ref == R.INFTY
    M, D = pkg("core.matching"), pkg("core.detection").Detection

    class Trk:
        def __init__(self, rows):
            self.features = list(rows)
    tracks = [Trk(g) for g in case.galleries]
    dets = [D(np.array([0, 0, 10, 20], np.float32), 0.9, "person", case.det_feat[j] if case.has_feat[j] else None) for j in range(case.n)]
    via_metric = M.appearance_cost_metric(tracks, dets, list(range(T)), list(range(case.n)))
    # the C entry itself, with copies of detection features behind every gallery's live rows
    direct = np.empty((T, case.n), np.float32)
    gal = case.padded(fill=R.poison_rows(case))
    lib.call("aic_appearance_cost", 0, lib.ptr(gal), lib.ptr(case.glen), T, R.BUDGET, dim, lib.ptr(case.det_feat), lib.ptr(case.has_feat),
             case.n, lib.ptr(direct))
    for name, got in (("metric", via_metric), ("direct", direct)):
        assert got.shape == ref.shape and np.array_equal(got == np.float32(1e5), inf), (name, dim)
        err = float(np.abs(got.astype(np.float64) - ref)[~inf].max())
        print(f"entry {name} dim {dim}: appearance {err:.2e} of {R.app_bound(dim):.2e}")
        assert err <= R.app_bound(dim), (name, dim, err)
    assert np.array_equal(via_metric, direct)


def test_device_path_refuses_dim_30(seed):
    trk = planted_tracker(seed, R.plant(30, 1))
    with pytest.raises(pkg("_lib").AicError):
        trk.option("device_assoc", 1)


@pytest.mark.parametrize("dim", DIMS_BOTH)
def test_device_costs_against_fp64(seed, dim):
    """Three consecutive frames on the device path, one frame per call: the planted frame (161 detections), then two frames of 33
    detections that look like the newest, the oldest and other rows of the galleries as exported before the frame.  The full gallery
    evicts in frame 1, so from frame 2 on its ring is read from a head != 0.  Every frame: the three matrices against float64 of the state
    exported before it, and bit for bit against a host-path tracker fed the same frames (budget 130)."""
    case = R.plant(dim)
    dev, host = planted_tracker(seed, case, device=True), planted_tracker(seed, case)
    evicted = 0
    for f in range(3):
        st = dev.export_state()
        gal = R.split_galleries(st["galleries"], st["gallery_len"])
        if f == 0:
            det, feat, has = R.boxes(seed["mean"], seed["cov"], case.n), case.det_feat, case.has_feat
            assert all(np.array_equal(a, b) for a, b in zip(gal, case.galleries))
        else:
            assert st["track_id"][:T].tolist() == seed["track_id"].tolist()
            det = R.boxes(st["mean"][:T], st["cov"][:T], 33, seed=f)
            feat, has = R.follow_up(gal[:T], 33, f, dim)
        n = len(det)
        ref = R.frame64(st["mean"], st["cov"], gal, det, feat, has)
        for trk in (dev, host):
            trk.predict()
            trk.update_arrays(det, np.full(n, 0.9, np.float32), np.zeros(n, np.int32), feat, has)
        got, got_host = dev.last_costs(), host.last_costs()
        m = check_costs(got, ref, st["mean"], st["cov"], det, dim, (dim, f))
        print(f"device dim {dim} frame {f} ({len(st['mean'])} x {n}): appearance {m[0]:.2e} of {R.app_bound(dim):.2e}; "
              f"Mahalanobis kernel {m[1]:.2e}, oracle {m[2]:.2e}")
        for a, b in zip(got, got_host):
            assert a.shape == b.shape and np.array_equal(a, b), (dim, f)
        assert sorted(dev.last_matches()) == sorted(host.last_matches()), (dim, f)
        full = [int(tid) for tid, g in zip(st["track_id"], st["gallery_len"]) if g == R.BUDGET]
        evicted += sum(1 for tid, j in dev.last_matches() if tid in full and has[j])
    assert evicted >= 2                                              # a full gallery was matched (and evicted) before a later frame read it


def test_sixteen_frame_epoch_equals_single_frames(seed):
    """Host path, device path frame by frame, and ONE sixteen-frame epoch (update_batch) from the planted state at dim 68, on the scene's
    next sixteen frames with identity features: appearance matching happens (every gallery holds its identity's row), the galleries of
    130 and 129 rows evict inside the epoch, so the prep kernel's suffix minima are read across its batch boundary at row 112.
    The costs of a multi-frame epoch are not exported, so one match is made to hang on them: the four elements of the K tail are scaled
    to carry most of every feature vector, and the identity of the track with the EMPTY gallery goes undetected for two frames of the
    epoch.  It comes back with time_since_update = 3, out of the IoU stage's reach, and all its gallery is rows the epoch appended: only
    the epoch's detection-to-detection distances (cos_tile, tail included) can re-identify it."""
    dim, k = 68, 16
    syn = pkg("synthetic")
    sc = syn.Scene(**{**R.SCENE, "gaps": [(0, 10, 11)]})             # the seed run ended at frame 4: the same tracks

    def features(ids, f):
        x = syn.identity_features(ids, f, dim=dim, noise=0.03)
        x[:, 64:] *= 8                                               # 80 % of the energy in the element-guarded tail
        return x
    case = R.own_rows(R.plant(dim), features(np.arange(T), 4))
    host, dev, batch = planted_tracker(seed, case), planted_tracker(seed, case, device=True), planted_tracker(seed, case)
    batch.option("epoch_frames", k)                                   # no device_assoc option: update_batch always runs the epoch kernels
    frames = []
    for f in range(5, 5 + k):
        b, conf, cls, ids = sc.detections(f)
        tlwh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float32)
        frames.append((tlwh, conf, cls, features(ids, f), np.ones(len(ids), np.uint8)))
    res = batch.update_batch(frames)
    by_appearance, back = 0, None
    for i, fr in enumerate(frames):
        tsu = dict(zip(host.export_arrays()["track_id"].tolist(), host.export_arrays()["time_since_update"].tolist()))
        for trk in (host, dev):
            trk.predict()
            trk.update_arrays(*fr)
        rows_h, conf_h = host.outputs()
        rows_d, conf_d = dev.outputs()
        rows_b, conf_b, match_b = res[i]
        assert np.array_equal(rows_h, rows_d) and np.array_equal(rows_h, rows_b), i
        assert np.array_equal(conf_h, conf_d) and np.array_equal(conf_h, conf_b), i
        assert sorted(host.last_matches()) == sorted(dev.last_matches()) == sorted(match_b), i
        app = host.last_costs()[0]
        by_appearance += sum(1 for tid, j in host.last_matches() if tid <= T and app[tid - 1, j] <= 0.2)
        for tid, j in host.last_matches():
            if tid == 1 and tsu[1] >= 2:
                back = (5 + i, float(app[0, j]))
    assert back is not None and back[0] == 12 and back[1] <= 0.2, back   # the empty-gallery track came back through the epoch's own rows
    assert by_appearance >= T * k // 2                               # appearance matching really happens: most matches pass the cosine threshold
    sh, sd, sb = host.export_state(), dev.export_state(), batch.export_state()
    assert (sh["gallery_len"][T - 2:T] == R.BUDGET).all() and (sh["hits"][T - 2:T] >= seed["hits"][T - 2:] + 3).all()   # 129 and 130 rows: evicted inside the epoch
    for other in (sd, sb):
        for key in ("track_id", "state", "hits", "age", "time_since_update", "cls", "gallery_len", "mean", "cov", "galleries"):
            assert np.array_equal(sh[key], other[key]), key
        assert sh["next_track_id"] == other["next_track_id"]
