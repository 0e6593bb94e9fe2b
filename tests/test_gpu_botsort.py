"""BoT-SORT on the device (csrc/kernels_botsort.hip) against the NumPy oracle (tests/botsort_oracle.py), frame by frame: rows, ids,
classes, scores, states, frames, list order, has_feat, the Kalman state AND the smoothed features are np.array_equal (the oracle states
every sum in the kernel's order, so there is no tolerance and no "not guaranteed" caveat)."""
import numpy as np
import pytest

from botsort_oracle import BoTSORT as Oracle
from conftest import pkg
from test_botsort_oracle import CROSSING, crossing_scene, ids_by_position

pytestmark = pytest.mark.gpu

KEYS = ("track_id", "state", "is_activated", "start_frame", "end_frame", "cls", "score", "has_feat", "mean", "cov", "smooth_feat")


def scene(n=30, frames=300, seed=3):
    """The occlusion scene of tests/test_gpu_bytetrack.py."""
    syn = pkg("synthetic")
    rng = np.random.default_rng(seed)
    gaps = [(int(t), int(a), int(a + rng.integers(3, 40))) for t, a in zip(rng.integers(0, n, n // 2), rng.integers(5, frames - 50, n // 2))]
    births = {int(t): int(f) for t, f in zip(rng.choice(n, n // 5, replace=False), rng.integers(1, frames // 2, n // 5))}
    return syn.Scene(seed=seed, n_targets=n, gaps=gaps, births=births, conf_range=(0.05, 0.95), jitter=1.5, shuffle=True)


def frames_of(sc, frames, feats=True, warps=None, dim=512):
    """Per frame (boxes, scores, cls, raw features or None, warp or None): the features are NOT unit length (the device normalises)."""
    syn = pkg("synthetic")
    out = []
    for f in range(frames):
        b, c, k, ident = sc.detections(f)
        k = (k + (np.arange(len(k)) % 3)).astype(np.int32)       # a few classes: cls follows the last matched detection
        ft = (syn.identity_features(ident, f, dim=dim, seed=7) * np.float32(1.5 + 0.01 * f)).astype(np.float32) if feats else None
        out.append((b, c, k, ft, None if warps is None else warps[f]))
    return out


def compare_export(dev, ora):
    e, o = dev.export(), ora.export(dev.feature_dim)
    assert e["n_tracked"] == o["n_tracked"]
    for key in KEYS:
        assert np.array_equal(e[key], o[key]), (key, np.abs(e[key].astype(np.float64) - o[key]).max())
    c = dev.counters()
    assert c["n_appearance"] == ora.n_appearance


def run_pair(dets, chunk, epoch_frames=0, lsap_fast=1, valid=None, **kw):
    dev = pkg("botsort").BoTSORT(**kw)
    dev.option("epoch_frames", epoch_frames)
    dev.option("lsap_fast", lsap_fast)
    ora = Oracle(**{k: v for k, v in kw.items() if k not in ("max_tracks", "feature_dim")})
    f = 0
    while f < len(dets):
        part = dets[f:f + chunk]
        vpart = None if valid is None else valid[f:f + chunk]
        got = dev.update_batch_arrays([p + (None if vpart is None else vpart[i],) for i, p in enumerate(part)])
        for i, ((b, c, k, ft, w), (rows, conf)) in enumerate(zip(part, got)):
            if ft is not None and vpart is not None:
                ft = [x if v else None for x, v in zip(ft, vpart[i])]
            want_rows, want_conf = Oracle.rows(ora.update_xyxy(b, c, k, ft, w))
            assert np.array_equal(rows, want_rows), (f, rows, want_rows)
            assert np.array_equal(conf, want_conf), f
            f += 1
    compare_export(dev, ora)
    return dev, ora


@pytest.mark.parametrize("epoch_frames,lsap_fast,with_reid", [(1, 1, 1), (16, 1, 1), (16, 0, 1), (1, 0, 0), (16, 1, 0)])
def test_device_matches_oracle(epoch_frames, lsap_fast, with_reid):
    dets = frames_of(scene(), 300)
    dev, ora = run_pair(dets, chunk=37, epoch_frames=epoch_frames, lsap_fast=lsap_fast, with_reid=bool(with_reid))
    c = dev.counters()
    has = dev.export()["has_feat"]
    assert len(has) > 0 and (has.all() if with_reid else not has.any())
    if with_reid:
        assert c["n_appearance"] > 0, "the scene does not exercise the appearance term"
    else:
        assert c["n_appearance"] == 0
    assert (c["n_fast"] > 0) == bool(lsap_fast) and (lsap_fast or c["n_lsap"] > 0)


def test_crossing_scene_on_the_device():
    mm = pkg("mot_metrics")
    syn = pkg("synthetic")
    dets, gt = crossing_scene(**CROSSING)
    for with_reid, want in ((True, [1, 2]), (False, [2, 1])):
        dev = pkg("botsort").BoTSORT(with_reid=with_reid)
        ora = Oracle(with_reid=with_reid)
        outs = []
        for f, (b, s, c, ident) in enumerate(dets):
            ft = syn.identity_features(ident, f, dim=512, seed=5)
            got = dev.update(b, s, c, ft)
            rows, _ = Oracle.rows(ora.update_xyxy(b, s, c, ft))
            assert [t[:5] for t in got] == [tuple(r[:5]) for r in rows.tolist()], f
            outs.append(got)
        assert ids_by_position(outs[-1]) == want
        assert mm.evaluate(gt, outs)["idsw"] == (0 if with_reid else 2)
        compare_export(dev, ora)


def test_crowd_exercises_the_large_lsap_and_the_matrix_in_hbm():
    sc = pkg("synthetic").Scene(seed=21, n_targets=150, conf_range=(0.05, 0.95), jitter=2.0, shuffle=True,
                                w_range=(30.0, 50.0), h_range=(80.0, 120.0))
    dets = frames_of(sc, 40)
    dev, _ = run_pair(dets, chunk=16, lsap_fast=0)
    assert len(dev.export()["track_id"]) > 100
    c = dev.counters()
    assert c["max_side"] > 128 and c["n_lsap"] > 0 and c["n_fast"] == 0 and c["n_appearance"] > 0


def test_camera_motion_warps():
    n = 40
    th = 0.004 * np.sin(np.arange(n) * 0.7)
    warps = [np.array([[np.cos(t), -np.sin(t), 1.5 * np.cos(i)], [np.sin(t), np.cos(t), -0.75 * np.sin(i)]], np.float32)
             for i, t in enumerate(th)]
    warps[5] = None                                               # a frame without an estimate: the identity
    dets = frames_of(scene(n=12, frames=80, seed=9), n, warps=warps)
    dev, ora = run_pair(dets, chunk=7)
    dev0, _ = run_pair(frames_of(scene(n=12, frames=80, seed=9), n), chunk=7)
    assert not np.array_equal(dev.export()["cov"], dev0.export()["cov"])      # the warp did something


def test_no_features_equals_with_reid_0_and_invalid_rows():
    sc = scene(n=12, frames=80, seed=9)
    a, _ = run_pair(frames_of(sc, 50, feats=False), chunk=16, with_reid=True)
    b, _ = run_pair(frames_of(sc, 50), chunk=16, with_reid=False)
    ea, eb = a.export(), b.export()
    for key in KEYS:
        assert np.array_equal(ea[key], eb[key]), key
    assert not ea["has_feat"].any()
    # every third row of a frame has no feature (an empty crop): it matches by IoU alone and leaves the track's feature alone
    dets = frames_of(sc, 50)
    valid = [(np.arange(len(d[0])) % 3 != 1).astype(np.int32) for d in dets]
    dev, _ = run_pair(dets, chunk=16, valid=valid)
    assert dev.counters()["n_appearance"] > 0
    # a small feature dimension (one partial 256-element pass)
    run_pair(frames_of(sc, 30, dim=64), chunk=16, feature_dim=64)


def test_update_tuples_and_empty_frames():
    dets = frames_of(scene(n=12, frames=80, seed=9), 20)
    dev = pkg("botsort").BoTSORT()
    ora = Oracle()
    for b, c, k, ft, _ in dets:
        got = dev.update(b, c, k, ft)
        rows, conf = Oracle.rows(ora.update_xyxy(b, c, k, ft))
        assert [t[:5] for t in got] == [tuple(r[:5]) for r in rows.tolist()] and [t[6] for t in got] == conf.tolist()
    out = dev.update(np.array([]), np.array([]), np.array([]))          # empty inputs are accepted
    assert isinstance(out, list) and dev.frame_id == 21
    dev.close()


def test_capacity_error_raises():
    L = pkg("_lib")
    sc = pkg("synthetic").Scene(seed=4, n_targets=20, conf_range=(0.8, 0.95))
    dev = pkg("botsort").BoTSORT(max_tracks=8)
    with pytest.raises(L.AicError) as ei:
        dev.update_batch_arrays(frames_of(sc, 2))
    assert ei.value.code == L.ERR_CAPACITY
    with pytest.raises(L.AicError):                            # the tracker refuses further updates, and has no state to export
        dev.update_batch_arrays(frames_of(sc, 1))
    with pytest.raises(L.AicError):
        dev.export()
    # more than 512 detections in a frame, and an extended problem beyond 512
    dev = pkg("botsort").BoTSORT()
    b = np.tile(np.array([[0, 0, 10, 10]], np.float32), (513, 1))
    with pytest.raises(L.AicError) as ei:
        dev.update(b, np.full(513, 0.9, np.float32), np.zeros(513, np.int32))
    assert ei.value.code == L.ERR_CAPACITY
    dev = pkg("botsort").BoTSORT()
    xs = np.arange(300, dtype=np.float32) * 4
    b = np.stack([xs % 1200, (xs // 1200) * 30, xs % 1200 + 3, (xs // 1200) * 30 + 3], 1).astype(np.float32)
    dev.update(b, np.full(300, 0.9, np.float32), np.zeros(300, np.int32))        # 300 tracks
    with pytest.raises(L.AicError) as ei:                       # pool 300 + 300 high detections far away: side 600
        dev.update(b + 5000, np.full(300, 0.9, np.float32), np.zeros(300, np.int32))
    assert ei.value.code == L.ERR_CAPACITY


# ---------------------------------------------------------------------------------------------------- the BoT-SORT pipeline
from conftest import ROOT  # noqa: E402


def _pipe(ypath, rpath, n, batch, inject, **kw):
    TP = pkg("pipeline").TrackingPipeline
    pipe = TP(ypath, rpath, (720, 1280), batch=batch, ring_frames=n, max_persons=128, dtype="fp16", inject=inject, tracker="botsort", **kw)
    pipe.option("taper", 0)                                     # one launch group: group_embeddings() then holds every crop of the run
    return pipe


def _oracle_rows_with(fed, emb, per, **kw):
    """The oracle on the detections handed to the tracker and the pipeline's OWN embeddings (raw rows; the oracle normalises them in the
    order the device does)."""
    assert per.tolist() == [len(x[0]) for x in fed]
    ora, out, r0 = Oracle(**kw), [], 0
    for (b, c, k), m in zip(fed, per):
        out.append(Oracle.rows(ora.update_xyxy(b, c, k, emb[r0:r0 + m] if m else None)))
        r0 += m
    return out, ora


def _same(tracks, want):
    for f, (got, (rows, conf)) in enumerate(zip(tracks, want)):
        assert [tuple(t[:5]) for t in got] == [tuple(r[:5]) for r in rows.tolist()], f
        assert [t[6] for t in got] == conf.tolist(), f


def test_pipeline_inject_against_oracle():
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    n = 48
    sc = scene(n=30, frames=n + 60, seed=5)
    planted = [sc.detections(f)[:3] for f in range(n)]
    pipe = _pipe(ypath, rpath, n, n, True)
    assert pipe.reid is not None and pipe.tracker_core is None
    pipe.upload(0, sc.render_batch(0, n))
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    emb, per = pipe.group_embeddings()
    assert emb.shape == (sum(len(p[0]) for p in planted), 512)
    want, ora = _oracle_rows_with(planted, emb, per)
    _same(tracks, want)
    assert sum(len(t) for t in tracks) > 10 * n and ora.n_appearance > 0
    last = pipe.last_embeddings()
    assert np.array_equal(last, emb[len(emb) - per[-1]:])
    pipe.close()


def test_pipeline_own_detections_against_oracle():
    cfg = pkg("config")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    n = 32
    sc = pkg("synthetic").Scene(seed=11, n_targets=30)
    pipe = _pipe(ypath, rpath, n, n, False)
    assert abs(pipe.params.conf_thresh - 0.1) < 1e-7           # the detector hands over everything above track_low_thresh
    pipe.upload(0, sc.render_batch(0, n))
    tracks, dets = pipe.run(0, n, want_dets=True)
    emb, per = pipe.group_embeddings()
    lut = np.array([nm in cfg.CLASSES_TO_TRACK for nm in cfg.CLASSES])
    fed = []
    for b, s, l in dets:
        keep = (l >= 0) & (l < len(lut)) & lut[np.clip(l, 0, len(lut) - 1)] & (s > np.float32(0.1))
        fed.append((b[keep], s[keep], l[keep]))
    assert sum(len(x[0]) for x in fed) > 20 * n
    want, _ = _oracle_rows_with(fed, emb, per)
    _same(tracks, want)
    pipe.close()


def test_pipeline_rejects_deepsort_only_calls():
    import ctypes as C
    L = pkg("_lib")
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = _pipe(ypath, rpath, 16, 16, True)
    th = C.c_void_p()
    assert L.load().aic_pipeline_tracker(pipe._h, C.byref(th)) == L.ERR_INVALID
    assert "BoT-SORT" in L.load().aic_last_error().decode()
    for key in ("device_assoc", "device_assoc_limit", "device_filter"):
        assert L.load().aic_pipeline_option(pipe._h, key.encode(), 1) == L.ERR_INVALID, key
    assert L.load().aic_pipeline_exchange_enable(pipe._h, None, None, 0, 0) == L.ERR_INVALID
    pipe.option("dual_lane_frames", 0)
    pipe.option("in_flight", 2)
    pipe.close()


def test_other_trackers_after_a_botsort_pipeline():
    """A DeepSORT, a ByteTrack and an OC-SORT pipeline built in the same process after a BoT-SORT one give the rows they give without it."""
    import torch
    from bytetrack_oracle import BYTETracker as BtOracle
    from ocsort_oracle import OCSort as OcOracle
    from oracle import deepsort_oracle as O, image_oracle as I, nets_oracle as N
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP = pkg("pipeline").TrackingPipeline
    n = 16
    sc = scene(n=10, frames=n + 60, seed=5)
    planted = [sc.detections(f)[:3] for f in range(n)]
    frames = sc.render_batch(0, n)
    pipe = _pipe(ypath, rpath, n, n, True)
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    _same(tracks, _oracle_rows_with(planted, *pipe.group_embeddings())[0])
    pipe.close()
    for kind, make in (("bytetrack", BtOracle), ("ocsort", OcOracle)):
        pipe = TP(ypath, None, (720, 1280), batch=8, ring_frames=n, max_persons=128, dtype="fp16", inject=True, tracker=kind)
        pipe.upload(0, frames)
        pipe.inject(0, planted)
        o = make()
        _same(pipe.run(0, n)[0], [make.rows(o.update_xyxy(b, c, k)) for b, c, k in planted])
        pipe.close()
    sc = pkg("synthetic").Scene(seed=5, n_targets=6)             # DeepSORT on the scene of smoke()
    n = 8
    planted = [sc.detections(f)[:3] for f in range(n)]
    frames = sc.render_batch(0, n)
    pipe = TP(ypath, rpath, (720, 1280), batch=4, ring_frames=n, max_persons=8, dtype="fp16", inject=True)
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    eo = N.EngineOracle(rpath)
    trk = O.OracleTracker()
    for f in range(n):
        boxes, conf, _ = planted[f]
        crops, valid = I.crops_to_batch(frames[f], boxes)
        emb = eo.run(torch.from_numpy(crops))[eo.outputs[0][0]][:, :, 0, 0].numpy()
        tlwh = np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], 1)
        trk.predict()
        trk.update(list(tlwh), list(conf), ["person"] * len(boxes), [emb[i] if valid[i] else None for i in range(len(boxes))])
        assert [t[4] for t in tracks[f]] == [t[4] for t in trk.output_tuples()], f
    pipe.close()


@pytest.mark.parametrize("batch", [1, 16])
def test_cli_botsort(tmp_path, batch):
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    rc = pkg("cli").main(["--input", "synthetic:640x360:6:24", "--output_dir", str(tmp_path), "--yolo_engine", ypath,
                          "--reid_engine", rpath, "--tracker", "botsort", "--batch", str(batch)])
    assert rc == 0
    out = list(tmp_path.glob("*.jsonl"))
    assert len(out) == 1 and len(out[0].read_text().splitlines()) == 24
