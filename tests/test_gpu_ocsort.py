"""OC-SORT on the device (csrc/kernels_ocsort.hip) against the NumPy oracle (tests/ocsort_oracle.py): ids, rows, class, score, every
counter and the exported filter state are np.array_equal frame by frame (the oracle's 7x7 products are the kernel's ordered fp32
sums, so no tolerance is needed)."""
import numpy as np
import pytest

from conftest import ROOT, pkg
from ocsort_oracle import OCSort as Oracle
from test_gpu_bytetrack import frames_of

pytestmark = pytest.mark.gpu


def scene(n=30, frames=300, seed=4):
    """The scene of test_gpu_bytetrack.py; seed 4, with which the oracle alone reaches ORU replays (longest gap 28), the OCR stage
    (4 pairs), the read-off (25 problems) and the LSAP (278): tests/test_ocsort_oracle.py::test_scene_reaches_every_path."""
    syn = pkg("synthetic")
    rng = np.random.default_rng(seed)
    gaps = [(int(t), int(a), int(a + rng.integers(3, 40))) for t, a in zip(rng.integers(0, n, n // 2), rng.integers(5, frames - 50, n // 2))]
    births = {int(t): int(f) for t, f in zip(rng.choice(n, n // 5, replace=False), rng.integers(1, frames // 2, n // 5))}
    return syn.Scene(seed=seed, n_targets=n, gaps=gaps, births=births, conf_range=(0.05, 0.95), jitter=1.5, shuffle=True)


def compare_export(dev, ora):
    e, o = dev.export(), ora.export()
    for key in pkg("ocsort").OCSort.KEYS:
        assert e[key].shape == o[key].shape and np.array_equal(e[key], o[key]), (key, e[key], o[key])


def run_pair(dets, chunk, epoch_frames=0, lsap_fast=1, **kw):
    dev = pkg("ocsort").OCSort(**kw)
    dev.option("epoch_frames", epoch_frames)
    dev.option("lsap_fast", lsap_fast)
    ora = Oracle(lsap_fast=bool(lsap_fast), **{k: v for k, v in kw.items() if k != "max_tracks"})
    f = 0
    while f < len(dets):
        part = dets[f:f + chunk]
        got = dev.update_batch_arrays(part)
        for (b, c, k), (rows, conf) in zip(part, got):
            want_rows, want_conf = Oracle.rows(ora.update_xyxy(b, c, k))
            assert np.array_equal(rows, want_rows), (f, rows, want_rows)
            assert np.array_equal(conf, want_conf), f
            f += 1
    compare_export(dev, ora)
    c = dev.counters()
    assert c == {k: ora.stats[k] for k in c}, (c, ora.stats)
    return dev


@pytest.mark.parametrize("epoch_frames,lsap_fast,use_byte", [(1, 1, False), (16, 1, False), (16, 0, False), (1, 0, True), (16, 1, True)])
def test_device_matches_oracle(epoch_frames, lsap_fast, use_byte):
    dets = frames_of(scene(), 300)
    dev = run_pair(dets, chunk=37, epoch_frames=epoch_frames, lsap_fast=lsap_fast, use_byte=use_byte)
    c = dev.counters()
    print(c)
    assert c["n_oru"] > 0 and c["max_gap"] > 3 and c["n_lsap"] > 0
    assert (c["n_fast"] > 0) == bool(lsap_fast)
    if use_byte:
        assert c["n_byte"] > 0
    else:
        assert c["n_ocr"] > 0


def test_update_tuples_and_export_after_single_frames():
    dets = frames_of(scene(n=12, frames=80, seed=9), 40)
    dev = pkg("ocsort").OCSort()
    ora = Oracle()
    for b, c, k in dets:
        got = dev.update(b, c, k)
        rows, conf = Oracle.rows(ora.update_xyxy(b, c, k))
        assert [t[4] for t in got] == rows[:, 4].tolist()
        assert [t[:4] for t in got] == [tuple(r) for r in rows[:, :4].tolist()]
        compare_export(dev, ora)
    out = dev.update(np.array([]), np.array([]), np.array([]))          # empty inputs are accepted
    assert isinstance(out, list) and dev.frame_count == 41


def test_other_parameters():
    dets = frames_of(scene(n=20, frames=120, seed=6), 120)
    run_pair(dets, chunk=16, det_thresh=0.5, max_age=10, min_hits=2, iou_threshold=0.25, delta_t=5, inertia=0.4, first_track_id=100)
    run_pair(dets, chunk=16, delta_t=1, inertia=0.0)


def test_crowd_exercises_the_large_lsap():
    # 150 persons: both sides of stage 1 exceed 128 (lsap_wave) and the matrix (> 91 x 91) lives in HBM
    sc = pkg("synthetic").Scene(seed=21, n_targets=150, conf_range=(0.3, 0.95), jitter=2.0, shuffle=True,
                                w_range=(30.0, 50.0), h_range=(80.0, 120.0))
    dets = frames_of(sc, 40)
    dev = run_pair(dets, chunk=16, lsap_fast=0)
    assert len(dev.export()["track_id"]) > 100
    c = dev.counters()
    assert c["max_side"] > 128 and c["n_lsap"] > 0 and c["n_fast"] == 0


def test_capacity_error_raises():
    L = pkg("_lib")
    sc = pkg("synthetic").Scene(seed=4, n_targets=20, conf_range=(0.8, 0.95))
    dev = pkg("ocsort").OCSort(max_tracks=8)
    with pytest.raises(L.AicError) as ei:
        dev.update_batch_arrays(frames_of(sc, 2))
    assert ei.value.code == L.ERR_CAPACITY
    with pytest.raises(L.AicError):                            # the tracker refuses further updates, and has no state to export
        dev.update_batch_arrays(frames_of(sc, 1))
    with pytest.raises(L.AicError):
        dev.export()
    dev = pkg("ocsort").OCSort()                               # more than 512 detections in a frame
    b = np.tile(np.array([[0, 0, 10, 10]], np.float32), (513, 1))
    with pytest.raises(L.AicError) as ei:
        dev.update(b, np.full(513, 0.9, np.float32), np.zeros(513, np.int32))
    assert ei.value.code == L.ERR_CAPACITY


# ---------------------------------------------------------------------------------------------------- the OC-SORT pipeline
def _pipe(ypath, n, batch, inject, tracker="ocsort", **kw):
    TP = pkg("pipeline").TrackingPipeline
    return TP(ypath, None, (720, 1280), batch=batch, ring_frames=n, max_persons=128, dtype="fp16", inject=inject, tracker=tracker, **kw)


def _oracle_rows(frames_dets, passes=1, **kw):
    ora = Oracle(**kw)
    out = []
    for _ in range(passes):
        out = [Oracle.rows(ora.update_xyxy(b, c, k)) for b, c, k in frames_dets]
    return out


def _same(tracks, want):
    for f, (got, (rows, conf)) in enumerate(zip(tracks, want)):
        assert [tuple(t[:5]) for t in got] == [tuple(r[:5]) for r in rows.tolist()], f
        assert [t[6] for t in got] == conf.tolist(), f


def test_pipeline_inject_against_oracle():
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    n = 48
    sc = scene(n=30, frames=n + 60, seed=5)
    planted = [sc.detections(f)[:3] for f in range(n)]
    frames = sc.render_batch(0, n)
    pipe = _pipe(ypath, n, 16, True)
    assert pipe.reid is None and pipe.tracker_core is None and abs(pipe.params.conf_thresh - 0.6) < 1e-7
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    assert sum(len(t) for t in tracks) > 0                     # not vacuous: tracks are output
    _same(tracks, _oracle_rows(planted))
    pipe.close()
    pipe = _pipe(ypath, n, 16, True, use_byte=True, min_hits=2)
    assert abs(pipe.params.conf_thresh - 0.1) < 1e-7
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    _same(tracks, _oracle_rows(planted, use_byte=True, min_hits=2))
    pipe.close()


def test_pipeline_own_detections_against_oracle():
    cfg = pkg("config")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    n = 32
    sc = pkg("synthetic").Scene(seed=11, n_targets=30)
    pipe = _pipe(ypath, n, 16, False, det_thresh=0.3, conf_thresh=0.1)
    pipe.upload(0, sc.render_batch(0, n))
    tracks, dets = pipe.run(0, n, want_dets=True)
    lut = np.array([nm in cfg.CLASSES_TO_TRACK for nm in cfg.CLASSES])
    fed = []
    for b, s, l in dets:
        keep = (l >= 0) & (l < len(lut)) & lut[np.clip(l, 0, len(lut) - 1)]
        fed.append((b[keep], s[keep], l[keep]))
    assert sum(len(x[0]) for x in fed) > 20 * n and sum(len(t) for t in tracks) > 0
    _same(tracks, _oracle_rows(fed, det_thresh=0.3))
    pipe.close()


def test_pipeline_rejects_deepsort_only_calls():
    import ctypes as C
    L = pkg("_lib")
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = _pipe(ypath, 16, 16, True)
    th = C.c_void_p()
    assert L.load().aic_pipeline_tracker(pipe._h, C.byref(th)) == L.ERR_INVALID
    assert "OC-SORT" in L.load().aic_last_error().decode()
    for key in ("device_assoc", "device_assoc_limit", "device_filter"):
        assert L.load().aic_pipeline_option(pipe._h, key.encode(), 1) == L.ERR_INVALID, key
    pipe.option("dual_lane_frames", 0)
    pipe.option("in_flight", 2)
    with pytest.raises(L.AicError):
        pipe.last_embeddings()
    pipe.close()


def test_other_trackers_after_an_ocsort_pipeline(engines):
    """The shared stage B call site: a ByteTrack and a DeepSORT pipeline built in the same process after an OC-SORT one still give their
    oracles' rows."""
    import torch
    from bytetrack_oracle import BYTETracker as BtOracle
    from oracle import deepsort_oracle as O, image_oracle as I, nets_oracle as N
    ypath, rpath = engines
    n = 16
    sc = scene(n=10, frames=n + 60, seed=5)
    planted = [sc.detections(f)[:3] for f in range(n)]
    frames = sc.render_batch(0, n)
    pipe = _pipe(ypath, n, 8, True)
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    _same(pipe.run(0, n)[0], _oracle_rows(planted))
    pipe.close()
    pipe = _pipe(ypath, n, 8, True, tracker="bytetrack")
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    bo = BtOracle()
    _same(pipe.run(0, n)[0], [BtOracle.rows(bo.update_xyxy(b, c, k)) for b, c, k in planted])
    pipe.close()
    # DeepSORT on the scene of smoke() (every score above DeepSORT's min_confidence, which the oracle chain below does not apply)
    sc = pkg("synthetic").Scene(seed=5, n_targets=6)
    n = 8
    planted = [sc.detections(f)[:3] for f in range(n)]
    frames = sc.render_batch(0, n)
    TP = pkg("pipeline").TrackingPipeline
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
def test_cli_ocsort(tmp_path, batch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    rc = pkg("cli").main(["--input", "synthetic:640x360:6:24", "--output_dir", str(tmp_path), "--yolo_engine", ypath,
                          "--tracker", "ocsort", "--batch", str(batch)])
    assert rc == 0
    out = list(tmp_path.glob("*.jsonl"))
    assert len(out) == 1 and len(out[0].read_text().splitlines()) == 24
