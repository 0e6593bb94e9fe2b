"""ByteTrack on the device (csrc/kernels_bytetrack.hip) against the NumPy oracle (tests/bytetrack_oracle.py): ids, rows, class, score,
state and list order are np.array_equal frame by frame; the exported Kalman state is within the DeepSORT chain's tolerance."""
import numpy as np
import pytest

from bytetrack_oracle import BYTETracker as Oracle
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu


def scene(n=30, frames=300, seed=3):
    syn = pkg("synthetic")
    rng = np.random.default_rng(seed)
    gaps = [(int(t), int(a), int(a + rng.integers(3, 40))) for t, a in zip(rng.integers(0, n, n // 2), rng.integers(5, frames - 50, n // 2))]
    births = {int(t): int(f) for t, f in zip(rng.choice(n, n // 5, replace=False), rng.integers(1, frames // 2, n // 5))}
    return syn.Scene(seed=seed, n_targets=n, gaps=gaps, births=births, conf_range=(0.05, 0.95), jitter=1.5, shuffle=True)


def frames_of(sc, frames):
    out = []
    for f in range(frames):
        b, c, k, _ = sc.detections(f)
        k = (k + (np.arange(len(k)) % 3)).astype(np.int32)       # a few classes: cls follows the last matched detection
        out.append((b, c, k))
    return out


# Rows are compared exactly, but they are rint() of a Kalman mean that is only close to the oracle's (see compare_export), and the
# costs built from it meet thresholds: exact row parity holds for these seeds, it is not guaranteed for a scene that puts a box on
# a .5 pixel or a cost on a threshold edge (such a divergence would not be a kernel bug).
def compare_export(dev, ora):
    e, o = dev.export(), ora.export()
    assert e["n_tracked"] == o["n_tracked"]
    for key in ("track_id", "state", "is_activated", "start_frame", "end_frame", "cls", "score"):
        assert np.array_equal(e[key], o[key]), key
    # Kalman predict / initiate are bit-exact; the update's K S K^T is LAPACK / BLAS on the oracle side, an ordered fp32 sum on the
    # device: the tolerance of the DeepSORT chain tests (tests/test_gpu_pre_tracker.py)
    assert np.allclose(e["mean"], o["mean"], rtol=1e-5, atol=1e-3), np.abs(e["mean"] - o["mean"]).max()
    assert np.allclose(e["cov"], o["cov"], rtol=1e-4, atol=1e-4), np.abs(e["cov"] - o["cov"]).max()


def run_pair(dets, chunk, epoch_frames=0, lsap_fast=1, **kw):
    dev = pkg("bytetrack").BYTETracker(**kw)
    dev.option("epoch_frames", epoch_frames)
    dev.option("lsap_fast", lsap_fast)
    ora = Oracle(**{k: v for k, v in kw.items() if k != "max_tracks"})
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
    return dev


@pytest.mark.parametrize("epoch_frames,lsap_fast", [(1, 1), (16, 1), (16, 0), (1, 0)])
def test_device_matches_oracle(epoch_frames, lsap_fast):
    dets = frames_of(scene(), 300)
    run_pair(dets, chunk=37, epoch_frames=epoch_frames, lsap_fast=lsap_fast)


def test_update_tuples_and_export_after_single_frames():
    dets = frames_of(scene(n=12, frames=80, seed=9), 40)
    dev = pkg("bytetrack").BYTETracker()
    ora = Oracle()
    for b, c, k in dets:
        got = dev.update(b, c, k)
        want = ora.update_xyxy(b, c, k)
        rows, conf = Oracle.rows(want)
        assert [t[4] for t in got] == rows[:, 4].tolist()
        assert [t[:4] for t in got] == [tuple(r) for r in rows[:, :4].tolist()]
    compare_export(dev, ora)
    out = dev.update(np.array([]), np.array([]), np.array([]))          # empty inputs are accepted
    assert isinstance(out, list) and dev.frame_id == 41


def test_crowd_exercises_the_large_lsap():
    # 150 persons: the pool and the high band together exceed 128 (lsap_wave), within 512
    sc = pkg("synthetic").Scene(seed=21, n_targets=150, conf_range=(0.05, 0.95), jitter=2.0, shuffle=True,
                                w_range=(30.0, 50.0), h_range=(80.0, 120.0))
    dets = frames_of(sc, 60)
    dev = run_pair(dets, chunk=16, lsap_fast=0)
    assert len(dev.export()["track_id"]) > 100
    c = dev.counters()
    assert c["max_side"] > 128 and c["n_lsap"] > 0 and c["n_fast"] == 0     # lsap_wave, with the matrix beyond the LDS arena (> 111)


def test_capacity_error_raises():
    L = pkg("_lib")
    sc = pkg("synthetic").Scene(seed=4, n_targets=20, conf_range=(0.8, 0.95))
    dev = pkg("bytetrack").BYTETracker(max_tracks=8)
    with pytest.raises(L.AicError) as ei:
        dev.update_batch_arrays(frames_of(sc, 2))
    assert ei.value.code == L.ERR_CAPACITY
    with pytest.raises(L.AicError):                            # the tracker refuses further updates, and has no state to export
        dev.update_batch_arrays(frames_of(sc, 1))
    with pytest.raises(L.AicError):
        dev.export()
    # more than 512 detections in a frame, and an extended problem beyond 512
    dev = pkg("bytetrack").BYTETracker()
    b = np.tile(np.array([[0, 0, 10, 10]], np.float32), (513, 1))
    with pytest.raises(L.AicError) as ei:
        dev.update(b, np.full(513, 0.9, np.float32), np.zeros(513, np.int32))
    assert ei.value.code == L.ERR_CAPACITY
    dev = pkg("bytetrack").BYTETracker()
    xs = np.arange(300, dtype=np.float32) * 4
    b = np.stack([xs % 1200, (xs // 1200) * 30, xs % 1200 + 3, (xs // 1200) * 30 + 3], 1).astype(np.float32)
    dev.update(b, np.full(300, 0.9, np.float32), np.zeros(300, np.int32))        # 300 tracks
    with pytest.raises(L.AicError) as ei:                       # pool 300 + 300 high detections far away: side 600
        dev.update(b + 5000, np.full(300, 0.9, np.float32), np.zeros(300, np.int32))
    assert ei.value.code == L.ERR_CAPACITY


# ---------------------------------------------------------------------------------------------------- the ByteTrack pipeline
def _pipe(ypath, n, batch, inject, **kw):
    TP = pkg("pipeline").TrackingPipeline
    return TP(ypath, None, (720, 1280), batch=batch, ring_frames=n, max_persons=128, dtype="fp16", inject=inject,
              tracker="bytetrack", **kw)


def _oracle_rows(frames_dets, passes=1):
    ora = Oracle()
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
    pipe = _pipe(ypath, n, 16, True)                           # no ReID engine object anywhere
    assert pipe.reid is None and pipe.tracker_core is None
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    _same(tracks, _oracle_rows(planted))
    pipe.close()
    # run_from_host_passes, two passes: one continuous stream over the clip twice; the rows are the second pass's
    pipe = _pipe(ypath, n, 16, True)
    pipe.inject(0, planted)
    host = np.ascontiguousarray(frames)
    nt, rows, _ = pipe.run_raw_from_host_passes(host, 2)
    tconf = pipe._raw_bufs()[2]
    for f, (wr, wc) in enumerate(_oracle_rows(planted, passes=2)):
        assert nt[f] == len(wr), f
        assert np.array_equal(rows[f, :nt[f]], wr) and np.array_equal(tconf[f, :nt[f]], wc), f
    pipe.close()


def test_pipeline_own_detections_against_oracle():
    cfg = pkg("config")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    n = 32
    sc = pkg("synthetic").Scene(seed=11, n_targets=30)
    pipe = _pipe(ypath, n, 16, False)
    assert abs(pipe.params.conf_thresh - 0.1) < 1e-7           # the detector hands over ByteTrack's low band
    pipe.upload(0, sc.render_batch(0, n))
    tracks, dets = pipe.run(0, n, want_dets=True)
    lut = np.array([nm in cfg.CLASSES_TO_TRACK for nm in cfg.CLASSES])
    fed = []
    for b, s, l in dets:
        keep = (l >= 0) & (l < len(lut)) & lut[np.clip(l, 0, len(lut) - 1)]
        fed.append((b[keep], s[keep], l[keep]))
    assert sum(len(x[0]) for x in fed) > 20 * n
    _same(tracks, _oracle_rows(fed))
    pipe.close()


def test_pipeline_rejects_deepsort_only_calls():
    import ctypes as C
    L = pkg("_lib")
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = _pipe(ypath, 16, 16, True)
    th = C.c_void_p()
    assert L.load().aic_pipeline_tracker(pipe._h, C.byref(th)) == L.ERR_INVALID
    for key in ("device_assoc", "device_assoc_limit", "device_filter"):
        assert L.load().aic_pipeline_option(pipe._h, key.encode(), 1) == L.ERR_INVALID, key
    pipe.option("dual_lane_frames", 0)
    pipe.option("in_flight", 2)
    with pytest.raises(L.AicError):
        pipe.last_embeddings()
    pipe.close()


@pytest.mark.parametrize("batch", [1, 16])
def test_cli_bytetrack(tmp_path, batch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    rc = pkg("cli").main(["--input", "synthetic:640x360:6:24", "--output_dir", str(tmp_path), "--yolo_engine", ypath,
                          "--tracker", "bytetrack", "--batch", str(batch)])
    assert rc == 0
    out = list(tmp_path.glob("*.jsonl"))
    assert len(out) == 1 and len(out[0].read_text().splitlines()) == 24
