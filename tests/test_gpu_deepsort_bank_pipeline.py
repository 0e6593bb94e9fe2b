"""The DeepSORT bank in the pipeline (aic_pipeline_create_deepsort_bank, DeepSortBank::run_group): S cameras per
launch group, the bank kernels in their tick-major form (frame_stride = S, a row map over interleaved frames), boxes and embeddings
read where stage A left them in HBM.  A camera of the bank runs the single tracker's code in its arithmetic order, so everything is
held against plain DeepSORT pipelines with the device association ("device_assoc" 2) fed the same camera: rows, confidences,
embeddings, exported state and galleries are np.array_equal / list-equal.  There is no tolerance in this file."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import ROOT, pkg
from test_gpu_botsort_bank import cameras

pytestmark = pytest.mark.gpu

KEYS = ("track_id", "state", "hits", "age", "time_since_update", "cls", "gallery_len", "conf", "mean", "cov")
HW = (720, 1280)
_ENG = {}


def engines(yolo_items=12, reid_items=384, trained=False):
    """Engine objects shared by the pipelines of this file (one pipeline runs at a time): loaded once per size."""
    key = (yolo_items, reid_items, trained)
    if key not in _ENG:
        ef, eng = pkg("engine_file"), pkg("hip_engine").HipEngine
        ypath, rpath = ef.ensure_seeded_engines(ROOT)
        if trained:
            ypath = ef.ensure_trained_detector(ROOT)
        _ENG[key] = (eng(ypath, dtype="fp16", max_items=yolo_items, warm_up=False), eng(rpath, dtype="fp16", max_items=reid_items, warm_up=False))
    return _ENG[key]


def single(batch=4, eng=None, **kw):
    y, r = eng or engines()
    kw = dict(dict(max_persons=32, max_tracks=32, inject=True), **kw)
    pipe = pkg("pipeline").TrackingPipeline(y, r, HW, batch=batch, ring_frames=batch, dtype="fp16", **kw)
    pipe.option("taper", 0)
    pipe.option("device_assoc", 2)
    return pipe


def bank(S=3, batch=12, ring=None, eng=None, **kw):
    y, r = eng or engines()
    kw = dict(dict(max_persons=32, max_tracks=32, inject=True), **kw)
    pipe = pkg("pipeline").TrackingPipeline.deepsort_bank(y, r, HW, cameras=S, batch=batch, ring_frames=ring or batch, dtype="fp16", **kw)
    pipe.option("taper", 0)
    return pipe


def tick_major(per_cam):
    """per_cam[s][t] -> the flat tick-major list: item t * S + s."""
    return [per_cam[s][t] for t in range(len(per_cam[0])) for s in range(len(per_cam))]


def run(pipe, frames, planted=None):
    pipe.upload(0, np.ascontiguousarray(frames))
    if planted is not None:
        pipe.inject(0, planted)
    tracks, _ = pipe.run(0, len(frames))
    emb, per = pipe.group_embeddings()
    return tracks, emb, per


def same_state(bk, s, one):
    """Every exported field and every gallery of camera s equal the single pipeline's tracker."""
    a, b = one.tracker_core.export_arrays(), bk.bank.export(s)
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), (s, key)
    for i, gl in enumerate(a["gallery_len"]):
        assert np.array_equal(one.tracker_core._gallery(i, int(gl)), bk.bank.export_gallery(s, i, int(gl))), (s, i)
    return a


def compare(bk, ones, frames, planted, ticks, S, last_group_ticks=None):
    """One run call of `ticks` ticks on the bank pipeline against the same ticks on the singles: rows, confidences, embeddings."""
    rows, emb, per = run(bk, tick_major(frames), tick_major(planted))
    off = np.concatenate([[0], np.cumsum(per)])
    g = last_group_ticks or ticks                              # group_embeddings holds the call's last launch group
    for s in range(S):
        want, wemb, wper = run(ones[s], frames[s], planted[s])
        assert rows[s::S] == want, s                           # (x1, y1, x2, y2, id, class, conf) per row
        assert per[s::S].tolist() == wper[-g:].tolist(), s
        mine = [emb[off[i]:off[i + 1]] for i in range(s, g * S, S)]
        woff = np.concatenate([[0], np.cumsum(wper)])
        assert np.array_equal(np.concatenate(mine), wemb[woff[len(wper) - g]:]), s
    return rows


# ---------------------------------------------------------------------------------------------------- 1. bank pipeline == three singles
def test_bank_pipeline_equals_three_single_pipelines():
    frames, planted = cameras()
    bk = bank()
    assert bk.streams == 3 and bk.cameras == 3 and bk.tracker_core is None
    ones = [single() for _ in range(3)]
    for t0 in (0, 4):                                          # two runs of 4 ticks; camera 1 reconnects between them
        if t0:
            bk.reset_stream(1)
            ones[1].close()
            ones[1] = single()
        rows = compare(bk, ones, [f[t0:t0 + 4] for f in frames], [p[t0:t0 + 4] for p in planted], 4, 3)
    for s in range(3):
        a = same_state(bk, s, ones[s])
        assert (a["state"] == 2).any(), s                      # a confirmed track on every camera
        assert any(rows[t * 3 + s] for t in range(4)), s
    assert bk.counters()["assoc_device_frames"] == 24 and bk.counters()["assoc_host_frames"] == 0
    for p in ones + [bk]:
        p.close()


# ---------------------------------------------------------------------------------------------------- 2. ragged groups
def ragged():
    """Camera 0 never has a detection; camera 1 in ticks 1, 2, 3, 6 only; camera 2 carries a box that lies outside the frame (it clamps
    to an empty crop: feature None) beside its valid ones in every tick."""
    frames, planted = cameras()
    none = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    outside = np.array([[-80.0, 40.0, -20.0, 160.0]], np.float32)
    p2 = [(np.concatenate([b[:2], outside, b[2:]]), np.concatenate([c[:2], [np.float32(0.9)], c[2:]]).astype(np.float32),
           np.concatenate([k[:2], [0], k[2:]]).astype(np.int32)) for b, c, k in planted[2]]
    return frames, [[none] * 8, [planted[1][t] if t in (1, 2, 3, 6) else none for t in range(8)], p2]


@pytest.mark.parametrize("epoch_frames", [1, 0])
@pytest.mark.parametrize("lsap_fast", [0, 1])
def test_ragged_groups_equal_the_singles(epoch_frames, lsap_fast):
    frames, planted = ragged()
    bk = bank(batch=12, ring=24)                               # 8 ticks = two launch groups of 4
    bk.option("epoch_frames", epoch_frames)
    bk.bank.option("lsap_fast", lsap_fast)
    ones = [single(batch=8) for _ in range(3)]
    for o in ones:
        o.tracker_core.option("lsap_fast", lsap_fast)
        o.tracker_core.option("epoch_frames", epoch_frames)
    rows = compare(bk, ones, frames, planted, 8, 3, last_group_ticks=4)
    assert not any(rows[0::3]) and any(rows[1::3]) and any(rows[2::3])
    for s in range(3):
        a = same_state(bk, s, ones[s])
        assert (len(a["track_id"]) == 0) == (s == 0)
        assert bk.bank.counters(s) == ones[s].tracker_core.assoc_counters(), s
    a2 = bk.bank.export(2)
    assert a2["gallery_len"].min() == 0 and a2["gallery_len"].max() > 0      # the track of the empty crop never got a gallery row
    assert (bk.bank.counters(2)[0] > 0) == bool(lsap_fast)
    for p in ones + [bk]:
        p.close()


# ---------------------------------------------------------------------------------------------------- 3. the common-k cut
def test_the_row_budget_cuts_the_epoch_for_every_camera():
    """Camera 0 holds 130 boxes per frame: 16 ticks are 2080 rows, past TRK_DEV_DNMAX = 2048, so the bank's first epoch ends after 15
    ticks for BOTH cameras (k is common to a launch) while the single pipeline of camera 1 (3 boxes per frame) runs one epoch of 16."""
    frames, planted = cameras()
    eng = engines(32, 2304)
    gx, gy = np.meshgrid(np.arange(13) * 96.0 + 10.0, np.arange(10) * 70.0 + 4.0)
    grid = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 60.0, gy.ravel() + 62.0], 1).astype(np.float32)
    assert len(grid) == 130 and 16 * 130 > 2048 >= 15 * 130
    crowd = [(grid + np.float32(0.5 * t), np.full(130, 0.8, np.float32), np.zeros(130, np.int32)) for t in range(16)]
    few = [tuple(a[:3] for a in planted[1][t % 8]) for t in range(16)]
    fr = [np.concatenate([frames[0], frames[0]]), np.concatenate([frames[1], frames[1]])]
    kw = dict(max_persons=160, max_tracks=256, nn_budget=16, eng=eng)
    bk = bank(S=2, batch=32, **kw)
    ones = [single(batch=16, **kw) for _ in range(2)]
    rows = compare(bk, ones, fr, [crowd, few], 16, 2)
    assert max(len(r) for r in rows[0::2]) == 130 and 0 < max(len(r) for r in rows[1::2]) <= 3
    for s in range(2):
        same_state(bk, s, ones[s])
    for p in ones + [bk]:
        p.close()


# ---------------------------------------------------------------------------------------------------- 4. the detector's own detections
def test_own_detections_through_the_device_filter():
    syn = pkg("synthetic")
    eng = engines(12, 768, trained=True)
    scs = [syn.Scene(seed=1 + s, n_targets=6 - s, width=1280, height=720) for s in range(3)]
    frames = [sc.render_batch(0, 12) for sc in scs]
    # every detector call holds 12 frames on both sides: three groups of 4 ticks here, one group of 12 frames per single
    bk = bank(batch=12, ring=36, eng=eng, inject=False, max_persons=64, max_tracks=64)
    ones = [single(batch=12, eng=eng, inject=False, max_persons=64, max_tracks=64) for _ in range(3)]
    flat = np.ascontiguousarray(np.stack(frames, 1).reshape(36, 720, 1280, 3))
    bk.upload(0, flat)
    rows, nd = bk.run(0, 36)
    total = 0
    for s in range(3):
        ones[s].upload(0, frames[s])
        want, wnd = ones[s].run(0, 12)
        assert rows[s::3] == want, s
        assert nd[s::3].tolist() == wnd.tolist(), s
        total += sum(len(r) for r in want)
        same_state(bk, s, ones[s])
    assert total > 3
    c = bk.counters()
    assert c["filter_device_groups"] == 3 and c["filter_host_groups"] == 0 and c["assoc_device_frames"] == 36
    for p in ones + [bk]:
        p.close()


# ---------------------------------------------------------------------------------------------------- 5. a camera that exhausts max_tracks
def test_a_camera_that_exhausts_max_tracks_stops_alone():
    """max_tracks 16; camera 1 gets 14 more boxes in tick 3, which would need more than 16 track slots.  The run call delivers the group
    -- camera 1 up to tick 2, the other cameras whole -- and returns AIC_ERR_CAPACITY naming the camera; run calls are then refused
    until reset_stream(1), after which camera 1 starts afresh beside the others, which went on."""
    L = pkg("_lib")
    lib = L.load()
    frames, planted = cameras()
    gx, gy = np.meshgrid(np.arange(7) * 150.0 + 40.0, np.arange(2) * 300.0 + 60.0)
    more = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 60.0, gy.ravel() + 140.0], 1).astype(np.float32)
    p1 = list(planted[1])
    b, c, k = p1[3]
    p1[3] = (np.concatenate([b, more]), np.concatenate([c, np.full(14, 0.8, np.float32)]), np.concatenate([k, np.zeros(14, np.int32)]))
    planted = [planted[0], p1, planted[2]]
    kw = dict(max_tracks=16)
    bk = bank(**kw)
    ones = [single(**kw) for _ in range(3)]
    mp = bk.max_persons
    bk.upload(0, np.ascontiguousarray(tick_major([f[:4] for f in frames])))
    bk.inject(0, tick_major([p[:4] for p in planted]))
    nt, r6, cf = np.zeros(12, np.int32), np.zeros((12, mp, 6), np.int32), np.zeros((12, mp), np.float32)
    rc = lib.aic_pipeline_run(bk._h, 0, 12, L.ptr(nt), L.ptr(r6), L.ptr(cf), None, None, None, None)
    assert rc == L.ERR_CAPACITY
    msg = lib.aic_last_error()
    assert b"stream 1" in msg and b"max_tracks" in msg and b"frame 3" in msg

    def rows_of(pipe, fr, pl):
        tracks, _, _ = run(pipe, fr, pl)
        return [[t[:5] for t in f] for f in tracks], [[t[6] for t in f] for f in tracks]

    for s in range(3):
        n = 3 if s == 1 else 4                                  # camera 1: the ticks before the failing one
        want, wconf = rows_of(ones[s], frames[s][:n], planted[s][:n])
        for t in range(n):
            f = t * 3 + s
            assert r6[f, :nt[f], :5].tolist() == [list(w[:4]) + [w[4]] for w in want[t]], (s, t)
            assert cf[f, :nt[f]].tolist() == [np.float32(x) for x in wconf[t]], (s, t)
        assert any(want), s                                     # confirmed rows exist before the failing tick
    assert nt[3 * 3 + 1] == 0                                   # nothing from the failing frame on
    assert lib.aic_pipeline_run(bk._h, 0, 12, L.ptr(nt), L.ptr(r6), L.ptr(cf), None, None, None, None) == L.ERR_INVALID
    assert b"reset" in lib.aic_last_error()
    with pytest.raises(L.AicError):
        bk.bank.export(1)                                       # no frame boundary to report
    same_state(bk, 0, ones[0])
    same_state(bk, 2, ones[2])
    bk.reset_stream(1)
    ones[1].close()
    ones[1] = single(**kw)
    compare(bk, ones, [f[4:8] for f in frames], [p[4:8] for p in cameras()[1]], 4, 3)
    for s in range(3):
        same_state(bk, s, ones[s])
    for p in ones + [bk]:
        p.close()


# ---------------------------------------------------------------------------------------------------- 6. link_cameras
def test_link_cameras_on_the_pipeline_and_on_a_bank_fed_its_embeddings():
    frames, planted = cameras()
    fr, pl = [frames[0], frames[0], frames[2]], [planted[0], planted[0], planted[2]]      # cameras 0 and 1 show the same frames
    bk = bank()
    dim = int(bk.reid.out_dim)
    alone = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=32, feature_dim=dim)
    links = 0
    for t0 in (0, 4):
        tracks, emb, per = run(bk, tick_major([f[t0:t0 + 4] for f in fr]), tick_major([p[t0:t0 + 4] for p in pl]))
        links += bk.link_cameras()
        off = np.concatenate([[0], np.cumsum(per)])
        feed = []
        for s in range(3):                                      # the pipeline's own embeddings and boxes, stream-major
            cam = []
            for t in range(4):
                b, c, k = pl[s][t0 + t]
                b = np.asarray(b, np.float32)
                tlwh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1)
                i = t * 3 + s
                assert per[i] == len(b)
                cam.append((tlwh, c, k, emb[off[i]:off[i + 1]]))
            feed.append(cam)
        got = alone.update_arrays(feed)
        for s in range(3):
            for t in range(4):
                assert [tuple(r) for r in got[s][t][0][:, :5].tolist()] == [tuple(x[:5]) for x in tracks[t * 3 + s]], (t0, s, t)
        alone.link_cameras()
    n_conf = 0
    for s in range(3):
        a, b = bk.bank.export(s), alone.export(s)               # run_group (tick-major, from HBM) == update (stream-major, staged)
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (s, key)
        ids = a["track_id"][a["state"] == 2]
        n_conf += len(ids)
        assert len(ids) > 0 and (bk.global_ids(s, ids) >= 0).all()
        assert np.array_equal(bk.global_ids(s, ids), alone.global_ids(s, ids)), s
    a0, a1 = bk.bank.export(0), bk.bank.export(1)
    ids = a0["track_id"][a0["state"] == 2]
    assert np.array_equal(a0["track_id"], a1["track_id"])
    assert np.array_equal(bk.global_ids(0, ids), bk.global_ids(1, ids))       # every confirmed track and its twin
    assert links >= len(ids)
    bk.reset_stream(1)
    assert (bk.global_ids(1, ids) == -1).all() and (bk.global_ids(0, ids) >= 0).all()
    alone.close()
    bk.close()


# ---------------------------------------------------------------------------------------------------- 7. rejections
def test_rejections_on_the_bank_pipeline_and_the_pinned_ones_beside_it():
    L = pkg("_lib")
    lib = L.load()
    TP = pkg("pipeline").TrackingPipeline
    y, r = engines()
    bk = bank()
    for slot, count in ((0, 4), (1, 3), (2, 9)):               # run ranges are whole ticks
        assert lib.aic_pipeline_run(bk._h, slot, count, None, None, None, None, None, None, None) == L.ERR_INVALID, (slot, count)
    for key, v in ((b"device_assoc", 0), (b"device_assoc", 2), (b"device_assoc_limit", 64), (b"streams", 3), (b"gmc", 4)):
        assert lib.aic_pipeline_option(bk._h, key, v) == L.ERR_INVALID, key
        assert lib.aic_last_error()
    h = C.c_void_p()
    assert lib.aic_pipeline_tracker(bk._h, C.byref(h)) == L.ERR_INVALID and not h.value
    dummy = (C.c_float * 4)()
    assert lib.aic_pipeline_exchange_enable(bk._h, dummy, dummy, 16, 1) == L.ERR_INVALID
    assert lib.aic_pipeline_reset_stream(bk._h, 3) == L.ERR_INVALID and lib.aic_pipeline_reset_stream(bk._h, 2) == L.OK
    for key, v in ((b"epoch_frames", 4), (b"epoch_frames", 0), (b"device_filter", 1), (b"tracker_cus", 2)):
        assert lib.aic_pipeline_option(bk._h, key, v) == L.OK, key
    assert lib.aic_pipeline_option(bk._h, b"epoch_frames", 17) == L.ERR_INVALID
    assert lib.aic_pipeline_deepsort_bank(bk._h, C.byref(h)) == L.OK and h.value
    # the plain DeepSORT pipeline beside it keeps its three rejections, and has no bank
    with pytest.raises(ValueError):
        TP(y, r, HW, batch=12, ring_frames=12, tracker="deepsort", streams=3)
    one = single(batch=12)
    assert one.tracker_core is not None
    assert lib.aic_pipeline_option(one._h, b"streams", 3) == L.ERR_INVALID
    assert lib.aic_pipeline_option(one._h, b"epoch_frames", 4) == L.ERR_INVALID
    assert lib.aic_pipeline_reset_stream(one._h, 0) == L.ERR_INVALID
    h2 = C.c_void_p()
    assert lib.aic_pipeline_deepsort_bank(one._h, C.byref(h2)) == L.ERR_INVALID and not h2.value
    x = pkg("xcam").CrossCamera(3, 32, int(one.reid.out_dim))
    n = C.c_int32()
    assert lib.aic_pipeline_link_cameras(one._h, x._h, C.byref(n)) == L.ERR_INVALID
    with pytest.raises(ValueError):
        one.link_cameras()
    with pytest.raises(SystemExit):
        pkg("cli").parse_arguments(["--inputs", "a,b,c", "--tracker", "deepsort"])
    x.close()
    one.close()
    bk.close()
    # create-time rejections: geometry, the camera count, and the bank's own (no device association without a gallery budget)
    lo, hi = pkg("config").track_class_mask()
    for batch, ring, streams, budget, tracks in ((8, 12, 3, 100, 32), (6, 8, 3, 100, 32), (6, 6, 0, 100, 32), (6, 6, 257, 100, 32),
                                                 (6, 6, 3, 0, 32), (6, 6, 3, 100, 513)):
        tp = L.TrackerParams(0.2, 0.7, budget, 70, 3, tracks, 0, 1)
        prm = L.PipelineParams(720, 1280, batch, ring, 16, 0.1, 0.5, 300, 0.0, 1, (C.c_uint64 * 2)(lo, hi), tp)
        hp = C.c_void_p()
        rc = lib.aic_pipeline_create_deepsort_bank(y._h, r._h, C.byref(prm), streams, C.byref(hp))
        assert rc == L.ERR_INVALID and not hp.value, (batch, ring, streams, budget, tracks)


def test_a_frame_with_more_than_512_detections_is_a_capacity_error():
    L = pkg("_lib")
    lib = L.load()
    frames, _ = cameras()
    gx, gy = np.meshgrid(np.arange(27) * 46.0 + 4.0, np.arange(19) * 36.0 + 4.0)
    grid = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 40.0, gy.ravel() + 30.0], 1).astype(np.float32)
    assert len(grid) == 513
    none = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32))
    bk = bank(S=3, batch=3, ring=3, eng=engines(12, 768), max_persons=520, max_tracks=32)
    bk.upload(0, np.ascontiguousarray(np.stack([f[0] for f in frames])))
    bk.inject(0, [none, (grid, np.full(513, 0.8, np.float32), np.zeros(513, np.int32)), none])
    assert lib.aic_pipeline_run(bk._h, 0, 3, None, None, None, None, None, None, None) == L.ERR_CAPACITY
    assert b"512" in lib.aic_last_error()
    assert all(len(bk.bank.export(s)["track_id"]) == 0 for s in range(3))     # nothing was launched for any camera
    bk.close()


# ---------------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_inputs_with_deepsort_bank_writes_one_output_per_stream(tmp_path):
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    # 1280x720: the size the trained detector sees persons at; every detector call that is compared holds 12 frames
    srcs = ["synthetic:1280x720:6:12:1", "synthetic:1280x720:4:16:2", "synthetic:1280x720:5:12:3"]
    common = ["--yolo_engine", ypath, "--reid_engine", rpath, "--batch", "12"]
    assert cli.main(["--inputs", ",".join(srcs), "--tracker", "deepsort_bank", "--output_dir", str(tmp_path / "all")] + common) == 0
    n_tracks = 0
    for k, src in enumerate(srcs):
        assert cli.main(["--input", src, "--tracker", "deepsort", "--output_dir", str(tmp_path / f"one{k}")] + common) == 0
        got = list((tmp_path / "all").glob(f"*_s{k}.jsonl"))
        want = list((tmp_path / f"one{k}").glob("*.jsonl"))
        assert len(got) == 1 and len(want) == 1
        g = [json.loads(l) for l in got[0].read_text().splitlines()]
        w = [json.loads(l) for l in want[0].read_text().splitlines()]
        assert len(g) == 12 and g == w[:12], k                 # the shortest source ends the run
        n_tracks += sum(len(fr["tracks"]) for fr in g)
    assert n_tracks > 1
    with pytest.raises(SystemExit):
        cli.main(["--tracker", "deepsort_bank", "--input", srcs[0], "--yolo_engine", ypath])
