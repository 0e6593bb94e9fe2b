"""The BoT-SORT bank and the camera-motion bank on the device: S cameras per launch, one kernel block per stream
(csrc/kernels_botsort.hip, csrc/kernels_gmc.hip, csrc/epoch_bank.hpp).  A stream of a bank runs the single tracker's code in the single
tracker's arithmetic order, so everything is np.array_equal to single objects fed the same frames: any difference is cross-stream
contamination.  There is no tolerance in this file."""
import json

import numpy as np
import pytest

import gmc_oracle as G
import test_gpu_botsort as TBS
import test_gpu_gmc as TG
from botsort_oracle import BoTSORT as Oracle
from conftest import ROOT, pkg
from test_botsort_oracle import CROSSING, crossing_scene, ids_by_position

pytestmark = pytest.mark.gpu

CLOCKS = ("cost_cycles", "kernel_cycles")                       # shader-clock totals: the only fields that differ from run to run


def stream_frames(sc, frames, seed, dim, warps=None, f0=0):
    """Per frame (boxes, scores, cls, raw features, warp or None) with the stream's own identity_features seed; the features are
    scaled off unit length (the device normalises)."""
    syn = pkg("synthetic")
    out = []
    for f in range(f0, f0 + frames):
        b, c, k, ident = sc.detections(f)
        k = (k + (np.arange(len(k)) % 3)).astype(np.int32)
        ft = (syn.identity_features(ident, f, dim=dim, seed=seed) * np.float32(0.5 + 0.02 * f)).astype(np.float32)
        out.append((b, c, k, ft, None if warps is None else warps[f]))
    return out


def same_frames(got, want, what):
    assert len(got) == len(want), what
    for f, ((r, c), (wr, wc)) in enumerate(zip(got, want)):
        assert np.array_equal(r, wr) and np.array_equal(c, wc), (what, f, r, wr)


def same_state(bk, s, one):
    e, o = bk.export(s), one.export()
    assert e.keys() == o.keys() and "smooth_feat" in e and "has_feat" in e
    for key in e:
        assert np.array_equal(e[key], o[key]), (s, key)
    cb, co = bk.counters(s), one.counters()
    assert cb.keys() == co.keys()
    assert {k: v for k, v in cb.items() if k not in CLOCKS} == {k: v for k, v in co.items() if k not in CLOCKS}, s


def run_bank_and_singles(dets, plan, options=(), **kw):
    """dets[s]: the frames of stream s; plan: per call the frames handed to every stream.  The bank against len(dets) BoTSORT objects."""
    B = pkg("botsort")
    S = len(dets)
    bk = B.BoTSORTBank(S, **kw)
    ones = [B.BoTSORT(**kw) for _ in range(S)]
    for t in [bk] + ones:
        for key, v in options:
            t.option(key, v)
    pos = [0] * S
    for call in plan:
        parts = [dets[s][pos[s]:pos[s] + call[s]] for s in range(S)]
        got = bk.update_arrays(parts)
        for s in range(S):
            same_frames(got[s], ones[s].update_batch_arrays(parts[s]), (s, pos[s]))
            pos[s] += len(parts[s])
    for s in range(S):
        same_state(bk, s, ones[s])
    return bk, ones, pos


# ---------------------------------------------------------------------------------------------------- bank == singles
CROWDS = [(30, 3), (12, 9), (5, 11), (1, 7)]                     # persons, scene seed
_RAGGED = {}


def ragged_dets():
    if not _RAGGED:
        _RAGGED["d"] = [stream_frames(TBS.scene(n=n, frames=300, seed=seed), 40, seed=20 + s, dim=64) for s, (n, seed) in enumerate(CROWDS)]
    return _RAGGED["d"]


@pytest.mark.parametrize("epoch_frames", [1, 0])
@pytest.mark.parametrize("lsap_fast", [0, 1])
def test_ragged_bank_equals_singles(epoch_frames, lsap_fast):
    dets = ragged_dets()
    cyc = (0, 1, 3, 17, 16)                                     # an idle call, a call across the 16-frame epoch, a full epoch
    plan, pos, i = [], [0] * 4, 0
    while min(pos) < 40:
        call = [min(cyc[(i + s) % 5], 40 - pos[s]) for s in range(4)]
        pos = [p + c for p, c in zip(pos, call)]
        plan.append(call)
        i += 1
    assert any(0 in c for c in plan) and any(17 in c for c in plan)
    bk, ones, done = run_bank_and_singles(dets, plan, (("epoch_frames", epoch_frames), ("lsap_fast", lsap_fast)), feature_dim=64)
    assert done == [40] * 4
    assert all(bk.export(s)["has_feat"].all() and len(bk.export(s)["track_id"]) > 0 for s in range(4))
    assert bk.counters(0)["n_appearance"] > 0
    assert (bk.counters(0)["n_fast"] > 0) == bool(lsap_fast)


def test_every_stream_reads_its_own_rows_of_the_warps():
    n = 24
    warps = []
    for s in range(3):                                         # a different rotation + translation per stream and frame
        th = 0.004 * np.sin(np.arange(n) * (0.7 + 0.2 * s) + s)
        warps.append([np.array([[np.cos(t), -np.sin(t), (1.5 + s) * np.cos(i)], [np.sin(t), np.cos(t), -(0.75 + s) * np.sin(i)]], np.float32)
                      for i, t in enumerate(th)])
    warps.append(None)                                         # and a stream without camera motion: the bank hands it the identity
    dets = [stream_frames(TBS.scene(n=12, frames=80, seed=9), n, seed=7, dim=64, warps=w) for w in warps]
    bk, ones, _ = run_bank_and_singles(dets, [[7, 1, 16, 3], [1, 7, 1, 16], [16, 16, 7, 5]], feature_dim=64)
    covs = [bk.export(s)["cov"] for s in range(4)]
    for s in range(3):                                         # the same scene in every stream: only the warps tell them apart
        assert covs[s].shape != covs[3].shape or not np.array_equal(covs[s], covs[3]), s


def test_two_crowds_in_one_launch_use_their_own_scratch_and_features():
    Scene = pkg("synthetic").Scene
    crowd = dict(n_targets=150, conf_range=(0.05, 0.95), jitter=2.0, shuffle=True, w_range=(30.0, 50.0), h_range=(80.0, 120.0))
    dets = [stream_frames(Scene(seed=21, **crowd), 20, seed=31, dim=512),
            stream_frames(Scene(seed=5, n_targets=4, conf_range=(0.3, 0.95), jitter=1.0), 20, seed=32, dim=512),
            stream_frames(Scene(seed=22, **crowd), 20, seed=33, dim=512)]
    bk, _, _ = run_bank_and_singles(dets, [[16, 16, 16], [4, 4, 4]], (("lsap_fast", 0),))
    for s in (0, 2):                                           # both crowds' extended matrices are beyond the LDS arena, in one launch
        c = bk.counters(s)
        assert c["max_side"] > 128 and c["n_appearance"] > 0, (s, c)
        assert len(bk.export(s)["track_id"]) > 100
    assert bk.feature_dim == 512 and bk.counters(1)["max_side"] < 64


# ---------------------------------------------------------------------------------------------------- against the oracle
def test_middle_stream_on_the_crossing_scene_against_the_oracle():
    mm = pkg("mot_metrics")
    syn = pkg("synthetic")
    dets, gt = crossing_scene(**CROSSING)

    def mirrored(b):
        return np.stack([1280 - b[:, 2], b[:, 1], 1280 - b[:, 0], b[:, 3]], 1).astype(np.float32)

    bk = pkg("botsort").BoTSORTBank(3)
    ora = Oracle()
    outs = []
    for f, (b, s, c, ident) in enumerate(dets):
        mine = syn.identity_features(ident, f, dim=512, seed=5)
        # the neighbours: the same scene mirrored, other people (a leak of smoothed features between the slices breaks the rescue)
        got = bk.update([(mirrored(b), s, c, syn.identity_features(ident, f, dim=512, seed=6)), (b, s, c, mine),
                         (mirrored(b), s, c, syn.identity_features(ident, f, dim=512, seed=8))])
        rows, _ = Oracle.rows(ora.update_xyxy(b, s, c, mine))
        assert [t[:5] for t in got[1]] == [tuple(r[:5]) for r in rows.tolist()], f
        outs.append(got[1])
    assert ids_by_position(outs[-1]) == [1, 2]
    assert mm.evaluate(gt, outs)["idsw"] == 0
    view = type("V", (), {"export": lambda self: bk.export(1), "counters": lambda self: bk.counters(1), "feature_dim": 512})()
    TBS.compare_export(view, ora)
    for s in (0, 2):
        assert sorted(bk.export(s)["track_id"].tolist()) == [1, 2]


# ---------------------------------------------------------------------------------------------------- failure is contained
def _raw_update(bk, fps, frames, cap, n_out, status):
    L = pkg("_lib")
    counts, xyxy, conf, cls, feat, valid, warps = pkg("botsort")._pack_frames(frames, bk.feature_dim)
    fps = np.asarray(fps, np.int32)
    return L.load().aic_botsort_bank_update(bk._h, L.ptr(fps), L.ptr(counts), L.ptr(xyxy), L.ptr(conf), L.ptr(cls), L.ptr(feat),
                                            L.ptr(valid), L.ptr(warps), cap, L.ptr(n_out), None, None, L.ptr(status))


def test_a_failing_stream_stops_alone():
    """max_tracks = 8: the 20-person stream exhausts the track slots (the capacity error the trackers report), its neighbours do not."""
    L = pkg("_lib")
    B = pkg("botsort")
    Scene = pkg("synthetic").Scene
    kw = dict(max_tracks=8, first_track_id=7, feature_dim=64)
    dets = [stream_frames(Scene(seed=31, n_targets=5, conf_range=(0.8, 0.95)), 8, seed=1, dim=64),
            stream_frames(Scene(seed=4, n_targets=20, conf_range=(0.8, 0.95)), 8, seed=2, dim=64),
            stream_frames(Scene(seed=32, n_targets=5, conf_range=(0.8, 0.95)), 8, seed=3, dim=64)]
    bk = B.BoTSORTBank(3, **kw)
    ones = [B.BoTSORT(**kw) for _ in range(3)]
    for f0 in (0, 2):                                          # the failing call and the next
        got = bk.update_arrays([d[f0:f0 + 2] for d in dets])
        assert got[1] is None and list(bk.failed) == [1]
        for s in (0, 2):
            same_frames(got[s], ones[s].update_batch_arrays(dets[s][f0:f0 + 2]), (s, f0))
    with pytest.raises(L.AicError) as ei:
        bk.export(1)
    assert ei.value.code == L.ERR_INVALID
    for s in (0, 2):
        same_state(bk, s, ones[s])
    # the raw call: status holds the code per stream and the call is OK; with status NULL the stopped stream's code comes back
    n_out, status = np.full(1, -1, np.int32), np.zeros(3, np.int32)
    assert _raw_update(bk, [0, 1, 0], [dets[1][4]], 8, n_out, status) == L.OK
    assert status.tolist() == [0, L.ERR_CAPACITY, 0] and n_out[0] == 0
    assert _raw_update(bk, [0, 1, 0], [dets[1][4]], 8, n_out, None) == L.ERR_CAPACITY
    assert b"stream 1" in L.load().aic_last_error()
    # a fresh bank: the failure itself through the raw call with status NULL
    bk2 = B.BoTSORTBank(3, **kw)
    n6 = np.zeros(6, np.int32)
    rc = _raw_update(bk2, [2, 2, 2], [fr for d in dets for fr in d[:2]], 8, n6, None)
    assert rc == L.ERR_CAPACITY and b"stream 1" in L.load().aic_last_error()
    assert n6[0] > 0 and n6[4] > 0                             # the other streams' frames of the same call were processed
    # a camera reconnecting: the stream equals a fresh single tracker (no tracks, no smoothed features, ids from first_track_id)
    bk.reset(1)
    assert not bk.failed
    again = stream_frames(Scene(seed=33, n_targets=5, conf_range=(0.8, 0.95)), 6, seed=4, dim=64)
    fresh = B.BoTSORT(**kw)
    got = bk.update_arrays([[], again, []])
    want = fresh.update_batch_arrays(again)
    same_frames(got[1], want, "after reset")
    same_state(bk, 1, fresh)
    assert min(int(r[:, 4].min()) for r, _ in want if len(r)) == 7
    for s in (0, 2):                                           # untouched by the neighbour's reset
        same_state(bk, s, ones[s])
    # reset of a healthy stream with tracks and features: as a fresh single as well
    bk.reset(0)
    assert len(bk.export(0)["track_id"]) == 0
    fresh0 = B.BoTSORT(**kw)
    same_frames(bk.update_arrays([dets[0][4:8], [], []])[0], fresh0.update_batch_arrays(dets[0][4:8]), "healthy stream after reset")
    same_state(bk, 0, fresh0)


def test_a_frame_with_513_detections_rejects_the_whole_call():
    L = pkg("_lib")
    B = pkg("botsort")
    Scene = pkg("synthetic").Scene
    bk = B.BoTSORTBank(2, feature_dim=64)
    ok = stream_frames(Scene(seed=41, n_targets=4, conf_range=(0.8, 0.95)), 3, seed=1, dim=64)
    bk.update_arrays([ok[:1], ok[:1]])
    before = [bk.export(s) for s in range(2)]
    big = (np.tile(np.array([[0, 0, 10, 10]], np.float32), (513, 1)), np.full(513, 0.9, np.float32), np.zeros(513, np.int32),
           np.ones((513, 64), np.float32))
    with pytest.raises(L.AicError) as ei:
        bk.update_arrays([ok[1:3], [big]])
    assert ei.value.code == L.ERR_CAPACITY and not bk.failed
    one = B.BoTSORT(feature_dim=64)
    one.update_batch_arrays(ok[:1])
    for s in range(2):                                         # nothing was launched: no stream advanced
        same_state(bk, s, one)
        for key in before[s]:
            assert np.array_equal(before[s][key], bk.export(s)[key]), key
    got = bk.update_arrays([ok[1:3], ok[1:3]])
    same_frames(got[0], one.update_batch_arrays(ok[1:3]), "after the rejected call")


# ---------------------------------------------------------------------------------------------------- the camera-motion bank
GH, GW = 320, 384                                                # at s = 4: 80 x 96 gray pixels, 4 x 5 blocks (tests/test_gpu_gmc.py, test_smallest_shapes: one block needs 32 * s a side)
PANS = [(5.0, 2.0), (-3.0, 4.0), (7.0, -6.0)]


def pan_scenes(ticks):
    """frames[s], boxes[s] of three panning cameras, and the same tick-major."""
    syn = pkg("synthetic")
    scs = [syn.PanningScene(seed=40 + s, width=GW, height=GH, pan=p, n_targets=2, w_range=(20.0, 30.0), h_range=(30.0, 50.0), speed=1.0,
                            pad=128) for s, p in enumerate(PANS)]
    frames = [sc.render_batch(0, ticks) for sc in scs]
    boxes = [[sc.detections(f)[0] for f in range(ticks)] for sc in scs]
    tick_frames = np.ascontiguousarray(np.stack(frames, 1).reshape(ticks * 3, GH, GW, 3))
    tick_boxes = [boxes[i % 3][i // 3] for i in range(ticks * 3)]
    return frames, boxes, tick_frames, tick_boxes


def test_camera_motion_bank_equals_singles_and_the_oracle():
    gm = pkg("gmc")
    T = 6
    frames, boxes, tf, tb = pan_scenes(T)
    ones = [gm.CameraMotion(GH, GW) for _ in range(3)]
    want_w = [o.apply_batch(frames[s][:5], boxes[s][:5]) for s, o in enumerate(ones)]
    want_s = [o.stats for o in ones]
    ow, os_, _ = TG.oracle_stream(frames[1][:5], boxes[1][:5], 4)
    assert np.array_equal(want_w[1], ow) and np.array_equal(want_s[1], os_)
    assert all(st[1:, 0].all() for st in want_s) and len({w[1:].tobytes() for w in want_w}) == 3    # three different, estimated motions
    bk = gm.CameraMotionBank(3, GH, GW)
    got = bk.apply_ticks(tf[:15], tb[:15])                       # 5 ticks in one call
    for s in range(3):
        assert np.array_equal(got[s::3], want_w[s]) and np.array_equal(bk.stats[s::3], want_s[s]), s
    bk2 = gm.CameraMotionBank(3, GH, GW)                        # 2 + 3 ticks: the carried levels of every camera
    a = bk2.apply_ticks(tf[:6], tb[:6])
    sa = bk2.stats
    b = bk2.apply_ticks(tf[6:15], tb[6:15])
    assert np.array_equal(np.concatenate([a, b]), got) and np.array_equal(np.concatenate([sa, bk2.stats]), bk.stats)
    # camera 1 reconnects: its next frame is a first frame (identity, every block skipped), cameras 0 and 2 go on
    bk2.reset(1)
    c = bk2.apply_ticks(tf[15:18], tb[15:18])
    nb = int(want_s[0][0, 1])
    assert nb == 20
    assert np.array_equal(c[1], G.IDENTITY) and bk2.stats[1].tolist() == [0, nb, 0, 0]
    for s in (0, 2):
        w = ones[s].apply_batch(frames[s][5:6], boxes[s][5:6])
        assert np.array_equal(c[s], w[0]) and np.array_equal(bk2.stats[s], ones[s].stats[0]) and ones[s].stats[0, 0] == 1, s
    L = pkg("_lib")
    with pytest.raises(L.AicError):
        bk2.reset(3)
    with pytest.raises(ValueError):
        bk2.apply_ticks(tf[:4])
    for o in ones + [bk, bk2]:
        o.close()


# ---------------------------------------------------------------------------------------------------- the pipeline
_CAMS = {}


def cameras():
    """Three panning 720p cameras, 8 ticks: frames[s] and planted boxes[s]."""
    if not _CAMS:
        syn = pkg("synthetic")
        scs = [syn.PanningScene(seed=60 + s, width=1280, height=720, pan=p, n_targets=5 + s, speed=1.5, pad=256)
               for s, p in enumerate([(9.0, -3.0), (-6.0, 5.0), (4.0, 8.0)])]
        _CAMS["frames"] = [sc.render_batch(0, 8) for sc in scs]
        _CAMS["planted"] = [[sc.detections(f)[:3] for f in range(8)] for sc in scs]
    return _CAMS["frames"], _CAMS["planted"]


def _single(gmc):
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = pkg("pipeline").TrackingPipeline(ypath, rpath, (720, 1280), batch=4, ring_frames=4, max_persons=32, dtype="fp16", inject=True,
                                            tracker="botsort", gmc=gmc)
    pipe.option("taper", 0)
    return pipe


def _bank(gmc, **kw):
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = pkg("pipeline").TrackingPipeline.botsort_bank(ypath, rpath, (720, 1280), cameras=3, gmc=gmc, batch=12, ring_frames=12,
                                                         max_persons=32, dtype="fp16", inject=True, **kw)
    pipe.option("taper", 0)
    return pipe


def _run(pipe, frames, planted):
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, len(frames))
    emb, per = pipe.group_embeddings()
    return TG._rows(tracks), emb, per


@pytest.mark.parametrize("gmc", [0, 4])
def test_pipeline_bank_equals_single_pipelines(gmc):
    frames, planted = cameras()
    bank = _bank(gmc)
    assert bank.streams == 3
    ones = [_single(gmc) for _ in range(3)]
    for t0 in (0, 4):                                          # two runs of 4 ticks; camera 1 reconnects between them
        if t0:
            bank.reset_stream(1)
            ones[1].close()
            ones[1] = _single(gmc)
        tick_frames = np.ascontiguousarray(np.stack([f[t0:t0 + 4] for f in frames], 1).reshape(12, 720, 1280, 3))
        rows, emb, per = _run(bank, tick_frames, [planted[i % 3][t0 + i // 3] for i in range(12)])
        off = np.concatenate([[0], np.cumsum(per)])
        assert sum(len(r) for r in rows) > 12
        for s in range(3):
            want, wemb, wper = _run(ones[s], frames[s][t0:t0 + 4], planted[s][t0:t0 + 4])
            assert rows[s::3] == want, (t0, s)
            assert per[s::3].tolist() == wper.tolist()
            mine = np.concatenate([emb[off[i]:off[i + 1]] for i in range(s, 12, 3)])
            assert np.array_equal(mine, wemb), (t0, s)
            if gmc:
                gw, w = bank.group_warps(), ones[s].group_warps()
                assert gw.shape == (12, 2, 3) and np.array_equal(gw[s::3], w), (t0, s)
                first = t0 == 0 or s == 1                      # a camera's first frame: the identity; every later one is estimated
                assert np.array_equal(w[0], G.IDENTITY) == first and not any(np.array_equal(x, G.IDENTITY) for x in w[1:])
    for p in ones + [bank]:
        p.close()


def test_pinned_rejections_hold_beside_a_bank_pipeline():
    L = pkg("_lib")
    TP = pkg("pipeline").TrackingPipeline
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    lib = L.load()
    with pytest.raises(ValueError):
        TP(ypath, rpath, (720, 1280), batch=12, ring_frames=12, tracker="botsort", streams=2)
    pipe = TP(ypath, rpath, (720, 1280), batch=12, ring_frames=12, max_persons=16, dtype="fp16", inject=True, tracker="botsort")
    assert lib.aic_pipeline_option(pipe._h, b"streams", 3) == L.ERR_INVALID
    assert lib.aic_pipeline_reset_stream(pipe._h, 0) == L.ERR_INVALID
    pipe.close()
    bank = _bank(4)
    assert lib.aic_pipeline_reset_stream(bank._h, 0) == L.OK and lib.aic_pipeline_reset_stream(bank._h, 2) == L.OK
    assert lib.aic_pipeline_reset_stream(bank._h, 3) == L.ERR_INVALID
    assert lib.aic_pipeline_option(bank._h, b"streams", 3) == L.ERR_INVALID      # the camera count is fixed at creation
    for slot, count in ((0, 4), (1, 3)):                       # run ranges are whole ticks
        assert lib.aic_pipeline_run(bank._h, slot, count, None, None, None, None, None, None, None) == L.ERR_INVALID, (slot, count)
    bank.close()
    import ctypes as C
    eng = pkg("hip_engine").HipEngine
    y, r = eng(ypath, dtype="fp16", max_items=8, warm_up=False), eng(rpath, dtype="fp16", max_items=64, warm_up=False)
    lo, hi = pkg("config").track_class_mask()
    tp = L.TrackerParams(0.2, 0.7, 1, 1, 1, 1, 0, 1)
    bp = pkg("botsort").botsort_params(feature_dim=int(r.out_dim))
    h = C.c_void_p()
    for batch, ring, streams in ((8, 12, 3), (6, 8, 3), (6, 6, 0), (6, 6, 257)):
        prm = L.PipelineParams(720, 1280, batch, ring, 16, 0.1, 0.5, 300, 0.0, 1, (C.c_uint64 * 2)(lo, hi), tp)
        rc = lib.aic_pipeline_create_botsort_bank(y._h, r._h, C.byref(prm), C.byref(bp), streams, C.byref(h))
        assert rc == L.ERR_INVALID and not h.value, (batch, ring, streams)


# ---------------------------------------------------------------------------------------------------- the CLI
def test_cli_inputs_with_botsort_writes_one_output_per_stream(tmp_path):
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    # 1280x720: the size the trained detector sees persons at; every detector call that is compared holds 12 frames
    srcs = ["synthetic:1280x720:6:12:1", "synthetic:1280x720:4:16:2", "synthetic:1280x720:5:12:3"]
    common = ["--yolo_engine", ypath, "--reid_engine", rpath, "--tracker", "botsort", "--gmc", "4", "--batch", "12"]
    assert cli.main(["--inputs", ",".join(srcs), "--output_dir", str(tmp_path / "all")] + common) == 0
    n_tracks = 0
    for k, src in enumerate(srcs):
        assert cli.main(["--input", src, "--output_dir", str(tmp_path / f"one{k}")] + common) == 0
        got = list((tmp_path / "all").glob(f"*_s{k}.jsonl"))
        want = list((tmp_path / f"one{k}").glob("*.jsonl"))
        assert len(got) == 1 and len(want) == 1
        g = [json.loads(l) for l in got[0].read_text().splitlines()]
        w = [json.loads(l) for l in want[0].read_text().splitlines()]
        assert len(g) == 12 and g == w[:12], k                 # the shortest source ends the run
        n_tracks += sum(len(fr["tracks"]) for fr in g)
    assert n_tracks > 0
    with pytest.raises(SystemExit):
        cli.main(["--inputs", ",".join(srcs), "--yolo_engine", ypath, "--tracker", "deepsort"])
