"""Tracker banks on the device: S streams per launch, one kernel block per stream (csrc/kernels_bytetrack.hip, kernels_ocsort.hip,
csrc/epoch_bank.hpp).  A stream of a bank runs the single tracker's code in the single tracker's arithmetic order, so everything is
np.array_equal to single trackers fed the same frames: any difference is cross-stream contamination.  Against the oracles the
scenes and tolerances are those of tests/test_gpu_bytetrack.py / tests/test_gpu_ocsort.py."""
import json

import numpy as np
import pytest

import test_gpu_bytetrack as TB
import test_gpu_ocsort as TO
from conftest import ROOT, pkg
from test_gpu_bytetrack import frames_of

pytestmark = pytest.mark.gpu

KINDS = ["bytetrack", "ocsort"]


def single(kind, **kw):
    return pkg("bytetrack").BYTETracker(**kw) if kind == "bytetrack" else pkg("ocsort").OCSort(**kw)


def bank(kind, streams, **kw):
    return pkg("bytetrack").BYTETrackerBank(streams, **kw) if kind == "bytetrack" else pkg("ocsort").OCSortBank(streams, **kw)


def same_frames(got, want, what):
    assert len(got) == len(want), what
    for f, ((r, c), (wr, wc)) in enumerate(zip(got, want)):
        assert np.array_equal(r, wr) and np.array_equal(c, wc), (what, f, r, wr)


def same_state(bk, s, one):
    e, o = bk.export(s), one.export()
    assert e.keys() == o.keys()
    for key in e:
        assert np.array_equal(e[key], o[key]), (s, key)
    assert bk.counters(s) == one.counters(), s


def run_bank_and_singles(kind, dets, plan, options=(), **kw):
    """dets[s]: the frames of stream s; plan: per call the frames handed to every stream.  The bank against len(dets) singles."""
    S = len(dets)
    bk = bank(kind, S, **kw)
    ones = [single(kind, **kw) for _ in range(S)]
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
SCENES5 = [(30, 3), (12, 9), (5, 11), (20, 4), (1, 7)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("options", [(), (("epoch_frames", 1), ("lsap_fast", 0))])
def test_bank_equals_singles_on_ragged_calls(kind, options):
    dets = [frames_of(TB.scene(n=n, frames=300, seed=seed), 60) for n, seed in SCENES5]
    cyc = (0, 1, 3, 17, 16)                                     # an idle call, a call across the 16-frame epoch, a full epoch
    plan, pos, i = [], [0] * 5, 0
    while min(pos) < 60:
        call = [min(cyc[(i + s) % 5], 60 - pos[s]) for s in range(5)]
        pos = [p + c for p, c in zip(pos, call)]
        plan.append(call)
        i += 1
    assert len(plan) > 5
    _, _, done = run_bank_and_singles(kind, dets, plan, options)
    assert done == [60] * 5


# ---------------------------------------------------------------------------------------------------- against the oracles
def test_bytetrack_bank_against_the_oracle():
    dets = [frames_of(TB.scene(n=30, frames=300, seed=3), 80), frames_of(TB.scene(n=12, frames=80, seed=9), 80)]
    bk = bank("bytetrack", 2)
    oras = [TB.Oracle(), TB.Oracle()]
    for f0 in range(0, 80, 23):
        got = bk.update_arrays([d[f0:f0 + 23] for d in dets])
        for s in range(2):
            for (b, c, k), (rows, conf) in zip(dets[s][f0:f0 + 23], got[s]):
                wr, wc = TB.Oracle.rows(oras[s].update_xyxy(b, c, k))
                assert np.array_equal(rows, wr) and np.array_equal(conf, wc), (s, f0)
    for s in range(2):
        view = type("V", (), {"export": lambda self, s=s: bk.export(s)})()
        TB.compare_export(view, oras[s])


def test_ocsort_bank_against_the_oracle():
    dets = [frames_of(TO.scene(), 80), frames_of(TO.scene(n=12, frames=80, seed=9), 80)]
    bk = bank("ocsort", 2)
    oras = [TO.Oracle(), TO.Oracle()]
    for f0 in range(0, 80, 23):
        got = bk.update_arrays([d[f0:f0 + 23] for d in dets])
        for s in range(2):
            for (b, c, k), (rows, conf) in zip(dets[s][f0:f0 + 23], got[s]):
                wr, wc = TO.Oracle.rows(oras[s].update_xyxy(b, c, k))
                assert np.array_equal(rows, wr) and np.array_equal(conf, wc), (s, f0)
    for s in range(2):
        view = type("V", (), {"export": lambda self, s=s: bk.export(s)})()
        TO.compare_export(view, oras[s])
        c = bk.counters(s)
        assert c == {k: oras[s].stats[k] for k in c}, (s, c, oras[s].stats)


# ---------------------------------------------------------------------------------------------------- per-stream HBM scratch
def test_two_crowds_use_their_own_hbm_scratch():
    Scene = pkg("synthetic").Scene
    dets = [frames_of(Scene(seed=seed, n_targets=150, conf_range=(0.05, 0.95), jitter=2.0, shuffle=True, w_range=(30.0, 50.0),
                            h_range=(80.0, 120.0)), 20) for seed in (21, 22)]
    bk, _, _ = run_bank_and_singles("bytetrack", dets, [[16, 16], [4, 4]], (("lsap_fast", 0),))
    for s in range(2):
        assert bk.counters(s)["max_side"] > 128, s             # both streams' extended matrices are beyond the LDS arena, in one launch


# ---------------------------------------------------------------------------------------------------- many blocks
@pytest.mark.parametrize("kind", KINDS)
def test_forty_streams_one_tick_per_call(kind):
    Scene = pkg("synthetic").Scene
    dets = [frames_of(Scene(seed=100 + s, n_targets=3, conf_range=(0.05, 0.95), jitter=1.5, shuffle=True), 20) for s in range(40)]
    run_bank_and_singles(kind, dets, [[1] * 40] * 20)


# ---------------------------------------------------------------------------------------------------- failure is contained
@pytest.mark.parametrize("kind", KINDS)
def test_a_failing_stream_stops_alone(kind):
    L = pkg("_lib")
    Scene = pkg("synthetic").Scene
    kw = dict(max_tracks=8, first_track_id=7)
    dets = [frames_of(Scene(seed=31, n_targets=5, conf_range=(0.8, 0.95)), 8),
            frames_of(Scene(seed=4, n_targets=20, conf_range=(0.8, 0.95)), 8),
            frames_of(Scene(seed=32, n_targets=5, conf_range=(0.8, 0.95)), 8)]
    bk = bank(kind, 3, **kw)
    ones = [single(kind, **kw) for _ in range(3)]
    for f0 in (0, 2):                                          # the failing call and the next
        got = bk.update_arrays([d[f0:f0 + 2] for d in dets])
        assert got[1] is None and 1 in bk.failed and list(bk.failed) == [1]
        for s in (0, 2):
            same_frames(got[s], ones[s].update_batch_arrays(dets[s][f0:f0 + 2]), (s, f0))
    with pytest.raises(L.AicError) as ei:
        bk.export(1)
    assert ei.value.code == L.ERR_INVALID
    for s in (0, 2):
        same_state(bk, s, ones[s])
    # the raw call: status holds the code per stream and the call is OK; with status NULL the stopped stream's code comes back
    fps = np.array([0, 1, 0], np.int32)
    b, c, k = dets[1][4]
    b, c, k = np.ascontiguousarray(b, np.float32), np.ascontiguousarray(c, np.float32), np.ascontiguousarray(k, np.int32)
    counts = np.array([len(b)], np.int32)
    n_out, status = np.full(1, -1, np.int32), np.zeros(3, np.int32)
    fn = getattr(L.load(), f"aic_{kind}_bank_update")
    args = (bk._h, L.ptr(fps), L.ptr(counts), L.ptr(b), L.ptr(c), L.ptr(k), 8, L.ptr(n_out), None, None)
    assert fn(*args, L.ptr(status)) == L.OK
    assert status.tolist() == [0, L.ERR_CAPACITY, 0] and n_out[0] == 0
    assert fn(*args, None) == L.ERR_CAPACITY
    assert b"stream 1" in L.load().aic_last_error()
    # a fresh bank: the failure itself through the raw call with status NULL
    bk2 = bank(kind, 3, **kw)
    flat = [fr for d in dets for fr in d[:2]]
    bb = np.ascontiguousarray(np.concatenate([x[0] for x in flat]), np.float32)
    cc = np.ascontiguousarray(np.concatenate([x[1] for x in flat]), np.float32)
    kk = np.ascontiguousarray(np.concatenate([x[2] for x in flat]), np.int32)
    cnt = np.array([len(x[0]) for x in flat], np.int32)
    n6 = np.zeros(6, np.int32)
    rc = fn(bk2._h, L.ptr(np.array([2, 2, 2], np.int32)), L.ptr(cnt), L.ptr(bb), L.ptr(cc), L.ptr(kk), 8, L.ptr(n6), None, None, None)
    assert rc == L.ERR_CAPACITY and b"stream 1" in L.load().aic_last_error()
    assert n6[0] > 0 and n6[4] > 0                             # the other streams' frames of the same call were processed
    # a camera reconnecting: the stream equals a fresh single tracker, ids from first_track_id
    bk.reset(1)
    assert not bk.failed
    again = frames_of(Scene(seed=33, n_targets=5, conf_range=(0.8, 0.95)), 6)
    fresh = single(kind, **kw)
    got = bk.update_arrays([[], again, []])
    want = fresh.update_batch_arrays(again)
    same_frames(got[1], want, "after reset")
    same_state(bk, 1, fresh)
    assert min(int(r[:, 4].min()) for r, _ in want if len(r)) == 7
    for s in (0, 2):                                           # untouched by the neighbour's reset
        same_state(bk, s, ones[s])


@pytest.mark.parametrize("kind", KINDS)
def test_a_frame_with_513_detections_rejects_the_whole_call(kind):
    L = pkg("_lib")
    Scene = pkg("synthetic").Scene
    bk = bank(kind, 2)
    ok = frames_of(Scene(seed=41, n_targets=4, conf_range=(0.8, 0.95)), 3)
    bk.update_arrays([ok[:1], ok[:1]])
    before = [bk.export(s) for s in range(2)]
    big = (np.tile(np.array([[0, 0, 10, 10]], np.float32), (513, 1)), np.full(513, 0.9, np.float32), np.zeros(513, np.int32))
    with pytest.raises(L.AicError) as ei:
        bk.update_arrays([ok[1:3], [big]])
    assert ei.value.code == L.ERR_CAPACITY and not bk.failed
    one = single(kind)
    one.update_batch_arrays(ok[:1])
    for s in range(2):                                         # nothing was launched: no stream advanced
        same_state(bk, s, one)
        for key in before[s]:
            assert np.array_equal(before[s][key], bk.export(s)[key]), key
    got = bk.update_arrays([ok[1:3], ok[1:3]])
    same_frames(got[0], one.update_batch_arrays(ok[1:3]), "after the rejected call")


def test_update_one_tick_with_a_missing_camera():
    Scene = pkg("synthetic").Scene
    dets = frames_of(Scene(seed=51, n_targets=4, conf_range=(0.8, 0.95)), 3)
    bk, one = bank("bytetrack", 3), single("bytetrack")
    for d in dets:
        got = bk.update([d, None, d])
        want = one.update(*d)
        assert got[0] == want and got[2] == want and got[1] == []
    assert bk.export(1)["track_id"].size == 0


# ---------------------------------------------------------------------------------------------------- the pipeline
def _pipe(ypath, tracker, n, batch, **kw):
    TP = pkg("pipeline").TrackingPipeline
    return TP(ypath, None, (720, 1280), batch=batch, ring_frames=n, max_persons=128, dtype="fp16", inject=True, tracker=tracker, **kw)


_SINGLE_PIPES = {}


def _planted():
    return [[TB.scene(n=n, frames=120, seed=seed).detections(f)[:3] for f in range(24)] for n, seed in ((30, 5), (12, 9), (5, 11))]


def _single_pipelines(ypath, tracker):
    """tracks[s][t] of three single-stream pipelines on the de-interleaved boxes (computed once per tracker)."""
    if tracker not in _SINGLE_PIPES:
        out = []
        for planted in _planted():
            pipe = _pipe(ypath, tracker, 24, 12)
            pipe.upload(0, np.zeros((24, 720, 1280, 3), np.uint8))
            pipe.inject(0, planted)
            out.append(pipe.run(0, 24)[0])
            pipe.close()
        _SINGLE_PIPES[tracker] = out
    return _SINGLE_PIPES[tracker]


# batch 48: the taper's shrinking groups (48, 15, 9 frames) round to whole ticks
@pytest.mark.parametrize("tracker,batch,group_frames,taper", [("bytetrack", 12, 0, 1), ("bytetrack", 12, 3, 1), ("bytetrack", 12, 0, 0),
                                                              ("ocsort", 12, 0, 1), ("bytetrack", 48, 0, 1)])
def test_pipeline_streams_equal_single_stream_pipelines(tracker, batch, group_frames, taper):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    want = _single_pipelines(ypath, tracker)
    planted = _planted()
    pipe = _pipe(ypath, tracker, 72, batch, streams=3)
    pipe.option("group_frames", group_frames)
    pipe.option("taper", taper)
    pipe.upload(0, np.zeros((72, 720, 1280, 3), np.uint8))
    pipe.inject(0, [planted[i % 3][i // 3] for i in range(72)])          # tick-major: slot t * 3 + s
    tracks, _ = pipe.run(0, 72)
    assert all(sum(len(t) for t in w) > 0 for w in want)                   # every stream has rows to compare
    for i in range(72):
        assert tracks[i] == want[i % 3][i // 3], (i % 3, i // 3)
    pipe.close()


def test_pipeline_streams_rejections():
    L = pkg("_lib")
    TP = pkg("pipeline").TrackingPipeline
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    for kw in (dict(tracker="deepsort"), dict(tracker="botsort")):
        pipe = TP(ypath, rpath, (720, 1280), batch=12, ring_frames=12, max_persons=16, dtype="fp16", inject=True, **kw)
        assert L.load().aic_pipeline_option(pipe._h, b"streams", 3) == L.ERR_INVALID, kw
        assert L.load().aic_pipeline_reset_stream(pipe._h, 0) == L.ERR_INVALID, kw
        pipe.close()
    with pytest.raises(L.AicError) as ei:                       # batch is not a multiple of streams
        _pipe(ypath, "bytetrack", 24, 8, streams=3)
    assert ei.value.code == L.ERR_INVALID
    pipe = _pipe(ypath, "bytetrack", 24, 12, streams=3)
    pipe.upload(0, np.zeros((24, 720, 1280, 3), np.uint8))
    pipe.inject(0, [p for tick in zip(*_planted()) for p in tick][:24])
    lib = L.load()
    for slot, count in ((0, 4), (1, 3), (2, 12)):
        assert lib.aic_pipeline_run(pipe._h, slot, count, None, None, None, None, None, None, None) == L.ERR_INVALID, (slot, count)
    assert lib.aic_pipeline_option(pipe._h, b"streams", 4) == L.OK          # nothing has run yet (batch 12 holds whole ticks of 4)
    assert lib.aic_pipeline_option(pipe._h, b"streams", 3) == L.OK
    pipe.run(0, 24)
    assert lib.aic_pipeline_option(pipe._h, b"streams", 4) == L.ERR_INVALID  # frames have gone through the tracker
    pipe.reset_stream(2)
    with pytest.raises(L.AicError):
        pipe.reset_stream(3)
    pipe.close()


def test_pipeline_stream_that_exhausts_max_tracks_delivers_nothing_of_its_group():
    """max_tracks 16, at most 5 planted boxes per camera; camera 1 gets 18 more boxes in tick 2: more rows than its table holds.  An epoch
    tracker's check raises BEFORE any row of the launch group is copied out (the DeepSORT bank pipeline delivers the other cameras' rows and
    then raises: test_a_camera_that_exhausts_max_tracks_stops_alone): the caller's track arrays are untouched, run calls are refused until
    reset_stream(1)."""
    L = pkg("_lib")
    lib = L.load()
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    planted = [[(b[:5], c[:5], k[:5]) for b, c, k in cam[:4]] for cam in _planted()]
    gx, gy = np.meshgrid(np.arange(9) * 135.0 + 40.0, np.arange(2) * 300.0 + 60.0)
    more = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 60.0, gy.ravel() + 140.0], 1).astype(np.float32)
    b, c, k = planted[1][2]
    planted[1][2] = (np.concatenate([b, more]), np.concatenate([c, np.full(18, 0.8, np.float32)]), np.concatenate([k, np.zeros(18, np.int32)]))
    pipe = _pipe(ypath, "bytetrack", 12, 12, streams=3, max_tracks=16)
    pipe.option("taper", 0)                                      # the call is one launch group
    pipe.upload(0, np.zeros((12, 720, 1280, 3), np.uint8))
    pipe.inject(0, [planted[i % 3][i // 3] for i in range(12)])  # tick-major: slot t * 3 + s
    mp = pipe.max_persons
    nt, r6, cf = np.full(12, -7, np.int32), np.full((12, mp, 6), -7, np.int32), np.full((12, mp), -7.0, np.float32)
    args = (pipe._h, 0, 12, L.ptr(nt), L.ptr(r6), L.ptr(cf), None, None, None, None)
    assert lib.aic_pipeline_run(*args) == L.ERR_CAPACITY
    msg = lib.aic_last_error()
    assert b"stream 1" in msg and b"max_tracks" in msg, msg
    assert (nt == -7).all() and (r6 == -7).all() and (cf == -7.0).all()     # nothing of the group was delivered
    assert lib.aic_pipeline_run(*args) == L.ERR_INVALID
    assert (nt == -7).all() and (r6 == -7).all() and (cf == -7.0).all()
    pipe.reset_stream(1)
    planted[1][2] = (b, c, k)                                    # the camera reconnects to a scene its table holds
    pipe.inject(0, [planted[i % 3][i // 3] for i in range(12)])
    assert lib.aic_pipeline_run(*args) == L.OK
    assert (nt >= 0).all()
    pipe.close()


def test_cli_inputs_writes_one_output_per_stream(tmp_path):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    srcs = ["synthetic:640x360:6:24:1", "synthetic:640x360:4:16:2"]      # every detector call of the three runs holds 8 frames
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--batch", "8"]
    assert cli.main(["--inputs", ",".join(srcs), "--output_dir", str(tmp_path / "both")] + common) == 0
    for k, src in enumerate(srcs):
        assert cli.main(["--input", src, "--output_dir", str(tmp_path / f"one{k}")] + common) == 0
        got = list((tmp_path / "both").glob(f"*_s{k}.jsonl"))
        want = list((tmp_path / f"one{k}").glob("*.jsonl"))
        assert len(got) == 1 and len(want) == 1
        g = [json.loads(l) for l in got[0].read_text().splitlines()]
        w = [json.loads(l) for l in want[0].read_text().splitlines()]
        assert len(g) == 16 and g == w[:16], k                 # the shortest source ends the run
    with pytest.raises(SystemExit):
        cli.main(["--inputs", ",".join(srcs), "--input", srcs[0]] + common)
    with pytest.raises(SystemExit):
        cli.main(["--inputs", ",".join(srcs), "--yolo_engine", ypath, "--tracker", "deepsort"])
