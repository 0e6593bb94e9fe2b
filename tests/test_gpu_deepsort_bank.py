"""The DeepSORT bank (aic_deepsort_bank_*, csrc/deepsort_bank.hpp; block s of trk_epoch_kernel = stream s) against what it must equal:
the trajectories the reference wrote (tests/golden/traj*.npz), and single device trackers (aic_tracker_update_batch) fed the same frames
stream by stream.  A stream of a bank is the single tracker's code in its arithmetic order, so everything is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_rows_equal_or_on_rounding_edge, fixture_float_rows, pkg
from oracle import deepsort_oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("track_id", "state", "hits", "age", "time_since_update", "cls", "gallery_len", "conf", "mean", "cov")


def _single(tk, max_tracks, first=1):
    """A TrackerCore over an aic_tracker with the bank's parameters (the class's own constructor fixes first_track_id = 1)."""
    L, TC = pkg("_lib"), pkg("core.tracker_core").TrackerCore
    p = pkg("deepsort_bank").deepsort_bank_params(max_tracks=max_tracks, feature_dim=0, first_track_id=first, **tk)
    h = C.c_void_p()
    L.call("aic_tracker_create", 0, C.byref(p), C.byref(h))
    t = TC._from_handle(h, p)
    t._owned = True
    return t


def _options(objs, **opts):
    for o in objs:
        for k, v in opts.items():
            o.option(k, v)


def _frames(scene, f0, n, dim, seed, noise=0.01, featless=0, valid=None):
    """n frames of a synthetic.Scene from frame f0 as update_batch tuples (tlwh, conf, cls, feats, has)."""
    syn = pkg("synthetic")
    out = []
    for f in range(f0, f0 + n):
        boxes, conf, cls, ids = scene.detections(f)
        tlwh = boxes.copy()
        tlwh[:, 2:] -= tlwh[:, :2]
        has = np.ones(len(ids), np.uint8)
        if featless:
            has[(np.arange(len(ids)) + f) % featless == 0] = 0
        if valid is not None:
            has[:] = valid
        out.append((tlwh.astype(np.float32), conf, cls, syn.identity_features(ids, f, dim=dim, seed=seed, noise=noise), has))
    return out


def _step(bank, singles, per_stream, skip=()):
    """One bank call and the same frames through the singles; the rows and conf of every frame must be equal.  Returns the bank's result."""
    got = bank.update_arrays(per_stream)
    for s, (trk, frames) in enumerate(zip(singles, per_stream)):
        if s in skip or not frames:
            continue
        want = trk.update_batch(frames, cap_rows=bank.max_tracks)
        assert len(got[s]) == len(want), s
        for i, ((r, c), (wr, wc, _)) in enumerate(zip(got[s], want)):
            assert np.array_equal(r, wr) and np.array_equal(c, wc), (s, i)
    return got


def _same_state(bank, singles, skip=(), galleries=True):
    """Export, every gallery and the counters of every stream equal the single tracker's."""
    for s, trk in enumerate(singles):
        if s in skip:
            continue
        a, b = trk.export_arrays(), bank.export(s)
        for key in KEYS:
            assert np.array_equal(a[key], b[key]), (s, key)
        if galleries and trk._dim:
            for i, gl in enumerate(a["gallery_len"]):
                assert np.array_equal(trk._gallery(i, int(gl)), bank.export_gallery(s, i, int(gl))), (s, i)
        assert trk.assoc_counters() == bank.counters(s), s


_inputs = {}


def _traj(name, n):
    """The first n frames of the fixture's inputs, computed once per session: frame -> update_batch tuple."""
    from golden.traj_config import scene_inputs
    if name not in _inputs:
        frames = []
        for f in range(n):
            tlwh, conf, ids, feats, has = scene_inputs(name, f)
            frames.append((tlwh, conf, np.zeros(len(ids), np.int32), feats, has.astype(np.uint8)))
        _inputs[name] = frames
    return _inputs[name]


@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("name", ["traj8", "traj30"])
def test_reference_fixtures_inside_a_bank(gpu, golden, name, K):
    """A bank has ONE parameter set and feature dimension, and traj8 (budget-4 rings that wrap inside epochs, dim 32) and traj30 (defaults,
    dim 512) were written with different ones: each fixture gets its own bank of three streams -- the fixture, an idle stream (no frames
    in odd calls, empty frames in even ones) and the same fixture one call behind -- fed in chunks of K frames.  Ids and rows of every
    frame, and ids, states, hits, age, tsu and gallery lengths after every call, equal the fixture the reference wrote; export and
    every gallery equal a single aic_tracker fed the same frames."""
    from golden.traj_config import TRAJ
    g = golden(name)
    _, tk, frames, dim, _ = TRAJ[name]
    if name == "traj30":
        frames = 44                                              # a birth at 25, a 2-frame gap at 30 and one opening at 40: what a few seconds hold
    inp = _traj(name, frames)
    bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=64, feature_dim=dim, **tk)
    one = _single(tk, 64)
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), None, None)

    def check_rows(rows, f):
        no = int(g["n_out"][f])
        assert len(rows) == no, f
        if no:
            assert np.array_equal(rows[:, 4], g["out"][f, :no, 4]), f
            assert_rows_equal_or_on_rounding_edge(rows[:, :4], g["out"][f, :no, :4], fixture_float_rows(g, f, O), (name, f))

    def check_table(a, f):
        nt = int(g["n_tracks"][f])
        assert a["track_id"].tolist() == g["tid"][f, :nt].tolist(), f
        assert a["state"].tolist() == g["state"][f, :nt].tolist(), f
        assert a["hits"].tolist() == g["hits"][f, :nt].tolist() and a["age"].tolist() == g["age"][f, :nt].tolist(), f
        assert a["time_since_update"].tolist() == g["tsu"][f, :nt].tolist() and a["gallery_len"].tolist() == g["glen"][f, :nt].tolist(), f
        if nt:
            assert float(np.abs(a["mean"] - g["mean"][f, :nt]).max()) < 1e-3, f

    call, f0 = 0, 0
    while f0 - K < frames:                                       # the lagging stream needs one more call
        lead = inp[f0:min(f0 + K, frames)]
        lag = inp[f0 - K:min(f0, frames)] if f0 else []
        got = bank.update_arrays([lead, [] if call % 2 else [empty] * 2, lag])
        assert not bank.failed
        want = one.update_batch(lead, cap_rows=64) if lead else []
        for i, (rows, conf) in enumerate(got[0]):
            check_rows(rows, f0 + i)
            assert np.array_equal(rows, want[i][0]) and np.array_equal(conf, want[i][1]), f0 + i
        for i, (rows, _) in enumerate(got[2]):
            check_rows(rows, f0 - K + i)
        assert all(len(r) == 0 for r, _ in got[1])
        if lead:
            check_table(bank.export(0), f0 + len(lead) - 1)
        if lag:
            check_table(bank.export(2), min(f0, frames) - 1)
        if lead and (call % 4 == 0 or f0 + K >= frames):
            _same_state(bank, [one], galleries=dim <= 64 or f0 + K >= frames)
        call, f0 = call + 1, f0 + K
    assert len(bank.export(1)["track_id"]) == 0 and bank.counters(1) == (0, 0)
    last = bank.export(2)
    for key in KEYS:
        assert np.array_equal(last[key], one.export_arrays()[key]), key


@pytest.mark.parametrize("epoch_frames,lsap_fast,wave", [(1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 0), (1, 0, 1), (1, 1, 0)])
def test_ragged_calls_equal_the_single_trackers(gpu, epoch_frames, lsap_fast, wave):
    """Four streams of 30 / 12 / 5 / 1 persons with their own feature seeds, calls of 0 / 1 / 3 / 17 / 16 frames in rotation (a different
    phase per stream), budget-6 rings that wrap, featureless rows: rows, conf, export, galleries and counters equal the singles'."""
    syn = pkg("synthetic")
    tk = dict(nn_budget=6, max_age=8)
    persons = (30, 12, 5, 1)
    scenes = [syn.Scene(seed=40 + s, n_targets=n, jitter=1.5, shuffle=True, gaps=[(0, 6, 9), (n // 2, 12, 24)], births={n - 1: 7})
              for s, n in enumerate(persons)]
    bank = pkg("deepsort_bank").DeepSORTBank(4, max_tracks=64, feature_dim=64, **tk)
    singles = [_single(tk, 64) for _ in persons]
    _options([bank] + singles, epoch_frames=epoch_frames, lsap_fast=lsap_fast, wave_cascade=wave)
    sizes = (0, 1, 3, 17, 16)
    at = [0] * 4
    for call in range(5):
        per = []
        for s in range(4):
            n = sizes[(call + s) % 5]
            per.append(_frames(scenes[s], at[s], n, 64, seed=70 + s, noise=0.03, featless=5))
            at[s] += n
        _step(bank, singles, per)
        _same_state(bank, singles, galleries=call == 4)
    fast, slow = zip(*(bank.counters(s) for s in range(4)))
    assert (sum(fast) == 0) == (lsap_fast == 0) and (lsap_fast or sum(slow) > 0), (fast, slow)


def test_streams_that_differ_in_kind_in_one_launch(gpu):
    """One launch, five kinds of block: 70 detections per frame (past the one-wavefront cascade), two streams of 150 persons whose
    matrices go to HBM scratch (each must use its own slice), 3 persons, and detections none of which has a feature (no SM for that
    stream); max_tracks 256 at feature_dim 512.  8 frames in one call, results equal the singles'."""
    syn = pkg("synthetic")
    wide = dict(width=1920, height=1080, w_range=(30, 60), h_range=(90, 150), y_range=(50, 850), jitter=1.0, shuffle=True)
    tk = dict(nn_budget=4)
    scenes = [syn.Scene(seed=50, n_targets=70, **wide), syn.Scene(seed=51, n_targets=150, **wide), syn.Scene(seed=52, n_targets=150, **wide),
              syn.Scene(seed=53, n_targets=3), syn.Scene(seed=54, n_targets=9)]
    bank = pkg("deepsort_bank").DeepSORTBank(5, max_tracks=256, feature_dim=512, **tk)
    singles = [_single(tk, 256) for _ in scenes]
    per = [_frames(sc, 0, 8, 512, seed=80 + s, valid=0 if s == 4 else None) for s, sc in enumerate(scenes)]
    got = _step(bank, singles, per)
    assert all(len(got[s][-1][0]) > 0 for s in range(5))
    _same_state(bank, singles, galleries=False)
    for s in (0, 3):
        a = bank.export(s)
        for i in (0, len(a["track_id"]) - 1):
            assert np.array_equal(singles[s]._gallery(i, int(a["gallery_len"][i])), bank.export_gallery(s, i, int(a["gallery_len"][i])))
    assert not bank.export(4)["gallery_len"].any()


def test_common_epoch_length_is_cut_by_the_fullest_stream(gpu):
    """5 frames x 450 detections are more than the 2048 rows of an epoch: the launch's common k is cut for every stream, the small
    stream beside it included.  Only the results are asserted: equal to the singles', which cut their own epochs."""
    syn = pkg("synthetic")
    big = syn.Scene(seed=60, n_targets=450, width=3840, height=2160, w_range=(20, 40), h_range=(40, 80), y_range=(20, 2000), jitter=0.5)
    small = syn.Scene(seed=61, n_targets=4, jitter=1.0)
    tk = dict(nn_budget=4)
    bank = pkg("deepsort_bank").DeepSORTBank(2, max_tracks=512, feature_dim=32, **tk)
    singles = [_single(tk, 512), _single(tk, 512)]
    got = _step(bank, singles, [_frames(big, 0, 5, 32, seed=90), _frames(small, 0, 7, 32, seed=91)])
    assert len(got[0][-1][0]) > 400 and len(got[1][-1][0]) == 4
    _same_state(bank, singles, galleries=False)


def test_a_failing_stream_stops_alone(gpu, lib):
    """max_tracks 8; the middle stream's scene grows from 5 to 12 persons at frame 4.  The kernel reports the exhausted table itself
    (header err = 1): the stream's rows before that frame are delivered, its status is AIC_ERR_CAPACITY, export is refused, the neighbours
    equal the singles; reset(1) starts it afresh from first_track_id."""
    syn = pkg("synthetic")
    tk = dict(nn_budget=5)
    scenes = [syn.Scene(seed=30, n_targets=4, jitter=1.0), syn.Scene(seed=31, n_targets=12, births={i: 4 for i in range(5, 12)}),
              syn.Scene(seed=32, n_targets=6, jitter=1.0)]
    bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=8, feature_dim=64, first_track_id=100, **tk)
    singles = [_single(tk, 8, first=100) for _ in scenes]
    per = [_frames(sc, 0, 7, 64, seed=20 + s) for s, sc in enumerate(scenes)]
    got = _step(bank, singles, per, skip=(1,))
    assert got[1] is None and list(bank.failed) == [1]
    want = singles[1].update_batch(per[1][:4], cap_rows=8)          # the frames before the failing one
    fps = np.array([0, 7, 0], np.int32)
    # what the call delivered for the stopped stream: read again through the C ABI, which now delivers nothing for it and, with
    # status = NULL, returns the stream's code
    counts = np.array([len(f[0]) for f in per[1]], np.int32)
    tot = int(counts.sum())
    n_out = np.full(7, -1, np.int32)
    rc = lib.load().aic_deepsort_bank_update(bank._h, lib.ptr(fps), lib.ptr(counts), lib.ptr(np.zeros((tot, 4), np.float32)),
                                             lib.ptr(np.zeros(tot, np.float32)), lib.ptr(np.zeros(tot, np.int32)), None, None, 8,
                                             lib.ptr(n_out), None, None, None)
    assert rc == lib.ERR_CAPACITY and b"capacity" in lib.load().aic_last_error() and n_out.tolist() == [0] * 7
    with pytest.raises(lib.AicError) as e:
        bank.export(1)
    assert e.value.code == lib.ERR_INVALID
    _same_state(bank, singles, skip=(1,))
    # a bank of one shows the rows of the failing call itself: frames 0..3 as the single's, none from frame 4 on
    status = np.zeros(3, np.int32)
    b3 = pkg("deepsort_bank").DeepSORTBank(1, max_tracks=8, feature_dim=64, first_track_id=100, **tk)
    flat = per[1]
    tlwh, conf, cls = (np.ascontiguousarray(np.concatenate([f[k] for f in flat])) for k in range(3))
    feats = np.ascontiguousarray(np.concatenate([f[3] for f in flat]))
    n_out, out6, oc = np.zeros(7, np.int32), np.zeros((7, 8, 6), np.int32), np.zeros((7, 8), np.float32)
    lib.call("aic_deepsort_bank_update", b3._h, lib.ptr(np.array([7], np.int32)), lib.ptr(counts), lib.ptr(tlwh), lib.ptr(conf),
             lib.ptr(cls.astype(np.int32)), lib.ptr(feats), None, 8, lib.ptr(n_out), lib.ptr(out6), lib.ptr(oc), lib.ptr(status[:1]))
    assert status[0] == lib.ERR_CAPACITY and n_out[4:].tolist() == [0, 0, 0]
    assert n_out[:4].tolist() == [len(w[0]) for w in want] and n_out[3] == 5
    for i, (wr, wc, _) in enumerate(want):
        assert np.array_equal(out6[i, :n_out[i]], wr) and np.array_equal(oc[i, :n_out[i]], wc), i
    # the camera reconnects
    bank.reset(1)
    assert not bank.failed and len(bank.export(1)["track_id"]) == 0
    fresh = _single(tk, 8, first=100)
    singles[1] = fresh
    small = syn.Scene(seed=33, n_targets=5, jitter=1.0)
    per = [_frames(scenes[0], 7, 4, 64, seed=20), _frames(small, 0, 4, 64, seed=25), _frames(scenes[2], 7, 4, 64, seed=22)]
    got = _step(bank, singles, per)
    assert got[1][-1][0][:, 4].tolist() == [100, 101, 102, 103, 104]
    _same_state(bank, singles)


def test_a_513_detection_frame_rejects_the_whole_call(gpu, lib):
    """More than 512 detections in one frame: AIC_ERR_CAPACITY before anything is staged; the bank is unchanged and goes on as the singles."""
    syn = pkg("synthetic")
    tk = dict(nn_budget=5)
    scenes = [syn.Scene(seed=35, n_targets=5, jitter=1.0), syn.Scene(seed=36, n_targets=7, jitter=1.0)]
    bank = pkg("deepsort_bank").DeepSORTBank(2, max_tracks=16, feature_dim=64, **tk)
    singles = [_single(tk, 16), _single(tk, 16)]
    _step(bank, singles, [_frames(sc, 0, 5, 64, seed=10 + s) for s, sc in enumerate(scenes)])
    huge = (np.tile(np.array([[5, 5, 20, 40]], np.float32), (513, 1)), np.full(513, 0.9, np.float32), np.zeros(513, np.int32), None, None)
    with pytest.raises(lib.AicError) as e:
        bank.update_arrays([_frames(scenes[0], 5, 2, 64, seed=10), [huge]])
    assert e.value.code == lib.ERR_CAPACITY and "512" in str(e.value)
    assert not bank.failed
    _same_state(bank, singles)
    _step(bank, singles, [_frames(sc, 5, 4, 64, seed=10 + s) for s, sc in enumerate(scenes)])
    _same_state(bank, singles)
