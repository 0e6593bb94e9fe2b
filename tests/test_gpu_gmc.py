"""Camera motion on the device (csrc/kernels_gmc.hip) against the NumPy specification (tests/gmc_oracle.py): warps and stats are
np.array_equal -- the sums of the fit are integers and the fp64 sequence has a stated order, so there is no tolerance anywhere."""
import json

import numpy as np
import pytest

import gmc_oracle as G
from botsort_oracle import BoTSORT as Oracle
from conftest import ROOT, pkg
from test_gmc_oracle import GAP, PAYOFF, payoff_scene, tie_frames

pytestmark = pytest.mark.gpu

H, W = 360, 640


def oracle_stream(frames, boxes, s, min_inliers=8, est=None):
    est = est or G.Stream(s, min_inliers)
    out = [est.apply(f, None if boxes is None else boxes[i]) for i, f in enumerate(frames)]
    return np.stack([w for w, _ in out]), np.stack([G.stats4(st) for _, st in out]), [st for _, st in out]


@pytest.fixture(scope="module")
def moving():
    sc = pkg("synthetic").PanningScene(seed=4, pan=(5.3, 2.7), rot_deg=0.5, zoom=1.01, n_targets=4, speed=2.0, pad=128)
    return sc.render_batch(0, 6), [sc.detections(f)[0] for f in range(6)]


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("with_boxes", [False, True])
def test_estimator_against_oracle(moving, s, with_boxes):
    import torch
    frames, boxes = moving
    boxes = boxes if with_boxes else None
    want_w, want_s, full = oracle_stream(frames, boxes, s)
    assert want_s[1:, 0].all() and (not with_boxes or any(st["masked"] for st in full))
    cm = pkg("gmc").CameraMotion(H, W, downscale=s)
    got = cm.apply_batch(frames, boxes)                            # host memory, one call
    assert np.array_equal(cm.stats, want_s), (cm.stats, want_s)
    assert np.array_equal(got, want_w), np.abs(got - want_w).max()
    cm.reset()                                                     # device memory, 3 + 3: the carried gray level
    t = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    a = cm.apply_batch((t[:3].data_ptr(), 3), None if boxes is None else boxes[:3])
    sa = cm.stats
    b = cm.apply_batch((t[3:].data_ptr(), 3), None if boxes is None else boxes[3:])
    assert np.array_equal(np.concatenate([a, b]), want_w) and np.array_equal(np.concatenate([sa, cm.stats]), want_s)
    one = cm.apply(frames[5], None if boxes is None else boxes[5])  # the same frame again: no motion
    w0, st0 = G.estimate(frames[5], frames[5], None if boxes is None else boxes[5], s)
    assert np.array_equal(one, w0) and np.array_equal(cm.stats[0], G.stats4(st0))
    cm.close()


def _texture(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return np.floor(pkg("synthetic")._smooth_noise(rng, h + 64, w + 64) + 0.5).astype(np.uint8)


def _pair(h, w, dx, dy, seed=0):
    t = _texture(h, w, seed)
    return np.stack([t[32:32 + h, 32:32 + w], t[32 - dy:32 - dy + h, 32 - dx:32 - dx + w]])


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("case", ["one_block", "degenerate", "short_of_second_column", "odd", "all_masked", "ties", "border"])
def test_smallest_shapes(s, case):
    boxes, mi = None, 8
    if case == "one_block":
        frames = _pair(32 * s, 32 * s, s, 0)
    elif case == "degenerate":                                     # one block and min_inliers = 1: the fit stops on V <= 0
        frames, mi = _pair(32 * s, 32 * s, s, 0), 1
    elif case == "short_of_second_column":
        frames = _pair(32 * s, 48 * s - 1, s, s)
    elif case == "odd":                                            # not multiples of s; two blocks and a fit from two
        frames, mi = _pair(32 * s + s - 1, 48 * s + 3 * s - 1, 2 * s, -s), 2
    elif case == "all_masked":
        frames = _pair(64 * s, 80 * s, s, 0)
        boxes = [np.zeros((0, 4), np.float32), np.array([[0, 0, 80 * s, 64 * s]], np.float32)]
    elif case == "ties":                                           # four equal minima at dy = 0: the first, dx = -6, is interior and must win
        frames = tie_frames(s)
    else:                                                          # the true minimum on the border of the search square
        frames = _pair(64 * s, 80 * s, 8 * s, 0)
    h, w = frames.shape[1:3]
    want_w, want_s, full = oracle_stream(frames, boxes, s, mi)
    st = full[1]
    if case == "one_block":
        assert st["blocks"] == 1 and st["kept"] == 1
    elif case == "degenerate":
        assert st["degenerate"] == 1 and want_s[1].tolist() == [0, 1, 1, 1]
    elif case == "short_of_second_column":
        assert st["blocks"] == 1 and st["kept"] == 1
    elif case == "odd":
        assert st["blocks"] == 2 and st["ok"] == 1 and np.array_equal(want_w[1], np.array([[1, 0, 2 * s], [0, 1, -s]], np.float32))
    elif case == "all_masked":
        assert st["masked"] == st["blocks"] == 12
    elif case == "ties":
        assert st["ok"] == 1 and st["inliers"] == 12 and np.array_equal(want_w[1], np.array([[1, 0, -6 * s], [0, 1, 0]], np.float32))
    else:
        assert st["border"] == st["blocks"] == 12
    cm = pkg("gmc").CameraMotion(h, w, downscale=s, min_inliers=mi)
    got = cm.apply_batch(frames, boxes)
    assert np.array_equal(cm.stats, want_s), (cm.stats, want_s)
    assert np.array_equal(got, want_w)
    cm.close()


def test_more_blocks_than_fit_threads():
    """1280 x 720 at s = 2: 819 blocks for the 256 threads of the fit kernel (strided loops, rank counting over all of them)."""
    frames = _pair(720, 1280, 6, -4, seed=3)
    want_w, want_s, _ = oracle_stream(frames, None, 2)
    assert want_s[1].tolist() == [1, 819, 819, 819]
    cm = pkg("gmc").CameraMotion(720, 1280, downscale=2)
    assert np.array_equal(cm.apply_batch(frames), want_w) and np.array_equal(cm.stats, want_s)
    cm.close()


@pytest.mark.parametrize("epoch_frames", [1, 16])
def test_tracker_with_estimated_warps(epoch_frames):
    """BoTSORT fed CameraMotion's warps on the payoff scene against the oracle fed gmc_oracle's: rows, ids, mean and covariance,
    with one frame and with 16 frames per epoch launch (calls of 13 frames: epochs of 13 at 16, and an epoch never starts at 0 mod 16)."""
    from test_gpu_botsort import run_pair
    sc, n = payoff_scene(), 40
    frames = sc.render_batch(0, n)
    dets = [sc.detections(f) for f in range(n)]
    want_w, want_s, _ = oracle_stream(frames, [d[0] for d in dets], 4)
    cm = pkg("gmc").CameraMotion(H, W)
    got_w = np.concatenate([cm.apply_batch(frames[:17], [d[0] for d in dets[:17]]), cm.apply_batch(frames[17:], [d[0] for d in dets[17:]])])
    assert np.array_equal(got_w, want_w)
    feats = pkg("synthetic").identity_features
    fed = [(b, c, k, feats(ident, f, dim=512, seed=7), got_w[f]) for f, (b, c, k, ident) in enumerate(dets)]
    dev, ora = run_pair(fed, chunk=13, epoch_frames=epoch_frames)
    ids = set(dev.export()["track_id"].tolist())
    assert max(ids) <= PAYOFF["n_targets"], ids                    # no id was born after the gap
    dev0, _ = run_pair([f[:4] + (None,) for f in fed], chunk=13, epoch_frames=epoch_frames, with_reid=False)
    assert max(dev0.export()["track_id"].tolist()) > PAYOFF["n_targets"]
    cm.close()


# ------------------------------------------------------------------------------------------------------------------- the pipeline
def _pipe(n, batch, **kw):
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    pipe = pkg("pipeline").TrackingPipeline(ypath, rpath, (H, W), batch=batch, ring_frames=n, max_persons=32, dtype="fp16", inject=True,
                                            tracker="botsort", **kw)
    pipe.option("taper", 0)
    return pipe


def _tlwh_boxes(b):
    """The boxes as the tracker's rows hold them: x2 = x + (x2 - x) in fp32."""
    b = np.asarray(b, np.float32)
    return np.stack([b[:, 0], b[:, 1], b[:, 0] + (b[:, 2] - b[:, 0]), b[:, 1] + (b[:, 3] - b[:, 1])], 1).astype(np.float32)


def _rows(tracks):
    return [[tuple(t[:5]) + (t[6],) for t in fr] for fr in tracks]


@pytest.mark.parametrize("epoch_frames", [1, 16])
def test_pipeline_with_gmc_against_oracle(epoch_frames):
    """One launch group of 32 frames: 32 epochs of one frame or two of 16, each reading its rows of the device warps.  Then the same
    frames as two groups of 16, in two calls and in one (the gray level carried from group to group)."""
    n, g = 32, 16
    sc = pkg("synthetic").PanningScene(seed=6, pan=(9.0, -3.0), n_targets=5, speed=1.5, pad=384)
    frames = sc.render_batch(0, n)
    planted = [sc.detections(f)[:3] for f in range(n)]
    want_w, _, _ = oracle_stream(frames, [_tlwh_boxes(p[0]) for p in planted], 4)
    assert not any(np.array_equal(w, G.IDENTITY) for w in want_w[1:]) and len({w.tobytes() for w in want_w}) > n // 2
    pipe = _pipe(n, n, gmc=4)
    pipe.option("epoch_frames", epoch_frames)
    pipe.upload(0, frames)
    pipe.inject(0, planted)
    tracks, _ = pipe.run(0, n)
    assert np.array_equal(pipe.group_warps(), want_w)
    emb, per = pipe.group_embeddings()
    ora, r0 = Oracle(), 0
    for f in range(n):
        b, c, k = planted[f]
        rows, conf = Oracle.rows(ora.update_xyxy(b, c, k, emb[r0:r0 + per[f]] if per[f] else None, want_w[f]))
        r0 += per[f]
        assert [tuple(t[:5]) for t in tracks[f]] == [tuple(r[:5]) for r in rows.tolist()], f
        assert [t[6] for t in tracks[f]] == conf.tolist(), f
    pipe.close()
    ora0 = Oracle()                                                # the warp matters on this scene: without it the oracle's rows differ
    r0, differs = 0, False
    for f in range(n):
        b, c, k = planted[f]
        rows, _ = Oracle.rows(ora0.update_xyxy(b, c, k, emb[r0:r0 + per[f]] if per[f] else None))
        r0 += per[f]
        differs |= [tuple(t[:5]) for t in tracks[f]] != [tuple(r[:5]) for r in rows.tolist()]
    assert differs
    two = _pipe(n, g, gmc=4)
    two.option("epoch_frames", epoch_frames)
    two.upload(0, frames)
    two.inject(0, planted)
    got = []
    for g0 in (0, g):
        got += two.run(g0, g)[0]
        assert np.array_equal(two.group_warps(), want_w[g0:g0 + g])
    assert _rows(got) == _rows(tracks)
    two.close()
    both = _pipe(n, g, gmc=4)                                      # the two groups inside ONE call (producer and consumer threads)
    both.option("epoch_frames", epoch_frames)
    both.upload(0, frames)
    both.inject(0, planted)
    assert _rows(both.run(0, n)[0]) == _rows(tracks)
    assert np.array_equal(both.group_warps(), want_w[g:])
    both.close()


def test_pipeline_gmc_0_is_the_parent_and_other_pipelines_reject_it():
    L = pkg("_lib")
    n = 16
    sc = pkg("synthetic").PanningScene(seed=6, pan=(9.0, -3.0), n_targets=5, pad=256)
    frames, planted = sc.render_batch(0, n), [sc.detections(f)[:3] for f in range(n)]
    out = []
    for kw, toggle in ((dict(), False), (dict(gmc=0), False), (dict(gmc=4), True)):
        pipe = _pipe(n, n, **kw)
        if toggle:
            pipe.option("gmc", 0)                                  # switched on, then off again before the first frame
        pipe.upload(0, frames)
        pipe.inject(0, planted)
        out.append(_rows(pipe.run(0, n)[0]))
        with pytest.raises(L.AicError):
            pipe.group_warps()
        assert L.load().aic_pipeline_option(pipe._h, b"gmc", 3) == L.ERR_INVALID
        pipe.close()
    assert out[0] == out[1] == out[2] and sum(len(f) for f in out[0]) > n
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP = pkg("pipeline").TrackingPipeline
    for kind, reid in (("deepsort", rpath), ("bytetrack", None), ("ocsort", None)):
        pipe = TP(ypath, reid, (H, W), batch=4, ring_frames=4, max_persons=8, dtype="fp16", inject=True, tracker=kind)
        assert L.load().aic_pipeline_option(pipe._h, b"gmc", 4) == L.ERR_INVALID, kind
        pipe.close()


def test_other_trackers_after_a_gmc_pipeline():
    from test_gpu_botsort import test_other_trackers_after_a_botsort_pipeline as others
    others()


def test_cli_gmc_batch_1_and_16(tmp_path):
    """A panning clip through the CLI: the per-frame path (CameraMotion + BoTSORT.update) and the pipeline give the same tuples with
    --gmc 4, and the ids survive the detection gap, which they do not with --gmc 0 -- both paths use the warp.  (--conf_thresh 0.5:
    at BoT-SORT's 0.1 the detector's low-score boxes cover most blocks of this clip, and a masked frame gets the identity.)"""
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    sc = pkg("synthetic").PanningScene(seed=8, width=1280, height=720, pan=(12.0, 4.0), n_targets=8, tiled=True, w_range=(40.0, 80.0),
                                       h_range=(120.0, 200.0), reverse_at=12, gaps=[(t, 10, 15) for t in range(8)], pad=256)
    frames = sc.render_batch(0, 24)
    for t, a, b in sc.gaps:                                        # a gap the detector sees too: the persons are painted over
        for f in range(a, b + 1):
            frames[f] = sc.background(f)
    np.save(tmp_path / "pan.npy", frames)
    lines = {}
    for gmc, batch in ((4, 1), (4, 16), (0, 1)):
        d = tmp_path / f"{gmc}_{batch}"
        rc = pkg("cli").main(["--input", str(tmp_path / "pan.npy"), "--output_dir", str(d), "--yolo_engine", ypath, "--reid_engine", rpath,
                              "--tracker", "botsort", "--gmc", str(gmc), "--batch", str(batch), "--conf_thresh", "0.5"])
        assert rc == 0
        out = list(d.glob("*.jsonl"))
        assert len(out) == 1
        lines[gmc, batch] = [json.loads(x)["tracks"] for x in out[0].read_text().splitlines()]
    ids = {key: [sorted(t[4] for t in fr) for fr in v] for key, v in lines.items()}
    assert len(lines[4, 1]) == 24 and len(ids[4, 1][9]) >= 6
    assert lines[4, 1] == lines[4, 16]
    assert set(ids[4, 1][9]) <= set(ids[4, 1][16])                 # with the warp every id survives the gap and the sweep reversal
    assert not set(ids[0, 1][9]) <= set(ids[0, 1][16])             # without it, ids are lost
