"""Sparse box branches: a detect run may run the detector's box branches only at the anchors its NMS will read, from lists
made on the device.  Which path a run took may change time only: every output here is compared `array_equal` with a child process that
runs the dense head (AICAM_NO_SPARSE_BOX=1).

Small engine: YOLOv8n on 96 x 160 inputs (maps 12 x 20, 6 x 10, 3 x 5) with head_ref's "spans" box plant, 4 frames, lists forced.  The
thresholds are chosen from a dense run's max logits so that the candidate set is, in turn: empty; down to the best map-corner anchor;
down to an anchor on every edge of every level; down to two adjacent anchors of level 0; every anchor.  Each case asserts that its set
holds what it claims, that the query reports the list path and the counts NumPy derives from the dense max logits (the neighbour count
is the size of the UNION of the 3 x 3 neighbourhoods), and that the detections and the boxes at the candidate anchors are the child's.
The same cases run once more in two children with level 0's first box conv unmerged (AICAM_MERGE_MAXPX=100), where it is listed too.
One case runs under a device-side live count, one follows an armed run with a decode at a lower threshold.

Trained / seeded detectors at 32 frames of synthetic.Scene and the pipeline on 64 frames: the path the library chooses."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

HW, N_SMALL, N_BIG, MAX_DET = (96, 160), 4, 32, 100
LEVELS = tuple((HW[0] // s, HW[1] // s) for s in (8, 16, 32))
A0 = np.concatenate([[0], np.cumsum([h * w for h, w in LEVELS])])
IOU = 0.6
CASES = ("empty", "corner", "edges", "adjacent", "all")


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


def _stop_on_device_error(fn):
    """A HIP error ends the session: nothing more is started on a device that has just faulted."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except pkg("_lib").AicError as e:
            pytest.exit(f"{fn.__name__}: the library reported an error, stopping: {e}", returncode=1)
    return wrapped


# ---------------------------------------------------------------------------------------------------------------- the small engine
def small_engine(path):
    import head_ref as H
    c = H.Case("sparse_96x160", HW, 80, 41, N_SMALL, N_SMALL, (), (H.D25,) * 3, (None, None, None), False, "spans", (0.1, 0.1, 0.1))
    H.ef.write_engine(path, H.build(c).g)
    return path


def small_frames():
    return np.random.default_rng(77).integers(0, 256, (N_SMALL,) + HW + (3,), dtype=np.uint8)


def logit_thr(conf):
    """Model::logit_of: the fp32 threshold NMS and the candidate pass compare with, from the fp32 conf the call carries."""
    c = float(np.float32(conf))
    return np.float32(np.log(c / (1.0 - c)))


def conf_below(ml, v):
    """A conf whose threshold lies strictly between v and the next lower max logit: exactly the anchors with max logit >= v pass."""
    lower = ml[ml < v]
    lo = float(lower.max()) if lower.size else float(v) - 1.0
    conf = np.float32(1.0 / (1.0 + np.exp(-(0.5 * (float(v) + lo)))))
    assert lo < logit_thr(conf) < v and 0.0 < conf < 1.0, (lo, logit_thr(conf), v)
    return float(conf)


def level_maps(ml):
    """[n, A] -> per level [n, h, w]"""
    return [ml[:, A0[l]:A0[l + 1]].reshape(len(ml), h, w) for l, (h, w) in enumerate(LEVELS)]


def choose_confs(ml):
    """conf per case from the dense max logits [n, A] (this module's docstring)."""
    maps = level_maps(ml)
    corner = max(float(m[:, ys, xs].max()) for m in maps for ys in (0, -1) for xs in (0, -1))
    edges = min(float(e.max()) for m in maps for e in (m[:, 0, :], m[:, -1, :], m[:, :, 0], m[:, :, -1]))
    m0 = maps[0]
    adjacent = max(float(np.minimum(m0[:, :, :-1], m0[:, :, 1:]).max()), float(np.minimum(m0[:, :-1, :], m0[:, 1:, :]).max()))
    top = float(ml.max())
    empty = np.float32(1.0 / (1.0 + np.exp(-(top + 1.0))))
    assert logit_thr(empty) > top and empty < 1.0
    return {"empty": float(empty), "corner": conf_below(ml, corner), "edges": conf_below(ml, edges), "adjacent": conf_below(ml, adjacent),
            "all": conf_below(ml, float(ml.min()))}


def expected_counts(ml, conf, n_live=None):
    """(level 0, 1, 2 candidates, level-0 neighbourhood pixels) of frames [0, n_live) and the candidate mask [n, A]."""
    cand = ml >= logit_thr(conf)
    if n_live is not None:
        cand[n_live:] = False
    maps = level_maps(cand)
    m0 = maps[0]
    pad = np.zeros((m0.shape[0], m0.shape[1] + 2, m0.shape[2] + 2), bool)
    pad[:, 1:-1, 1:-1] = m0
    h, w = LEVELS[0]
    union = np.zeros_like(m0)
    for dy in range(3):
        for dx in range(3):
            union |= pad[:, dy:dy + h, dx:dx + w]
    return tuple(int(m.sum()) for m in maps) + (int(union.sum()),), cand


def scenario_small(path, confs, force):
    """Every case on one engine.  -> {name: array}: detections, the boxes / max logits of the workspace, the query's answer."""
    eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=N_SMALL, warm_up=False)
    out = {}
    try:
        if force:
            eng.sparse_box(force=True)
        f = small_frames()

        def call(tag, conf, again=False, **kw):
            if again:
                nd, boxes, scores, labels = eng.detect_decode_np(N_SMALL, HW, conf=conf, iou=IOU, max_det=MAX_DET)
            else:
                nd, boxes, scores, labels = eng.detect_np(f, conf=conf, iou=IOU, max_det=MAX_DET, **kw)
            q = eng.sparse_box()
            b, m, l = eng.read_det_np(N_SMALL)
            out.update({f"{tag}_nd": nd, f"{tag}_boxes": boxes, f"{tag}_scores": scores, f"{tag}_labels": labels, f"{tag}_wsbox": b,
                        f"{tag}_ml": m, f"{tag}_lab": l,
                        f"{tag}_q": np.array([q["listed"], *q["counts"], q["counted"], q["shape_ok"], q["lead0"]], np.int64)})

        # a box at every anchor that no run of this engine computes (all-equal DFL logits decode to 7.5 cells per side): what the empty
        # case must leave in place
        z = eng.yolo_postprocess_np(np.zeros((N_SMALL, int(A0[-1]), 64), np.float32), np.zeros((N_SMALL, int(A0[-1]), 80), np.float32))
        out["planted_wsbox"] = eng.read_det_np(N_SMALL)[0]
        assert np.array_equal(out["planted_wsbox"], z["boxes"])
        for name in CASES:
            call(name, confs[name])
        call("live", confs["edges"], n_live=2)                       # frames 2, 3 are past the device-side count
        # an armed run at a high threshold, then decode + NMS alone at a lower one, on what that run left
        call("high", confs["corner"])
        call("lower", confs["edges"], again=True)
    finally:
        eng.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- trained / seeded
def scene_frames(n, seed=9):
    return pkg("synthetic").Scene(seed=seed, n_targets=6).render_batch(0, n)


def scenario_detectors(force_seeded):
    """Two calls of 32 Scene frames on the trained detector (the library chooses), two on the seeded one (forced, then not)."""
    ef = pkg("engine_file")
    out = {}
    fr = scene_frames(N_BIG)
    for which, path in (("trained", ef.ensure_trained_detector(ROOT)), ("seeded", ef.ensure_seeded_engines(ROOT)[0])):
        eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=N_BIG, warm_up=False)
        try:
            for i in range(2):
                if which == "seeded" and force_seeded:
                    eng.sparse_box(force=(i == 0))
                conf = 0.25 if which == "trained" else 0.02
                nd, boxes, scores, labels = eng.detect_np(fr, conf=conf, iou=IOU, max_det=MAX_DET)
                q = eng.sparse_box()
                out.update({f"{which}{i}_nd": nd, f"{which}{i}_boxes": boxes, f"{which}{i}_scores": scores, f"{which}{i}_labels": labels,
                            f"{which}{i}_q": np.array([q["listed"], *q["counts"], q["counted"], q["shape_ok"], q["lead0"]], np.int64)})
        finally:
            eng.close()
    return out


def scenario_pipeline():
    ef = pkg("engine_file")
    n = 64
    fr = scene_frames(n)
    pipe = pkg("pipeline").TrackingPipeline(ef.ensure_trained_detector(ROOT), ef.ensure_seeded_engines(ROOT)[1], (720, 1280), batch=N_BIG,
                                            ring_frames=n, max_persons=64, dtype="fp16", inject=False)
    for k, v in {"taper": 0, "dual_lane_frames": 0}.items():      # two 32-frame groups on ONE engine
        pipe.option(k, v)
    pipe.upload(0, fr)
    tracks, nd = pipe.run(0, n)
    q = pipe.yolo.sparse_box()
    return {"rows": np.array([[f] + [float(v) for v in t[:5]] for f in range(n) for t in tracks[f]], np.float64).reshape(-1, 6),
            "nd": np.asarray(nd), "q": np.array([q["listed"], *q["counts"], q["counted"]], np.int64)}


def main(argv):
    what, out_dir = argv[1], argv[2]
    if what == "small":
        confs = dict(np.load(os.path.join(out_dir, "confs.npz")))
        out = scenario_small(os.path.join(out_dir, "small.aicw"), {k: float(v) for k, v in confs.items()}, os.environ.get("AICAM_NO_SPARSE_BOX") is None)
    elif what == "detectors":
        out = scenario_detectors(False)
    else:
        out = scenario_pipeline()
    tag = argv[3]
    for k, v in out.items():
        np.save(os.path.join(out_dir, f"{tag}_{k}.npy"), v)


if __name__ == "__main__":
    main(sys.argv)
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------------
def _child(what, out_dir, tag, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("AICAM_NO_SPARSE_BOX", "AICAM_SPARSE_BOX_FORCE")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, str(out_dir), tag], env=e, capture_output=True, text=True, timeout=600)
    print(r.stdout[-300:], r.stderr[-800:])
    assert r.returncode == 0, f"child {what} / {tag} failed"


def _ref(out_dir, tag, k):
    return np.load(os.path.join(out_dir, f"{tag}_{k}.npy"))


def _assert_dets_equal(out, out_dir, tag, prefix):
    for k in ("nd", "boxes", "scores", "labels"):
        ref = _ref(out_dir, tag, f"{prefix}_{k}")
        assert ref.shape == out[f"{prefix}_{k}"].shape and np.array_equal(ref, out[f"{prefix}_{k}"]), (prefix, k, int((ref != out[f"{prefix}_{k}"]).sum()))


@pytest.fixture(scope="module")
def small(gpu, tmp_path_factory):
    """The small engine, the confs of the cases (from a dense in-process run's max logits), the dense child's outputs."""
    assert "AICAM_NO_SPARSE_BOX" not in os.environ and "AICAM_SPARSE_BOX_FORCE" not in os.environ, "this process has to choose its paths itself"
    d = tmp_path_factory.mktemp("sparse_box")
    path = small_engine(str(d / "small.aicw"))
    eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=N_SMALL, warm_up=False)
    try:
        eng.detect_np(small_frames(), conf=0.5, iou=IOU, max_det=MAX_DET)
        q = eng.sparse_box()
        assert q["shape_ok"] and not q["listed"] and not q["counted"], q          # four frames, not forced: the per-frame path stays dense
        _, ml, _ = eng.read_det_np(N_SMALL)
    finally:
        eng.close()
    assert np.isfinite(ml).all() and len(np.unique(ml)) > ml.size // 2
    confs = choose_confs(ml)
    np.savez(str(d / "confs.npz"), **confs)
    _child("small", d, "dense", AICAM_NO_SPARSE_BOX="1")
    return {"dir": d, "path": path, "confs": confs, "ml": ml}


def _check_small(out, small, tag_ref, lead0):
    d, ml, confs = small["dir"], small["ml"], small["confs"]
    assert np.array_equal(_ref(d, tag_ref, "all_ml"), ml)
    sets = {}
    for name, conf, n_live in [(c, confs[c], None) for c in CASES] + [("live", confs["edges"], 2), ("high", confs["corner"], None), ("lower", confs["edges"], None)]:
        counts, cand = expected_counts(ml, conf, n_live)
        sets[name] = cand
        q = out[f"{name}_q"]
        assert q[0] == 1 and q[5] == 1 and q[6] == 1 and q[7] == lead0, (name, q)
        assert tuple(q[1:5]) == counts, f"{name}: the device counted {tuple(q[1:5])}, NumPy {counts}"
        assert np.array_equal(out[f"{name}_ml"], ml) and np.array_equal(out[f"{name}_lab"], _ref(d, tag_ref, f"{name}_lab"))
        n = N_SMALL if n_live is None else n_live
        for k in ("nd", "boxes", "scores", "labels"):
            ref = _ref(d, tag_ref, f"{name}_{k}")
            assert np.array_equal(ref[:n], out[f"{name}_{k}"][:n]), (name, k)
        if n_live is not None:
            assert not out[f"{name}_nd"][n:].any() and not out[f"{name}_boxes"][n:].any()           # left as the caller passed them
        ws, ws_ref = out[f"{name}_wsbox"], _ref(d, tag_ref, f"{name}_wsbox")
        assert np.array_equal(ws[cand], ws_ref[cand]), f"{name}: boxes at candidate anchors differ from the dense head's"
        assert np.isfinite(ws_ref).all()
    maps = {k: level_maps(v) for k, v in sets.items()}
    # ---- each case holds what it claims
    assert not sets["empty"].any() and not out["empty_nd"].any() and tuple(out["empty_q"][1:5]) == (0, 0, 0, 0)
    assert any(m[:, ys, xs].any() for m in maps["corner"] for ys in (0, -1) for xs in (0, -1)), "no corner anchor among the candidates"
    for l, m in enumerate(maps["edges"]):
        for e in (m[:, 0, :], m[:, -1, :], m[:, :, 0], m[:, :, -1]):
            assert e.any(), f"level {l}: an edge without a candidate"
    m0 = maps["adjacent"][0]
    assert (m0[:, :, :-1] & m0[:, :, 1:]).any() or (m0[:, :-1, :] & m0[:, 1:, :]).any(), "no two adjacent candidates on level 0"
    c_adj, _ = expected_counts(ml, confs["adjacent"])
    assert c_adj[3] < 9 * c_adj[0], "the neighbourhoods of the adjacent case share no pixel"
    assert sets["all"].all() and tuple(out["all_q"][1:5]) == tuple(h * w * N_SMALL for h, w in LEVELS) + (LEVELS[0][0] * LEVELS[0][1] * N_SMALL,)
    # ---- nothing written where no candidate is: the empty case left every planted box in place
    assert np.array_equal(out["empty_wsbox"], out["planted_wsbox"]) and np.abs(out["planted_wsbox"]).max() > 0, "the empty case wrote boxes"
    assert not np.array_equal(_ref(d, tag_ref, "empty_wsbox"), out["planted_wsbox"])              # (the dense head writes them all)
    assert out["all_nd"].sum() > 0 and out["edges_nd"].sum() > 0
    # ---- a decode below the armed run's threshold: `lower` ran after `high` on the same engine and equals the dense child's (checked above);
    # the live case: frames past the count added no list entry (counts above are those of frames 0, 1 only)
    assert sets["lower"].sum() > sets["high"].sum()


@_stop_on_device_error
def test_small_engine_cases_equal_the_dense_head(gpu, small):
    out = scenario_small(small["path"], small["confs"], True)
    _check_small(out, small, "dense", lead0=0)


@_stop_on_device_error
def test_small_engine_with_level0_lead_listed(gpu, small):
    """The same cases with 22.box0.0 a launch of its own (no merge with 22.cls0.0 on maps above 100 pixels): it runs on the neighbour list."""
    d = small["dir"]
    _child("small", d, "dense_unmerged", AICAM_NO_SPARSE_BOX="1", AICAM_MERGE_MAXPX="100")
    _child("small", d, "lists_unmerged", AICAM_MERGE_MAXPX="100")
    names = {f[len("lists_unmerged_"):-4] for f in os.listdir(d) if f.startswith("lists_unmerged_")}
    out = {k: _ref(d, "lists_unmerged", k) for k in names}
    _check_small(out, small, "dense_unmerged", lead0=1)


@_stop_on_device_error
def test_unarmed_run_after_a_listed_run_is_dense(gpu, small):
    """A run that is not armed (aic_yolo_decode) right behind a listed run: dense, a box at EVERY anchor, the bits it gives with the
    lists off."""
    eng = pkg("hip_engine").HipEngine(small["path"], dtype="fp16", max_items=N_SMALL, warm_up=False)
    try:
        eng.sparse_box(force=True)
        f = small_frames()
        eng.detect_np(f, conf=small["confs"]["corner"], iou=IOU, max_det=MAX_DET)
        assert eng.sparse_box()["listed"]
        x = np.random.default_rng(5).random((N_SMALL, 3) + HW, dtype=np.float32)
        b1, m1, _ = eng.yolo_decode_np(x)
        assert not eng.sparse_box()["listed"], "a run that was not armed took the lists"
        eng.sparse_box(force=False)
        b2, m2, _ = eng.yolo_decode_np(x)
        assert np.array_equal(b1, b2) and np.array_equal(m1, m2) and np.abs(b1).max() > 0
        assert (np.abs(b1).reshape(N_SMALL, -1, 4).max(-1) > 0).all(), "an anchor without a box behind an unarmed run"
    finally:
        eng.close()


@_stop_on_device_error
def test_trained_and_seeded_detectors_at_32_frames(gpu, tmp_path):
    _child("detectors", tmp_path, "dense", AICAM_NO_SPARSE_BOX="1")
    out = scenario_detectors(True)
    for p in ("trained0", "trained1", "seeded0", "seeded1"):
        _assert_dets_equal(out, tmp_path, "dense", p)
        assert out[f"{p}_nd"].sum() > 0
    q0, q1 = out["trained0_q"], out["trained1_q"]
    assert q0[0] == 0 and q0[5] == 1, f"the first call knows no counts yet: dense, and counted ({q0})"
    assert q1[0] == 1 and q1[7] == 1, f"the trained detector's second call did not take the lists ({q1})"
    assert 0 < q1[1:4].sum() and q1[1] <= q1[4] <= min(9 * q1[1], 6400 * N_BIG // 4), q1         # the lists the choice allows: a quarter of the map
    s0, s1 = out["seeded0_q"], out["seeded1_q"]
    assert s0[0] == 1 and s0[1:4].sum() > 1000 * N_BIG, f"forced, the seeded head lists thousands of candidates per frame ({s0})"
    assert s1[0] == 0, f"not forced, the seeded detector's second call must stay dense ({s1})"


@_stop_on_device_error
def test_pipeline_rows_equal_the_dense_head(gpu, tmp_path):
    _child("pipeline", tmp_path, "dense", AICAM_NO_SPARSE_BOX="1")
    out = scenario_pipeline()
    for k in ("rows", "nd"):
        ref = _ref(tmp_path, "dense", k)
        assert ref.shape == out[k].shape and np.array_equal(ref, out[k]), k
    assert len(out["rows"]) > 0 and out["nd"].sum() > 0
    assert out["q"][0] == 1, f"the second 32-frame group did not take the lists ({out['q']})"
