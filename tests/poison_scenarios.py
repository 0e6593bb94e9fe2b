"""Scenarios whose outputs must not depend on what device memory held before the library wrote it, and the
comparer of two recordings.  No GPU is touched on import.

Run as a script this file is one child of tests/test_gpu_poison.py: `python tests/poison_scenarios.py GROUP OUT_DIR TAG [dirty]` runs
one group in a process whose environment carries AICAM_POISON_ALLOC (csrc/poison_pattern.hpp: every fresh allocation of the library is
filled with zeros, with a big finite value, or with NaN / -1 bytes) and saves every output array as OUT_DIR/TAG_<key>.npy, the
allocation probe's four arrays among them.  Every scenario records the FULL arrays the Python wrappers return: rows past a count,
slots past the live ones, statuses, counters, exported state.

`dirty` (groups in DIRTY, the stateless handles): the child first gives each handle one call of the largest size it takes, on other
content, then runs the same calls -- stale data INSIDE a handle, which a poison at allocation time cannot reach.  Its outputs must
equal the zero child's.

The inputs are those of the existing case modules, at their smallest."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODES = ("zero", "big", "nan")
PROBE_KEYS = ("probe_f32", "probe_i32", "probe_u8", "probe_pinned_u8")

# The only outputs a comparison may skip: readers of engine workspace that include/aicam.h documents as holding stale data.
# (group, key pattern as fnmatch reads it, the line of include/aicam.h that allows it); masked() says where such an output IS compared
EXCEPTIONS = (
    ("detector", "*_wsbox",
     " * boxes[n,A,4], max class logit[n,A], label[n,A].  After a run that took the lists only candidate anchors hold that run's boxes. */"),
)


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


# ------------------------------------------------------------------------------------------------------------------------ comparer
def _match(pattern, key):
    import fnmatch
    return fnmatch.fnmatchcase(key, pattern)


def excepted(group, key):
    return any(g == group and _match(pat, key) for g, pat, _ in EXCEPTIONS)


def masked(group, key, a, ref_all):
    """An excepted output compared where the header does define it.  *_wsbox: the boxes at this run's candidate anchors (the mask is
    recorded by the scenario beside it as <tag>_wscand); elsewhere the workspace holds an earlier run's boxes or the allocation's."""
    if key.endswith("_wsbox"):
        cand = ref_all[key[:-len("_wsbox")] + "_wscand"].astype(bool)
        return a[cand]
    raise KeyError(key)


def compare(ref, got, group=None):
    """ref, got: {key: array}.  -> list of findings, empty when got is ref byte for byte: (key, what, index) with what one of "missing",
    "unexpected", "dtype", "shape", "bytes" and index the first differing element's index tuple (None where there is none)."""
    out = []
    for k in sorted(set(ref) | set(got)):
        if k not in got:
            out.append((k, "missing", None))
            continue
        if k not in ref:
            out.append((k, "unexpected", None))
            continue
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        if a.dtype != b.dtype:
            out.append((k, "dtype", None))
            continue
        if a.shape != b.shape:
            out.append((k, "shape", None))
            continue
        if group is not None and excepted(group, k):
            a, b = masked(group, k, a, ref), masked(group, k, b, ref)
        shape = a.shape
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.tobytes() == b.tobytes():                               # bytes: a NaN equals the same NaN, -0.0 is not +0.0
            continue
        ab = a.reshape(-1).view(np.uint8).reshape(a.size, -1)        # (one row of bytes per element)
        bb = b.reshape(-1).view(np.uint8).reshape(b.size, -1)
        first = int(np.flatnonzero((ab != bb).any(1))[0])
        out.append((k, "bytes", tuple(int(i) for i in np.unravel_index(first, shape)) if shape else ()))
    return out


def load_recording(out_dir, tag):
    pre = tag + "_"
    return {f[len(pre):-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir)) if f.startswith(pre) and f.endswith(".npy")}


def probe_shows(mode, rec):
    """Does the recorded allocation probe show `mode`'s fill?  (dirty runs under zero.)"""
    f, i, u, p = (rec[k] for k in PROBE_KEYS)
    if mode == "zero":
        return not f.view(np.uint32).any() and not i.any() and not u.any() and not p.any()
    if mode == "big":
        return (f.view(np.uint32) == 0x7B7B7B7B).all() and (i == 31611).all() and (u == 123).all() and (p == 123).all()
    return bool(np.isnan(f).all()) and (i == -1).all() and (u == 255).all() and (p == 255).all()


# ------------------------------------------------------------------------------------------------------------------------ detector
def group_detector(out_dir, dirty):
    """test_gpu_sparse_box.small_engine (YOLOv8n on 96 x 160), 4 frames: a dense detect, the lists forced at the "edges" threshold, a
    device-side live count of 2, a decode at a lower threshold behind an armed run, a raw decode, two letterboxed calls (48 x 160
    frames have borders above and below: the second may run row windows)."""
    import test_gpu_sparse_box as S
    path = S.small_engine(os.path.join(out_dir, "small.aicw"))
    eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=S.N_SMALL, warm_up=False)
    out = {}
    try:
        f = S.small_frames()
        rng = np.random.default_rng(78)
        if dirty:                                                    # every frame slot, every output row the cap allows, other content
            eng.detect_np(rng.integers(0, 256, f.shape, dtype=np.uint8), conf=1e-4, iou=0.99, max_det=1024)
            eng.yolo_decode_np(rng.random((S.N_SMALL, 3) + S.HW, dtype=np.float32))

        def record(tag, res, ml=None, conf=None, n_live=None):
            nd, boxes, scores, labels = res
            q = eng.sparse_box()
            b, m, l = eng.read_det_np(S.N_SMALL)
            out.update({f"{tag}_nd": nd, f"{tag}_boxes": boxes, f"{tag}_scores": scores, f"{tag}_labels": labels, f"{tag}_ml": m, f"{tag}_lab": l,
                        f"{tag}_q": np.array([q["listed"], *q["counts"], q["counted"], q["shape_ok"], q["lead0"]], np.int64)})
            if ml is not None:                                       # a listed run: the workspace boxes are defined at its candidates only
                out[f"{tag}_wsbox"], out[f"{tag}_wscand"] = b, S.expected_counts(ml, conf, n_live)[1]
            else:
                out[f"{tag}_allbox"] = b

        record("dense", eng.detect_np(f, conf=0.5, iou=S.IOU, max_det=S.MAX_DET))
        ml = out["dense_ml"]
        confs = S.choose_confs(ml)
        eng.sparse_box(force=True)
        record("edges", eng.detect_np(f, conf=confs["edges"], iou=S.IOU, max_det=S.MAX_DET), ml, confs["edges"])
        record("live", eng.detect_np(f, conf=confs["edges"], iou=S.IOU, max_det=S.MAX_DET, n_live=2), ml, confs["edges"], 2)
        record("high", eng.detect_np(f, conf=confs["corner"], iou=S.IOU, max_det=S.MAX_DET), ml, confs["corner"])
        record("lower", eng.detect_decode_np(S.N_SMALL, S.HW, conf=confs["edges"], iou=S.IOU, max_det=S.MAX_DET), ml, confs["edges"])
        eng.sparse_box(force=False)
        x = np.random.default_rng(5).random((S.N_SMALL, 3) + S.HW, dtype=np.float32)
        out["decode_boxes"], out["decode_ml"], out["decode_lab"] = eng.yolo_decode_np(x)
        band = np.random.default_rng(79).integers(0, 256, (2, S.N_SMALL, 48, 160, 3), dtype=np.uint8)
        for i in range(2):
            nd, boxes, scores, labels = eng.detect_np(band[i], conf=confs["edges"], iou=S.IOU, max_det=S.MAX_DET)
            out.update({f"band{i}_nd": nd, f"band{i}_boxes": boxes, f"band{i}_scores": scores, f"band{i}_labels": labels})
            out[f"band{i}_rb"] = np.array([[int(v) for v in eng.row_band(op, 48, 160).values()] for op in range(14)], np.int64)
    finally:
        eng.close()
    return out


def group_detectors32(out_dir, dirty):
    """test_gpu_sparse_box.scenario_detectors as it stands: 32 frames, the trained and the seeded engine, two calls each."""
    import test_gpu_sparse_box as S
    return S.scenario_detectors(False)


# ---------------------------------------------------------------------------------------------------------------------------- reid
def group_reid(out_dir, dirty):
    """The seeded ReID engine on crop_cases' smallest bank that holds its 128 x 64 crops: reid_infer_np with a live count below n,
    embed_boxes_np on one frame, embed_bank_np at byte offsets 1 and 3 (boxes_for has boxes the frame clips, empty and inverted ones)."""
    import crop_cases as K
    rpath = pkg("engine_file").ensure_seeded_engines(ROOT)[1]
    shape = (128, 64)
    bank = K.STEM_BANK_OF[shape]
    frames, (boxes, fo) = K.bank(bank), K.boxes_for(shape, bank)
    n = len(boxes)
    crops, _ = K.expected(shape, bank_name=bank)
    eng = pkg("hip_engine").HipEngine(rpath, dtype="fp16", max_items=n, warm_up=False)
    out = {}
    try:
        if dirty:
            eng.reid_infer_np(np.random.default_rng(128).uniform(-1, 1, crops.shape).astype(np.float32))
        out["live_emb"] = eng.reid_infer_np(crops, n_live=n - 5)
        out["full_emb"] = eng.reid_infer_np(crops)
        out["boxes_emb"], out["boxes_valid"] = eng.embed_boxes_np(frames[1], boxes)
        for off in (1, 3):
            out[f"bank{off}_emb"], out[f"bank{off}_valid"] = eng.embed_bank_np(frames, boxes, fo, byte_offset=off)
        out["banklive_emb"], out["banklive_valid"] = eng.embed_bank_np(frames, boxes, fo, byte_offset=2, n_live=n - 5)
    finally:
        eng.close()
    return out


# ------------------------------------------------------------------------------------------------------------------------ pipeline
PIPE_TRACKERS = (("deepsort_dev", dict(tracker="deepsort"), {"device_assoc": 2}), ("deepsort_host", dict(tracker="deepsort"), {"device_assoc": 0}),
                 ("bytetrack", dict(tracker="bytetrack"), {}), ("ocsort", dict(tracker="ocsort"), {}), ("botsort_gmc", dict(tracker="botsort", gmc=2), {}))


def _pipeline_run_full(pipe, slot, count):
    """aic_pipeline_run with every output it has, whole arrays (TrackingPipeline.run cuts them at the counts)."""
    L = pkg("_lib")
    mp, md = pipe.max_persons, pipe.max_det
    r = {"nt": np.zeros(count, np.int32), "rows": np.zeros((count, mp, 6), np.int32), "tconf": np.zeros((count, mp), np.float32),
         "nd": np.zeros(count, np.int32), "det_boxes": np.zeros((count, md, 4), np.float32), "det_scores": np.zeros((count, md), np.float32),
         "det_labels": np.zeros((count, md), np.int32)}
    L.call("aic_pipeline_run", pipe._h, int(slot), int(count), *(L.ptr(r[k]) for k in ("nt", "rows", "tconf", "nd", "det_boxes", "det_scores", "det_labels")))
    return r


def group_pipeline(out_dir, dirty):
    """TrackingPipeline on the seeded engines, 16 frames of synthetic.Scene in groups of 8, injected detections; one run per tracker."""
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    syn = pkg("synthetic")
    n = 16
    sc = syn.Scene(seed=21, n_targets=12, gaps=[(2, 6, 9), (5, 12, 20)], births={11: 5})
    fr = sc.render_batch(0, n)
    dets = [sc.detections(f)[:3] for f in range(n)]
    out = {}
    for name, kw, opts in PIPE_TRACKERS:
        pipe = pkg("pipeline").TrackingPipeline(ypath, rpath, (720, 1280), batch=8, ring_frames=n, max_persons=16, dtype="fp16", inject=True, **kw)
        try:
            for k, v in opts.items():
                pipe.option(k, v)
            pipe.upload(0, fr)
            pipe.inject(0, dets)
            for k, v in _pipeline_run_full(pipe, 0, n).items():
                out[f"{name}_{k}"] = v
            out[f"{name}_counters"] = np.array(list(pipe.counters().values()), np.int64)
            if pipe.reid is not None:
                out[f"{name}_last_emb"] = pipe.last_embeddings()
            if pipe.tracker_core is not None:                        # the DeepSORT tracker's exported state; the other pipelines export none
                for k, v in pipe.tracker_core.export_arrays().items():
                    out[f"{name}_state_{k}"] = v
            if kw.get("gmc"):
                out[f"{name}_warps"] = pipe.group_warps()
        finally:
            pipe.close()
    return out


# ----------------------------------------------------------------------------------------------------------------------- analytics
def rec(out, prefix, obj):
    """Everything a wrapper returned, flattened into out[prefix...]: arrays as they are, numbers as 0-d arrays, the members of tuples,
    lists, dicts and result objects under their names.  Strings (messages) and None are not outputs of the device."""
    if obj is None or isinstance(obj, str):
        return
    if isinstance(obj, np.ndarray):
        out[prefix] = obj
    elif isinstance(obj, (bool, int, float, np.generic)):
        out[prefix] = np.asarray(obj)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            rec(out, f"{prefix}_{k}", v)
    elif hasattr(obj, "_fields"):
        for k in obj._fields:
            rec(out, f"{prefix}_{k}", getattr(obj, k))
    elif isinstance(obj, (tuple, list)):
        out[prefix + "_len"] = np.asarray(len(obj))
        for i, v in enumerate(obj):
            rec(out, f"{prefix}_{i}", v)
    elif hasattr(obj, "__dict__"):
        rec(out, prefix, {k: v for k, v in vars(obj).items() if not k.startswith("_")})
    else:
        raise TypeError(f"{prefix}: {type(obj)}")


def _slot_stage(out, tag, stage, calls, cap, with_frames=True):
    """A stage that walks a slot table (best shots, colours, heat maps): every call, its exports, a flush at cap 1, a drain."""
    for i, (frames, rows) in enumerate(calls):
        rec(out, f"{tag}_call{i}", stage.update(frames, rows, cap=cap) if with_frames else stage.update(rows, cap=cap))
        for s in range(stage.streams):
            rec(out, f"{tag}_call{i}_export{s}", stage.export(s))
    rec(out, f"{tag}_flush", stage.flush(cap=1))
    rec(out, f"{tag}_drain", stage.drain(cap=16))
    for s in range(stage.streams):
        rec(out, f"{tag}_end_export{s}", stage.export(s))


def group_analytics(out_dir, dirty):
    """Zones, best shots, colours, left objects, scene watch and heat maps on slot_life_scene.calls() (3 streams of 48 x 64, 14 ticks in
    calls of 5, 1, 8; stream 2 stops at capacity), then each on the smallest case of its own module; state exported after the calls."""
    import bestshot_cases as BC
    import colours_cases as CC
    import heat_cases as HC
    import left_cases as LC
    import scene_cases as SC
    import slot_life_scene as SL
    import zones_cases as ZC
    out = {}
    calls = SL.calls()
    S = SL.STREAMS

    def zones(tag, zc, geometry, per_call):
        for s in range(zc.streams):
            zc.set_zones(s, *geometry)
        for i, frames in enumerate(per_call):
            rec(out, f"{tag}_call{i}", zc.update(frames, cap_events=8))
        for s in range(zc.streams):
            rec(out, f"{tag}_counters{s}", zc.counters(s))
        zc.close()

    zones("zones_life", pkg("zones").ZoneCounter(S, max_tracks=SL.MAX_TRACKS, forget_after=SL.FORGET_AFTER), ZC.GEOMETRY[1],
          [[[tick[s] for tick in rows] for s in range(S)] for _, rows in calls])
    zones("zones_own", pkg("zones").ZoneCounter(1, max_tracks=8, forget_after=2), ZC.GEOMETRY[2], [[ZC.walkers(3, 12, 5, 3)]])

    def stage(tag, make, calls_, cap, with_frames=True):
        st = make()
        try:
            _slot_stage(out, tag, st, calls_, cap, with_frames)
        finally:
            st.close()

    stage("bestshot_life", lambda: pkg("bestshot").BestShots(S, SL.HW, **SL.BS_KW), calls, SL.CAP)
    stage("colours_life", lambda: pkg("colours").TrackColours(S, SL.HW, **SL.CL_KW), calls, SL.CAP)
    stage("heat_life", lambda: pkg("heatmap").HeatMaps(S, SL.HW, cell=8, **SL.CL_KW), calls, SL.CAP, with_frames=False)
    b, c = BC.CASES[3], CC.CASES[3]                                  # "capacity stop": 3 ticks, 2 streams, one of which stops
    stage("bestshot_own", lambda: pkg("bestshot").BestShots(b["streams"], b["hw"], **b["kw"]), b["calls"], b["cap"])
    stage("colours_own", lambda: pkg("colours").TrackColours(c["streams"], c["hw"], **c["kw"]), c["calls"], c["cap"])

    w = HC.walk_case()
    hm = pkg("heatmap").HeatMaps(w["streams"], w["hw"], **{**w["kw"], "anchor": "foot"})
    try:
        for i, op in enumerate(w["ops"]):
            rec(out, f"heat_own_op{i}", hm.update(op[1], cap=w["cap"]) if op[0] == "update" else hm.flush(op[1], cap=w["cap"]))
        rec(out, "heat_own_export", hm.export(0))
        rec(out, "heat_own_layers", hm.layers(0))
    finally:
        hm.close()
    hl = pkg("heatmap").HeatMaps(S, SL.HW, cell=8, **SL.CL_KW)       # the layers of the life-cycle scene, every stream, stopped ones too
    try:
        hl.update(calls[0][1], cap=SL.CAP)
        for s in range(S):
            rec(out, f"heat_life_layers{s}", hl.layers(s))
    finally:
        hl.close()

    def frames_stage(tag, st, frame_calls, **kw):
        try:
            for i, (frames, rows) in enumerate(frame_calls):
                rec(out, f"{tag}_call{i}", st.update(frames, rows, want_masks=True, **kw))
            for s in range(st.streams):
                rec(out, f"{tag}_export{s}", st.export(s))
        finally:
            st.close()

    frames_stage("left_life", pkg("leftobj").LeftObjects(S, SL.HW, cell=8, max_objects=4, warmup=1, min_ticks=1, fast_shift=1), calls, cap_events=8)
    frames_stage("scene_life", pkg("scene").SceneWatch(S, SL.HW, cell=8, warmup=2), calls)
    lc = LC.seeded("poison", (32, 48), 8, streams=2, ticks=12, seed=4, max_objects=4)
    frames_stage("left_own", pkg("leftobj").LeftObjects(2, lc["hw"], cell=lc["cell"], max_objects=lc["max_objects"], **lc["options"]),
                 [(lc["frames"][:5], lc["rows"][:5]), (lc["frames"][5:], lc["rows"][5:])], cap_events=4)
    sc = SC.seeded("poison", (32, 48), 8, streams=2, ticks=28, seed=4)
    frames_stage("scene_own", pkg("scene").SceneWatch(2, sc["hw"], cell=sc["cell"], **sc["options"]),
                 [(sc["frames"][:9], sc["rows"][:9]), (sc["frames"][9:], sc["rows"][9:])])
    return out


# --------------------------------------------------------------------------------------------------------------------------- banks
# Not recorded anywhere: the BoT-SORT counters' shader-clock totals.  They are times, different in every run of the same process on the
# same memory (tests/test_gpu_botsort_bank.py CLOCKS): no statement about memory can be made from them.
CLOCKS = ("cost_cycles", "kernel_cycles")
BANK_PLAN = ([16, 0, 3], [4, 0, 1])        # frames per call of stream 0 (the crowd), 1 (never fed: empty), 2 (four persons)


def _bank_run(out, tag, bk, dets, plan=BANK_PLAN):
    pos = [0] * len(dets)
    for i, call in enumerate(plan):
        parts = [dets[s][pos[s]:pos[s] + call[s]] for s in range(len(dets))]
        rec(out, f"{tag}_call{i}", bk.update_arrays(parts))
        pos = [p + c for p, c in zip(pos, call)]
    for s in range(len(dets)):
        rec(out, f"{tag}_export{s}", bk.export(s))
        c = bk.counters(s)
        rec(out, f"{tag}_counters{s}", {k: v for k, v in c.items() if k not in CLOCKS} if isinstance(c, dict) else c)


def group_banks(out_dir, dirty):
    """The ByteTrack, OC-SORT, BoT-SORT and DeepSORT banks at 3 streams with ragged frame counts: a crowd of 150 whose matrices lie
    beyond the kernels' LDS arena (byte_family_cases.ARENA_SIDE, ocsort_edge_cases.LDS_ARENA_FLOATS: the per-stream HBM scratch slices),
    a stream that is never fed, four persons.  Then tests/test_gpu_xcam.py's cameras: cross-camera linking over a DeepSORT bank with
    an archive attached, one archive put and search."""
    import byte_family_cases as BF
    import ocsort_edge_cases as OE
    import test_gpu_botsort_bank as TBB
    import test_gpu_deepsort_bank as TDB
    import test_gpu_xcam as TX
    from test_gpu_bytetrack import frames_of
    Scene = pkg("synthetic").Scene
    crowd = dict(n_targets=150, conf_range=(0.05, 0.95), jitter=2.0, shuffle=True, w_range=(30.0, 50.0), h_range=(80.0, 120.0))
    few = dict(n_targets=4, conf_range=(0.3, 0.95), jitter=1.0)
    out = {}
    dets = [frames_of(Scene(seed=21, **crowd), 20), [], frames_of(Scene(seed=5, **few), 20)]
    for kind, make in (("bytetrack", pkg("bytetrack").BYTETrackerBank), ("ocsort", pkg("ocsort").OCSortBank)):
        bk = make(3)
        try:
            bk.option("lsap_fast", 0)
            _bank_run(out, kind, bk, dets)
            side = bk.counters(0).get("max_side")                # (the OC-SORT bank counts no sides: its crowd is the same 150)
            assert side is None or (side > BF.ARENA_SIDE["bytetrack"] and side * side > OE.LDS_ARENA_FLOATS), (kind, side)
        finally:
            bk.close()
    fdets = [TBB.stream_frames(Scene(seed=21, **crowd), 20, seed=31, dim=64), [], TBB.stream_frames(Scene(seed=5, **few), 20, seed=32, dim=64)]
    bk = pkg("botsort").BoTSORTBank(3, feature_dim=64)
    try:
        bk.option("lsap_fast", 0)
        _bank_run(out, "botsort", bk, fdets)
        assert bk.counters(0)["max_side"] > BF.ARENA_SIDE["botsort"]
    finally:
        bk.close()
    ddets = [TDB._frames(Scene(seed=21, **crowd), 0, 20, 64, seed=31), [], TDB._frames(Scene(seed=5, **few), 0, 20, 64, seed=32, featless=3)]
    bk = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=256, feature_dim=64)
    try:
        _bank_run(out, "deepsort", bk, ddets)
        for i, gl in enumerate(bk.export(2)["gallery_len"]):
            out[f"deepsort_gallery2_{i}"] = bk.export_gallery(2, i, int(gl))
    finally:
        bk.close()
    # cross-camera linking, tests/test_gpu_xcam.py::test_deepsort_bank_pack's cameras, with an archive behind the passes
    cams = [[0, 1, 2, 3], [2], []]
    bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=16, feature_dim=TX.DIM, n_init=3, nn_budget=2)
    xc = pkg("xcam").CrossCamera(3, 16, TX.DIM, TX.THR)
    ar = pkg("archive").IdentityArchive(64, TX.DIM)
    try:
        xc.attach_archive(ar)
        for tick in range(4):
            bank.update_arrays([[TX.deepsort_tick(p, c, tick)] for c, p in enumerate(cams)])
            if tick == 1:
                out["xcam_links_tentative"] = np.asarray(bank.link_cameras(xc))
                rec(out, "xcam_tentative_tables", xc.tables())
                out["xcam_tentative_shards"] = xc.shards()
        out["xcam_links"] = np.asarray(bank.link_cameras())
        rec(out, "xcam_tables", xc.tables())
        out["xcam_shards"] = xc.shards()
        rec(out, "xcam_size", xc.size())
        for s in range(3):
            ids = bank.export(s)["track_id"]
            out[f"xcam_global{s}"] = xc.global_ids(s, np.concatenate([ids, [99]]).astype(np.int32))
        rec(out, "xcam_archive", ar.export())
        rows = np.stack([TX.person_feature(p, 7, 9) for p in range(5)]).astype(np.float32)
        ar.put(np.arange(100, 105), 7, 50, rows)
        rec(out, "archive_search", ar.search(np.stack([TX.person_feature(p, 1, 3) for p in (2, 4, 0)]).astype(np.float32), k=3, exclude_camera=0))
        rec(out, "archive_export", ar.export())
    finally:
        ar.close(), xc.close(), bank.close()
    return out


# -------------------------------------------------------------------------------------------------------------------------- codecs
def group_codecs(out_dir, dirty):
    """JPEG out (jpeg_cases.bank at 4:2:0, 4:4:4 and with a restart interval of 3 MCUs), JPEG in (jpegdec_cases' 16 x 16 files with two
    refused ones between them), NV12 and I420 in and out (tight, and pitched into a prefilled buffer), render with rows, primitives and
    masks at 3 x 70 x 131 (tests/test_gpu_render.py), one camera-motion estimate (tests/test_gpu_gmc.py's odd pair)."""
    import jpeg_cases as JC
    import jpegdec_cases as JD
    import test_gpu_gmc as TG
    import test_gpu_render as TR
    out = {}
    rng = np.random.default_rng(91)
    other = lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)          # noqa: E731

    bank = JC.bank(4)
    for tag, sub, restart in (("jpeg420", "420", 0), ("jpeg444", "444", 0), ("jpeg420r3", "420", 3)):
        enc = pkg("jpeg").JpegEncoder(bank.shape[1:3], max_images=4, quality=85, restart=restart, subsampling=sub)
        try:
            room = 4 * enc.worst_case_bytes()
            if dirty:
                enc.encode_packed(other(bank.shape), out=np.zeros(room, np.uint8))
            buf, off, status = enc.encode_packed(bank, out=np.zeros(room, np.uint8))
            out.update({f"{tag}_buf": buf, f"{tag}_offsets": off, f"{tag}_status": status})
        finally:
            enc.close()

    good = [f for name, f, hw in JD.well_formed() if hw == (16, 16)]
    bad = {name: f for name, f, hw, _ in JD.refused() if hw == (16, 16)}
    files = [good[0], bad["truncated-interval"], good[1], bad["markers-swapped"], good[2]]
    dec = pkg("jpegdec").JpegDecoder(16, 16, max_images=len(files))
    try:
        if dirty:
            dec.decode([good[3], good[2], good[1], good[0], good[3]])
        rec(out, "jpegdec", dec.decode(files))
        assert out["jpegdec_1"].tolist()[0] == 0 and out["jpegdec_1"][1] != 0 and out["jpegdec_1"][3] != 0
    finally:
        dec.close()

    F = pkg("frames")
    bgr = np.random.default_rng(92).integers(0, 256, (3, 6, 40, 3), dtype=np.uint8)
    for fmt in ("nv12", "i420"):
        if dirty:
            F.to_bgr(F.from_bgr(other((4, 16, 64, 3)), fmt), fmt)
        yuv = F.from_bgr(bgr, fmt)
        out[f"{fmt}_tight"], out[f"{fmt}_back"] = yuv, F.to_bgr(yuv, fmt)
        pitched = F.from_bgr(bgr, fmt, pitch=64, frame_stride=700, out=np.full(2 * 700 + 64 * 9, 0x5A, np.uint8))
        out[f"{fmt}_pitched"], out[f"{fmt}_pitched_back"] = pitched, F.to_bgr(pitched, fmt, hw=(6, 40), pitch=64, frame_stride=700)

    shape = (3, 70, 131)
    fr = TR.frames_of(shape, 3)
    rows, counts = TR.rows_for(*shape, 4)
    prims = TR.prims_for(*shape)
    cams = np.array([1, 0, 1], np.int32)
    r = pkg("render").Renderer(cameras=2, redact="box", style="mosaic", cell=8, classes={0, 2}, mask_color=(9, 8, 7), pad=1)
    try:
        for c, polys in TR.MASKS.items():
            r.set_masks(c, polys)
        if dirty:
            r.render(other((4, 96, 160, 3)), *TR.rows_for(4, 96, 160, 9), TR.prims_for(4, 96, 160))
        out["render_all"] = r.render(fr.copy(), rows, counts, prims, cams)
        out["render_masks_only"] = r.render(fr.copy())
    finally:
        r.close()

    s = 2
    pair = TG._pair(32 * s + s - 1, 48 * s + 3 * s - 1, 2 * s, -s)            # "odd": sizes that are no multiples of the downscale
    cm = pkg("gmc").CameraMotion(pair.shape[1], pair.shape[2], downscale=s, min_inliers=2)
    try:
        out["gmc_warps"], out["gmc_stats"] = cm.apply_batch(pair), cm.stats
    finally:
        cm.close()
    return out


GROUPS = {"detector": group_detector, "detectors32": group_detectors32, "reid": group_reid, "pipeline": group_pipeline, "banks": group_banks,
          "analytics": group_analytics, "codecs": group_codecs}
DIRTY = ("detector", "reid", "codecs")     # groups of stateless handles with a dirty variant


def run_group(group, out_dir, dirty=False):
    L = pkg("_lib")
    out = {"probe_" + k: v for k, v in L.debug_alloc_probe().items()}          # first: nothing this process freed can be behind it
    if group != "probe":
        out.update(GROUPS[group](out_dir, dirty))
    return out


def main(argv):
    group, out_dir, tag = argv[1], argv[2], argv[3]
    out = run_group(group, out_dir, dirty=len(argv) > 4 and argv[4] == "dirty")
    for k, v in out.items():
        np.save(os.path.join(out_dir, f"{tag}_{k}.npy"), np.asarray(v))


if __name__ == "__main__":
    main(sys.argv)
    sys.exit(0)
