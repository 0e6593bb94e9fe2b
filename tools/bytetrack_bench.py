"""ByteTrack and OC-SORT pipelines on the bench's headline workload, next to DeepSORT in the same process.

1280x720, 30 planted persons (inject = 1), YOLOv8n on the trained weights, fp16, 512-frame launch groups (bench.py's clip: 256
frames forward then backward).  Prints ONE JSON line: frames/s of the ByteTrack and the OC-SORT pipeline (both detector-only) from
HBM-resident frames and from host memory, the tracker stream's time per launch group and per 16-frame epoch (HIP events on the tracker kernels), the DeepSORT
pipeline's frames/s measured the same way, and MOTA / IDF1 / ID switches of the three trackers against the planted identities on one scene whose scores
are widened to (0.05, 0.95) so that ByteTrack's low band is used.  BoT-SORT appears twice: its pipeline (with the ReID engine, as
DeepSORT's) in the same columns -- then with the camera-motion option gmc = 4, then with gmc = 0 again, back to back -- and the tracker object alone (BoTSORT.update_batch_arrays, 512 frames per call,
synthetic.identity_features as the appearance input) with the shader-clock share of its appearance pass.  Its quality figures are given
with identity_features on the occlusion scene, and with the real ReID net on that scene and on the headline clip.  Reports numbers;
gates on nothing.

    python tools/bytetrack_bench.py [--steps 2] [--warmup 1]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--metric_frames", type=int, default=300)
    args = ap.parse_args()
    L, ef, syn, mm = pkg("_lib"), pkg("engine_file"), pkg("synthetic"), pkg("mot_metrics")
    TP = pkg("pipeline").TrackingPipeline
    L.load()
    dev = 0
    _, rpath = ef.ensure_seeded_engines(ROOT)
    ypath = ef.ensure_trained_detector(ROOT)
    H, W, R, persons = 720, 1280, 256, 30
    sc = syn.Scene(seed=0, n_targets=persons, width=W, height=H)
    order = list(range(R)) + list(range(R - 1, -1, -1))
    host = np.empty((2 * R, H, W, 3), np.uint8)
    host[:R] = sc.render_batch(0, R)
    host[R:] = host[:R][::-1]
    TP.pin(host)
    dets = [sc.detections(f)[:3] for f in range(R)]

    def rates(pipe):
        pipe.inject(0, [dets[f] for f in order])
        out = {}
        for mode in ("resident", "host"):
            if mode == "resident":
                pipe.upload(0, host)
                run = lambda k: pipe.run_raw_passes(0, 2 * R, k)       # noqa: E731
            else:
                run = lambda k: pipe.run_raw_from_host_passes(host, k)  # noqa: E731
            run(args.warmup)
            L.call("aic_device_sync", dev)
            L.call("aic_prof_reset", dev)
            L.call("aic_prof_enable", dev, 1 << 6)                     # class 6: tracker kernels, HIP events
            t0 = time.perf_counter()
            run(args.steps)
            L.call("aic_device_sync", dev)
            dt = time.perf_counter() - t0
            prof = L.prof_read(dev)["tracker"]
            L.call("aic_prof_enable", dev, 0)
            groups = args.steps * 2 * R / pipe.batch
            out[mode] = dict(fps=round(args.steps * 2 * R / dt, 1), tracker_ms_per_group=round(prof["ms"] / groups, 3),
                             tracker_launches=prof["launches"],
                             tracker_ms_per_launch=round(prof["ms"] / max(prof["launches"], 1), 4))
        return out

    bt = TP(ypath, None, (H, W), batch=512, ring_frames=2 * R, max_persons=32, device=dev, dtype="fp16", inject=True, tracker="bytetrack")
    res_bt = rates(bt)
    bt.close()
    oc = TP(ypath, None, (H, W), batch=512, ring_frames=2 * R, max_persons=32, device=dev, dtype="fp16", inject=True, tracker="ocsort")
    res_oc = rates(oc)
    oc.close()
    bs = TP(ypath, rpath, (H, W), batch=512, ring_frames=2 * R, max_persons=32, device=dev, dtype="fp16", inject=True, tracker="botsort")
    bs.option("split_streams", 1)
    res_bsp = rates(bs)
    bs.option("gmc", 4)                                                # the same pipeline, camera motion estimated per frame
    res_bsp_gmc = rates(bs)
    bs.option("gmc", 0)
    res_bsp_again = rates(bs)                                          # ... and off again: the spread of the gmc = 0 figure in this process
    # quality on the headline clip's first pass with the real ReID net
    bs2 = TP(ypath, rpath, (H, W), batch=512, ring_frames=2 * R, max_persons=32, device=dev, dtype="fp16", inject=True, tracker="botsort")
    bs2.upload(0, host)
    bs2.inject(0, [dets[f] for f in order])
    m = mm.evaluate(mm.scene_ground_truth(sc, R), bs2.run(0, R)[0])
    headline = dict(botsort_real_reid=dict(mota=round(m["mota"], 4), idf1=round(m["idf1"], 4), idsw=m["idsw"]))
    bs.close(), bs2.close()
    ds = TP(ypath, rpath, (H, W), batch=512, ring_frames=2 * R, max_persons=32, device=dev, dtype="fp16", inject=True)
    ds.option("split_streams", 1)                                      # as bench.py's headline
    res_ds = rates(ds)
    ds.close()

    # BoT-SORT, tracker level: the clip's planted detections with identity features, 512 frames per call
    def botsort_rates():
        trk = pkg("botsort").BoTSORT(device=dev)
        group = [dets[f] + (syn.identity_features(sc.detections(f)[3], f),) for f in order]
        for _ in range(args.warmup):
            trk.update_batch_arrays(group, cap_rows=32)
        L.call("aic_device_sync", dev)
        L.call("aic_prof_reset", dev)
        L.call("aic_prof_enable", dev, 1 << 6)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            trk.update_batch_arrays(group, cap_rows=32)
        L.call("aic_device_sync", dev)
        dt = time.perf_counter() - t0
        prof = L.prof_read(dev)["tracker"]
        L.call("aic_prof_enable", dev, 0)
        res = dict(tracker_only_fps_from_host_arrays=round(args.steps * 2 * R / dt, 1), tracker_ms_per_group=round(prof["ms"] / args.steps, 3),
                   tracker_launches=prof["launches"], tracker_ms_per_launch=round(prof["ms"] / max(prof["launches"], 1), 4),
                   counters=trk.counters())
        res["cost_pass_share_of_kernel"] = round(res["counters"]["cost_cycles"] / max(res["counters"]["kernel_cycles"], 1), 4)
        res["cost_pass_cycles_per_frame"] = round(res["counters"]["cost_cycles"] / ((args.warmup + args.steps) * 2 * R), 1)
        res["kernel_cycles_per_frame"] = round(res["counters"]["kernel_cycles"] / ((args.warmup + args.steps) * 2 * R), 1)
        trk.close()
        return res
    res_bs = botsort_rates()

    # MOTA / IDF1 on one scene with widened scores (ByteTrack's second band in use)
    n = args.metric_frames
    ms = syn.Scene(seed=7, n_targets=persons, width=W, height=H, conf_range=(0.05, 0.95),
                   gaps=[(t, 40 + 7 * t, 52 + 7 * t) for t in range(0, persons, 3)])
    frames = ms.render_batch(0, n)
    gt = mm.scene_ground_truth(ms, n)
    metrics = {}
    # ocsort: upstream's defaults (only scores above det_thresh = 0.6 take part, which on this scene is 2 detections in 5);
    # ocsort_byte: use_byte = 1, the band 0.1 < s < 0.6 keeps tracks alive as it does for ByteTrack
    for name in ("bytetrack", "ocsort", "ocsort_byte", "deepsort", "botsort_real_reid"):
        kw = dict(tracker=name.split("_")[0], **(dict(use_byte=True) if name == "ocsort_byte" else {})) if name != "deepsort" else {}
        p = TP(ypath, rpath if name in ("deepsort", "botsort_real_reid") else None, (H, W), batch=32, ring_frames=n, max_persons=64, device=dev,
               dtype="fp16", inject=True, **kw)
        p.upload(0, frames)
        p.inject(0, [ms.detections(f)[:3] for f in range(n)])
        tracks, _ = p.run(0, n)
        m = mm.evaluate(gt, tracks)
        metrics[name] = dict(mota=round(m["mota"], 4), idf1=round(m["idf1"], 4), idsw=m["idsw"])
        p.close()
    for name, reid in (("botsort", True), ("botsort_no_reid", False)):
        trk = pkg("botsort").BoTSORT(device=dev, with_reid=reid)
        outs = [trk.update(*ms.detections(f)[:3], syn.identity_features(ms.detections(f)[3], f)) for f in range(n)]
        m = mm.evaluate(gt, outs)
        metrics[name] = dict(mota=round(m["mota"], 4), idf1=round(m["idf1"], 4), idsw=m["idsw"])
        trk.close()
    print(json.dumps(dict(workload="1280x720, 30 planted persons, YOLOv8n (trained) fp16, 512-frame groups, inject=1",
                          bytetrack=res_bt, ocsort=res_oc, botsort_pipeline=res_bsp, botsort_pipeline_gmc4=res_bsp_gmc, botsort_pipeline_gmc0_again=res_bsp_again, botsort=res_bs, deepsort=res_ds, headline_metrics=headline, metrics=metrics, steps=args.steps)))


if __name__ == "__main__":
    main()
