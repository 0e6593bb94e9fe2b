"""Host wall time of the output stage per tick: S frames of 1280 x 720, 30 tracked boxes per frame with their
labels and the info panel, ending in the library's stream synchronise.  Median (min..max) of 5 passes after a warm-up, in ms per tick.

    python tools/render_bench.py [--out FILE.json]

Columns:
  (i)   one Renderer.render call, annotation only
  (ii)  the same call plus redact="box", style mosaic:16
  (iii) the loop of visualization.draw_frame per frame with the same primitives (the path before the renderer, unchanged)
  (iv)  device-resident frames: the render call (annotation only) against a loop of aic_overlay with AIC_DEVICE -- the kernels and
        their list uploads without the frame copies
Kernel time alone is not measured here (no profiler run), nor are crowded tiles (hundreds of primitives in one tile)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, ROWS, PASSES = 720, 1280, 30, 5


def scene(S, seed=0):
    V = importlib.import_module("ai-camera_amd.visualization")
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (S, H, W, 3), dtype=np.uint8)
    rows, prims, tracks = [], [], []
    for f in range(S):
        x, y = rng.integers(0, W - 120, ROWS), rng.integers(30, H - 260, ROWS)
        w, h = rng.integers(40, 120, ROWS), rng.integers(100, 260, ROWS)
        tr = [(int(x[i]), int(y[i]), int(x[i] + w[i]), int(y[i] + h[i]), 100 * f + i, "person", 0.87) for i in range(ROWS)]
        tracks.append(tr)
        rows.append(np.array([[t[0], t[1], t[2], t[3], t[4], 0] for t in tr], np.int32))
        prims.append(V.info_prims(V.track_prims(V.PrimList(), tr), ["AICamera: YOLOv8 + ByteTrack", f"Input: camera {f} (stream {f})"]))
    return frames, np.concatenate(rows), np.full(S, ROWS, np.int32), prims, tracks


def timed(fn):
    fn()                                                    # warm-up: buffers grown, code paths touched
    ts = []
    for _ in range(PASSES):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    V = importlib.import_module("ai-camera_amd.visualization")
    R = importlib.import_module("ai-camera_amd.render")
    L = importlib.import_module("ai-camera_amd._lib")
    out = {"frame": [H, W], "rows_per_frame": ROWS, "passes": PASSES, "unit": "ms per tick (host wall time, ends in the stream synchronise)", "S": {}}
    for S in (1, 16, 64):
        frames, rows, counts, prims, tracks = scene(S)
        work = frames.copy()
        plain, redact = R.Renderer(cameras=S), R.Renderer(cameras=S, redact="box", style="mosaic", cell=16)
        dev = torch.from_numpy(frames).cuda()
        lists = [p.arrays() for p in prims]

        def overlay_device_loop():
            for f in range(S):
                p, t = lists[f]
                L.call("aic_overlay", 0, L.ptr(int(dev[f].data_ptr())), H, W, L.DEVICE, L.ptr(p), len(p), L.ptr(t), len(t))

        def draw_frame_loop():
            for f in range(S):
                V.render(work[f], prims[f])

        res = {"i_render_annotate": timed(lambda: plain.render(work, prims=prims)),
               "ii_render_annotate_redact": timed(lambda: redact.render(work, rows, counts, prims)),
               "iii_draw_frame_loop": timed(draw_frame_loop),
               "iv_device_render": timed(lambda: plain.render(dev, prims=prims)),
               "iv_device_overlay_loop": timed(overlay_device_loop)}
        out["S"][str(S)] = res
        plain.close(), redact.close()
        print(f"S={S:3d}  " + "  ".join(f"{k}: {v['median']:.3f} ({v['min']:.3f}..{v['max']:.3f})" for k, v in res.items()), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
