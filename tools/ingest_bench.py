"""Frame ingest in NV12 against BGR24: the headline scene of bench.py (1280 x 720, 30 persons, planted detections,
batch 512, a clip of 2 x ring frames walked forward then backward) streamed from page-locked host memory, in ONE process with the arms
alternating:

    arm A   the clip as BGR24 frames -- yuv_oracle.decode(yuv_oracle.encode(frames)), so both arms do identical work behind the ring
    arm B   the same frames as NV12, unpacked into the ring on the copy stream

and, in the same run, the unpack kernel alone over 512 frames of 720p in HBM, timed with device events (aic_prof_read, class 2), against
a device-to-device copy that moves the same total bytes (read + written).

    python tools/ingest_bench.py [--ring 1024] [--batch 512] [--steps 4] [--rounds 5] [--out FILE.json]

Printed: frames/s per arm (median, min..max over the rounds; the spread of arm A is what the run cannot resolve), the H2D rate each arm
sustains, the unpack's GB/s, the copy's GB/s and their ratio.  Not measured here: the unpack under the pipeline's own kernels (its
share of a launch group), I420, pitched surfaces, the encoder direction."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import yuv_oracle as Y   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ring", type=int, default=1024, help="rendered frames R; a pass walks 2R frames (bench.py's --ring)")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--persons", type=int, default=30)
    ap.add_argument("--steps", type=int, default=4, help="passes per timed call")
    ap.add_argument("--rounds", type=int, default=5, help="timed calls per arm; the arms alternate")
    ap.add_argument("--kernel-frames", type=int, default=512)
    ap.add_argument("--threads", type=int, default=16, help="host threads preparing the clip with the oracle")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = importlib.import_module("ai-camera_amd._lib")
    ef = importlib.import_module("ai-camera_amd.engine_file")
    syn = importlib.import_module("ai-camera_amd.synthetic")
    TP = importlib.import_module("ai-camera_amd.pipeline").TrackingPipeline
    H, W, R = 720, 1280, args.ring
    ypath, rpath = ef.ensure_trained_detector(ROOT), ef.ensure_seeded_engines(ROOT)[1]
    sc = syn.Scene(seed=0, n_targets=args.persons, width=W, height=H)
    t0 = time.perf_counter()
    bgr = np.empty((2 * R, H, W, 3), np.uint8)
    nv12 = np.empty((2 * R, H * 3 // 2, W), np.uint8)

    def prepare(lo):
        hi = min(R, lo + 16)
        nv12[lo:hi] = Y.encode(sc.render_batch(lo, hi - lo), Y.NV12)
        bgr[lo:hi] = Y.decode(nv12[lo:hi], Y.NV12)
    with ThreadPoolExecutor(args.threads) as ex:
        list(ex.map(prepare, range(0, R, 16)))
    bgr[R:], nv12[R:] = bgr[:R][::-1], nv12[:R][::-1]
    print(f"clip of {2 * R} frames prepared in {time.perf_counter() - t0:.1f} s", flush=True)
    TP.pin(bgr), TP.pin(nv12)
    order = list(range(R)) + list(range(R - 1, -1, -1))
    dets = [sc.detections(f)[:3] for f in range(R)]
    mp = max(32, (args.persons + 7) // 8 * 8)
    pipe = TP(ypath, rpath, (H, W), batch=args.batch, ring_frames=2 * R, max_persons=mp, dtype="fp16", inject=True)
    pipe.inject(0, [dets[f] for f in order])
    pipe.option("split_streams", 1)

    def arm(fmt, frames):
        pipe.set_pixel_format(fmt)
        L.call("aic_device_sync", 0)
        t = time.perf_counter()
        nt, _, _ = pipe.run_raw_from_host_passes(frames, args.steps)
        dt = time.perf_counter() - t
        return 2 * R * args.steps / dt, nt.copy()
    arm("bgr24", bgr), arm("nv12", nv12)                      # warm-up: arenas, second lane, the YUV staging ring
    fps = {"bgr24": [], "nv12": []}
    rows = {}
    for _ in range(args.rounds):
        for fmt, frames in (("bgr24", bgr), ("nv12", nv12)):
            f, nt = arm(fmt, frames)
            fps[fmt].append(f)
            rows[fmt] = nt
    assert np.array_equal(rows["bgr24"], rows["nv12"]), "the arms disagree on the track counts"
    pipe.close()
    TP.unpin(bgr), TP.unpin(nv12)
    res = {"frame": [H, W], "ring": R, "batch": args.batch, "steps": args.steps, "rounds": args.rounds, "arms": {}}
    for fmt, fb in (("bgr24", H * W * 3), ("nv12", H * W * 3 // 2)):
        v = fps[fmt]
        med = statistics.median(v)
        res["arms"][fmt] = dict(fps_median=med, fps_min=min(v), fps_max=max(v), h2d_GBps=med * fb / 1e9)
        print(f"{fmt:6s} {med:9.0f} frames/s ({min(v):.0f}..{max(v):.0f})   H2D {med * fb / 1e9:5.1f} GB/s", flush=True)
    a, b = res["arms"]["bgr24"], res["arms"]["nv12"]
    res["bgr24_spread_fps"] = a["fps_max"] - a["fps_min"]
    res["nv12_minus_bgr24_fps"] = b["fps_median"] - a["fps_median"]
    print(f"nv12 - bgr24 = {res['nv12_minus_bgr24_fps']:+.0f} frames/s; the bgr24 arm's own spread is {res['bgr24_spread_fps']:.0f}")

    # the unpack kernel alone, device events (class 2 brackets aic_frames_to_bgr's launch), against a DtoD copy of the same total bytes
    K = args.kernel_frames
    src = torch.from_numpy(nv12[:K].copy()).cuda()
    dst = torch.empty((K, H, W, 3), dtype=torch.uint8, device="cuda")
    moved = K * H * W * 4.5                                   # 1.5 bytes read + 3 written per pixel
    a_, b_ = torch.empty(int(moved // 2), dtype=torch.uint8, device="cuda"), torch.empty(int(moved // 2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def unpack_ms():
        L.call("aic_prof_reset", 0)
        L.call("aic_frames_to_bgr", 0, L.ptr(int(src.data_ptr())), K, H, W, L.PIX_NV12, 0, 0, 0, 0, L.DEVICE, L.ptr(int(dst.data_ptr())))
        return L.prof_read(0)["misc"]["ms"]

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b_.copy_(a_)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    L.call("aic_prof_enable", 0, 1 << 2)
    unpack_ms(), copy_ms()
    ku, kc = [], []
    for _ in range(7):                                        # alternating, as the arms
        ku.append(unpack_ms())
        kc.append(copy_ms())
    L.call("aic_prof_enable", 0, 0)
    assert np.array_equal(dst[:2].cpu().numpy(), bgr[:2])
    u, c = statistics.median(ku), statistics.median(kc)
    res["unpack"] = dict(frames=K, ms_median=u, ms_min=min(ku), ms_max=max(ku), GBps=moved / u / 1e6, per_frame_us=u * 1e3 / K)
    res["dtod_copy"] = dict(bytes_moved=moved, ms_median=c, ms_min=min(kc), ms_max=max(kc), GBps=moved / c / 1e6)
    res["unpack_over_copy"] = res["unpack"]["GBps"] / res["dtod_copy"]["GBps"]
    print(f"unpack {K} x 720p: {u:.3f} ms ({min(ku):.3f}..{max(ku):.3f}) = {res['unpack']['GBps']:.0f} GB/s, {res['unpack']['per_frame_us']:.2f} us per frame; "
          f"DtoD copy of the same bytes: {c:.3f} ms = {res['dtod_copy']['GBps']:.0f} GB/s; ratio {res['unpack_over_copy']:.2f}")
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
