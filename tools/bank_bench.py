#!/usr/bin/env python3
"""Tracker banks against loops over single trackers, and the conv CU reserve of a multi-stream pipeline (run by hand).

    python tools/bank_bench.py tracker  [--kinds bytetrack,ocsort] [--streams 1,8,32,128,256] [--ticks 256]
    python tools/bank_bench.py pipeline [--streams 1,8,32] [--reserve 1,2,4,8,16] [--ring 512] [--batch 256]

tracker:  S synthetic 30-person streams for `ticks` ticks, fed one tick per call and 16 ticks per call, to a bank of S streams
          (one launch of S blocks per epoch) and to S single trackers in a loop (S launches and syncs per epoch: what a caller had
          before the banks).  Prints frames/s and ms per tick.
pipeline: the ByteTrack pipeline on the trained detector's own detections, ring resident in HBM, `streams` tick-major streams, the
          epoch blocks' CU reserve ("tracker_cus") swept.  Prints frames/s.
Every configuration is a child process of its own under `timeout`, and the first one that fails ends the run.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


def stream_frames(seed, ticks):
    import numpy as np
    sc = pkg("synthetic").Scene(seed=seed, n_targets=30, conf_range=(0.3, 0.95), jitter=1.5, shuffle=True)
    return [tuple(np.ascontiguousarray(a) for a in sc.detections(f)[:3]) for f in range(ticks)]


def step_tracker(kind, S, ticks):
    base = [stream_frames(seed, ticks) for seed in range(min(S, 8))]       # 8 distinct scenes, reused round-robin
    dets = [base[s % len(base)] for s in range(S)]
    mod = pkg("bytetrack" if kind == "bytetrack" else "ocsort")
    Bank, One = (mod.BYTETrackerBank, mod.BYTETracker) if kind == "bytetrack" else (mod.OCSortBank, mod.OCSort)
    out = dict(kind=kind, streams=S, ticks=ticks)
    for per_call in (1, 16):
        bk = Bank(S)
        bk.update_arrays([d[:per_call] for d in dets])                       # warm-up call (module load, staging buffers)
        bk.close()
        bk = Bank(S)
        t0 = time.perf_counter()
        for t in range(0, ticks, per_call):
            bk.update_arrays([d[t:t + per_call] for d in dets])
        t_bank = time.perf_counter() - t0
        bk.close()
        ones = [One() for _ in range(S)]
        t0 = time.perf_counter()
        for t in range(0, ticks, per_call):
            for s in range(S):
                ones[s].update_batch_arrays(dets[s][t:t + per_call])
        t_loop = time.perf_counter() - t0
        for o in ones:
            o.close()
        out[f"bank_{per_call}"] = dict(fps=S * ticks / t_bank, ms_per_tick=1e3 * t_bank / ticks)
        out[f"loop_{per_call}"] = dict(fps=S * ticks / t_loop, ms_per_tick=1e3 * t_loop / ticks)
    print(json.dumps(out), flush=True)


def step_pipeline(S, reserve, ring, batch, steps):
    import numpy as np
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    sc = pkg("synthetic").Scene(seed=0, n_targets=30)
    uniq = sc.render_batch(0, 64)
    pipe = pkg("pipeline").TrackingPipeline(ypath, None, (720, 1280), batch=batch, ring_frames=ring, max_persons=64, dtype="fp16",
                                            tracker="bytetrack", streams=S)
    pipe.option("tracker_cus", reserve)
    for i in range(0, ring, 64):                                            # every stream walks the same 64-frame clip
        pipe.upload(i, uniq[[((i + j) // S) % 64 for j in range(min(64, ring - i))]])
    pipe.run_raw(0, ring)                                                   # warm-up
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        pipe.run_raw(0, ring)
        times.append(time.perf_counter() - t0)
    pipe.close()
    print(json.dumps(dict(streams=S, tracker_cus=reserve, ring=ring, batch=batch, fps_median=ring / float(np.median(times)),
                          fps_min=ring / max(times), fps_max=ring / min(times))), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("mode", choices=("tracker", "pipeline", "step-tracker", "step-pipeline"))
    p.add_argument("--kinds", default="bytetrack,ocsort")
    p.add_argument("--streams", default=None)
    p.add_argument("--ticks", type=int, default=256)
    p.add_argument("--reserve", default="1,2,4,8,16")
    p.add_argument("--ring", type=int, default=512)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--limit", type=int, default=150, help="seconds a configuration may take")
    a = p.parse_args()
    if a.mode == "step-tracker":
        return step_tracker(a.kinds, int(a.streams), a.ticks)
    if a.mode == "step-pipeline":
        return step_pipeline(int(a.streams), int(a.reserve), a.ring, a.batch, a.steps)
    me = [sys.executable, os.path.abspath(__file__)]
    if a.mode == "tracker":
        jobs = [me + ["step-tracker", "--kinds", k, "--streams", s, "--ticks", str(a.ticks)]
                for k in a.kinds.split(",") for s in (a.streams or "1,8,32,128,256").split(",")]
    else:
        jobs = [me + ["step-pipeline", "--streams", s, "--reserve", r, "--ring", str(a.ring), "--batch", str(a.batch), "--steps", str(a.steps)]
                for s in (a.streams or "1,8,32").split(",") for r in (a.reserve.split(",") if int(s) > 1 else ["1"])]
    for job in jobs:                                                        # each GPU step under its own time limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(a.limit)] + job).returncode
        if rc:
            print(f"step failed (exit {rc}): {' '.join(job[2:])}", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
