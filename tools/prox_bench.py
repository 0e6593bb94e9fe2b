#!/usr/bin/env python3
"""Times the proximity stage on the device: bank milliseconds per tick at S = 1 / 16 / 256 cameras with 30 rows per
camera and with 512 rows per camera (the quadratic worst case), rows in device memory, five passes sorted; the S = 256 bank against 256
single handles at the same commit.  One JSON line per figure.

    python tools/prox_bench.py [--ticks 16] [--passes 5] [--singles 256]

For the kernel's own time run it under a kernel trace of its own and read prox_walk_kernel from the statistics."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HW = (720, 1280)


def crowd(rng, streams, ticks, n):
    """[ticks * streams * n, 6] rows of n walkers per camera who drift a few pixels a tick, tick-major, and the counts."""
    x = rng.integers(40, HW[1] - 40, (streams, n))
    y = rng.integers(200, HW[0] - 10, (streams, n))
    h = rng.integers(120, 220, (streams, n))
    ids = np.broadcast_to(np.arange(n), (streams, n))
    out = np.zeros((ticks, streams, n, 6), np.int32)
    for t in range(ticks):
        x = np.clip(x + rng.integers(-4, 5, x.shape), 0, HW[1] - 1)
        y = np.clip(y + rng.integers(-2, 3, y.shape), 0, HW[0] - 1)
        out[t] = np.stack([x - 20, y - h, x + 20, y, ids, np.zeros_like(x)], -1)
    return out.reshape(-1, 6), np.full(ticks * streams, n, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=16)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--singles", type=int, default=256, help="single handles to set against the bank of as many cameras (0: skip)")
    args = ap.parse_args()
    import torch
    M = importlib.import_module("ai-camera_amd.proximity")
    rng = np.random.default_rng(55)

    def timed(stages, rows, counts, per_stage_rows=None):
        ms = []
        for _ in range(args.passes + 1):                                     # the first pass allocates and takes the slots: dropped
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k, st in enumerate(stages):
                r, c = (rows, counts) if per_stage_rows is None else per_stage_rows[k]
                st.update(r, counts=c, ticks=args.ticks, cap=0, cap_pairs=0)
            ms.append((time.perf_counter() - t0) * 1e3 / args.ticks)
        return sorted(ms[1:])

    for n in (30, 512):
        for S in (1, 16, 256):
            rows, counts = crowd(rng, S, args.ticks, n)
            st = M.Proximity(S, HW, max_tracks=512 if n > 128 else 128)
            d_rows, d_counts = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
            ms = timed([st], d_rows, d_counts)
            print(json.dumps(dict(what="bank", streams=S, rows_per_camera=n, ticks=args.ticks, ms_per_tick=[round(v, 4) for v in ms])), flush=True)
            st.close()
    if args.singles:
        S, n = args.singles, 30
        rows, counts = crowd(rng, S, args.ticks, n)
        bank = M.Proximity(S, HW)
        ms_bank = timed([bank], torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
        bank.close()
        per = rows.reshape(args.ticks, S, n, 6)
        singles = [M.Proximity(1, HW) for _ in range(S)]
        fed = [(torch.from_numpy(np.ascontiguousarray(per[:, s]).reshape(-1, 6)).cuda(), torch.from_numpy(np.full(args.ticks, n, np.int32)).cuda())
               for s in range(S)]
        ms_single = timed(singles, None, None, fed)
        for st in singles:
            st.close()
        print(json.dumps(dict(what="bank against singles", streams=S, rows_per_camera=n, ticks=args.ticks, bank_ms_per_tick=[round(v, 4) for v in ms_bank],
                              singles_ms_per_tick=[round(v, 4) for v in ms_single])), flush=True)


if __name__ == "__main__":
    main()
