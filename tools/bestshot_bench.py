#!/usr/bin/env python3
"""Time the best-shot stage (ai-camera_amd/bestshot.py) on the GPU.

    python tools/bestshot_bench.py [--ticks 8] [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/bestshot_bench.py --design out.json                               write the table into DESIGN.md section 38

For S in {1, 16, 256} cameras x 30 rows per frame on 1280 x 720 noise frames with the default 64 x 128 thumbnails, host wall time per
tick (one frame of every camera; every call ends in the library's own stream synchronise), median over --repeats passes of --ticks
ticks after one warm-up pass.  The frames lie in device memory, as a pipeline's ring holds them; the rows come from the host.
  bank      one BestShots(streams=S), one update per tick
  singles   S BestShots(streams=1) objects, one update each per tick: the per-stream loop the bank removes, at the same commit
  oracle    tests/bestshot_oracle.py over the first ticks, the NumPy loop a user would otherwise write (once; it is slow)
The bank and the singles are compared with the oracle before anything is timed.  "stored" counts the candidate thumbnails the
could-still-win filter let through against the candidates scored: over the first pass (fresh tracks over independent noise frames: tick
k beats the best of k - 1 earlier ones with chance 1 / k) and over a timed pass (the same frames again: the steady state of tracks
whose best shot is behind them)."""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

BEGIN, END = "<!-- bestshot_bench:begin -->", "<!-- bestshot_bench:end -->"
H, W, ROWS = 720, 1280, 30


def scene(S, ticks, seed=0):
    """rows[t][s]: ROWS walkers of 40 x 120 pixels per camera bouncing through the frame."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform([0, 120], [W, H], (S, ROWS, 2))
    vel = rng.uniform(-12, 12, (S, ROWS, 2))
    ids = np.arange(1, ROWS + 1, dtype=np.int32)
    out = []
    for _ in range(ticks):
        pos += vel
        for d, lo, hi in ((0, 0, W), (1, 120, H)):
            bad = (pos[..., d] < lo) | (pos[..., d] > hi)
            vel[..., d][bad] *= -1
            pos[..., d] = np.clip(pos[..., d], lo, hi)
        p = np.rint(pos).astype(np.int32)
        tick = []
        for s in range(S):
            r = np.zeros((ROWS, 6), np.int32)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = p[s, :, 0] - 20, p[s, :, 1] - 120, p[s, :, 0] + 19, p[s, :, 1] - 1, ids
            tick.append(r)
        out.append(tick)
    return out


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def measure(S, ticks, repeats, oracle_ticks):
    import torch
    B = importlib.import_module("ai-camera_amd.bestshot")
    import bestshot_oracle as BO
    rows = scene(S, ticks)
    gen = torch.Generator(device="cuda").manual_seed(S)
    frames = torch.randint(0, 256, (ticks, S, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    bank = B.BestShots(S, (H, W))
    bank.option("stats", 1)
    ones = [B.BestShots(1, (H, W)) for _ in range(S)]

    def run_bank():
        return [bank.update(frames[t:t + 1], rows[t:t + 1]) for t in range(ticks)]

    def run_singles():
        return [[o.update(frames[t:t + 1, s:s + 1], [[rows[t][s]]]) for s, o in enumerate(ones)] for t in range(ticks)]

    # ---- the same answers everywhere, first: the tables after the first ticks, stream by stream
    oracles = [BO.BestShotOracle((H, W), stream=s) for s in range(S)]
    host = frames[:oracle_ticks].cpu().numpy()
    t0 = time.perf_counter()
    BO.run_bank(oracles, host, rows[:oracle_ticks], 16)
    t_oracle = time.perf_counter() - t0
    for t in range(oracle_ticks):
        bank.update(frames[t:t + 1], rows[t:t + 1])
        for s, o in enumerate(ones):
            o.update(frames[t:t + 1, s:s + 1], [[rows[t][s]]])
    for s in range(S):
        want = oracles[s].export()
        for what, (ev, th) in (("bank", bank.export(s)), ("singles", ones[s].export(0))):
            assert len(ev) == len(want) == ROWS, (what, s, len(ev), len(want))
            for k, (e, t) in enumerate(want):
                e = e.copy()
                e[1] = s if what == "bank" else 0
                assert np.array_equal(ev[k], e) and np.array_equal(th[k], t), (what, s, k)
    for s in range(S):
        bank.reset(s)
        ones[s].reset(0)
    c0 = bank.counters()
    run_bank()                                                               # the first pass: fresh tracks
    c1 = bank.counters()
    res = dict(streams=S, ticks=ticks, rows=ROWS, repeats=repeats, oracle_ticks=oracle_ticks,
               first_pass=dict(candidates=(c1["candidates"] - c0["candidates"]) / ticks, stored=(c1["stored"] - c0["stored"]) / ticks))
    t = timed(run_bank, repeats)
    c2 = bank.counters()
    passes = repeats + 1
    res["steady"] = dict(candidates=(c2["candidates"] - c1["candidates"]) / ticks / passes, stored=(c2["stored"] - c1["stored"]) / ticks / passes)
    res["bank_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    run_singles()
    t = timed(run_singles, repeats)
    res["singles_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    res["oracle_ms_per_tick"] = [round(1e3 * t_oracle / oracle_ticks, 4)]
    for o in ones + [bank]:
        o.close()
    return res


def table(results):
    def cell(r, key):
        v = r[key + "_ms_per_tick"]
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if len(v) > 1 else f"{v[0]:.1f}"
    lines = ["| S | bank, 1 tick per call | S single-stream objects | NumPy oracle loop | singles / bank | stored / candidates per tick, first pass | steady state |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        ratio = statistics.median(r["singles_ms_per_tick"]) / statistics.median(r["bank_ms_per_tick"])
        f, s = r["first_pass"], r["steady"]
        lines.append(f"| {r['streams']} | {cell(r, 'bank')} | {cell(r, 'singles')} | {cell(r, 'oracle')} | {ratio:.2f} | "
                     f"{f['stored']:.1f} / {f['candidates']:.1f} | {s['stored']:.1f} / {s['candidates']:.1f} |")
    r = results[0]
    lines.append("")
    lines.append(f"ms per tick (one 1280 x 720 frame of every camera, frames in device memory), median (min..max) of {r['repeats']} passes after a "
                 f"warm-up pass; {r['rows']} rows per camera, 64 x 128 thumbnails; ticks per pass: " +
                 ", ".join(f"S = {x['streams']}: {x['ticks']}" for x in results) + "; the oracle loop ran once over " +
                 ", ".join(f"{x['oracle_ticks']}" for x in results) + " ticks.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=8, help="ticks per pass (at S = 256 a tick of frames is 708 MB of device memory)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle_ticks", type=int, default=2)
    ap.add_argument("--json", type=str, default=None, help="write the results here")
    ap.add_argument("--design", type=str, default=None, help="read results from this file and write the table into DESIGN.md; measures nothing")
    a = ap.parse_args()
    if a.design:
        results = json.loads(Path(a.design).read_text())
        path = ROOT / "DESIGN.md"
        text = path.read_text()
        i, j = text.index(BEGIN) + len(BEGIN), text.index(END)
        path.write_text(text[:i] + "\n" + table(results) + "\n" + text[j:])
        return 0
    import torch                                                             # noqa: F401 -- before libaicam.so: one HIP runtime
    if importlib.import_module("ai-camera_amd._lib").device_count() < 1:
        print("no GPU: nothing is measured (there is no CPU path to time)", file=sys.stderr)
        return 1
    results = []
    for S in (int(x) for x in a.streams.split(",")):
        results.append(measure(S, a.ticks if S < 256 else min(a.ticks, 4), a.repeats, min(a.oracle_ticks, a.ticks)))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
