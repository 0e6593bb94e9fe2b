#!/usr/bin/env python3
"""Time the scene-watch stage (ai-camera_amd/scene.py) on the GPU.

    python tools/scene_bench.py [--ticks 8] [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/scene_bench.py --design out.json                               write the table into DESIGN.md section 39

S cameras of 1280 x 720 at c = 8, frames (random bytes: every load is a miss, every cell is busy) and 30 rows per camera in device
memory, one tick per call.  Three ways to the same records:

  bank      one SceneWatch(streams=S), one update per tick
  singles   S SceneWatch(streams=1) objects, one update each per tick: the per-stream loop the bank removes, at the same commit
  oracle    tests/scene_oracle.py over the first ticks, the NumPy loop a user would otherwise write (once; it is slow)

Before anything is timed the three are compared: records and exported state must be equal.  Times are host wall time per tick, ending in
the library's stream synchronise.  "frame GB/s" is S x 1280 x 720 x 3 bytes over the bank's median tick -- the whole call, all five
kernels and the copies of the records, not the gray kernel alone (--only_bank under rocprofv3 --kernel-trace --stats gives that)."""
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

BEGIN, END = "<!-- scene_bench:begin -->", "<!-- scene_bench:end -->"
H, W, CELL, ROWS = 720, 1280, 8, 30
ROOF_TBS = 6.3


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def measure(S, ticks, repeats, oracle_ticks, only_bank=False):
    import torch
    SW = importlib.import_module("ai-camera_amd.scene").SceneWatch
    import scene_oracle as SO
    rng = np.random.default_rng(S)
    gen = torch.Generator(device="cuda").manual_seed(S)
    frames = torch.randint(0, 256, (ticks, S, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    x1, y1 = rng.integers(0, W - 40, (ticks, S, ROWS)), rng.integers(0, H - 120, (ticks, S, ROWS))
    rows = np.stack([x1, y1, x1 + 39, y1 + 119, np.broadcast_to(np.arange(1, ROWS + 1), x1.shape), np.zeros_like(x1)], -1).astype(np.int32)
    d_rows = torch.from_numpy(rows).cuda()
    d_counts = torch.full((S,), ROWS, dtype=torch.int32, device="cuda")
    d_counts1 = d_counts[:1].contiguous()
    d_rows1 = [[d_rows[t, s].contiguous() for s in range(S)] for t in range(ticks)] if not only_bank else None
    torch.cuda.synchronize()
    kw = dict(warmup=1)                                                      # ready from the second tick on: every branch is on the clock
    bank = SW(S, (H, W), CELL, **kw)

    def run_bank():
        return [bank.update(frames[t:t + 1], d_rows[t].reshape(-1, 6), d_counts) for t in range(ticks)]

    res = dict(streams=S, ticks=ticks, rows=ROWS, repeats=repeats, oracle_ticks=oracle_ticks)
    if not only_bank:
        ones = [SW(1, (H, W), CELL, **kw) for _ in range(S)]

        def run_singles():
            return [[o.update(frames[t:t + 1, s:s + 1], d_rows1[t][s], d_counts1) for s, o in enumerate(ones)] for t in range(ticks)]

        # ---- the same answers everywhere, first
        oracles = [SO.SceneOracle((H, W), CELL, **kw) for _ in range(S)]
        host = frames[:oracle_ticks].cpu().numpy()
        t0 = time.perf_counter()
        want = SO.run(oracles, host, [[rows[t, s] for s in range(S)] for t in range(oracle_ticks)])
        t_oracle = time.perf_counter() - t0
        got = [bank.update(frames[t:t + 1], d_rows[t].reshape(-1, 6), d_counts) for t in range(oracle_ticks)]
        assert np.array_equal(np.concatenate([g.records for g in got]), want[0]), "bank records differ from the oracle's"
        assert np.array_equal(np.concatenate([g.row_motion for g in got]), want[2]), "bank row_motion differs from the oracle's"
        for s, o in enumerate(ones):
            for t in range(oracle_ticks):
                r = o.update(frames[t:t + 1, s:s + 1], d_rows1[t][s], d_counts1)
                assert np.array_equal(r.records[0, 0], want[0][t, s]), ("single", s, t)
            e, w = o.export(0), oracles[s].export()
            b = bank.export(s)
            assert all(np.array_equal(e[k], w[i]) and np.array_equal(b[k], w[i]) for i, k in enumerate(("bg", "dev", "prev", "scalars"))), s
        res["oracle_ms_per_tick"] = [round(1e3 * t_oracle / oracle_ticks, 4)]
    t = timed(run_bank, repeats)
    res["bank_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    res["frame_gbs"] = round(S * H * W * 3 / (statistics.median(t) / ticks) / 1e9, 1)
    if not only_bank:
        t = timed(run_singles, repeats)
        res["singles_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
        for o in ones:
            o.close()
    bank.close()
    return res


def table(results):
    def cell(r, key):
        v = r.get(key + "_ms_per_tick")
        if not v:
            return "-"
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if len(v) > 1 else f"{v[0]:.1f}"
    lines = ["| S | bank, 1 tick per call | S single-stream objects | NumPy oracle loop | singles / bank | frame bytes per second, whole call | of 6.3 TB/s |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        ratio = statistics.median(r["singles_ms_per_tick"]) / statistics.median(r["bank_ms_per_tick"]) if r.get("singles_ms_per_tick") else float("nan")
        lines.append(f"| {r['streams']} | {cell(r, 'bank')} | {cell(r, 'singles')} | {cell(r, 'oracle')} | {ratio:.2f} | {r['frame_gbs']:.0f} GB/s | "
                     f"{100 * r['frame_gbs'] / (1e3 * ROOF_TBS):.1f} % |")
    r = results[0]
    lines.append("")
    lines.append(f"ms per tick (one 1280 x 720 frame of every camera, c = 8, frames and {r['rows']} rows per camera in device memory), median "
                 f"(min..max) of {r['repeats']} passes after a warm-up pass; ticks per pass: " +
                 ", ".join(f"S = {x['streams']}: {x['ticks']}" for x in results) + "; the oracle loop ran once over " +
                 ", ".join(f"{x['oracle_ticks']}" for x in results) + " ticks.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=8, help="ticks per pass (at S = 256 a tick of frames is 708 MB of device memory)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle_ticks", type=int, default=2)
    ap.add_argument("--only_bank", action="store_true", help="time the bank alone, compare nothing: the run to put under a profiler")
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
        results.append(measure(S, a.ticks if S < 256 else min(a.ticks, 4), a.repeats, min(a.oracle_ticks, a.ticks), a.only_bank))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
