#!/usr/bin/env python3
"""Time the left-objects stage (ai-camera_amd/leftobj.py) on the GPU.

    python tools/left_bench.py [--ticks 8] [--repeats 5] [--json out.json]      measure (needs the MI355X)
    python tools/left_bench.py --design out.json                                write the table into DESIGN.md section 44

S cameras of 1280 x 720 at c = 8, frames and 30 rows per camera in device memory, one tick per call.  The scene is planted so that the
blob kernel has work: per camera a noisy gradient (its own noise, the same on every tick) on which 20 blocks of 3 x 4 .. 6 x 8 cells
come to rest at tick 2; with warmup 1, min_ticks 2, fast_shift 1 they are candidates from tick 7 on and objects from then on.  After
12 such ticks (the warm-up, which is also what is compared) the timed passes repeat the resting frame: every tick labels about 20
blobs of some 600 candidate cells and matches them to their 20 slots.  Three ways to the same records:

  bank      one LeftObjects(streams=S), one update per tick
  singles   S LeftObjects(streams=1) objects, one update each per tick: the per-stream loop the bank removes, at the same commit
  oracle    tests/left_oracle.py, the NumPy loop a user would otherwise write (over the warm-up ticks of the first and the last camera)

Before anything is timed they are compared: records, objects, events and exported state must be equal.  Times are host wall time per
tick, ending in the library's stream synchronise -- the whole call, all kernels and the copies of records and objects, not one kernel
(--only_bank under rocprofv3 --kernel-trace --stats gives those)."""
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

BEGIN, END = "<!-- left_bench:begin -->", "<!-- left_bench:end -->"
H, W, CELL, ROWS, BLOCKS, SETTLE = 720, 1280, 8, 30, 20, 12
OPTIONS = dict(warmup=1, min_ticks=2, fast_shift=1, alarm_hold=3)


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def planted(S, torch):
    """(base, resting) uint8 [1, S, H, W, 3] on the device, rows int32 [S, ROWS, 6]: people walk the upper half, the blocks rest below."""
    gen = torch.Generator(device="cuda").manual_seed(S)
    ramp = 60 + (torch.arange(W, device="cuda")[None, :] * 100) // W + (torch.arange(H, device="cuda")[:, None] * 40) // H
    base = (ramp[None, :, :, None] + torch.randint(-6, 7, (S, H, W, 3), device="cuda", generator=gen)).clamp(0, 255).to(torch.uint8)
    rest = base.clone()
    rng = np.random.default_rng(S)
    for s in range(S):
        for k in range(BLOCKS):                                              # a 5 x 4 lattice of places 256 x 90 px apart: no two blocks touch
            bh, bw = int(rng.integers(3, 7)) * CELL, int(rng.integers(4, 9)) * CELL
            y, x = 360 + (k // 5) * 88 + int(rng.integers(0, 3)) * CELL, (k % 5) * 256 + int(rng.integers(0, 20)) * CELL
            rest[s, y:y + bh, x:x + bw] = int(rng.integers(200, 256))
    x1, y1 = rng.integers(0, W - 40, (S, ROWS)), rng.integers(0, 200, (S, ROWS))
    rows = np.stack([x1, y1, x1 + 39, y1 + 119, np.broadcast_to(np.arange(1, ROWS + 1), x1.shape), np.zeros_like(x1)], -1).astype(np.int32)
    return base[None].contiguous(), rest[None].contiguous(), rows


def measure(S, ticks, repeats, only_bank=False):
    import torch
    LOb = importlib.import_module("ai-camera_amd.leftobj").LeftObjects
    import left_oracle as LO
    base, rest, rows = planted(S, torch)
    d_rows = torch.from_numpy(rows).cuda()
    d_counts = torch.full((S,), ROWS, dtype=torch.int32, device="cuda")
    d_counts1 = d_counts[:1].contiguous()
    d_rows1 = [d_rows[s].contiguous() for s in range(S)]
    torch.cuda.synchronize()
    frame = lambda t: base if t < 2 else rest
    bank = LOb(S, (H, W), CELL, **OPTIONS)
    res = dict(streams=S, ticks=ticks, rows=ROWS, repeats=repeats, settle=SETTLE)
    got = [bank.update(frame(t), d_rows.reshape(-1, 6), d_counts, cap_events=2 * 32 * S) for t in range(SETTLE)]      # room for every slot's two
    last = got[-1].records[0]
    res["blobs_per_camera"] = round(float(last[:, 3].mean()), 1)
    res["cand_per_camera"] = round(float(last[:, 2].mean()), 1)
    res["objects_per_camera"] = round(float(last[:, 4].mean()), 1)
    if not only_bank:
        ones = [LOb(1, (H, W), CELL, **OPTIONS) for _ in range(S)]
        single = [[o.update(frame(t)[:, s:s + 1], d_rows1[s], d_counts1) for s, o in enumerate(ones)] for t in range(SETTLE)]
        for t in range(SETTLE):                                              # the same answers everywhere, first
            for s in range(S):
                assert np.array_equal(single[t][s].records[0, 0], got[t].records[0, s]), ("single records", t, s)
                assert np.array_equal(single[t][s].objects[0, 0], got[t].objects[0, s]), ("single objects", t, s)
        t_oracle, n_oracle = 0.0, 0
        for s in sorted({0, S - 1}):
            o = LO.LeftOracle((H, W), CELL, **OPTIONS)
            host = [base[0, s].cpu().numpy(), rest[0, s].cpu().numpy()]
            for t in range(SETTLE):
                t0 = time.perf_counter()
                rec, obj, ev, _, _ = o.tick(host[t >= 2], rows[s], 0, s)
                t_oracle += time.perf_counter() - t0
                n_oracle += 1
                assert np.array_equal(rec, got[t].records[0, s]), ("oracle records", t, s)
                assert np.array_equal(obj, got[t].objects[0, s]), ("oracle objects", t, s)
                assert np.array_equal(ev, got[t].events_of(s, 0)), ("oracle events", t, s)
            e, w = bank.export(s), o.export()
            assert all(np.array_equal(e[k], w[i]) for i, k in enumerate(("fast", "slow", "still", "last_id", "last_tick", "slots", "scalars"))), s
        res["oracle_ms_per_tick"] = [round(1e3 * S * t_oracle / n_oracle, 4)]    # per tick of the whole bank: S cameras, one after the other

    def run_bank():
        return [bank.update(rest, d_rows.reshape(-1, 6), d_counts) for _ in range(ticks)]

    t = timed(run_bank, repeats)
    res["bank_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    if not only_bank:
        def run_singles():
            return [[o.update(rest[:, s:s + 1], d_rows1[s], d_counts1) for s, o in enumerate(ones)] for _ in range(ticks)]
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
    lines = ["| S | bank, 1 tick per call | S single-stream objects | NumPy oracle loop (S cameras) | singles / bank | blobs / candidate cells per camera |",
             "|---|---|---|---|---|---|"]
    for r in results:
        ratio = statistics.median(r["singles_ms_per_tick"]) / statistics.median(r["bank_ms_per_tick"]) if r.get("singles_ms_per_tick") else float("nan")
        lines.append(f"| {r['streams']} | {cell(r, 'bank')} | {cell(r, 'singles')} | {cell(r, 'oracle')} | {ratio:.2f} | "
                     f"{r['blobs_per_camera']} / {r['cand_per_camera']} |")
    r = results[0]
    lines.append("")
    lines.append(f"ms per tick (one 1280 x 720 frame of every camera, c = 8, frames and {r['rows']} rows per camera in device memory), median "
                 f"(min..max) of {r['repeats']} passes of {r['ticks']} ticks after a warm-up pass, on the resting scene after {r['settle']} settling "
                 "ticks; the oracle loop is its time per camera and tick over the settling ticks of the first and last camera, times S.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=8, help="ticks per pass")
    ap.add_argument("--repeats", type=int, default=5)
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
        results.append(measure(S, a.ticks, a.repeats, a.only_bank))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
