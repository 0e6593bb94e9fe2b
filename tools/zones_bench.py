#!/usr/bin/env python3
"""Time the zone / line counting stage (ai-camera_amd/zones.py) on the GPU.

    python tools/zones_bench.py [--ticks 64] [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/zones_bench.py --design out.json                                write the table into DESIGN.md section 27

For S in {1, 16, 256} cameras x 30 rows per frame x 4 zones x 2 lines, host wall time per tick (one frame of every camera; every call
ends in the library's own stream synchronise), median over --repeats passes of --ticks ticks after one warm-up pass:
  bank-1    one ZoneCounter(streams=S), one update per tick
  bank-16   the same, 16 ticks per update
  singles   S ZoneCounter(streams=1) objects, one update each per tick: the per-stream loop the bank removes, at the same commit
  oracle    tests/zones_oracle.py, the pure-Python loop a user would otherwise write (one pass; it is slow)
The results of all four are compared before anything is timed."""
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

BEGIN, END = "<!-- zones_bench:begin -->", "<!-- zones_bench:end -->"
ZONES = [[(100, 100), (600, 100), (600, 400), (100, 400)], [(700, 50), (1200, 300), (700, 650)],
         [(200, 450), (500, 450), (500, 550), (350, 550), (350, 700), (200, 700)], [(900, 400), (1250, 400), (1250, 700), (900, 700)]]
LINES = [((640, 0), (640, 720)), ((0, 360), (1280, 360))]


def scene(S, ticks, rows=30, seed=0):
    """frames[s][t]: `rows` walkers per camera bouncing through a 1280 x 720 frame."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform([0, 0], [1280, 720], (S, rows, 2))
    vel = rng.uniform(-12, 12, (S, rows, 2))
    ids = np.arange(1, rows + 1, dtype=np.int32)
    out = [[] for _ in range(S)]
    for _ in range(ticks):
        pos += vel
        for d, hi in ((0, 1280), (1, 720)):
            bad = (pos[..., d] < 0) | (pos[..., d] > hi)
            vel[..., d][bad] *= -1
            pos[..., d] = np.clip(pos[..., d], 0, hi)
        p = np.rint(pos).astype(np.int32)
        for s in range(S):
            r = np.zeros((rows, 6), np.int32)
            r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4] = p[s, :, 0] - 20, p[s, :, 1] - 120, p[s, :, 0] + 20, p[s, :, 1], ids
            out[s].append(r)
    return out


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def measure(S, ticks, repeats):
    Z = importlib.import_module("ai-camera_amd.zones")
    import zones_oracle as ZO
    frames = scene(S, ticks)

    def bank(chunk):
        zc = Z.ZoneCounter(streams=S)
        for s in range(S):
            zc.set_zones(s, ZONES, LINES)

        def run():
            for s in range(S):
                zc.reset(s)
            return [zc.update([f[t:t + chunk] for f in frames]) for t in range(0, ticks, chunk)]
        return zc, run

    ones = [Z.ZoneCounter(streams=1) for _ in range(S)]
    for o in ones:
        o.set_zones(0, ZONES, LINES)

    def singles():
        for o in ones:
            o.reset(0)
        return [[o.update([[f[t]]]) for o, f in zip(ones, frames)] for t in range(ticks)]

    b1, run1 = bank(1)
    b16, run16 = bank(16)
    # ---- the same answers everywhere, first
    oracles = [ZO.ZonesOracle(ZONES, LINES) for _ in range(S)]
    t0 = time.perf_counter()
    want = [ZO.run_bank(oracles, [[f[t]] for f in frames], 256) for t in range(ticks)]
    t_oracle = time.perf_counter() - t0
    got1, got16, gots = run1(), run16(), singles()
    for t in range(ticks):
        assert np.array_equal(got1[t].events, want[t][1]) and np.array_equal(got1[t].occupancy, want[t][2]), ("bank-1", t)
        assert np.array_equal(got16[t // 16].events.reshape(S, 16, 256, 8)[:, t % 16], want[t][1]), ("bank-16", t)     # stream-major
        assert all(np.array_equal(gots[t][s].events[0], want[t][1][s]) for s in range(S)), ("singles", t)
    n_events = int(sum(w[0].sum() for w in want))
    res = dict(streams=S, ticks=ticks, rows=30, zones=len(ZONES), lines=len(LINES), events=n_events, repeats=repeats)
    for name, fn in (("bank_1", run1), ("bank_16", run16), ("singles", singles)):
        t = timed(fn, repeats)
        res[name + "_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    res["oracle_ms_per_tick"] = [round(1e3 * t_oracle / ticks, 4)]
    for o in ones + [b1, b16]:
        o.close()
    return res


def table(results):
    def cell(r, key):
        v = r[key + "_ms_per_tick"]
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if len(v) > 1 else f"{v[0]:.3f}"
    lines = ["| S | bank, 1 tick per call | bank, 16 ticks per call | S single-stream objects | NumPy oracle loop | singles / bank-1 |", "|---|---|---|---|---|---|"]
    for r in results:
        ratio = statistics.median(r["singles_ms_per_tick"]) / statistics.median(r["bank_1_ms_per_tick"])
        lines.append(f"| {r['streams']} | {cell(r, 'bank_1')} | {cell(r, 'bank_16')} | {cell(r, 'singles')} | {cell(r, 'oracle')} | {ratio:.2f} |")
    r = results[0]
    lines.append("")
    lines.append(f"ms per tick (one frame of every camera), median (min..max) of {r['repeats']} passes of {r['ticks']} ticks after a warm-up pass; "
                 f"{r['rows']} rows x {r['zones']} zones x {r['lines']} lines per camera; the oracle loop ran once.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=64, help="a multiple of 16")
    ap.add_argument("--repeats", type=int, default=5)
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
    if a.ticks % 16:
        ap.error("--ticks must be a multiple of 16")
    if importlib.import_module("ai-camera_amd._lib").device_count() < 1:
        print("no GPU: nothing is measured (there is no CPU path to time)", file=sys.stderr)
        return 1
    results = []
    for S in (int(x) for x in a.streams.split(",")):
        results.append(measure(S, a.ticks, a.repeats))
        print(json.dumps(results[-1]), flush=True)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
