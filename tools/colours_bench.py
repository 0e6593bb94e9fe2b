#!/usr/bin/env python3
"""Time the clothing-colour stage (ai-camera_amd/colours.py) on the GPU.

    python tools/colours_bench.py [--ticks 8] [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/colours_bench.py --design out.json                               write the table into DESIGN.md section 45

For S in {1, 16, 256} cameras x 30 rows per frame on 1280 x 720 noise frames with the default parts, host wall time per tick (one frame
of every camera; every call ends in the library's own stream synchronise), median over --repeats passes of --ticks ticks after one
warm-up pass.  Frames AND rows lie in device memory, as a pipeline's ring and a tracker bank hold them.
  bank      one TrackColours(streams=S), one update per tick
  singles   S TrackColours(streams=1) objects, one update each per tick: the per-stream loop the bank removes, at the same commit
  oracle    tests/colours_oracle.py over the first ticks, the NumPy loop a user would otherwise write (once; it is slow)
The bank and the singles are compared with the oracle before anything is timed.  "part bytes" is what the sample kernel really reads of
the frames per tick: 3 bytes for every pixel of every sampled part."""
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

BEGIN, END = "<!-- colours_bench:begin -->", "<!-- colours_bench:end -->"
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


def measure(S, ticks, repeats, oracle_ticks, singles=True):
    import torch
    M = importlib.import_module("ai-camera_amd.colours")
    import colours_oracle as CO
    rows = scene(S, ticks)
    gen = torch.Generator(device="cuda").manual_seed(S)
    frames = torch.randint(0, 256, (ticks, S, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    d_rows = [torch.from_numpy(np.concatenate(tick)).cuda() for tick in rows]                     # [S * ROWS, 6] per tick
    d_one = [[torch.from_numpy(r).cuda() for r in tick] for tick in rows]
    counts, one = torch.full((S,), ROWS, dtype=torch.int32, device="cuda"), torch.full((1,), ROWS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bank = M.TrackColours(S, (H, W))
    ones = [M.TrackColours(1, (H, W)) for _ in range(S if singles else 0)]

    def run_bank():
        return [bank.update(frames[t:t + 1], d_rows[t], counts=counts) for t in range(ticks)]

    def run_singles():
        return [[o.update(frames[t:t + 1, s:s + 1], d_one[t][s], counts=one) for s, o in enumerate(ones)] for t in range(ticks)]

    # ---- the same answers everywhere, first: the tables after the first ticks, stream by stream, and every row tag
    oracles = [CO.ColoursOracle((H, W), stream=s) for s in range(S)]
    host = frames[:oracle_ticks].cpu().numpy()
    t0 = time.perf_counter()
    want = CO.run_bank(oracles, host, rows[:oracle_ticks], 16)
    t_oracle = time.perf_counter() - t0
    sampled_px = 0                                                           # pixels of the sampled parts of the last oracle tick
    for s, o in enumerate(oracles):
        r = np.asarray(rows[oracle_ticks - 1][s], np.int64)
        for i in range(len(r)):
            for part in range(2):
                P = CO.clip(CO.part_of(r[i], o.fracs[part], o.inset_q8), H, W)
                if P is not None and P[2] - P[0] + 1 >= o.min_w and P[3] - P[1] + 1 >= o.min_h and CO.cover_q8(r, i, P, H, W) <= o.max_cover_q8:
                    sampled_px += (P[2] - P[0] + 1) * (P[3] - P[1] + 1)
    tags = []
    for t in range(oracle_ticks):
        tags.append(bank.update(frames[t:t + 1], d_rows[t], counts=counts).row_tags)
        for s, o in enumerate(ones):
            got = o.update(frames[t:t + 1, s:s + 1], d_one[t][s], counts=one).row_tags
            assert np.array_equal(got, tags[-1][s * ROWS:(s + 1) * ROWS]), ("singles", t, s)
    assert np.array_equal(np.concatenate(tags), want[2]), "row tags"
    for s in range(S):
        exp = oracles[s].export()
        for what, ev in (("bank", bank.export(s)),) + ((("singles", ones[s].export(0)),) if singles else ()):
            assert len(ev) == len(exp) == ROWS, (what, s, len(ev), len(exp))
            for k, e in enumerate(exp):
                e = e.copy()
                e[1] = s if what == "bank" else 0
                assert np.array_equal(ev[k], e), (what, s, k)
    for s in range(S):
        bank.reset(s)
    for o in ones:
        o.reset(0)
    res = dict(streams=S, ticks=ticks, rows=ROWS, repeats=repeats, oracle_ticks=oracle_ticks, part_bytes_per_tick=3 * sampled_px,
               frame_bytes_per_tick=S * H * W * 3)
    t = timed(run_bank, repeats)
    res["bank_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    t = timed(run_singles, repeats) if singles else t
    res["singles_ms_per_tick"] = [round(1e3 * x / ticks, 4) for x in sorted(t)]
    res["oracle_ms_per_tick"] = [round(1e3 * t_oracle / oracle_ticks, 4)]
    for o in ones + [bank]:
        o.close()
    return res


def table(results):
    def cell(r, key):
        v = r[key + "_ms_per_tick"]
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if len(v) > 1 else f"{v[0]:.1f}"
    lines = ["| S | bank, 1 tick per call | S single-stream objects | NumPy oracle loop | singles / bank | part bytes read per tick | of the frames |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        ratio = statistics.median(r["singles_ms_per_tick"]) / statistics.median(r["bank_ms_per_tick"])
        lines.append(f"| {r['streams']} | {cell(r, 'bank')} | {cell(r, 'singles')} | {cell(r, 'oracle')} | {ratio:.2f} | "
                     f"{r['part_bytes_per_tick'] / 1e6:.2f} MB | {100 * r['part_bytes_per_tick'] / r['frame_bytes_per_tick']:.1f} % |")
    r = results[0]
    lines.append("")
    lines.append(f"ms per tick (one 1280 x 720 frame of every camera; frames and rows in device memory), median (min..max) of {r['repeats']} passes "
                 f"after a warm-up pass; {r['rows']} rows per camera, default parts; ticks per pass: " +
                 ", ".join(f"S = {x['streams']}: {x['ticks']}" for x in results) + "; the oracle loop ran once over " +
                 ", ".join(f"{x['oracle_ticks']}" for x in results) + " ticks.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=8, help="ticks per pass (at S = 256 a tick of frames is 708 MB of device memory)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle_ticks", type=int, default=2)
    ap.add_argument("--bank_only", action="store_true", help="no single-stream objects: what a kernel trace of the bank alone needs")
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
        results.append(measure(S, a.ticks if S < 256 else min(a.ticks, 4), a.repeats, min(a.oracle_ticks, a.ticks), not a.bank_only))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
