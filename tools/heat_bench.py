#!/usr/bin/env python3
"""Time the heat-map stage (ai-camera_amd/heatmap.py) on the GPU.

    python tools/heat_bench.py [--ticks 8] [--repeats 5] [--frames 256] [--json out.json]     measure (needs the MI355X)
    python tools/heat_bench.py --only update | render                                          one half (a kernel trace of its own)
    python tools/heat_bench.py --design out.json                                               write the tables into DESIGN.md section 49

update   For S in {1, 16, 256} cameras x 30 rows per frame (the walkers of tools/colours_bench.py on 1280 x 720), host wall time per tick
         (one frame of every camera; every call ends in the library's own stream synchronise), sorted over --repeats passes of --ticks
         ticks after one warm-up pass.  Rows lie in device memory, as a tracker bank holds them.  The bank is compared with
         tests/heat_oracle.py (row tags, exported tables, all layers) before anything is timed.
render   --frames frames of 1280 x 720 x 3, in device memory and in (pageable) host memory, cell 16, log scale, alpha 160, floor 8.  The
         call is timed on the host clock around a call that ends in the library's stream synchronise, and, for device frames, by a
         pair of device events around it.  Two layers: FULL (every cell at or above the floor: every byte is read and written) and TENTH
         (a blob over about a tenth of the frame).  The HBM floor is two times the frame bytes over 8.0 TB/s (the peak in
         MI355X_MICROARCH.md).  Kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/heat_bench.py --only render`
         in a run of its own and are typed into the JSON by hand (key kernel_us) before --design."""
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
sys.path.insert(0, str(ROOT / "tools"))

BEGIN, END = "<!-- heat_bench:begin -->", "<!-- heat_bench:end -->"
H, W, ROWS, CELL = 720, 1280, 30, 16
PEAK_BYTES_PER_S = 8.0e12


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return t


def measure_update(S, ticks, repeats, oracle_ticks):
    import torch
    from colours_bench import scene
    M = importlib.import_module("ai-camera_amd.heatmap")
    import heat_oracle as HO
    rows = scene(S, ticks)
    d_rows = [torch.from_numpy(np.concatenate(tick)).cuda() for tick in rows]                     # [S * ROWS, 6] per tick
    counts = torch.full((S,), ROWS, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bank = M.HeatMaps(S, (H, W), cell=CELL)
    oracles = [HO.HeatOracle((H, W), cell=CELL, stream=s) for s in range(S)]
    want = HO.run_bank(oracles, rows[:oracle_ticks], 16)
    tags = [bank.update(d_rows[t], counts=counts).row_tags for t in range(oracle_ticks)]
    assert np.array_equal(np.concatenate(tags), want[2]), "row tags"
    for s in range(S):
        lay = bank.layers(s)
        assert np.array_equal(np.stack([lay[n] for n in HO.LAYERS]), oracles[s].layers), ("layers", s)
        exp = oracles[s].export()
        ev = bank.export(s)
        assert len(ev) == len(exp) == ROWS and all(np.array_equal(a, b) for a, b in zip(ev, exp)), ("tables", s)
        bank.reset(s)
    t = timed(lambda: [bank.update(d_rows[k], counts=counts) for k in range(ticks)], repeats)
    bank.close()
    return dict(kind="update", streams=S, ticks=ticks, rows=ROWS, repeats=repeats, bank_ms_per_tick=[round(1e3 * x / ticks, 4) for x in sorted(t)])


def planted_layer(kind):
    """int32 [GH, GW] DWELL: FULL = every cell at least a quarter of the maximum; TENTH = one blob over about a tenth of the cells."""
    GH, GW = -(-H // CELL), -(-W // CELL)
    rng = np.random.default_rng(49)
    if kind == "full":
        return rng.integers(250, 1001, (GH, GW)).astype(np.int32)
    lay = np.zeros((GH, GW), np.int32)
    lay[10:24, 20:46] = rng.integers(250, 1001, (14, 26))                    # 364 of 3600 cells
    return lay


def measure_render(n_frames, repeats):
    import torch
    M = importlib.import_module("ai-camera_amd.heatmap")
    import heat_oracle as HO
    S = 16
    hm = M.HeatMaps(S, (H, W), cell=CELL)
    gen = torch.Generator(device="cuda").manual_seed(1)
    dev = torch.randint(0, 256, (n_frames, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
    host = dev.cpu().numpy()
    out = []
    for kind in ("full", "tenth"):
        lay = planted_layer(kind)
        for s in range(S):
            hm.load_layers(s, dict(dwell=lay))
        # ---- the same bytes as the oracle on the first two frames, first
        layers = np.zeros((12,) + lay.shape, np.int32)
        layers[HO.DWELL] = lay
        want = HO.render(host[:2], [0, 1], lambda c: layers, HO.DWELL, H, W, CELL)
        assert np.array_equal(hm.render(host[:2]), want), kind
        touched = float((want != host[:2]).any(axis=-1).mean())
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev_ms = []

        def on_device():
            ev0.record()
            hm.render(dev)
            ev1.record()
            torch.cuda.synchronize()
            ev_ms.append(ev0.elapsed_time(ev1))
        t_dev = timed(on_device, repeats)
        t_host = timed(lambda: hm.render(host), max(2, repeats // 2))
        floor_ms = 2.0 * dev.numel() / PEAK_BYTES_PER_S * 1e3
        out.append(dict(kind="render", layer=kind, frames=n_frames, repeats=repeats, touched_pixels=round(touched, 4), frame_bytes=dev.numel(),
                        hbm_floor_ms=round(floor_ms, 4), device_call_ms=[round(1e3 * x, 4) for x in sorted(t_dev)],
                        device_event_ms=[round(x, 4) for x in sorted(ev_ms[1:])], host_call_ms=[round(1e3 * x, 3) for x in sorted(t_host)], kernel_us=None))
    hm.close()
    return out


def table(results):
    upd, ren = [r for r in results if r["kind"] == "update"], [r for r in results if r["kind"] == "render"]
    lines = []
    if upd:
        lines += ["| S | heat bank, 1 tick per call: ms per tick, passes sorted | median |", "|---|---|---|"]
        for r in upd:
            v = r["bank_ms_per_tick"]
            lines.append(f"| {r['streams']} | {' '.join(f'{x:.4f}' for x in v)} | {statistics.median(v):.4f} |")
        r = upd[0]
        lines += ["", f"`python tools/heat_bench.py --only update`: {r['rows']} rows per camera in device memory, {r['repeats']} passes after a warm-up pass; "
                  "ticks per pass: " + ", ".join(f"S = {x['streams']}: {x['ticks']}" for x in upd) + ".", ""]
    if ren:
        lines += ["| layer | pixels changed | device frames: call ms (host clock) | device events ms | x HBM floor | kernel (trace) | host frames: call ms |",
                  "|---|---|---|---|---|---|---|"]
        for r in ren:
            med = statistics.median(r["device_event_ms"])
            k = "not measured" if r.get("kernel_us") is None else f"{r['kernel_us']:.0f} us = {r['kernel_us'] / 1e3 / r['hbm_floor_ms']:.2f} x"
            lines.append(f"| {r['layer']} | {100 * r['touched_pixels']:.1f} % | {statistics.median(r['device_call_ms']):.3f} "
                         f"({r['device_call_ms'][0]:.3f}..{r['device_call_ms'][-1]:.3f}) | {med:.3f} | {med / r['hbm_floor_ms']:.2f} | {k} | "
                         f"{statistics.median(r['host_call_ms']):.1f} |")
        r = ren[0]
        lines += ["", f"`python tools/heat_bench.py --only render`: {r['frames']} frames of 1280 x 720 ({r['frame_bytes'] / 1e6:.0f} MB), cell 16, log scale, "
                  f"alpha 160, floor 8; HBM floor = 2 x the frame bytes / 8.0 TB/s = {r['hbm_floor_ms']:.3f} ms; median (min..max) of {r['repeats']} passes "
                  "after a warm-up pass."]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=str, default="1,16,256")
    ap.add_argument("--ticks", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--oracle_ticks", type=int, default=2)
    ap.add_argument("--frames", type=int, default=256, help="frames of a render call (256 frames of 1280 x 720 are 708 MB)")
    ap.add_argument("--only", type=str, default=None, choices=("update", "render"))
    ap.add_argument("--json", type=str, default=None, help="write the results here")
    ap.add_argument("--design", type=str, default=None, help="read results from this file and write the tables into DESIGN.md; measures nothing")
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

    def keep(r):
        results.append(r)
        print(json.dumps(r), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    if a.only != "render":
        for S in (int(x) for x in a.streams.split(",")):
            keep(measure_update(S, a.ticks, a.repeats, min(a.oracle_ticks, a.ticks)))
    if a.only != "update":
        for r in measure_render(a.frames, a.repeats):
            keep(r)
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
