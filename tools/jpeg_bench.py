#!/usr/bin/env python3
"""Time the JPEG stage (ai-camera_amd/jpeg.py) on the GPU.

    python tools/jpeg_bench.py [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/jpeg_bench.py --design out.json                   write the table into DESIGN.md section 42

Banks of 1, 16 and 256 frames of 1280 x 720 (4:2:0) and of 512 thumbnails of 64 x 128 (4:4:4) at quality 85, rendered synthetic scenes
(a few distinct frames, repeated: what a camera frame compresses like), from host and from device memory, packed into host memory.
Before anything is timed the first and the last file of the bank are compared with tests/jpeg_oracle.py.  Times are host wall time per
encode_packed call, ending in the library's stream synchronise: both kernels, both passes, the copies in and out.  Beside them:

  floor     the bytes both kernels must move through HBM -- the frames read once, the coefficients written once and read by both
            passes, the files written once -- over 6.3 TB/s
  raw copy  the bank's frames copied device to host as they are: what leaves the device without this stage
  Pillow    PIL's encoder (libjpeg) on the same frames, quality and subsampling on 16 host threads, where PIL imports"""
import argparse
import importlib
import io
import json
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

BEGIN, END = "<!-- jpeg_bench:begin -->", "<!-- jpeg_bench:end -->"
ROOF_TBS = 6.3
QUALITY = 85
CONFIGS = (("720p", (720, 1280), "420", 1), ("720p", (720, 1280), "420", 16), ("720p", (720, 1280), "420", 256), ("thumb", (128, 64), "444", 512))


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return sorted(t)


def images_for(hw, n, distinct=8):
    syn = importlib.import_module("ai-camera_amd.synthetic")
    base = syn.Scene(seed=3, n_targets=8).render_batch(0, distinct)          # [distinct, 720, 1280, 3]
    if hw != (720, 1280):
        h, w = hw
        base = np.stack([base[i % distinct, 200 + 7 * i:200 + 7 * i + h, 300 + 11 * i:300 + 11 * i + w] for i in range(4 * distinct)])
    return np.ascontiguousarray(base[np.arange(n) % len(base)])


def pillow_ms(images, sub, repeats):
    try:
        from PIL import Image
    except Exception:                                                        # noqa: BLE001 -- absent: the column stays empty
        return None, None
    rgb = [np.ascontiguousarray(im[:, :, ::-1]) for im in images]

    def one(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "JPEG", quality=QUALITY, subsampling=2 if sub == "420" else 0, optimize=False)
        return buf.tell()

    with ThreadPoolExecutor(max_workers=16) as ex:
        sizes = []
        t = timed(lambda: sizes.append(sum(ex.map(one, rgb))), repeats)
    return t, sizes[-1]


def measure(name, hw, sub, n, repeats):
    import torch
    import jpeg_oracle as O
    J = importlib.import_module("ai-camera_amd.jpeg")
    host = images_for(hw, n)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    enc = J.JpegEncoder(hw, max_images=n, quality=QUALITY, subsampling=sub, max_bytes="worst")
    buf, off, status = enc.encode_packed(dev)
    assert not status.any()
    for i in sorted({0, n - 1}):
        assert buf[off[i]:off[i + 1]].tobytes() == O.encode(host[i], QUALITY, 0, int(sub)), f"image {i} differs from the oracle"
    out_bytes, in_bytes = int(off[n]), host.nbytes
    g = J.geometry(hw, 0, sub)
    coef_bytes = n * g["n_mcu"] * g["bpm"] * 128
    res = dict(name=name, hw=list(hw), subsampling=sub, images=n, repeats=repeats, in_bytes=in_bytes, out_bytes=out_bytes, coef_bytes=coef_bytes,
               floor_ms=round(1e3 * (in_bytes + 3 * coef_bytes + out_bytes) / (ROOF_TBS * 1e12), 4))
    out = np.empty(out_bytes, np.uint8)                                      # the caller's buffer, sized by the first call's offsets
    res["device_ms"] = [round(1e3 * x, 4) for x in timed(lambda: enc.encode_packed(dev, out=out), repeats)]
    res["host_ms"] = [round(1e3 * x, 4) for x in timed(lambda: enc.encode_packed(host, out=out), repeats)]
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")       # frames and files both stay on the device: no PCIe in the call
    res["device_out_ms"] = [round(1e3 * x, 4) for x in timed(lambda: enc.encode_packed(dev, out=d_out), repeats)]
    res["raw_copy_ms"] = [round(1e3 * x, 4) for x in timed(lambda: dev.cpu(), repeats)]
    t, size = pillow_ms(host, sub, min(repeats, 3))
    if t is not None:
        res["pillow_ms"], res["pillow_bytes"] = [round(1e3 * x, 4) for x in t], size
    enc.close()
    return res


def table(results):
    def cell(r, key):
        v = r.get(key)
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if v else "-"
    lines = ["| bank | device frames, ms per call | input GB/s | files left on the device, ms | HBM floor, ms | on the device / floor | host frames, ms per call | raw D2H copy of the frames, ms | "
             "Pillow, 16 threads, ms | compression | bytes / Pillow's |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        med, on_dev = statistics.median(r["device_ms"]), statistics.median(r["device_out_ms"])
        lines.append(f"| {r['images']} x {r['hw'][1]} x {r['hw'][0]}, {r['subsampling']} | {cell(r, 'device_ms')} | {r['in_bytes'] / med / 1e6:.1f} | "
                     f"{cell(r, 'device_out_ms')} | {r['floor_ms']:.4f} | {on_dev / r['floor_ms']:.1f} | {cell(r, 'host_ms')} | {cell(r, 'raw_copy_ms')} | {cell(r, 'pillow_ms')} | "
                     f"{r['in_bytes'] / r['out_bytes']:.1f} : 1 | " + (f"{r['out_bytes'] / r['pillow_bytes']:.3f} |" if r.get("pillow_bytes") else "- |"))
    lines.append("")
    lines.append(f"Quality {QUALITY}, restart interval one MCU row, files packed into host memory (third column: into device memory); median (min..max) of {results[0]['repeats']} calls after a "
                 "warm-up call; host wall time of the whole call.  Floor: (frame bytes + 3 x coefficient bytes + file bytes) / 6.3 TB/s.")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", type=str, default=None, help="comma-separated bank sizes to run, e.g. 1,16")
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
    only = {int(x) for x in a.only.split(",")} if a.only else None
    results = []
    for name, hw, sub, n in CONFIGS:
        if only is not None and n not in only:
            continue
        results.append(measure(name, hw, sub, n, a.repeats))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
