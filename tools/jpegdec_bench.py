#!/usr/bin/env python3
"""Time the JPEG decoding stage (ai-camera_amd/jpegdec.py) on the GPU.

    python tools/jpegdec_bench.py [--repeats 5] [--json out.json]     measure (needs the MI355X)
    python tools/jpegdec_bench.py --design out.json                   write the table into DESIGN.md section 43

Banks of 1, 16 and 256 files of 1280 x 720 (4:2:0, restart interval one MCU row), the 256 bank again with a single interval per image
(restart 65535: a camera that sends no restart markers) and 512 thumbnails of 64 x 128 (4:4:4), all quality 85, written by the device
encoder from rendered synthetic scenes.  Before anything is timed the first and the last picture of the bank are compared with libjpeg's
(Pillow), which tests/test_jpegdec_oracle.py holds equal to the specification.  Times are host wall time per decode_packed call into
device memory, ending in the library's stream synchronise: the host parse, the copies, all four kernels.  Beside them:

  floor      the bytes the kernels must move through HBM -- the files read once, the coefficients zeroed, written and read (3 x), the
             samples written and read, the frames written -- over 6.3 TB/s
  raw copy   the same frames copied host to device as they are, from pageable and from pinned memory: what upload pays without this stage
  NV12       the same frames as NV12 (1.5 bytes per pixel) copied host to device from pageable memory, without the unpack kernel
  Pillow     PIL's decoder (libjpeg) on the same files on 16 host threads, where PIL imports"""
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
sys.path.insert(0, str(ROOT / "tools"))

BEGIN, END = "<!-- jpegdec_bench:begin -->", "<!-- jpegdec_bench:end -->"
ROOF_TBS = 6.3
QUALITY = 85
CONFIGS = (((720, 1280), "420", 1, 0), ((720, 1280), "420", 16, 0), ((720, 1280), "420", 256, 0), ((720, 1280), "420", 256, 65535), ((128, 64), "444", 512, 0))


def timed(fn, repeats):
    fn()                                                                     # warm-up: allocations, code objects
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return sorted(t)


def pillow(files, repeats):
    try:
        from PIL import Image
    except Exception:                                                        # noqa: BLE001 -- absent: the column stays empty
        return None, None
    one = lambda f: np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))     # noqa: E731
    with ThreadPoolExecutor(max_workers=16) as ex:
        t = timed(lambda: list(ex.map(one, files)), repeats)
    return t, (one(files[0]), one(files[-1]))


def measure(hw, sub, n, restart, repeats):
    import torch
    from jpeg_bench import images_for
    J, D = importlib.import_module("ai-camera_amd.jpeg"), importlib.import_module("ai-camera_amd.jpegdec")
    host = images_for(hw, n)
    enc = J.JpegEncoder(hw, max_images=n, quality=QUALITY, restart=restart, subsampling=sub, max_bytes="worst")
    buf, off, status = enc.encode_packed(host)
    assert not status.any()
    buf = buf[:int(off[n])].copy()
    enc.close()
    files = [buf[off[i]:off[i + 1]].tobytes() for i in range(n)]
    g = J.geometry(hw, restart, sub)
    dec = D.JpegDecoder(hw[0], hw[1], max_images=n)
    d_out = torch.empty((n, hw[0], hw[1], 3), dtype=torch.uint8, device="cuda")
    _, st, _ = dec.decode_packed(buf, off, out=d_out)
    assert not st.any()
    got = d_out[[0, n - 1]].cpu().numpy()
    t_pil, ref = pillow(files, min(repeats, 3))
    if ref is not None:
        for k in range(2):
            assert np.array_equal(got[k], ref[k][:, :, ::-1]), f"image {(0, n - 1)[k]} differs from libjpeg's"
    blocks = n * g["n_mcu"] * g["bpm"]
    res = dict(hw=list(hw), subsampling=sub, images=n, restart=restart, intervals=g["intervals"], repeats=repeats, file_bytes=int(off[n]), frame_bytes=host.nbytes,
               floor_ms=round(1e3 * (int(off[n]) + 3 * blocks * 128 + 2 * blocks * 64 + host.nbytes) / (ROOF_TBS * 1e12), 4))
    ms = lambda t: [round(1e3 * x, 4) for x in t]                            # noqa: E731
    res["host_files_ms"] = ms(timed(lambda: dec.decode_packed(buf, off, out=d_out), repeats))
    d_buf = torch.from_numpy(buf).cuda()
    res["device_files_ms"] = ms(timed(lambda: dec.decode_packed(d_buf, off, out=d_out), repeats))

    def sync(fn):
        fn()
        torch.cuda.synchronize()
    res["raw_pageable_ms"] = ms(timed(lambda: sync(lambda: d_out.copy_(torch.from_numpy(host))), repeats))
    pinned = torch.from_numpy(host).pin_memory()
    res["raw_pinned_ms"] = ms(timed(lambda: sync(lambda: d_out.copy_(pinned, non_blocking=True)), repeats))
    del pinned
    nv12 = torch.zeros(host.nbytes // 2, dtype=torch.uint8)
    d_nv12 = torch.empty_like(nv12, device="cuda")
    res["nv12_pageable_ms"] = ms(timed(lambda: sync(lambda: d_nv12.copy_(nv12)), repeats))
    if t_pil is not None:
        res["pillow_ms"] = ms(t_pil)
    dec.close()
    return res


def table(results):
    def cell(r, key):
        v = r.get(key)
        return f"{statistics.median(v):.3f} ({v[0]:.3f}..{v[-1]:.3f})" if v else "-"
    lines = ["| bank | intervals per image | files in host memory, ms per call | files on the device, ms per call | HBM floor, ms | on the device / floor | raw frames H2D, pageable, ms | "
             "raw frames H2D, pinned, ms | NV12 H2D, pageable, ms | Pillow, 16 threads, ms | file bytes / raw bytes |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        on_dev = statistics.median(r["device_files_ms"])
        lines.append(f"| {r['images']} x {r['hw'][1]} x {r['hw'][0]}, {r['subsampling']} | {r['intervals']} | {cell(r, 'host_files_ms')} | {cell(r, 'device_files_ms')} | "
                     f"{r['floor_ms']:.4f} | {on_dev / r['floor_ms']:.1f} | {cell(r, 'raw_pageable_ms')} | {cell(r, 'raw_pinned_ms')} | {cell(r, 'nv12_pageable_ms')} | "
                     f"{cell(r, 'pillow_ms')} | {r['file_bytes'] / r['frame_bytes']:.3f} |")
    lines.append("")
    lines.append(f"Quality {QUALITY}, frames decoded into device memory; median (min..max) of {results[0]['repeats']} calls after a warm-up call; host wall time of the whole "
                 "call.  Floor: (file bytes + 3 x coefficient bytes + 2 x sample bytes + frame bytes) / 6.3 TB/s.")
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
    for hw, sub, n, restart in CONFIGS:
        if only is not None and n not in only:
            continue
        results.append(measure(hw, sub, n, restart, a.repeats))
        print(json.dumps(results[-1]), flush=True)
        if a.json:
            Path(a.json).parent.mkdir(parents=True, exist_ok=True)
            Path(a.json).write_text(json.dumps(results, indent=1))
    print(table(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
