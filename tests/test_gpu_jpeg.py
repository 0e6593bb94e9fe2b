"""JPEG out on the device (csrc/kernels_jpeg.hip) against tests/jpeg_oracle.py: integer arithmetic on both sides, so
the files are equal byte for byte, with their offsets and status.  Each case (tests/jpeg_cases.py) is the smallest image that can break
one part of the format; tests/test_jpeg_oracle.py shows through the oracle alone, and a decoder, that the cases reach those parts."""
import json

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import bestshot_cases as BC
import jpeg_cases as JC
import jpeg_oracle as O
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in JC.cases()}


def encoder(hw, quality=85, restart=0, subsampling=420, max_images=8, max_bytes="worst"):
    return pkg("jpeg").JpegEncoder(hw, max_images=max_images, quality=quality, restart=restart, subsampling=str(subsampling), max_bytes=max_bytes)


def on_device(images, shift=0):
    """The images in device memory, their first byte `shift` bytes behind an aligned address."""
    buf = torch.zeros(images.size + shift + 16, dtype=torch.uint8, device="cuda")
    view = buf[shift:shift + images.size].view(*images.shape)
    view.copy_(torch.from_numpy(images))
    assert view.data_ptr() % 16 == shift and view.is_contiguous()
    return view


def explain(enc, images, i, got, want, what):
    """The failure message of image i: the first differing byte, and whether the device's quantised coefficients already differ."""
    n = min(len(got), len(want))
    at = next((k for k in range(n) if got[k] != want[k]), n)
    coef = enc.coefficients(images)[i]
    ref = O.coefficients(images[i], enc.quality, enc.subsampling)
    where = "the transform: coefficients differ first at (mcu, block, k) = %s" % (np.argwhere(coef != ref)[0].tolist(),) if not np.array_equal(coef, ref) \
        else "the entropy coder: the quantised coefficients are equal"
    return f"{what}: image {i}: {len(got)} bytes, the oracle {len(want)}; first difference at byte {at} ({at - O.HEADER_BYTES} of the entropy data); {where}"


def check_bank(enc, images, want, what, frames=None):
    """encode_packed of images (or of `frames`, the same images in other memory) against the oracle's files `want`."""
    buf, off, status = enc.encode_packed(images if frames is None else frames)
    sizes = [len(w) for w in want]
    for i, w in enumerate(want):
        got = buf[off[i]:off[i + 1]].tobytes()
        assert got == w, explain(enc, images, i, got, w, what)
    assert off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and status.tolist() == [0] * len(want), (what, off, status)


@pytest.mark.parametrize("name", list(CASES))
def test_case_equals_the_oracle_from_host_and_device_memory(name):
    c = CASES[name]
    enc = encoder(c.image.shape[:2], c.quality, c.restart, c.subsampling)
    images, want = c.image[None], [JC.expected(name)]
    check_bank(enc, images, want, name + " host")
    for shift in (0, 3):
        check_bank(enc, images, want, f"{name} device+{shift}", on_device(images, shift))
    assert enc.header() == want[0][:O.HEADER_BYTES]
    enc.close()


@pytest.mark.parametrize("sub", (420, 444))
def test_banks_equal_single_calls_and_launch_cuts_change_nothing(sub):
    for n in (1, 2, 7):
        images = JC.bank(n)
        want = [O.encode(im, 85, 0, sub) for im in images]
        enc = encoder(images.shape[1:3], subsampling=sub)
        check_bank(enc, images, want, f"bank of {n}")
        check_bank(enc, images, want, f"bank of {n} device+3", on_device(images, 3))
        singles = [enc.encode(images[i:i + 1])[0] for i in range(n)]
        assert singles == want
        assert enc.counters() == dict(images=3 * n, bytes_in=3 * images.nbytes, bytes_out=3 * sum(map(len, want)))
        enc.close()
    # cuts: a 40 x 700 image has 101 KB (4:2:0) or 169 KB (4:4:4) of coefficients, so a budget of 1 MB cuts a bank of 24 in three or four
    images = np.stack([JC.scene(40, 700, 200 + i) for i in range(24)])
    a, b = encoder((40, 700), subsampling=sub, max_images=24), encoder((40, 700), subsampling=sub, max_images=24)
    b.option("launch_budget_mb", 1)
    fa, fb = a.encode(images), b.encode(images)
    assert fa == fb and fa[5] == O.encode(images[5], 85, 0, sub) and fa[23] == O.encode(images[23], 85, 0, sub)
    assert fb == b.encode(on_device(images, 3), device_frames=True)
    a.close(), b.close()


def test_options_between_calls_equal_a_fresh_handle():
    images = JC.bank(2, 33, 49)
    enc = encoder((33, 49))
    first = enc.encode(images)
    for key, value, kw in (("quality", 30, dict(quality=30)), ("restart", 2, dict(quality=30, restart=2)), ("quality", 100, dict(quality=100, restart=2)),
                           ("restart", 0, dict(quality=100))):
        enc.option(key, value)
        fresh = encoder((33, 49), **kw)
        got = enc.encode(images)
        assert got == fresh.encode(images) == [O.encode(im, kw["quality"], kw.get("restart", 0), 420) for im in images], (key, value)
        assert enc.header() == fresh.header() == got[0][:O.HEADER_BYTES]
        fresh.close()
    enc.option("quality", 85)
    assert enc.encode(images) == first
    enc.close()


def test_capacity_of_an_image_and_of_the_bank():
    L = pkg("_lib")
    images = JC.bank(5)
    want = [O.encode(im, 85, 0, 420) for im in images]
    k = int(np.argmax([len(w) for w in want]))                                # the largest: one byte less room drops it alone
    assert sorted(len(w) for w in want)[-2] < len(want[k])
    enc = encoder(images.shape[1:3], max_bytes=len(want[k]) - 1)
    buf, off, status = enc.encode_packed(images)
    assert status.tolist() == [L.ERR_CAPACITY if i == k else 0 for i in range(5)] and off[k + 1] == off[k]
    assert [buf[off[i]:off[i + 1]].tobytes() for i in range(5)] == [b"" if i == k else w for i, w in enumerate(want)]
    assert enc.encode(images)[k] is None
    enc.close()
    enc = encoder(images.shape[1:3], max_bytes=len(want[k]))
    assert enc.encode(images) == want
    # the bank: one byte short, in host and in device memory -- the offsets come back, nothing is written, the canary stays
    total = sum(map(len, want))
    for out in (np.full(total + 63, 0xA5, np.uint8), torch.full((total + 63,), 0xA5, dtype=torch.uint8, device="cuda")):
        with pytest.raises(L.AicError) as ei:
            enc.encode_packed(images, out=out, out_cap=total - 1)
        assert ei.value.code == L.ERR_CAPACITY
        assert ei.value.offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and not ei.value.status.any()
        host = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        assert (host == 0xA5).all()
        _, off, status = enc.encode_packed(images, out=out, out_cap=total)   # with room: the files, and the 63 bytes behind them untouched
        host = out if isinstance(out, np.ndarray) else out.cpu().numpy()
        assert host[:total].tobytes() == b"".join(want) and (host[total:] == 0xA5).all() and off[-1] == total
    enc.close()
    # what no image can exceed: the noise case at q100 fits
    c = CASES["noise-q100-r0-444"]
    enc = encoder((16, 16), 100, 0, 444)
    assert enc.encode(c.image[None]) == [JC.expected(c.name)]
    g = pkg("jpeg").geometry((16, 16), 0, "444")
    assert enc.worst_case_bytes() == g["worst_case_bytes"] == O.worst_case_bytes(16, 16, 0, 444) and g["default_max_bytes"] == O.default_max_bytes(16, 16, 0, 444)
    enc.close()


def test_no_images_is_a_no_op():
    enc = encoder((16, 16))
    buf, off, status = enc.encode_packed(np.zeros((0, 16, 16, 3), np.uint8))
    assert off.tolist() == [0] and len(status) == 0 and enc.encode(np.zeros((0, 16, 16, 3), np.uint8)) == []
    assert enc.counters() == dict(images=0, bytes_in=0, bytes_out=0)
    enc.close()


def test_best_shot_finals_through_one_encode_call():
    B = pkg("bestshot")
    case = next(c for c in BC.CASES if c["streams"] >= 2)
    bs = B.BestShots(case["streams"], case["hw"], **case["kw"])
    results = [bs.update(frames, rows, cap=case["cap"]) for frames, rows in case["calls"]] + [bs.flush()]
    enc = encoder((bs.thumb_h, bs.thumb_w), subsampling=444, max_images=4)      # fewer than the finals of the flush: several calls, one order
    n = 0
    for res in results:
        files = B.encode_finals(res, enc)
        thumbs = [res.thumbs[s, k] for s in range(case["streams"]) for k in range(int(res.n_final[s]))]
        assert files == [O.encode(t, 85, 0, 444) for t in thumbs]
        n += len(files)
    assert n >= 5
    bs.close(), enc.close()


class _Planted:
    """The scene's own boxes in place of the seeded detector's: the frame-by-frame run then has tracks to show."""

    def __init__(self, **kw):
        self.scene, self.i = pkg("synthetic").Scene(seed=1, n_targets=6, width=640, height=360, conf_range=(0.8, 0.95)), 0

    def detect(self, frame):
        self.i += 1
        return self.scene.detections(self.i - 1)


def test_cli_best_shots_as_jpg(tmp_path, monkeypatch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    monkeypatch.setattr(cli, "YOLODetector", _Planted)
    common = ["--input", "synthetic:640x360:6:16:1", "--yolo_engine", ypath, "--tracker", "bytetrack", "--best_shot_size", "32x64", "--no_save"]
    assert cli.main(common + ["--best_shots", str(tmp_path / "ppm")]) == 0
    assert cli.main(common + ["--best_shots", str(tmp_path / "jpg"), "--best_shot_format", "jpg", "--jpeg_quality", "90"]) == 0
    ppm = sorted((tmp_path / "ppm").glob("*.ppm"))
    assert len(ppm) >= 3 and sorted(p.stem for p in ppm) == sorted(p.stem for p in (tmp_path / "jpg").glob("*.jpg")) and not list((tmp_path / "jpg").glob("*.ppm"))
    head = b"P6\n32 64\n255\n"
    for p in ppm:
        rgb = np.frombuffer(p.read_bytes()[len(head):], np.uint8).reshape(64, 32, 3)
        assert (tmp_path / "jpg" / (p.stem + ".jpg")).read_bytes() == O.encode(np.ascontiguousarray(rgb[:, :, ::-1]), 90, 0, 444), p.name
    lines = [[json.loads(l) for l in (tmp_path / d / "index.jsonl").read_text().splitlines()] for d in ("ppm", "jpg")]
    assert [dict(l, file=l["file"] and l["file"].replace(".ppm", ".jpg")) for l in lines[0]] == lines[1]


def test_cli_motion_jpeg_output(tmp_path, monkeypatch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli, J = pkg("cli"), pkg("jpeg")
    monkeypatch.setattr(cli, "probe_cv2", lambda: None)                       # the twin run writes headerless frames
    H, W, T = 112, 192, 4
    for argv, name, S in ((["--input", f"synthetic:{W}x{H}:2:{T}:1"], "one", 1),
                          (["--inputs", f"synthetic:{W}x{H}:2:{T}:1,synthetic:{W}x{H}:3:{T}:2", "--batch", "2"], "two", 2)):
        common = argv + ["--yolo_engine", ypath, "--tracker", "bytetrack", "--output_filename", "out"]
        assert cli.main(common + ["--output_dir", str(tmp_path / name / "raw")]) == 0
        assert cli.main(common + ["--output_dir", str(tmp_path / name / "mjpeg"), "--output_codec", "mjpeg", "--jpeg_quality", "70", "--jpeg_restart", "3"]) == 0
        for s in range(S):
            stem = "out" if S == 1 else f"out_s{s}"
            raw = np.fromfile(tmp_path / name / "raw" / (stem + ".bgr24"), np.uint8).reshape(-1, H, W, 3)
            data = (tmp_path / name / "mjpeg" / (stem + ".mjpeg")).read_bytes()
            meta = json.loads((tmp_path / name / "mjpeg" / (stem + ".mjpeg.json")).read_text())
            assert meta["codec"] == "mjpeg" and meta["frames"] == len(raw) == T and (meta["width"], meta["height"], meta["quality"], meta["restart"]) == (W, H, 70, 3)
            off = meta["offsets"]
            assert len(off) == T + 1 and off[0] == 0 and off[-1] == len(data)
            for f in range(T):
                one = data[off[f]:off[f + 1]]
                assert one[:O.HEADER_BYTES] == J.header((H, W), 70, 3, "420") and one[-2:] == b"\xff\xd9", (name, s, f)
                if S > 1:                                                     # (one source: the frames carry the run's measured FPS as text)
                    assert one == O.encode(raw[f], 70, 3, 420), (name, s, f)
