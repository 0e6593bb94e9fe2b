"""The CLI's output stage on the GPU: with --inputs a tick's frames go through one Renderer.render call.  Every
written BGR24 frame is held to tests/render_oracle.py applied to the source's frame with that frame's tracks from the .jsonl and the
CLI's own label and info primitives; without a new flag the frames equal visualization.draw_frame's, as before."""
import json

import numpy as np
import pytest
import torch            # noqa: F401  (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import render_oracle as RO
from conftest import ROOT, pkg

W, H, FRAMES = 1280, 720, 4                                  # the trained detector's frame size; a few frames until ByteTrack confirms
SOURCES = [(5, 1), (3, 2)]                                   # (persons, seed)
ZONES = {"cameras": [{"zones": [[[200, 100], [1080, 100], [1080, 660], [200, 660]], [[0, 0], [640, 0], [0, 720]]], "lines": [[[640, 0], [640, 720]]]}]}
MASKS = {"cameras": [{"masks": [[[1200, 0], [1280, 0], [1280, 120], [1240, 60]]]}, {"masks": [[[0, 600], [180, 660], [80, 800]], [[600, 340], [680, 340], [680, 400], [600, 400]]]}]}


def run(tmp_path, name, extra):
    cli = pkg("cli")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    out = tmp_path / name
    specs = [f"synthetic:{W}x{H}:{p}:{FRAMES}:{s}" for p, s in SOURCES]
    assert cli.main(["--inputs", ",".join(specs), "--batch", "4", "--tracker", "bytetrack", "--yolo_engine", ypath, "--output_dir", str(out)] + extra) == 0
    res = []
    for k in range(len(SOURCES)):
        raw = [p for p in out.iterdir() if p.name.endswith(f"_s{k}.bgr24")][0]
        frames = np.fromfile(raw, np.uint8).reshape(-1, H, W, 3)
        lines = [json.loads(l) for l in open([p for p in out.iterdir() if p.name.endswith(f"_s{k}.jsonl")][0])]
        assert len(frames) == len(lines) == FRAMES
        res.append((frames, [[tuple(t) for t in l["tracks"]] for l in lines]))
    return res


def info(k):
    return ["AICamera: YOLOv8 + ByteTrack", f"Input: synthetic_{W}x{H}_{SOURCES[k][0]} (stream {k})"]


@pytest.mark.gpu
def test_cli_bank_frames_equal_the_oracle(gpu, tmp_path):
    V, Z, R, syn, config = pkg("visualization"), pkg("zones"), pkg("render"), pkg("synthetic"), pkg("config")
    (tmp_path / "z.json").write_text(json.dumps(ZONES))
    (tmp_path / "m.json").write_text(json.dumps(MASKS))
    res = run(tmp_path, "new", ["--redact", "box", "--draw_zones", "--zones", str(tmp_path / "z.json"), "--masks", str(tmp_path / "m.json")])
    geometry, masks = Z.load_zones_file(ZONES, 2), R.load_masks_file(MASKS, 2)
    ids = {n: i for i, n in enumerate(config.CLASSES)}
    redacted = 0
    for k, (frames, tracks) in enumerate(res):
        sc = syn.Scene(seed=SOURCES[k][1], n_targets=SOURCES[k][0], width=W, height=H)
        for f in range(FRAMES):
            pl = V.PrimList()
            V.zone_prims(pl, *geometry[k])
            V.info_prims(V.track_prims(pl, tracks[f]), info(k))
            rows = np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks[f]], np.int64).reshape(-1, 6)
            exp = RO.render(sc.render(f)[None], rows, [len(rows)], [pl.arrays()], [k], {k: masks[k]}, 2, redact="box", style="mosaic", cell=16)[0]
            assert np.array_equal(frames[f], exp), (k, f)
            redacted += len(rows)
    assert redacted > 0, "no track in any frame: the run redacted nothing"
    # the errors follow the --zones pattern: message, pipeline closed, exit code 1
    cli = pkg("cli")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    specs = ",".join(f"synthetic:{W}x{H}:{p}:2:{s}" for p, s in SOURCES)
    for extra in (["--redact_style", "mosaic:5"], ["--masks", str(tmp_path / "missing.json")]):
        assert cli.main(["--inputs", specs, "--tracker", "bytetrack", "--yolo_engine", ypath, "--output_dir", str(tmp_path / "bad")] + extra) == 1


@pytest.mark.gpu
def test_cli_bank_frames_without_new_flags_equal_draw_frame(gpu, tmp_path):
    V, syn = pkg("visualization"), pkg("synthetic")
    res = run(tmp_path, "old", [])
    for k, (frames, tracks) in enumerate(res):
        sc = syn.Scene(seed=SOURCES[k][1], n_targets=SOURCES[k][0], width=W, height=H)
        for f in range(FRAMES):
            assert np.array_equal(frames[f], V.draw_frame(sc.render(f).copy(), tracks[f], info(k))), (k, f)


@pytest.mark.gpu
def test_cli_single_input_uses_the_renderer_when_asked(gpu, tmp_path):
    V, R, syn, config, cli = pkg("visualization"), pkg("render"), pkg("synthetic"), pkg("config"), pkg("cli")
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    (tmp_path / "m.json").write_text(json.dumps({"cameras": MASKS["cameras"][1:]}))
    out = tmp_path / "one"
    assert cli.main(["--input", f"synthetic:{W}x{H}:4:4:3", "--tracker", "ocsort", "--yolo_engine", ypath, "--output_dir", str(out), "--redact", "head",
                     "--redact_style", "fill", "--masks", str(tmp_path / "m.json")]) == 0
    frames = np.fromfile([p for p in out.iterdir() if p.name.endswith(".bgr24")][0], np.uint8).reshape(-1, H, W, 3)
    lines = [json.loads(l) for l in open([p for p in out.iterdir() if p.name.endswith(".jsonl")][0])]
    masks = R.load_masks_file({"cameras": MASKS["cameras"][1:]}, 1)
    ids = {n: i for i, n in enumerate(config.CLASSES)}
    sc = syn.Scene(seed=3, n_targets=4, width=W, height=H)
    assert len(frames) == len(lines) == 4
    for f in range(4):
        tracks = [tuple(t) for t in lines[f]["tracks"]]
        rows = np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks], np.int64).reshape(-1, 6)
        exp = RO.render(sc.render(f)[None], rows, [len(rows)], None, None, {0: masks[0]}, 1, redact="head", style="fill")[0]
        # labels and the info panel are painted over (a); the panel's FPS line is the run's clock, so they are compared outside its box
        pl = V.info_prims(V.track_prims(V.PrimList(), tracks), ["AICamera: YOLOv8 + OC-SORT", f"Input: synthetic_{W}x{H}_4", "FPS: 0.00"])
        prims, text = pl.arrays()
        fps_row = prims[-1]                                   # the last primitive is the FPS line: its rows are left out
        y0, y1 = int(fps_row[2]), int(fps_row[2]) + 7 * V.SCALE_INFO
        exp = RO.render_frame(exp, prims=prims, text=text)
        keep = np.ones(H, bool)
        keep[y0:y1] = False
        assert np.array_equal(frames[f][keep], exp[keep]), f
