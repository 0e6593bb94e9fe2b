"""Row bands on the GPU: the detector run on frames whose letterbox borders are already in its activation buffers launches only the
tile rows that can depend on the frame (csrc/row_band.hpp, Model::run_frames) -- and computes the bits of the full maps.

The reference is the same engine file in a child process with AICAM_NO_ROW_BAND=1 (the switch is read once per process): every launch
computes its full map there.  Every comparison is array_equal.  32 frames per call: the smallest batch at which the six window forms
(fused stem, 16-channel 3x3, fused C2f, stride-2 3x3 with tail, 3x3 patch, streaming 1x1) all engage.

Run as a script this file is that child: `python tests/test_gpu_row_band.py <scenario> <out dir>`.
"""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N = 32
CONF = 0.02            # low: the seeded detector on noise keeps a few boxes per frame, so the final outputs say something
WIDE, FOUR3 = (360, 640), (480, 640)      # 16:9 (picture in rows 140 .. 499), 4:3 (80 .. 559); as wide as the input: no borders left / right
N_OPS = 14             # ops 0 - 13: the stem .. 5.conv


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


def frames(seed, n, hw):
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def engine_ops(path):
    return pkg("engine_file").read_engine(path).ops


def early_buffers(path):
    return sorted({int(o[4]) for o in engine_ops(path)[:N_OPS]})


def det(eng, f):
    nd, boxes, scores, labels = eng.detect_np(f, conf=CONF)
    return {"nd": nd, "boxes": boxes, "scores": scores, "labels": labels}


def flags(eng, hw):
    return [eng.row_band(op, hw[0], hw[1]) for op in range(N_OPS)]


# ---- the scenarios: each returns ({name: array}, [per call: the engine's answers about ops 0 - 13])
def scenario_populate(ypath):
    eng = pkg("hip_engine").HipEngine(ypath, dtype="fp16", max_items=N, warm_up=False)
    out, fl = {}, []
    det(eng, frames(1, N, WIDE))                                   # A: full maps, leaves the borders' rows in place
    fl.append(flags(eng, WIDE))
    for k, v in det(eng, frames(2, N, WIDE)).items():              # B: other frames
        out["B_" + k] = v
    fl.append(flags(eng, WIDE))
    for b in early_buffers(ypath):
        out[f"B_buf{b}"] = eng.read_buffer_np(b, N)
    eng.close()
    return out, fl


def scenario_geometry(ypath):
    eng = pkg("hip_engine").HipEngine(ypath, dtype="fp16", max_items=N, warm_up=False)
    out, fl = {}, []
    for i, hw in enumerate((WIDE, FOUR3, WIDE, WIDE, FOUR3)):
        for k, v in det(eng, frames(10 + i, N, hw)).items():
            out[f"c{i}_{k}"] = v
        fl.append(flags(eng, hw))
    eng.close()
    return out, fl


def scenario_slots(ypath):
    eng = pkg("hip_engine").HipEngine(ypath, dtype="fp16", max_items=N, warm_up=False)
    out, fl = {}, []
    for i, n in enumerate((8, N, N)):
        for k, v in det(eng, frames(20 + i, n, WIDE)).items():
            out[f"c{i}_{k}"] = v
        fl.append(flags(eng, WIDE))
    eng.close()
    return out, fl


def scenario_raw_run(ypath):
    eng = pkg("hip_engine").HipEngine(ypath, dtype="fp16", max_items=N, warm_up=False)
    out, fl = {}, []
    for k, v in det(eng, frames(30, N, WIDE)).items():
        out["c0_" + k] = v
    fl.append(flags(eng, WIDE))
    x = np.random.default_rng(31).uniform(0, 1, (4, 3, 640, 640)).astype(np.float32)
    out["raw_dfl"], out["raw_cls"] = eng.yolo_head_np(x)           # Model::run on a raw input tensor: writes every map of slots 0 - 3
    fl.append(flags(eng, WIDE))
    for i in (1, 2):
        for k, v in det(eng, frames(31 + i, N, WIDE)).items():
            out[f"c{i}_{k}"] = v
        fl.append(flags(eng, WIDE))
    eng.close()
    return out, fl


def scenario_pipeline(ypath, rpath):
    """-> the rows of two runs over the same 64 frames in groups of 32: the pipeline as it comes (the last group tapered to 16 + 16 frames,
    odd groups on the second lane's engine), and with the taper and the second lane off -- two 32-frame groups on ONE engine, the second
    of which can run windows; then the first engine's answers about ops 0 - 13."""
    syn = pkg("synthetic")
    n = 64
    sc = syn.Scene(seed=9, n_targets=6)
    fr = sc.render_batch(0, n)
    dets = [sc.detections(f)[:3] for f in range(n)]
    out, fl = {}, []
    for name, opts in (("default", {}), ("one_lane", {"taper": 0, "dual_lane_frames": 0})):
        pipe = pkg("pipeline").TrackingPipeline(ypath, rpath, (720, 1280), batch=N, ring_frames=n, max_persons=8, dtype="fp16", inject=True)
        for k, v in opts.items():
            pipe.option(k, v)
        pipe.upload(0, fr)
        pipe.inject(0, dets)
        tracks, nd = pipe.run(0, n)
        out[name + "_rows"] = np.array([[f] + [float(v) for v in t[:5]] for f in range(n) for t in tracks[f]], np.float64).reshape(-1, 6)
        out[name + "_per_frame"] = np.array([len(t) for t in tracks])
        out[name + "_nd"] = np.asarray(nd)
        fl.append([pipe.yolo.row_band(op, 720, 1280) for op in range(N_OPS)])
    return out, fl


SCENARIOS = {"populate": scenario_populate, "geometry": scenario_geometry, "slots": scenario_slots, "raw_run": scenario_raw_run}


def _engine_paths():
    return pkg("engine_file").ensure_seeded_engines(ROOT)


def main(argv):
    assert os.environ.get("AICAM_NO_ROW_BAND") == "1"
    ypath, rpath = _engine_paths()
    out_dir = argv[2]
    names = list(SCENARIOS) if argv[1] == "engine" else [argv[1]]
    for name in names:
        out, _ = scenario_pipeline(ypath, rpath) if name == "pipeline" else SCENARIOS[name](ypath)
        for k, v in out.items():
            np.save(os.path.join(out_dir, f"{name}_{k}.npy"), v)


if __name__ == "__main__":
    main(sys.argv)
    sys.exit(0)


# ---------------------------------------------------------------------------------------------------------------------------------
def _child(what, out_dir):
    env = dict(os.environ, AICAM_NO_ROW_BAND="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-300:], r.stderr[-600:])
    assert r.returncode == 0
    return str(out_dir)


@pytest.fixture(scope="module")
def reference(gpu, engines, tmp_path_factory):
    """The four engine scenarios with the row bands switched off, computed once by one child process."""
    assert "AICAM_NO_ROW_BAND" not in os.environ, "this process has to run WITH the row bands"
    return _child("engine", tmp_path_factory.mktemp("row_band_ref"))


def assert_equal_to_reference(ref_dir, name, out):
    for k, v in out.items():
        ref = np.load(os.path.join(ref_dir, f"{name}_{k}.npy"))
        assert ref.shape == v.shape and ref.dtype == v.dtype, (name, k)
        assert np.array_equal(ref, v), (name, k, int((ref != v).sum()))


def windowed(fl):
    return [f["windowed"] for f in fl]


def test_second_call_runs_windows_and_leaves_the_same_bits(gpu, engines, reference):
    """A populates; B runs ops 0 - 12 on row windows (5.conv, on the ping-pong kernel, has none).  Every buffer of ops 0 - 13 and the
    detections of B equal the full-map engine's."""
    out, (fa, fb) = scenario_populate(engines[0])
    assert not any(windowed(fa)) and all(f["slots"] == N for f in fa)
    assert windowed(fb) == [True] * 13 + [False], windowed(fb)
    assert [(f["lo"], f["hi"]) for f in fb] == [(70, 250), (35, 125), (35, 125), (34, 126), (33, 127), (33, 127), (16, 64), (16, 64), (15, 65),
                                                (14, 66), (13, 67), (12, 68), (12, 68), (6, 34)]
    for f in fb[:13]:                                              # a window holds its op's band and leaves rows of the map out
        assert f["win_y0"] <= f["lo"] and f["hi"] < f["win_y0"] + f["win_rows"] < f["rows"] + f["win_y0"], f
    assert_equal_to_reference(reference, "populate", out)
    assert out["B_nd"].sum() > 0
    written = [b for b in early_buffers(engines[0]) if out[f"B_buf{b}"].any()]
    assert len(written) >= 6                                       # (the fused forms never write their intermediates)
    for b in written:
        assert np.isfinite(out[f"B_buf{b}"]).all() and out[f"B_buf{b}"].astype(np.float32).std() > 1e-3


def test_a_change_of_geometry_runs_full_once(gpu, engines, reference):
    out, fl = scenario_geometry(engines[0])
    #                 16:9   4:3    16:9   16:9  4:3
    assert [any(windowed(f)) for f in fl] == [False, False, False, True, False]
    assert windowed(fl[3])[:13] == [True] * 13
    assert_equal_to_reference(reference, "geometry", out)


def test_item_slots_never_populated_run_full(gpu, engines, reference):
    out, fl = scenario_slots(engines[0])
    assert [f[0]["slots"] for f in fl] == [8, N, N]                # (8 frames populate too: the stem has its window at every launch size)
    assert [any(windowed(f)) for f in fl] == [False, False, True]
    assert_equal_to_reference(reference, "slots", out)


def test_a_run_on_a_raw_tensor_invalidates(gpu, engines, reference):
    out, fl = scenario_raw_run(engines[0])
    assert fl[1][0]["slots"] == 0                                  # behind Model::run nothing is known
    assert [any(windowed(f)) for f in fl] == [False, False, False, True]
    assert_equal_to_reference(reference, "raw_run", out)


def test_pipeline_rows_equal_the_switched_off_run(gpu, engines, tmp_path):
    """TrackingPipeline, injected detections, 64 frames in groups of 32: the track rows and the detector's counts equal those of a
    child with AICAM_NO_ROW_BAND=1 -- as the pipeline comes, and with the taper and the second lane off, where the second 32-frame
    group runs on the engine the first one populated: its ops 0 - 12 ran on windows."""
    assert "AICAM_NO_ROW_BAND" not in os.environ
    out, (fl_default, fl_one) = scenario_pipeline(*engines)
    assert windowed(fl_one) == [True] * 13 + [False], windowed(fl_one)
    assert fl_one[0]["slots"] == N
    ref = _child("pipeline", tmp_path)
    assert_equal_to_reference(ref, "pipeline", out)
    assert len(out["default_rows"]) > 0 and len(out["one_lane_rows"]) > 0
