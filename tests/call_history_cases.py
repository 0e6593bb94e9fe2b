"""Call histories whose last call must return a function of its own arguments, whatever other engines on the device were handed a
moment earlier, and the child that runs them.  Plain NumPy data; no GPU is touched on import.

Frame pairs (A, B): A is seeded random texture, B is A with one 8 x 8 x 3 patch XOR 0x80 inside BOX (BIG_BOX).  The patch positions
come from a seeded generator confined to the box and from nothing else: nothing here knows which bytes of a frame the library looks
at, and nothing may.

HISTORIES: id -> list of calls on named engines; Y is a detector (test_gpu_sparse_box.small_engine, YOLOv8n on 96 x 160), R and R2 are
ReID engines (the seeded engine), all fp16 on one device, warm_up=False, fresh per history.  The LAST call of a history is the one
recorded.  History "j" is a loop over the plugin classes and is run by run_plugin_loop.

Run as a script this file is one child of tests/test_gpu_call_history.py: `python tests/call_history_cases.py OUT_DIR TAG` runs every
history in a process whose environment does or does not carry AICAM_NO_FRAME_CACHE=1 (the library reads it once per process) and saves
every recorded array as OUT_DIR/TAG_<history>_<name>.npy -- the full arrays the wrappers return."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HW, BIG_HW = (96, 160), (720, 1280)
PATCH = 8
BOX = (40, 8, 100, 88)                     # x1, y1, x2, y2: 60 wide, 80 tall; ReID resamples it to 128 x 64
BIG_BOX = (600, 250, 720, 530)             # 120 wide, 280 tall
N_PATCH, N_PATCH_BIG = 8, 2
# row 0 is the patched box; then one beside it, one the frame clips on two sides, an inverted one (no crop: valid = 0)
BOXES = np.array([BOX, (100.5, 4.2, 150.9, 95.7), (-10.0, 30.0, 38.7, 101.0), (70.0, 50.0, 60.0, 90.0)], np.float32)
BIG_BOXES = np.array([BIG_BOX, (100.5, 40.2, 260.9, 395.7), (1200.0, 600.0, 1300.0, 760.0), (700.0, 500.0, 600.0, 900.0)], np.float32)
BOXES_T = np.array([(10, 20, 80, 150), (0, 0, 96, 160), (50.5, 100.5, 120.0, 170.0), (70.0, 50.0, 60.0, 90.0)], np.float32)   # for 160 x 96
CONF, IOU, MAX_DET = 0.25, 0.6, 100
MAX_ITEMS_Y, MAX_ITEMS_R = 4, 8
J_FRAMES = 12


def pkg(name):
    return importlib.import_module("ai-camera_amd." + name)


# ------------------------------------------------------------------------------------------------------------------------ frames
def texture(seed, hw):
    return np.random.default_rng(seed).integers(0, 256, tuple(hw) + (3,), dtype=np.uint8)


def patch_positions(seed, box, n, size=PATCH):
    """n (x, y) top-left corners of size x size patches inside box, distinct, from a seeded generator and the box alone."""
    rng = np.random.default_rng(seed)
    x1, y1, x2, y2 = box
    out = []
    while len(out) < n:
        p = (int(rng.integers(x1, x2 - size + 1)), int(rng.integers(y1, y2 - size + 1)))
        if p not in out:
            out.append(p)
    return out


def patched(a, pos):
    b = a.copy()
    x, y = pos
    b[y:y + PATCH, x:x + PATCH] ^= 0x80
    return b


PATCHES = patch_positions(1001, BOX, N_PATCH)
BIG_PATCHES = patch_positions(1002, BIG_BOX, N_PATCH_BIG)

_frames = {}


def frame(name):
    """A, Ak (A with patch k), C, Ck (the 720 x 1280 pair), O0 / O1 (two other small frames), AT (A's bytes viewed as 160 x 96)."""
    if name not in _frames:
        if name == "A":
            f = texture(11, HW)
        elif name == "C":
            f = texture(12, BIG_HW)
        elif name in ("O0", "O1"):
            f = texture(13 + int(name[1]), HW)
        elif name == "AT":
            f = frame("A").reshape(HW[1], HW[0], 3)
        elif name[0] == "A":
            f = patched(frame("A"), PATCHES[int(name[1:])])
        elif name[0] == "C":
            f = patched(frame("C"), BIG_PATCHES[int(name[1:])])
        else:
            raise KeyError(name)
        f.setflags(write=False)
        _frames[name] = f
    return _frames[name]


def boxes_of(frame_name):
    return BIG_BOXES if frame_name[0] == "C" else BOXES_T if frame_name == "AT" else BOXES


# --------------------------------------------------------------------------------------------------------------------- histories
# a call: ("detect", engine, frame or [frames]) | ("embed", engine, frame) | ("close", engine); "+" behind a frame's name: a copy of it
def _histories():
    h = {}
    for k in range(N_PATCH):
        h[f"a{k}"] = [("detect", "Y", "A"), ("embed", "R", f"A{k}")]
        h[f"c{k}"] = [("embed", "R", "A"), ("detect", "Y", f"A{k}")]
    for k in range(N_PATCH_BIG):
        h[f"abig{k}"] = [("detect", "Y", "C"), ("embed", "R", f"C{k}")]
        h[f"cbig{k}"] = [("embed", "R", "C"), ("detect", "Y", f"C{k}")]
    h["b"] = [("detect", "Y", "A"), ("embed", "R", "A+")]
    h["bbig"] = [("detect", "Y", "C"), ("embed", "R", "C+")]
    h["cref"] = [("embed", "R", "A"), ("detect", "Y", "A+")]
    h["cbigref"] = [("embed", "R", "C"), ("detect", "Y", "C+")]
    h["d"] = [("detect", "Y", "A"), ("detect", "Y", "A0"), ("embed", "R", "A")]
    h["e"] = [("detect", "Y", "A"), ("close", "Y"), ("embed", "R", "A")]
    h["f"] = [("detect", "Y", "A"), ("detect", "Y", ["O0", "O1"]), ("embed", "R", "A")]
    h["g"] = [("detect", "Y", "A"), ("detect", "Y", "C"), ("embed", "R", "A")]
    h["h"] = [("detect", "Y", "A"), ("embed", "R", "A"), ("embed", "R2", "A1")]
    h["i"] = [("detect", "Y", "A"), ("embed", "R", "AT")]
    return h


HISTORIES = _histories()
EMBED_OF_A = ("b", "d", "e", "f", "g")     # histories whose recorded call is R.embed(A, BOXES): one result
# the recorded call's frame differs from the earlier call's by one patch: (history, the history that records the same call on the unpatched frame)
PATCH_CASES = tuple((f"a{k}", "b") for k in range(N_PATCH)) + tuple((f"abig{k}", "bbig") for k in range(N_PATCH_BIG)) + \
    tuple((f"c{k}", "cref") for k in range(N_PATCH)) + tuple((f"cbig{k}", "cbigref") for k in range(N_PATCH_BIG)) + (("h", "b"),)
ORACLE_CASES = tuple(f"a{k}" for k in range(N_PATCH)) + tuple(f"abig{k}" for k in range(N_PATCH_BIG)) + ("b", "bbig", "d", "h")


def recorded_call(hid):
    return HISTORIES[hid][-1]


def recorded_frame(hid):
    """The frame of a history's recorded call, and its boxes (embed)."""
    name = recorded_call(hid)[2].rstrip("+")
    return frame(name), boxes_of(name)


# ------------------------------------------------------------------------------------------------------- (j): the plugin classes
MOVER = 4                                   # a 4 x 4 mover on a static background, somewhere else inside BOX in every frame
STATIC_BOX = (100.0, 10.0, 150.0, 90.0)
MOVER_POS = patch_positions(1003, BOX, J_FRAMES + 1, MOVER)


def mover_pos(f):
    return MOVER_POS[f]


def mover_box(f):
    """The planted box of the mover at frame f: the person stands, something small on them moves."""
    return tuple(float(v) for v in BOX)


def clip():
    """J_FRAMES + 1 frames: one background, one mover of seeded texture at mover_pos(f)."""
    if "clip" not in _frames:
        bg, mv = texture(21, HW), texture(22, (MOVER, MOVER))
        out = np.repeat(bg[None], J_FRAMES + 1, 0)
        for f in range(J_FRAMES + 1):
            x, y = mover_pos(f)
            out[f, y:y + MOVER, x:x + MOVER] = mv
        out.setflags(write=False)
        _frames["clip"] = out
    return _frames["clip"]


def planted(f):
    """(boxes xyxy [2, 4], confidences, class ids) handed to DeepSORT.update at frame f: the mover's box and a static one."""
    return np.array([mover_box(f), STATIC_BOX], np.float32), np.array([0.9, 0.8], np.float32), np.zeros(2, np.int32)


# ------------------------------------------------------------------------------------------------------------------- the child
def run_history(hid, ypath, rpath):
    """-> {name: array} of the last call."""
    HipEngine = pkg("hip_engine").HipEngine
    engines, out = {}, {}

    def engine(name):
        if name not in engines:
            engines[name] = HipEngine(ypath, dtype="fp16", max_items=MAX_ITEMS_Y, warm_up=False) if name == "Y" else \
                HipEngine(rpath, dtype="fp16", max_items=MAX_ITEMS_R, warm_up=False)
        return engines[name]

    def arg(name):
        return frame(name[:-1]).copy() if name.endswith("+") else frame(name)

    try:
        for call in HISTORIES[hid]:
            out = {}
            if call[0] == "close":
                engines.pop(call[1]).close()
            elif call[0] == "detect":
                y = engine(call[1])
                f = np.stack([arg(n) for n in call[2]]) if isinstance(call[2], list) else arg(call[2])
                out["nd"], out["boxes"], out["scores"], out["labels"] = y.detect_np(f, conf=CONF, iou=IOU, max_det=MAX_DET)
                out["raw_boxes"], out["raw_ml"], out["raw_lab"] = y.read_det_np(1 if f.ndim == 3 else len(f))
            else:
                out["emb"], out["valid"] = engine(call[1]).embed_boxes_np(arg(call[2]), boxes_of(call[2].rstrip("+")))
    finally:
        for e in engines.values():
            e.close()
    return out


def run_plugin_loop(ypath, rpath):
    """History (j): detect(frames[f + 1]), then DeepSORT.update(planted boxes of f, frames[f]), the detector one frame ahead."""
    pkg("hip_engine").HipEngine._warm_up = lambda self, iterations=5: None       # warm_up=False, which the plugin classes do not pass on
    with contextlib.redirect_stdout(io.StringIO()):
        det = pkg("detector").YOLODetector(engine_path=ypath, input_shape=HW, conf_threshold=CONF, nms_threshold=IOU, dtype="fp16", max_batch=1)
        trk = pkg("deepsort_tracker").DeepSORT(reid_model_path=rpath, dtype="fp16", max_tracks=16, reid_max_batch=MAX_ITEMS_R)
    out = {}
    frames = clip()
    try:
        for f in range(J_FRAMES):
            d = det.detect(frames[f + 1])
            for name, a in zip(("boxes", "scores", "labels", "kept"), d):
                out[f"det{f}_{name}"] = np.asarray(a)
            rows = trk.update(*planted(f), frames[f])
            out[f"upd{f}_rows"] = np.array([r[:5] for r in rows], np.int64).reshape(-1, 5)
            out[f"upd{f}_conf"] = np.array([r[6] for r in rows], np.float64)
        core = trk.tracker_core
        st = core.export_arrays()
        for k, v in st.items():
            out[f"state_{k}"] = v
        for i, gl in enumerate(st["gallery_len"]):                               # FIFO order: the newest feature is the last row
            out[f"gallery{i}"] = core._gallery(i, int(gl))
    finally:
        trk.reid_model.trt_engine.close(), trk.tracker_core.close(), det.trt_engine.close()
    return out


def main(argv):
    out_dir, tag = argv[1], argv[2]
    import test_gpu_sparse_box as S
    ypath = S.small_engine(os.path.join(out_dir, "small.aicw"))
    rpath = pkg("engine_file").ensure_seeded_engines(ROOT)[1]
    for hid in list(HISTORIES) + ["j"]:
        res = run_plugin_loop(ypath, rpath) if hid == "j" else run_history(hid, ypath, rpath)
        assert res, hid
        for k, v in res.items():
            np.save(os.path.join(out_dir, f"{tag}_{hid}_{k}.npy"), np.asarray(v))


if __name__ == "__main__":
    main(sys.argv)
    sys.exit(0)
