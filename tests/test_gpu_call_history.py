"""A per-call result never comes from an earlier call's frame.

Two children run every history of tests/call_history_cases.py, one after the other: one in the default environment, one under
AICAM_NO_FRAME_CACHE=1 ("never reuse a staged frame").  The variable goes into the children's environment only: a library that reads
it reads it once per process.  Since section 53 removed the reuse the library does not read it and both children run the same code;
the second child keeps the switch so that a reuse that comes back behind it is compared with no reuse again, and assertions 2 and 3
and the same-call check hold whatever the switch does.

1. The default child's recording equals the no-reuse child's byte for byte, for every history.
2. Not vacuous: in the no-reuse recording the result on a patched frame differs from the result on the unpatched one, at the patched
   box's row (ReID) or in the detector's raw tensors, in every patch case.
3. The no-reuse recording is right without any staging: the crops of the recorded call's frame from the CPU oracle, through
   reid_infer_np on a fresh engine in this process (which stages no frame), give the recorded embeddings bit for bit at valid rows.

A child that ends by a signal, runs into its time limit or reports a HIP error ends the session (pytest.exit): nothing more is started
on a device that may have faulted.  Child times measured on an MI355X are in DESIGN.md section 53; the limit is those with generous room."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import call_history_cases as H                                          # noqa: E402
import poison_scenarios as P                                            # noqa: E402
from oracle import image_oracle as I                                    # noqa: E402

pytestmark = pytest.mark.gpu

TIMEOUT_S = 60                             # seconds per child
SWITCH = "AICAM_NO_FRAME_CACHE"
HIP_ERROR_WORDS = ("AicError", "hipError", "HIP error", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")
ALL = tuple(H.HISTORIES) + ("j",)


def run_child(out_dir, tag, no_reuse):
    """One child under `timeout`.  Ends the session on a signal, a time limit or a HIP error; fails the test on any other failure."""
    env = {k: v for k, v in os.environ.items() if k != SWITCH}
    if no_reuse:
        env[SWITCH] = "1"
    t0 = time.perf_counter()
    cmd = ["timeout", "-k", "10", str(TIMEOUT_S), sys.executable, os.path.join(ROOT, "tests", "call_history_cases.py"), str(out_dir), tag]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    tail = (r.stdout[-300:] + r.stderr[-1500:])
    print(f"call-history child {tag}: {time.perf_counter() - t0:.1f} s, status {r.returncode}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or any(w in tail for w in HIP_ERROR_WORDS):
        pytest.exit(f"call-history child {tag} ended with status {r.returncode} (a signal, its {TIMEOUT_S} s limit or a HIP error); "
                    f"stopping, nothing more is started on this device:\n{tail}", returncode=1)
    assert r.returncode == 0, f"child {tag} failed:\n{tail}"
    return P.load_recording(str(out_dir), tag)


def of(rec, hid):
    pre = hid + "_"
    return {k[len(pre):]: v for k, v in rec.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def recordings(gpu, tmp_path_factory):
    assert SWITCH not in os.environ, "this process must not carry the switch: the children get it, one value each"
    d = tmp_path_factory.mktemp("call_history")
    recs = {"default": run_child(d, "default", False), "noreuse": run_child(d, "noreuse", True)}
    for tag, r in recs.items():
        for hid in ALL:
            assert of(r, hid), (tag, hid, "recorded nothing")
    return recs


@pytest.mark.parametrize("hid", ALL)
def test_default_equals_no_reuse(recordings, hid):
    f = P.compare(of(recordings["noreuse"], hid), of(recordings["default"], hid))
    assert not f, f"history {hid}: the result depends on an earlier call's frame: " + "; ".join(f"{k} {what} at {idx}" for k, what, idx in f[:8])


def _patch_differs(rec, hid, ref):
    a, b = of(rec, hid), of(rec, ref)
    if "emb" in a:
        assert a["valid"].tolist() == b["valid"].tolist() == [1, 1, 1, 0]
        return not np.array_equal(a["emb"][0], b["emb"][0])
    return not np.array_equal(a["raw_ml"], b["raw_ml"]) or not np.array_equal(a["raw_boxes"], b["raw_boxes"])


@pytest.mark.parametrize("hid,ref", H.PATCH_CASES, ids=[c[0] for c in H.PATCH_CASES])
def test_patch_changes_the_no_reuse_result(recordings, hid, ref):
    """A case that does not differ is a badly chosen patch: move the patch."""
    assert _patch_differs(recordings["noreuse"], hid, ref), (hid, ref)


@pytest.mark.parametrize("tag", ["noreuse", "default"])
def test_same_call_same_result_across_histories(recordings, tag):
    """R.embed(A, BOXES) behind five different histories, and R2.embed(A1) behind (h) and R.embed(A1) behind (a1): one result each."""
    rec = recordings[tag]
    first = of(rec, H.EMBED_OF_A[0])
    for hid in H.EMBED_OF_A[1:]:
        assert not P.compare(first, of(rec, hid)), (tag, hid)
    assert not P.compare(of(rec, "a1"), of(rec, "h")), tag
    j = of(rec, "j")
    assert all(len(j[f"upd{f}_rows"]) == 2 for f in range(H.J_FRAMES - 4, H.J_FRAMES)), "both planted tracks are confirmed and reported"
    assert j["state_gallery_len"].tolist() == [H.J_FRAMES] * 2 and j["gallery0"].shape[0] == H.J_FRAMES


@pytest.fixture(scope="module")
def staged_nothing(gpu):
    """reid_infer_np of the oracle's crops on a fresh engine in this process, per frame name: it stages no frame."""
    from importlib import import_module
    rpath = import_module("ai-camera_amd.engine_file").ensure_seeded_engines(ROOT)[1]
    eng = import_module("ai-camera_amd.hip_engine").HipEngine(rpath, dtype="fp16", max_items=H.MAX_ITEMS_R, warm_up=False)
    cache = {}

    def emb_of(hid):
        name = H.recorded_call(hid)[2].rstrip("+")
        if name not in cache:
            frame, boxes = H.recorded_frame(hid)
            crops, valid = I.crops_to_batch(frame, boxes)
            cache[name] = (eng.reid_infer_np(crops), valid)
        return cache[name]
    yield emb_of
    eng.close()


@pytest.mark.parametrize("hid", H.ORACLE_CASES)
def test_no_reuse_recording_equals_oracle_crops_through_the_engine(recordings, staged_nothing, hid):
    got = of(recordings["noreuse"], hid)
    ref, valid = staged_nothing(hid)
    assert got["valid"].tolist() == valid.tolist() == [1, 1, 1, 0]
    ok = valid.astype(bool)
    diff = np.abs(got["emb"][ok] - ref[ok]).max()
    print(f"{hid}: max |recorded - oracle crops through the engine| = {diff:.3e}")
    assert got["emb"][ok].any() and got["emb"][ok].tobytes() == ref[ok].tobytes(), (hid, diff)
