"""A cap_rows below a frame's row count on the C ABI: the one delivery routine of the tracker calls (ai-camera_amd/csrc/epoch_stage.hpp).

Every entry gets the same call twice on two fresh handles, once with cap_rows = 8 and once with cap_rows = 2, on four well-separated
detections that stay where they are, so that every tracker reports four rows per frame within the call.  The second call must report
the same TRUE counts, store the first two rows and confidences of the first call's, and leave everything else in the caller's arrays as
it found it.  The bank entries take two streams with 2 and 3 frames: a ragged stream is where a wrong frame index shows.
"""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = -77
DIM = 512
XYXY = np.array([[100, 100, 160, 220], [400, 120, 470, 260], [800, 300, 880, 480], [1100, 90, 1150, 200]], np.float32)
TLWH = np.concatenate([XYXY[:, :2], XYXY[:, 2:] - XYXY[:, :2]], 1)
CONF = np.array([0.9, 0.85, 0.8, 0.75], np.float32)
CLS = np.zeros(4, np.int32)
FEAT = np.zeros((4, DIM), np.float32)
FEAT[np.arange(4), np.arange(4) * 7] = 1.0                        # one identity per detection, orthogonal


def call_twice(update, fps):
    """update(cap, n_out, out6, out_conf) runs the call on a fresh handle.  fps: frames per stream, stream-major."""
    F, got = int(sum(fps)), {}
    for cap in (8, 2):
        n_out = np.full(F, SENTINEL, np.int32)
        out6 = np.full((F, cap, 6), SENTINEL, np.int32)
        out_conf = np.full((F, cap), SENTINEL, np.float32)
        update(cap, n_out, out6, out_conf)
        got[cap] = (n_out, out6, out_conf)
    (n8, r8, c8), (n2, r2, c2) = got[8], got[2]
    last = np.cumsum(fps) - 1
    assert (n8[last] == 4).all(), n8                              # every stream ends with its four tracks: cap_rows = 2 clips them
    assert np.array_equal(n2, n8)                                 # the true counts
    for f in range(F):
        k8, k2 = min(int(n8[f]), 8), min(int(n8[f]), 2)
        assert np.array_equal(r2[f, :k2], r8[f, :k2]) and np.array_equal(c2[f, :k2], c8[f, :k2]), f
        assert (r2[f, k2:] == SENTINEL).all() and (c2[f, k2:] == SENTINEL).all(), f
        assert (r8[f, k8:] == SENTINEL).all() and (c8[f, k8:] == SENTINEL).all(), f
        assert (r8[f, :k8] != SENTINEL).all(), f


def tiled(a, frames):
    return np.ascontiguousarray(np.concatenate([a] * frames))


def test_tracker_update_batch(gpu):
    L, k = pkg("_lib"), 3
    counts = np.full(k, 4, np.int32)
    tlwh, conf, cls, feat = tiled(TLWH, k), tiled(CONF, k), tiled(CLS, k), tiled(FEAT, k)

    def update(cap, n_out, out6, out_conf):
        t = pkg("core.tracker_core").TrackerCore(n_init=1, max_tracks=64)
        try:
            L.call("aic_tracker_update_batch", t._h, k, L.ptr(counts), L.ptr(tlwh), L.ptr(conf), L.ptr(cls), L.ptr(feat), L.HOST, None, DIM, cap,
                   L.ptr(n_out), L.ptr(out6), L.ptr(out_conf), None, None, None)
        finally:
            t.close()

    call_twice(update, [k])


BANKS = {
    "bytetrack": lambda: pkg("bytetrack").BYTETrackerBank(2, max_tracks=64),
    "ocsort": lambda: pkg("ocsort").OCSortBank(2, max_tracks=64),
    "botsort": lambda: pkg("botsort").BoTSORTBank(2, max_tracks=64, feature_dim=DIM),
    "deepsort": lambda: pkg("deepsort_bank").DeepSORTBank(2, n_init=1, max_tracks=64, feature_dim=DIM),
}


@pytest.mark.parametrize("kind", list(BANKS))
def test_bank_update(gpu, kind):
    L = pkg("_lib")
    fps = np.array([2, 3], np.int32)
    F = int(fps.sum())
    counts = np.full(F, 4, np.int32)
    boxes = tiled(TLWH if kind == "deepsort" else XYXY, F)
    conf, cls, feat = tiled(CONF, F), tiled(CLS, F), tiled(FEAT, F)
    status = np.zeros(2, np.int32)

    def update(cap, n_out, out6, out_conf):
        b = BANKS[kind]()
        try:
            head = (b._h, L.ptr(fps), L.ptr(counts), L.ptr(boxes), L.ptr(conf), L.ptr(cls))
            tail = (cap, L.ptr(n_out), L.ptr(out6), L.ptr(out_conf), L.ptr(status))
            extra = {"botsort": (L.ptr(feat), None, None), "deepsort": (L.ptr(feat), None)}.get(kind, ())
            L.call(f"aic_{kind}_bank_update", *head, *extra, *tail)
            assert not status.any(), status
        finally:
            b.close()

    call_twice(update, fps)
