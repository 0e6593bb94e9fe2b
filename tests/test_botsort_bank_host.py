"""The BoT-SORT bank and the camera-motion bank in the C ABI without a GPU: the symbols are declared and exported, `streams` and the
parameters are checked before the device, and the Python constructor of a bank pipeline refuses a bad camera count before it builds
anything."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_botsort_bank_{f}" for f in ("create", "destroy", "option", "update", "reset", "export", "counters")) + (
    "aic_gmc_bank_create", "aic_gmc_bank_destroy", "aic_gmc_bank_reset", "aic_gmc_bank_estimate", "aic_pipeline_create_botsort_bank")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().BoTSORTBank is pkg("botsort").BoTSORTBank
    assert pkg().CameraMotionBank is pkg("gmc").CameraMotionBank
    assert issubclass(pkg("botsort").BoTSORTBank, pkg("bytetrack").TrackerBank)


def _create(streams, **kw):
    L = pkg("_lib")
    p = pkg("botsort").botsort_params(**kw)
    h = C.c_void_p()
    return L.load().aic_botsort_bank_create(0, C.byref(p), streams, C.byref(h)), h


def _create_gmc(streams, h=360, w=640, **kw):
    L = pkg("_lib")
    p = L.GmcParams(downscale=kw.get("downscale", 4), min_inliers=kw.get("min_inliers", 8))
    out = C.c_void_p()
    return L.load().aic_gmc_bank_create(0, h, w, C.byref(p), streams, C.byref(out)), out


@pytest.mark.parametrize("streams", [0, -1, 257])
def test_streams_out_of_range_rejected_before_the_device(streams):
    L = pkg("_lib")
    rc, h = _create(streams)
    assert rc == L.ERR_INVALID and not h.value
    assert b"streams" in L.load().aic_last_error()
    rc, h = _create_gmc(streams)
    assert rc == L.ERR_INVALID and not h.value
    assert b"streams" in L.load().aic_last_error()


# the cases tests/test_botsort_host.py holds aic_botsort_create to
BAD = [dict(track_high_thresh=1.5), dict(track_low_thresh=0.7, track_high_thresh=0.6), dict(proximity_thresh=0.0),
       dict(appearance_thresh=1.01), dict(feat_alpha=1.0), dict(feat_alpha=-0.1), dict(feature_dim=510), dict(feature_dim=4100),
       dict(max_tracks=513), dict(first_track_id=-1), dict(frame_rate=0)]


@pytest.mark.parametrize("kw", BAD)
def test_bad_parameters_rejected_as_the_single_tracker_rejects_them(kw):
    L = pkg("_lib")
    rc, h = _create(4, **kw)
    assert rc == L.ERR_INVALID and not h.value
    bank_msg = L.load().aic_last_error()
    p = pkg("botsort").botsort_params(**kw)
    one = C.c_void_p()
    assert L.load().aic_botsort_create(0, C.byref(p), C.byref(one)) == L.ERR_INVALID and not one.value
    assert L.load().aic_last_error() == bank_msg


@pytest.mark.parametrize("kw", [dict(downscale=3), dict(min_inliers=-1), dict(h=100, w=640), dict(h=2160, w=3840, downscale=2)])
def test_bad_gmc_parameters_rejected_before_the_device(kw):
    L = pkg("_lib")
    rc, h = _create_gmc(3, **kw)
    assert rc == L.ERR_INVALID and not h.value


def test_no_device():
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_botsort_bank.py")
    rc, h = _create(4)
    assert rc == L.ERR_NO_DEVICE and not h.value
    rc, h = _create_gmc(4)
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("botsort").BoTSORTBank(4)
    with pytest.raises(L.NoDeviceError):
        pkg("gmc").CameraMotionBank(4, 360, 640)


def test_pipeline_bank_checks_the_camera_count_first():
    TP = pkg("pipeline").TrackingPipeline
    for cameras in (0, -1, 257):
        with pytest.raises(ValueError):
            TP.botsort_bank(None, None, (720, 1280), cameras=cameras)
    with pytest.raises(ValueError):                             # batch is not a multiple of cameras
        TP.botsort_bank(None, None, (720, 1280), cameras=3, batch=8, ring_frames=12)
    with pytest.raises(ValueError):                             # nor ring_frames
        TP.botsort_bank(None, None, (720, 1280), cameras=3, batch=12, ring_frames=16)
    with pytest.raises(TypeError):
        TP.botsort_bank(None, None, (720, 1280), cameras=3, batch=12, streams=3)
    with pytest.raises(ValueError):                             # the pinned rejection: `streams` stays ByteTrack's and OC-SORT's
        TP(None, None, (720, 1280), tracker="botsort", streams=2)
