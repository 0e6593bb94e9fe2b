"""ByteTrack C ABI without a GPU: the symbols are declared and exported, parameters are checked before the device, and every compute
entry point fails with AIC_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = ("aic_bytetrack_create", "aic_bytetrack_destroy", "aic_bytetrack_option", "aic_bytetrack_update_batch", "aic_bytetrack_export",
       "aic_bytetrack_counters", "aic_pipeline_create_bytetrack")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    assert "typedef struct aic_bytetrack_params" in hdr
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().BYTETracker is pkg("bytetrack").BYTETracker


def _create(**kw):
    L = pkg("_lib")
    p = pkg("bytetrack").bytetrack_params(**kw)
    h = C.c_void_p()
    return L.load().aic_bytetrack_create(0, C.byref(p), C.byref(h)), h


@pytest.mark.parametrize("kw", [dict(track_thresh=0.0), dict(track_thresh=1.5), dict(low_thresh=0.0), dict(match_thresh=1.01),
                                dict(low_thresh=0.5), dict(low_thresh=0.6), dict(max_tracks=513), dict(max_tracks=-1),
                                dict(track_buffer=-1), dict(frame_rate=0), dict(first_track_id=-3), dict(new_track_thresh=-0.2)])
def test_invalid_parameters_rejected_before_the_device(kw):
    L = pkg("_lib")
    rc, h = _create(**kw)
    assert rc == L.ERR_INVALID and not h.value


def test_no_device(monkeypatch):
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_bytetrack.py")
    rc, h = _create()
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("bytetrack").BYTETracker()
