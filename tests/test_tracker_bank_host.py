"""Tracker banks (ByteTrack, OC-SORT) in the C ABI without a GPU: the symbols are declared and exported, `streams` and the parameters
are checked before the device, and create fails with AIC_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_{t}_bank_{f}" for t in ("bytetrack", "ocsort") for f in ("create", "destroy", "option", "update", "reset", "export",
                                                                         "counters")) + ("aic_pipeline_reset_stream",)


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
    assert pkg().BYTETrackerBank is pkg("bytetrack").BYTETrackerBank
    assert pkg().OCSortBank is pkg("ocsort").OCSortBank


def _create(kind, streams, **kw):
    L = pkg("_lib")
    p = pkg("bytetrack").bytetrack_params(**kw) if kind == "bytetrack" else pkg("ocsort").ocsort_params(**kw)
    h = C.c_void_p()
    return getattr(L.load(), f"aic_{kind}_bank_create")(0, C.byref(p), streams, C.byref(h)), h


@pytest.mark.parametrize("kind", ["bytetrack", "ocsort"])
@pytest.mark.parametrize("streams", [0, -1, 257])
def test_streams_out_of_range_rejected_before_the_device(kind, streams):
    L = pkg("_lib")
    rc, h = _create(kind, streams)
    assert rc == L.ERR_INVALID and not h.value


@pytest.mark.parametrize("kind,kw", [("bytetrack", dict(track_thresh=1.5)), ("ocsort", dict(iou_threshold=0.0))])
def test_invalid_threshold_rejected_before_the_device(kind, kw):
    L = pkg("_lib")
    rc, h = _create(kind, 4, **kw)
    assert rc == L.ERR_INVALID and not h.value


@pytest.mark.parametrize("kind", ["bytetrack", "ocsort"])
def test_no_device(kind):
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_tracker_bank.py")
    rc, h = _create(kind, 4)
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        (pkg("bytetrack").BYTETrackerBank if kind == "bytetrack" else pkg("ocsort").OCSortBank)(4)


def test_pipeline_streams_needs_a_bank_tracker():
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline(None, None, (720, 1280), tracker="deepsort", streams=2)
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline(None, None, (720, 1280), tracker="botsort", streams=2)
