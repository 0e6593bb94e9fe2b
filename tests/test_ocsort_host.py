"""OC-SORT C ABI without a GPU: the symbols are declared and exported, parameters are checked before the device, and every compute
entry point fails with AIC_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = ("aic_ocsort_create", "aic_ocsort_destroy", "aic_ocsort_option", "aic_ocsort_update_batch", "aic_ocsort_export",
       "aic_ocsort_counters", "aic_pipeline_create_ocsort")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    assert "typedef struct aic_ocsort_params" in hdr
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().OCSort is pkg("ocsort").OCSort


def test_params_struct_matches_the_header():
    """Field order and types of aic_ocsort_params as ctypes sees them."""
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    body = re.search(r"typedef struct aic_ocsort_params \{(.*?)\} aic_ocsort_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    want = [(n, C.c_double if t == "double" else C.c_int32) for t, n in fields]
    assert [(n, t) for n, t in L.OCSortParams._fields_] == want and len(want) == 9


def _create(**kw):
    L = pkg("_lib")
    p = pkg("ocsort").ocsort_params(**kw)
    h = C.c_void_p()
    return L.load().aic_ocsort_create(0, C.byref(p), C.byref(h)), h


@pytest.mark.parametrize("kw", [dict(det_thresh=0.0), dict(det_thresh=1.5), dict(iou_threshold=0.0), dict(iou_threshold=1.01),
                                dict(inertia=-0.1), dict(inertia=1.5), dict(max_age=-1), dict(min_hits=-1), dict(delta_t=0),
                                dict(delta_t=9), dict(max_tracks=513), dict(max_tracks=-1), dict(first_track_id=-3),
                                dict(use_byte=True, det_thresh=0.1), dict(use_byte=True, det_thresh=0.05)])
def test_invalid_parameters_rejected_before_the_device(kw):
    L = pkg("_lib")
    rc, h = _create(**kw)
    assert rc == L.ERR_INVALID and not h.value


def test_null_arguments():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    assert lib.aic_ocsort_create(0, None, C.byref(h)) == L.ERR_INVALID
    assert lib.aic_ocsort_option(None, b"lsap_fast", 1) == L.ERR_INVALID
    assert lib.aic_ocsort_counters(None, None, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_pipeline_create_ocsort(None, None, None, C.byref(h)) == L.ERR_INVALID


def test_no_device(monkeypatch):
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_ocsort.py")
    rc, h = _create()
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("ocsort").OCSort()
