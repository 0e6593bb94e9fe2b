"""BoT-SORT C ABI without a GPU: the symbols are declared and exported, parameters are checked before the device, and every compute
entry point fails with AIC_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = ("aic_botsort_create", "aic_botsort_destroy", "aic_botsort_option", "aic_botsort_update_batch", "aic_botsort_export",
       "aic_botsort_counters", "aic_pipeline_create_botsort")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    assert "typedef struct aic_botsort_params" in hdr
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().BoTSORT is pkg("botsort").BoTSORT


def test_params_struct_matches_the_header():
    """Field order and types of aic_botsort_params as ctypes sees them, and upstream's defaults."""
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    body = re.search(r"typedef struct aic_botsort_params \{(.*?)\} aic_botsort_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    want = [(n, C.c_double if t == "double" else C.c_int32) for t, n in fields]
    assert [(n, t) for n, t in L.BoTSORTParams._fields_] == want and len(want) == 14
    p = pkg("botsort").botsort_params()
    assert (p.track_high_thresh, p.track_low_thresh, p.new_track_thresh, p.match_thresh) == (0.6, 0.1, 0.7, 0.8)
    assert (p.proximity_thresh, p.appearance_thresh, p.feat_alpha) == (0.5, 0.25, 0.9)
    assert (p.track_buffer, p.frame_rate, p.fuse_score, p.with_reid, p.feature_dim, p.max_tracks, p.first_track_id) == (30, 30, 1, 1, 512, 512, 1)


def _create(**kw):
    L = pkg("_lib")
    p = pkg("botsort").botsort_params(**kw)
    h = C.c_void_p()
    return L.load().aic_botsort_create(0, C.byref(p), C.byref(h)), h


@pytest.mark.parametrize("kw", [dict(track_high_thresh=0.0), dict(track_high_thresh=1.5), dict(track_low_thresh=0.0),
                                dict(track_low_thresh=0.6), dict(track_low_thresh=0.7), dict(new_track_thresh=0.0),
                                dict(new_track_thresh=1.1), dict(match_thresh=0.0), dict(match_thresh=1.01),
                                dict(proximity_thresh=0.0), dict(proximity_thresh=1.5), dict(appearance_thresh=0.0),
                                dict(appearance_thresh=2.0), dict(feat_alpha=-0.1), dict(feat_alpha=1.0), dict(track_buffer=-1),
                                dict(frame_rate=0), dict(feature_dim=510), dict(feature_dim=-4), dict(feature_dim=4100),
                                dict(max_tracks=513), dict(max_tracks=-1), dict(first_track_id=-3)])
def test_invalid_parameters_rejected_before_the_device(kw):
    L = pkg("_lib")
    rc, h = _create(**kw)
    assert rc == L.ERR_INVALID and not h.value


def test_null_arguments():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    assert lib.aic_botsort_create(0, None, C.byref(h)) == L.ERR_INVALID
    assert lib.aic_botsort_option(None, b"lsap_fast", 1) == L.ERR_INVALID
    assert lib.aic_botsort_counters(None, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_pipeline_create_botsort(None, None, None, None, C.byref(h)) == L.ERR_INVALID
    assert lib.aic_botsort_update_batch(None, 0, *([None] * 7), 0, None, None, None) == L.ERR_INVALID
    assert lib.aic_botsort_export(None, 0, *([None] * 13)) == L.ERR_INVALID


def test_no_device(monkeypatch):
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_botsort.py")
    rc, h = _create()
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("botsort").BoTSORT()
