"""The DeepSORT bank pipeline (aic_pipeline_create_deepsort_bank) without a GPU: the two new symbols and their
signatures, the rejections that come before any engine or device is touched, the CLI choice, and the rejections that stay pinned on
the plain DeepSORT forms.  (The third pinned one, option "streams" on a pipeline from aic_pipeline_create, needs a pipeline: it is in
tests/test_gpu_deepsort_bank_pipeline.py.)"""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NO_ENGINE = "/nonexistent/engine.aicw"                           # opening it would raise something else than what is expected here


def test_symbols_declared_with_their_signatures():
    L = pkg("_lib")
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "aicam.h")).read())
    lib = L.load()
    assert ("int aic_pipeline_create_deepsort_bank(aic_model* yolo, aic_model* reid, const aic_pipeline_params* p, int streams, "
            "aic_pipeline** out);") in hdr
    assert "int aic_pipeline_deepsort_bank(aic_pipeline* p, aic_deepsort_bank** out);" in hdr
    P, I = C.c_void_p, C.c_int
    assert L._SIGS["aic_pipeline_create_deepsort_bank"] == (I, [P, P, P, I, P])
    assert L._SIGS["aic_pipeline_deepsort_bank"] == (I, [P, P])
    for name in ("aic_pipeline_create_deepsort_bank", "aic_pipeline_deepsort_bank"):
        assert name in L.EXPORTS
        getattr(lib, name)


def test_null_arguments_are_invalid():
    L = pkg("_lib")
    lib = L.load()
    lo, hi = pkg("config").track_class_mask()
    tp = L.TrackerParams(0.2, 0.7, 100, 70, 3, 64, 0, 1)
    prm = L.PipelineParams(720, 1280, 12, 12, 16, 0.1, 0.5, 300, 0.0, 1, (C.c_uint64 * 2)(lo, hi), tp)
    h = C.c_void_p()
    assert lib.aic_pipeline_create_deepsort_bank(None, None, C.byref(prm), 3, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_pipeline_create_deepsort_bank(None, None, None, 3, None) == L.ERR_INVALID
    assert lib.aic_pipeline_deepsort_bank(None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_pipeline_deepsort_bank(None, None) == L.ERR_INVALID


@pytest.mark.parametrize("kw,exc", [(dict(cameras=0), ValueError), (dict(cameras=257), ValueError), (dict(cameras=-3), ValueError),
                                    (dict(cameras=3, batch=8), ValueError), (dict(cameras=3, batch=12, ring_frames=16), ValueError),
                                    (dict(cameras=3, batch=12, tracker="deepsort"), TypeError),
                                    (dict(cameras=3, batch=12, streams=3), TypeError)])
def test_classmethod_rejects_before_any_engine_is_opened(kw, exc):
    TP = pkg("pipeline").TrackingPipeline
    with pytest.raises(exc):
        TP.deepsort_bank(NO_ENGINE, NO_ENGINE, (720, 1280), **kw)


def test_python_forms_need_the_bank_pipeline():
    TP = pkg("pipeline").TrackingPipeline
    single = type("P", (), dict(tracker_kind="deepsort", cameras=0, xcam=None, _bank=None))()
    with pytest.raises(ValueError):
        TP.link_cameras(single)
    with pytest.raises(ValueError):
        TP.bank.fget(single)
    with pytest.raises(ValueError):
        TP.bank.fget(type("P", (), dict(tracker_kind="botsort", cameras=3, xcam=None, _bank=None))())


def test_cli_choice():
    cli = pkg("cli")
    a = cli.parse_arguments(["--inputs", "a,b", "--tracker", "deepsort_bank", "--link_cameras"])
    assert a.tracker == "deepsort_bank" and a.inputs == "a,b" and a.link_cameras and a.input is None
    assert not cli.parse_arguments(["--inputs", "a,b", "--tracker", "deepsort_bank"]).link_cameras
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--tracker", "deepsort_bank", "--input", "x"])
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--tracker", "deepsort_bank"])
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--tracker", "deepsort_bank", "--inputs", "a,b", "--gmc", "4"])


def test_pinned_rejections_of_the_plain_deepsort_forms_hold():
    TP = pkg("pipeline").TrackingPipeline
    cli = pkg("cli")
    with pytest.raises(ValueError):
        TP(NO_ENGINE, NO_ENGINE, (720, 1280), batch=12, ring_frames=12, tracker="deepsort", streams=3)
    with pytest.raises(ValueError):
        TP(NO_ENGINE, NO_ENGINE, (720, 1280), batch=12, ring_frames=12, streams=2)
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--inputs", "a,b,c", "--tracker", "deepsort"])
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--inputs", "a,b,c"])                # --tracker deepsort is the default and keeps its meaning
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--inputs", "a,b", "--tracker", "deepsort", "--link_cameras"])
    assert cli.parse_arguments(["--input", "x", "--tracker", "deepsort"]).tracker == "deepsort"
