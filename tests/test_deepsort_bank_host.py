"""The DeepSORT bank in the C ABI without a GPU: the symbols are declared and exported, `streams` and the parameters are checked before
the device, and the rejections that pin the plain DeepSORT pipeline to one stream still raise."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_deepsort_bank_{f}" for f in ("create", "destroy", "option", "update", "reset", "export", "export_gallery", "counters"))


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert pkg().DeepSORTBank is pkg("deepsort_bank").DeepSORTBank
    assert issubclass(pkg("deepsort_bank").DeepSORTBank, pkg("bytetrack").TrackerBank)


def _create(streams, **kw):
    L = pkg("_lib")
    p = pkg("deepsort_bank").deepsort_bank_params(**kw)
    h = C.c_void_p()
    return L.load().aic_deepsort_bank_create(0, C.byref(p), streams, C.byref(h)), h


@pytest.mark.parametrize("streams", [0, -1, 257])
def test_streams_out_of_range_rejected_before_the_device(streams):
    L = pkg("_lib")
    rc, h = _create(streams)
    assert rc == L.ERR_INVALID and not h.value
    assert b"streams" in L.load().aic_last_error()


@pytest.mark.parametrize("kw,word", [(dict(nn_budget=0), b"nn_budget"), (dict(max_tracks=513), b"max_tracks"),
                                     (dict(feature_dim=6), b"feature_dim")])
def test_what_the_device_association_cannot_run_is_rejected_before_the_device(kw, word):
    L = pkg("_lib")
    rc, h = _create(4, **kw)
    assert rc == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_no_device():
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_deepsort_bank.py")
    rc, h = _create(4)
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("deepsort_bank").DeepSORTBank(4)


def test_the_plain_deepsort_pipeline_and_cli_stay_one_stream():
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline(None, None, (720, 1280), tracker="deepsort", streams=2)
    with pytest.raises(SystemExit):
        pkg("cli").main(["--inputs", "a.npy,b.npy", "--tracker", "deepsort"])
