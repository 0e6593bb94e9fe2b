"""Camera-motion C ABI without a GPU: the symbols are declared and exported, the parameters are checked before the device, and the
compute entry point fails with AIC_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

NEW = ("aic_gmc_create", "aic_gmc_destroy", "aic_gmc_reset", "aic_gmc_estimate_batch", "aic_pipeline_group_warps")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    assert "typedef struct aic_gmc_params" in hdr and '"gmc"' in hdr
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
    lib = L.load()
    for name in NEW:
        getattr(lib, name)
    assert pkg().CameraMotion is pkg("gmc").CameraMotion


def test_params_struct_matches_the_header():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    body = re.search(r"typedef struct aic_gmc_params \{(.*?)\} aic_gmc_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t)\s+(\w+);", body, re.M)
    assert [(n, t) for n, t in L.GmcParams._fields_] == [(n, C.c_int32) for _, n in fields] and len(fields) == 2
    assert C.sizeof(L.GmcParams) == 8


def _create(h=360, w=640, downscale=4, min_inliers=8):
    L = pkg("_lib")
    p = L.GmcParams(downscale=downscale, min_inliers=min_inliers)
    out = C.c_void_p()
    return L.load().aic_gmc_create(0, h, w, C.byref(p), C.byref(out)), out


@pytest.mark.parametrize("kw", [dict(downscale=1), dict(downscale=3), dict(downscale=8), dict(downscale=-2), dict(min_inliers=-1),
                                dict(h=0), dict(w=-5), dict(h=127, w=640), dict(h=360, w=127), dict(h=63, w=63, downscale=2),
                                dict(h=2200, w=3900, downscale=2)])
def test_invalid_parameters_rejected_before_the_device(kw):
    L = pkg("_lib")
    rc, h = _create(**kw)
    assert rc == L.ERR_INVALID and not h.value


def test_null_arguments():
    L = pkg("_lib")
    lib = L.load()
    h, n = C.c_void_p(), C.c_int32()
    assert lib.aic_gmc_create(0, 360, 640, None, C.byref(h)) == L.ERR_INVALID
    p = L.GmcParams(4, 8)
    assert lib.aic_gmc_create(0, 360, 640, C.byref(p), None) == L.ERR_INVALID
    assert lib.aic_gmc_reset(None) == L.ERR_INVALID
    z = np.zeros((1, 360, 640, 3), np.uint8)
    assert lib.aic_gmc_estimate_batch(None, L.ptr(z), 1, L.HOST, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_pipeline_group_warps(None, None, 0, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_pipeline_option(None, b"gmc", 4) == L.ERR_INVALID
    assert lib.aic_gmc_destroy(None) == L.OK


def test_python_layer_rejects_gmc_without_botsort():
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline(None, None, (360, 640), tracker="bytetrack", gmc=4)
    with pytest.raises(SystemExit):
        pkg("cli").parse_arguments(["--input", "synthetic:640x360:2:4", "--tracker", "ocsort", "--gmc", "4"])
    assert pkg("cli").parse_arguments(["--input", "synthetic:640x360:2:4", "--tracker", "botsort", "--gmc", "2"]).gmc == 2


def test_no_device_error():
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_gmc.py")
    rc, h = _create()
    assert rc == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("gmc").CameraMotion(360, 640)
