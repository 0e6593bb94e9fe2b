"""The conv planner on launches with a pixel list (ConvArgs::pix_list, ai-camera_amd/csrc/conv_plan.cpp) on the CPU: built with the
system g++ beside a test-only probe (tests/sparse_box_probe.cpp), no hipcc, no GPU.

The four launches the sparse box branches list -- YOLOv8n's 22.box0.0 (80 x 80), 22.box0.1+.2 (80 x 80), 22.box1.1+.2 (40 x 40) and
22.box2.1+.2 (20 x 20), all 3x3 / 1 / 1, 64 -> 64 channels -- take the LDS-DMA implicit GEMM and nothing else at every launch size, with
the NT == 4 tile whose tail decodes boxes, in the K order their dense launches have; without a list the same layers keep their direct
forms at the bench's launch size, so the table says something.  fp32 engines have no list form."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-camera_amd", "csrc")
F32, F16 = 0, 1
DMA = 0
LAYERS = {"22.box0.0": (80, 80, 0), "22.box0.1+.2": (80, 80, 1), "22.box1.1+.2": (40, 40, 1), "22.box2.1+.2": (20, 20, 1)}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the planner test builds conv_plan.cpp with the system compiler")
    so = str(tmp_path_factory.mktemp("sparse_box") / "libsparsebox.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", os.path.join(CSRC, "conv_plan.cpp"),
                    os.path.join(ROOT, "tests", "sparse_box_probe.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.probe_list_plan.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
    return lib


def plan(probe, h, w, n, tail, listed, dtype=F16):
    L = np.array([h, w, n, tail, listed, dtype], np.int32)
    out = np.zeros(9, np.int64)
    rc = probe.probe_list_plan(L.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 256, out.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))
    return None if rc else dict(zip(("k_order", "form", "mt", "nt", "wm", "wn", "nstage", "tail", "list"), (int(v) for v in out)))


def test_header_constants_match():
    src = open(os.path.join(CSRC, "conv_plan.hpp")).read()
    assert "enum class ConvForm {\n    Dma," in src                     # Dma is form 0
    inc = open(os.path.join(ROOT, "include", "aicam.h")).read()
    assert "#define AIC_F32 0 " in inc and "#define AIC_F16 1 " in inc


@pytest.mark.parametrize("name", list(LAYERS))
@pytest.mark.parametrize("n", [1, 2, 8, 32, 512])
def test_listed_launch_takes_the_dma_family(probe, name, n):
    h, w, tail = LAYERS[name]
    p = plan(probe, h, w, n, tail, 1)
    assert p is not None, f"{name} n={n}: the planner refused a listed launch"
    dense = plan(probe, h, w, n, tail, 0)
    assert p["form"] == DMA and p["list"] == 1 and p["tail"] == tail, (name, n, p)
    assert p["nt"] == 4 and p["wn"] == 1, f"{name} n={n}: a wave must own all 64 channels of its pixels (the decoding tail's form): {p}"
    assert p["k_order"] == dense["k_order"], f"{name} n={n}: the list form walks K in another order than the dense launch ({p} / {dense})"
    assert dense["list"] == 0


def test_dense_launches_of_the_bench_keep_their_direct_forms(probe):
    """At 512 frames the four layers do not run on the Dma family when dense: the listed plan is a different decision, not a coincidence."""
    forms = {name: plan(probe, h, w, 512, tail, 0)["form"] for name, (h, w, tail) in LAYERS.items()}
    assert all(f != DMA for f in forms.values()), forms


def test_fp32_has_no_list_form(probe):
    assert plan(probe, 80, 80, 8, 0, 1, F32) is None
    assert plan(probe, 80, 80, 8, 0, 0, F32) is not None
