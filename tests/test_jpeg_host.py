"""The JPEG stage (aic_jpeg_*) without a GPU: the symbols, the host-only calls against tests/jpeg_oracle.py byte for
byte, every rejection that comes before the device (create, option and worst_case_bytes never touch it; on a machine without a GPU an
encode that got past the checks answers AIC_ERR_NO_DEVICE), the Python class and the CLI's flags, the HIP-free half under the sanitizers
as a stand-alone program, and the kernels' budget."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_oracle as O
from conftest import ROOT, pkg

NEW = tuple(f"aic_jpeg_{f}" for f in ("tables", "header", "config_default", "create", "destroy", "option", "worst_case_bytes", "encode", "coefficients",
                                      "counters"))


def test_symbols_declared_and_exported_abi_still_2():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert lib.aic_abi_version() == 2 and "#define AIC_ABI_VERSION 2" in hdr
    assert pkg().JpegEncoder is pkg("jpeg").JpegEncoder


@pytest.mark.parametrize("hw", ((1, 1), (720, 1280), (16384, 16383)))
@pytest.mark.parametrize("sub", (420, 444))
def test_header_and_tables_equal_the_oracle(hw, sub):
    L, J = pkg("_lib"), pkg("jpeg")
    lib = L.load()
    for q in (1, 50, 100):
        for restart in (0, 5, 65535):
            assert J.header(hw, q, restart, str(sub)) == O.header(*hw, q, restart, sub), (q, restart)
        ql, qc = J.tables(q)
        assert ql.dtype == np.uint8 and np.array_equal(ql, O.tables(q)[0]) and np.array_equal(qc, O.tables(q)[1])
    out, n = np.zeros(700, np.uint8), C.c_int(-1)
    assert lib.aic_jpeg_header(hw[0], hw[1], 85, 0, sub, L.ptr(out), 628, C.byref(n)) == L.ERR_CAPACITY and n.value == 629 and not out.any()
    assert lib.aic_jpeg_header(hw[0], hw[1], 85, 0, sub, L.ptr(out), 629, C.byref(n)) == L.OK and not out[629:].any()


def test_host_calls_reject():
    L = pkg("_lib")
    lib = L.load()
    a, b, n = np.zeros(64, np.uint8), np.zeros(64, np.uint8), C.c_int()
    for q in (0, 101, -5):
        assert lib.aic_jpeg_tables(q, L.ptr(a), L.ptr(b)) == L.ERR_INVALID and b"quality" in lib.aic_last_error()
    assert lib.aic_jpeg_tables(50, None, L.ptr(b)) == L.ERR_INVALID and lib.aic_jpeg_tables(50, L.ptr(a), None) == L.ERR_INVALID
    out = np.zeros(629, np.uint8)
    for h, w, q, r, s in ((0, 8, 85, 0, 420), (16385, 8, 85, 0, 420), (8, 0, 85, 0, 420), (8, 16385, 85, 0, 420), (8, 8, 0, 0, 420), (8, 8, 101, 0, 420),
                          (8, 8, 85, -1, 420), (8, 8, 85, 65536, 420), (8, 8, 85, 0, 422), (8, 8, 85, 0, 0)):
        assert lib.aic_jpeg_header(h, w, q, r, s, L.ptr(out), 629, C.byref(n)) == L.ERR_INVALID, (h, w, q, r, s)
    assert lib.aic_jpeg_header(8, 8, 85, 0, 420, None, 629, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_jpeg_header(8, 8, 85, 0, 420, L.ptr(out), 629, None) == L.ERR_INVALID


def config(L, **kw):
    cfg = L.JpegConfig()
    assert L.load().aic_jpeg_config_default(kw.pop("height", 48), kw.pop("width", 64), C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_config_default_and_create_reject():
    L = pkg("_lib")
    lib = L.load()
    cfg = config(L, height=720, width=1280)
    assert (cfg.max_images, cfg.height, cfg.width, cfg.quality, cfg.restart, cfg.subsampling) == (16, 720, 1280, 85, 0, 420)
    assert cfg.max_bytes == 629 + 3 * 1280 * 720 + 2 * 45 + 2 == O.default_max_bytes(720, 1280)
    assert config(L, height=17, width=33).max_bytes == O.default_max_bytes(17, 33)
    assert lib.aic_jpeg_config_default(8, 8, None) == L.ERR_INVALID
    h = C.c_void_p()
    for kw in (dict(quality=0), dict(quality=101), dict(height=0), dict(height=16385), dict(width=0), dict(width=16385), dict(subsampling=422),
               dict(restart=-1), dict(restart=65536), dict(max_images=0), dict(max_images=4097), dict(max_bytes=630), dict(max_bytes=-1)):
        cfg = config(L)
        for k, v in kw.items():
            setattr(cfg, k, v)
        assert lib.aic_jpeg_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value, kw
    cfg = config(L)
    assert lib.aic_jpeg_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and lib.aic_jpeg_create(0, None, C.byref(h)) == L.ERR_INVALID
    assert lib.aic_jpeg_create(0, C.byref(cfg), None) == L.ERR_INVALID and lib.aic_jpeg_destroy(None) == L.OK


@pytest.fixture()
def handle():
    """An encoder of up to 4 images of 48 x 64: creating one touches no device, so this works on every machine."""
    L = pkg("_lib")
    h, cfg = C.c_void_p(), config(L, max_images=4)
    assert L.load().aic_jpeg_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_jpeg_destroy(h) == L.OK


def test_option_and_worst_case(handle):
    L = pkg("_lib")
    lib = L.load()
    good = {"quality": (1, 100), "restart": (0, 1, 65535), "launch_budget_mb": (1, 65536)}
    bad = {"quality": (0, 101), "restart": (-1, 65536), "launch_budget_mb": (0, 65537)}
    for key, vals in good.items():
        for v in vals:
            assert lib.aic_jpeg_option(handle, key.encode(), v) == L.OK, (key, v)
    for key, vals in bad.items():
        for v in vals:
            assert lib.aic_jpeg_option(handle, key.encode(), v) == L.ERR_INVALID and key.split("_")[0].encode() in lib.aic_last_error(), (key, v)
    assert lib.aic_jpeg_option(handle, b"nonsense", 1) == L.ERR_INVALID and b"nonsense" in lib.aic_last_error()
    assert lib.aic_jpeg_option(handle, None, 1) == L.ERR_INVALID and lib.aic_jpeg_option(None, b"quality", 1) == L.ERR_INVALID
    v = C.c_int64()
    for restart in (0, 7):
        assert lib.aic_jpeg_option(handle, b"restart", restart) == L.OK
        assert lib.aic_jpeg_worst_case_bytes(handle, C.byref(v)) == L.OK and v.value == O.worst_case_bytes(48, 64, restart, 420)
    assert lib.aic_jpeg_worst_case_bytes(handle, None) == L.ERR_INVALID and lib.aic_jpeg_worst_case_bytes(None, C.byref(v)) == L.ERR_INVALID
    c = [C.c_int64(-1) for _ in range(3)]
    assert lib.aic_jpeg_counters(handle, *(C.byref(x) for x in c)) == L.OK and [x.value for x in c] == [0, 0, 0]
    assert lib.aic_jpeg_counters(None, None, None, None) == L.ERR_INVALID and lib.aic_jpeg_counters(handle, None, None, None) == L.OK


def test_encode_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    fr, out, off, st = np.zeros((4, 48, 64, 3), np.uint8), np.zeros(1 << 16, np.uint8), np.full(6, -7, np.int64), np.zeros(5, np.int32)
    base = dict(h=handle, fr=fr, fm=L.HOST, n=4, out=out, om=L.HOST, cap=out.size, off=off, st=st)

    def rc(**kw):
        a = dict(base, **kw)
        return lib.aic_jpeg_encode(a["h"], L.ptr(a["fr"]), a["fm"], a["n"], L.ptr(a["out"]), a["om"], a["cap"], L.ptr(a["off"]), L.ptr(a["st"]))
    for kw in (dict(n=5), dict(n=-1), dict(cap=-1), dict(fr=None), dict(out=None), dict(off=None), dict(st=None), dict(fm=2), dict(fm=-1), dict(om=2), dict(h=None)):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert (off == -7).all() and not out.any()
    assert rc(n=0, fr=None, out=None, cap=0) == L.OK and off[0] == 0            # no images: nothing to do, on every machine
    coef = np.zeros((4, 12, 6, 64), np.int16)
    for kw in (dict(n=5), dict(n=-1), dict(fr=None), dict(out=None), dict(fm=3)):
        a = dict(dict(fr=fr, fm=L.HOST, n=4, out=coef), **kw)
        assert lib.aic_jpeg_coefficients(handle, L.ptr(a["fr"]), a["fm"], a["n"], L.ptr(a["out"])) == L.ERR_INVALID, kw
    assert lib.aic_jpeg_coefficients(None, L.ptr(fr), L.HOST, 4, L.ptr(coef)) == L.ERR_INVALID
    if L.device_count() == 0:                                                 # what passes the checks reaches the device
        assert rc() == L.ERR_NO_DEVICE and rc(fm=L.DEVICE, om=L.DEVICE) == L.ERR_NO_DEVICE
        assert lib.aic_jpeg_coefficients(handle, L.ptr(fr), L.HOST, 4, L.ptr(coef)) == L.ERR_NO_DEVICE


def test_python_class_rejections_need_no_device():
    J, L, B = pkg("jpeg"), pkg("_lib"), pkg("bestshot")
    for kw in (dict(subsampling="422"), dict(subsampling=411)):
        with pytest.raises(ValueError):
            J.JpegEncoder((48, 64), **kw)
    for kw in (dict(quality=0), dict(quality=101), dict(restart=-1), dict(restart=65536), dict(max_images=0), dict(max_images=4097), dict(max_bytes=1)):
        with pytest.raises(L.AicError) as ei:
            J.JpegEncoder((48, 64), **kw)
        assert ei.value.code == L.ERR_INVALID
    for hw in ((0, 64), (48, 16385)):
        with pytest.raises(L.AicError):
            J.JpegEncoder(hw)
    e = J.JpegEncoder((48, 64), max_images=2, subsampling="444", max_bytes="worst")
    assert e.header() == O.header(48, 64, 85, 0, 444) and e.worst_case_bytes() == O.worst_case_bytes(48, 64, 0, 444)
    e.option("quality", 40), e.option("restart", 5)
    assert e.header() == O.header(48, 64, 40, 5, 444)
    with pytest.raises(L.AicError):
        e.option("quality", 0)
    fr = np.zeros((2, 48, 64, 3), np.uint8)
    for bad in (fr[0], fr[:, :, :, :2], np.zeros((3, 48, 64, 3), np.uint8), np.zeros((1, 48, 65, 3), np.uint8), fr.astype(np.int32)):
        with pytest.raises(ValueError):
            e.encode(bad)
    with pytest.raises(ValueError):
        e.encode(fr, device_frames=True)                                      # host memory named device memory
    for out, cap in ((np.zeros(8, np.int32), None), (np.zeros(8, np.uint8), 9), (np.zeros((4, 4), np.uint8)[:, ::2], None)):
        with pytest.raises(ValueError):
            e.encode_packed(fr, out=out, out_cap=cap)
    assert e.encode(fr[:0]) == [] and e.counters() == dict(images=0, bytes_in=0, bytes_out=0)
    e.close(), e.close()
    g = J.geometry((720, 1280))
    assert (g["n_mcu"], g["intervals"], g["default_max_bytes"], g["worst_case_bytes"]) == (3600, 45, O.default_max_bytes(720, 1280), O.worst_case_bytes(720, 1280))
    assert callable(B.write_jpeg) and callable(B.encode_finals)


def test_cli_flags(tmp_path):
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy"])
    assert (a.best_shot_format, a.output_codec, a.jpeg_quality, a.jpeg_restart) == ("ppm", "auto", 85, 0)
    a = cli.parse_arguments(["--input", "a.npy", "--output_codec", "mjpeg"])
    assert (a.output_codec, a.jpeg_quality, a.jpeg_restart) == ("mjpeg", 85, 0)
    for tracker in ("deepsort", "bytetrack", "ocsort", "botsort"):
        a = cli.parse_arguments(["--input", "a.npy", "--tracker", tracker, "--output_codec", "mjpeg", "--jpeg_quality", "60", "--jpeg_restart", "8", "--best_shots", "d",
                                 "--best_shot_format", "jpg"])
        assert (a.best_shot_format, a.output_codec, a.jpeg_quality, a.jpeg_restart) == ("jpg", "mjpeg", 60, 8)
    a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", "bytetrack", "--best_shots", "d", "--best_shot_format", "jpg", "--jpeg_quality", "100"])
    assert (a.best_shot_format, a.output_codec, a.jpeg_quality) == ("jpg", "auto", 100)
    for bad in (["--jpeg_quality", "50"], ["--jpeg_restart", "4"], ["--best_shot_format", "jpg"], ["--best_shot_format", "png", "--best_shots", "d"],
                ["--output_codec", "h264"], ["--output_codec", "mjpeg", "--jpeg_quality", "0"], ["--output_codec", "mjpeg", "--jpeg_quality", "101"],
                ["--output_codec", "mjpeg", "--jpeg_restart", "-1"], ["--output_codec", "mjpeg", "--jpeg_restart", "65536"],
                ["--best_shots", "d", "--best_shot_format", "jpg", "--jpeg_restart", "3"], ["--output_codec", "mjpeg", "--output_pixel_format", "nv12"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + bad)
    # the Motion-JPEG writer's files, fed with files an encoder made elsewhere
    w = cli.FrameWriter(tmp_path / "clip", (64, 48, 25.0), None, None, mjpeg=dict(quality=70, restart=0, device=0))
    w.write_encoded(b"\xff\xd8one\xff\xd9"), w.write_encoded(b"\xff\xd8three\xff\xd9")
    w.close()
    assert (tmp_path / "clip.mjpeg").read_bytes() == b"\xff\xd8one\xff\xd9\xff\xd8three\xff\xd9"
    meta = __import__("json").loads((tmp_path / "clip.mjpeg.json").read_text())
    assert meta == dict(width=64, height=48, fps=25.0, codec="mjpeg", quality=70, restart=0, subsampling="420", offsets=[0, 7, 16], frames=2)


def test_host_half_under_the_sanitizers_stand_alone(tmp_path):
    """jpeg_host.cpp + tests/jpeg_host_probe.cpp with the system g++ under -fsanitize=address,undefined, run as a program of its own."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the probe builds jpeg_host.cpp with the system compiler")
    exe = str(tmp_path / "jpeg_host_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",              # the runtimes inside the program: it runs as it is, whatever the environment preloads
                    os.path.join(ROOT, "ai-camera_amd", "csrc", "jpeg_host.cpp"), os.path.join(ROOT, "tests", "jpeg_host_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("probe ok") and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_kernels_have_no_scratch_no_spills_and_a_small_lds_tile():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "jpeg_" in k and "_kernel" in k}
    assert len(tab) == 5 and sum("jpeg_transform_kernel" in k for k in tab) == 2 and sum("jpeg_entropy_kernel" in k for k in tab) == 2, sorted(tab)
    for k, r in tab.items():                                                 # 256 threads; LDS at most 64 KB so that two blocks share a CU
        assert not r["scratch"] and not r["vgpr_spills"] and r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 64 * 1024, (k, r)
