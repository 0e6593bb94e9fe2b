"""The pixel-format conversions (aic_yuv_coeffs, aic_frames_to_bgr, aic_frames_from_bgr, aic_pipeline_read_frames)
without a GPU: the symbols, the coefficient tables against tests/yuv_oracle.py, every rejection that comes before the device, the loud
failure of a valid call on a machine without one, the kernels' budget and the CLI's raw: sources in NV12 / I420."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import yuv_oracle as Y
from conftest import ROOT, pkg

NEW = ("aic_yuv_coeffs", "aic_frames_to_bgr", "aic_frames_from_bgr", "aic_pipeline_read_frames")


def test_symbols_declared_and_exported_abi_still_2():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert lib.aic_abi_version() == 2 and "#define AIC_ABI_VERSION 2" in hdr
    for name, value in (("AIC_PIX_BGR24", 0), ("AIC_PIX_NV12", 1), ("AIC_PIX_I420", 2), ("AIC_YUV_BT601", 0), ("AIC_YUV_BT709", 1),
                        ("AIC_YUV_LIMITED", 0), ("AIC_YUV_FULL", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), hdr), name
    assert (L.PIX_BGR24, L.PIX_NV12, L.PIX_I420) == (Y.BGR24, Y.NV12, Y.I420)
    assert pkg().frames is pkg("frames")


def test_coeffs_equal_the_oracle():
    L, F = pkg("_lib"), pkg("frames")
    lib = L.load()
    for (m, mn) in ((Y.BT601, "bt601"), (Y.BT709, "bt709")):
        for (r, rn) in ((Y.LIMITED, "limited"), (Y.FULL, "full")):
            dec, enc, yo = F.coeffs(mn, rn)
            assert (dec.tolist(), enc.tolist(), yo) == tuple(Y.coeffs(m, r)), (mn, rn)
            assert dec.dtype == enc.dtype == np.int32
    dec, enc, yo = np.zeros(5, np.int32), np.zeros(9, np.int32), C.c_int32()
    for m, r in ((-1, 0), (2, 0), (0, -1), (0, 2)):
        assert lib.aic_yuv_coeffs(m, r, L.ptr(dec), L.ptr(enc), C.byref(yo)) == L.ERR_INVALID, (m, r)
    assert lib.aic_yuv_coeffs(0, 0, None, L.ptr(enc), C.byref(yo)) == L.ERR_INVALID
    assert lib.aic_yuv_coeffs(0, 0, L.ptr(dec), None, C.byref(yo)) == L.ERR_INVALID
    assert lib.aic_yuv_coeffs(0, 0, L.ptr(dec), L.ptr(enc), None) == L.ERR_INVALID
    for bad in ("bt2020", 2, None):
        with pytest.raises((ValueError, TypeError)):
            F.coeffs(bad)
    assert (F.frame_bytes("bgr24", 720, 1280), F.frame_bytes("nv12", 720, 1280), F.frame_bytes("i420", 720, 1280)) == (2764800, 1382400, 1382400)


@pytest.mark.parametrize("fn", ("aic_frames_to_bgr", "aic_frames_from_bgr"))
def test_rejects_before_the_device(fn):
    L = pkg("_lib")
    lib = L.load()
    h, w = 4, 8
    a, b = np.zeros(1 << 12, np.uint8), np.zeros(1 << 12, np.uint8)
    base = dict(dev=0, src=a, n=2, h=h, w=w, fmt=Y.NV12, pitch=0, fs=0, m=0, r=0, mem=L.HOST, dst=b)

    def rc(**kw):
        k = dict(base, **kw)
        return getattr(lib, fn)(k["dev"], L.ptr(k["src"]), k["n"], k["h"], k["w"], k["fmt"], k["pitch"], k["fs"], k["m"], k["r"], k["mem"], L.ptr(k["dst"]))
    for kw in (dict(h=3), dict(w=7), dict(h=5, w=7), dict(h=0), dict(w=0), dict(h=-2), dict(h=16386), dict(w=16386), dict(pitch=6), dict(pitch=-8),
               dict(fmt=Y.I420, pitch=9), dict(fs=47), dict(pitch=16, fs=95), dict(fs=-48), dict(fmt=Y.BGR24), dict(fmt=3), dict(fmt=-1), dict(m=2),
               dict(m=-1), dict(r=2), dict(r=-1), dict(mem=2), dict(mem=-1), dict(src=None), dict(dst=None), dict(n=-1), dict(dev=-1)):
        assert rc(**kw) == L.ERR_INVALID and lib.aic_last_error(), kw
    assert b"16384" in (rc(h=16386), lib.aic_last_error())[1] and b"even" in (rc(w=7), lib.aic_last_error())[1]
    assert b"pitch" in (rc(pitch=6), lib.aic_last_error())[1] and b"frame_stride" in (rc(fs=47), lib.aic_last_error())[1]
    # the same checks stand in front of device memory
    for kw in (dict(h=3), dict(fmt=Y.BGR24), dict(pitch=6), dict(fs=47)):
        assert rc(mem=L.DEVICE, **kw) == L.ERR_INVALID, kw
    # no frames: nothing to do, on every machine, whatever the pointers
    assert rc(n=0) == L.OK and rc(n=0, src=None, dst=None) == L.OK and rc(n=0, mem=L.DEVICE) == L.OK
    assert rc(n=0, h=3) == L.ERR_INVALID                                     # (a bad layout is still a bad layout)
    # legal layouts get past the checks: an odd NV12 pitch, the exact frame_stride, the largest sides
    if L.device_count() == 0:
        for kw in (dict(), dict(pitch=9), dict(fmt=Y.I420, pitch=10), dict(fs=48), dict(pitch=16, fs=96), dict(m=1, r=1)):
            assert rc(**kw) == L.ERR_NO_DEVICE, kw


def test_a_valid_call_without_a_gpu_fails_loudly():
    """No CPU path behind the conversions: the Python wrappers raise NoDeviceError, nothing is converted on the host."""
    L, F = pkg("_lib"), pkg("frames")
    if L.device_count() > 0:
        pytest.skip("GPU present")
    yuv = np.zeros((1, 6, 8), np.uint8)
    with pytest.raises(L.NoDeviceError):
        F.to_bgr(yuv, "nv12")
    with pytest.raises(L.NoDeviceError):
        F.from_bgr(np.zeros((1, 4, 8, 3), np.uint8), "i420", matrix="bt709", range="full")


def test_python_wrappers_reject_without_a_device():
    L, F = pkg("_lib"), pkg("frames")
    for bad in (np.zeros((1, 7, 8), np.uint8), np.zeros((6, 8, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            F.to_bgr(bad, "nv12")
    with pytest.raises(ValueError):
        F.to_bgr(np.zeros(100, np.uint8), "nv12", hw=(4, 8))                  # 100 bytes are no whole number of 48-byte frames
    with pytest.raises(ValueError):
        F.to_bgr(np.zeros((1, 6, 8), np.uint8), "yuyv")
    with pytest.raises(ValueError):
        F.from_bgr(np.zeros((1, 4, 8), np.uint8)[..., None], "nv12")
    with pytest.raises(ValueError):
        F.from_bgr(np.zeros((1, 4, 8, 3), np.uint8), "nv12", pitch=16, out=np.zeros(10, np.uint8))
    for call in (lambda: F.to_bgr(np.zeros((1, 9, 6), np.uint8), "bgr24"), lambda: F.to_bgr(np.zeros(27, np.uint8), "nv12", hw=(3, 6)),
                 lambda: F.from_bgr(np.zeros((1, 3, 6, 3), np.uint8), "nv12"), lambda: F.from_bgr(np.zeros((1, 4, 6, 3), np.uint8), "i420", pitch=7)):
        with pytest.raises(L.AicError) as ei:
            call()
        assert ei.value.code == L.ERR_INVALID
    assert F.to_bgr(np.zeros((0, 6, 8), np.uint8), "nv12").shape == (0, 4, 8, 3)
    assert F.from_bgr(np.zeros((0, 4, 8, 3), np.uint8), "i420").shape == (0, 6, 8)


def test_read_frames_rejects_null():
    L = pkg("_lib")
    out = np.zeros(16, np.uint8)
    assert L.load().aic_pipeline_read_frames(None, 0, 1, L.ptr(out)) == L.ERR_INVALID


def test_cli_raw_sources_in_yuv(tmp_path):
    cli = pkg("cli")
    rng = np.random.default_rng(5)
    w, h, t = 16, 6, 3
    data = rng.integers(0, 256, t * h * w * 3 // 2, dtype=np.uint8)
    path = tmp_path / "clip.nv12"
    data.tofile(path)
    for fmt in ("nv12", "i420"):
        arr = cli.raw_frames(str(path), w, h, fmt)
        assert arr.shape == (t, h * 3 // 2, w) and np.array_equal(np.asarray(arr).reshape(-1), data)
        name, frames, size = cli.frame_source(f"raw:{w}x{h}:{path}", pixel_format=fmt)
        frames = list(frames)
        assert name == "clip" and size[:2] == (w, h) and len(frames) == t
        assert all(f.shape == (h * 3 // 2, w) and f.flags["C_CONTIGUOUS"] for f in frames) and np.array_equal(frames[2], arr[2])
    # the same bytes as BGR24: 432 bytes hold one 16x6 frame and a partial one, which is ignored as before
    assert cli.raw_frames(str(path), w, h).shape == (1, h, w, 3)
    short = tmp_path / "short.nv12"
    data[:-5].tofile(short)
    for p, ww, hh in ((short, w, h), (path, w + 1, h), (path, w, h + 1), (path, 10, 6)):      # a partial frame; odd sizes; 432 / 90 frames
        with pytest.raises(SystemExit):
            cli.raw_frames(str(p), ww, hh, "nv12")
    (tmp_path / "empty.nv12").write_bytes(b"")
    with pytest.raises(SystemExit):
        cli.raw_frames(str(tmp_path / "empty.nv12"), w, h, "i420")
    a = cli.parse_arguments(["--input", f"raw:{w}x{h}:{path}"])
    assert (a.pixel_format, a.yuv_matrix, a.yuv_range, a.output_pixel_format) == ("bgr24", "bt601", "limited", "bgr24")
    a = cli.parse_arguments(["--input", f"raw:{w}x{h}:{path}", "--pixel_format", "nv12", "--yuv_matrix", "bt709", "--yuv_range", "full",
                             "--output_pixel_format", "nv12", "--batch", "4"])
    assert (a.pixel_format, a.yuv_matrix, a.yuv_range, a.output_pixel_format) == ("nv12", "bt709", "full", "nv12")
    a = cli.parse_arguments(["--inputs", f"raw:{w}x{h}:{path},raw:{w}x{h}:{path}", "--tracker", "bytetrack", "--pixel_format", "i420"])
    assert a.pixel_format == "i420"
    for bad in (["--input", "a.npy", "--pixel_format", "nv12"], ["--pixel_format", "nv12"], ["--input", "synthetic:64x64:1:2", "--pixel_format", "i420"],
                ["--inputs", f"raw:{w}x{h}:{path},a.npy", "--tracker", "bytetrack", "--pixel_format", "nv12"],
                ["--input", "a.npy", "--pixel_format", "yuyv"], ["--input", "a.npy", "--output_pixel_format", "i420"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(bad)
    a = cli.parse_arguments(["--input", "a.npy", "--output_pixel_format", "nv12"])              # any source may be written as NV12
    assert a.output_pixel_format == "nv12"


def test_frame_writer_names_the_nv12_file(tmp_path):
    """The headerless writer with pixel_format nv12: the suffix and the metadata say so (the pixels are the device's: tests/test_gpu_yuv.py)."""
    import json
    cli = pkg("cli")
    wr = cli.FrameWriter(tmp_path / "out", (16, 6, 25.0), None, None, "nv12", "bt709", "full")
    assert wr.path.name == "out.nv12" and wr.yuv == ("nv12", "bt709", "full")
    wr.close()
    meta = json.load(open(str(wr.path) + ".json"))
    assert meta == dict(width=16, height=6, fps=25.0, pixel_format="nv12", yuv_matrix="bt709", yuv_range="full", frames=0)
    wr = cli.FrameWriter(tmp_path / "out", (16, 6, 25.0), None)
    assert wr.path.name == "out.bgr24" and wr.yuv is None
    wr.write(np.zeros((6, 16, 3), np.uint8))
    wr.close()
    assert json.load(open(str(wr.path) + ".json")) == dict(width=16, height=6, fps=25.0, pixel_format="bgr24", frames=1)


def test_the_kernels_have_no_scratch_and_no_spills():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "yuv_to_bgr_kernel" in k or "bgr_to_yuv_kernel" in k}
    assert len(tab) == 12, sorted(tab)                                       # two directions x two formats x three access widths
    for k, r in tab.items():                                                 # pure streaming: no LDS, and few enough registers for full occupancy
        assert not r["scratch"] and not r["vgpr_spills"] and r["lds"] == 0 and r["vgpr"] + r["agpr"] <= 64, (k, r)
