"""The JPEG decoding stage (aic_jpegdec_*) without a GPU: the symbols, the probe against the oracle's parse on every
case, every rejection that comes before the device (create, option and probe never touch it; on a machine without a GPU a decode that
got past the checks answers AIC_ERR_NO_DEVICE), the Python class, the Motion-JPEG splitter, the HIP-free half together with the bit
reader and block decoder the kernels compile under the sanitizers as a stand-alone program, and the kernels' budget."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_oracle as E
import jpegdec_cases as K
import jpegdec_oracle as D
from conftest import ROOT, pkg

NEW = tuple(f"aic_jpegdec_{f}" for f in ("probe", "create", "destroy", "option", "decode", "coefficients", "counters")) + ("aic_pipeline_upload_jpeg",)


def test_symbols_declared_and_exported_abi_still_2():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert set(re.findall(r"\b(aic_jpegdec_[a-z0-9_]+)\s*\(", hdr)) == set(NEW[:-1]) == {n for n in L.EXPORTS if n.startswith("aic_jpegdec_")}
    assert lib.aic_abi_version() == 2 and "#define AIC_ABI_VERSION 2" in hdr
    assert pkg().JpegDecoder is pkg("jpegdec").JpegDecoder
    J = pkg("jpegdec")
    assert J.REASONS == D.REASONS
    for k, name in enumerate(D.REASONS[1:], 1):
        assert re.search(r"#define AIC_JPEGDEC_%s %d\b" % (name, k), hdr), name
    assert C.sizeof(L.JpegdecInfo) == 48 and C.sizeof(L.JpegdecConfig) == 12


def test_probe_equals_the_oracles_parse_on_every_case():
    J = pkg("jpegdec")
    for name, f, size, *_ in K.well_formed() + K.refused() + K.mutations()[:300]:
        assert J.probe(f) == D.probe(f), name                                 # no size is asked for: SIZE_MISMATCH only for a size out of range
    assert J.probe(K.well_formed()[0][1])["status"] == 0


def test_probe_and_create_reject():
    L = pkg("_lib")
    lib = L.load()
    info, a = L.JpegdecInfo(), np.zeros(8, np.uint8)
    assert lib.aic_jpegdec_probe(L.ptr(a), 8, None) == L.ERR_INVALID and lib.aic_jpegdec_probe(None, 8, C.byref(info)) == L.ERR_INVALID
    assert lib.aic_jpegdec_probe(L.ptr(a), -1, C.byref(info)) == L.ERR_INVALID
    assert lib.aic_jpegdec_probe(L.ptr(a), (64 << 20) + 1, C.byref(info)) == L.ERR_INVALID
    assert lib.aic_jpegdec_probe(None, 0, C.byref(info)) == L.OK and (info.status, info.reason) == (L.ERR_FORMAT, D.NOT_JPEG)
    h = C.c_void_p()
    for cfg in ((0, 8, 8), (4097, 8, 8), (1, 0, 8), (1, 16385, 8), (1, 8, 0), (1, 8, 16385)):
        c = L.JpegdecConfig(*cfg)
        assert lib.aic_jpegdec_create(0, C.byref(c), C.byref(h)) == L.ERR_INVALID and not h.value, cfg
    c = L.JpegdecConfig(4, 16, 16)
    assert lib.aic_jpegdec_create(-1, C.byref(c), C.byref(h)) == L.ERR_INVALID and lib.aic_jpegdec_create(0, None, C.byref(h)) == L.ERR_INVALID
    assert lib.aic_jpegdec_create(0, C.byref(c), None) == L.ERR_INVALID and lib.aic_jpegdec_destroy(None) == L.OK
    for cfg in ((1, 1, 1), (4096, 16384, 16384)):                             # the limits: creating touches no device, so no memory either
        c = L.JpegdecConfig(*cfg)
        assert lib.aic_jpegdec_create(0, C.byref(c), C.byref(h)) == L.OK and h.value and lib.aic_jpegdec_destroy(h) == L.OK


@pytest.fixture()
def handle():
    """A decoder of up to 4 images of 16 x 16: creating one touches no device, so this works on every machine."""
    L = pkg("_lib")
    h, cfg = C.c_void_p(), L.JpegdecConfig(4, 16, 16)
    assert L.load().aic_jpegdec_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_jpegdec_destroy(h) == L.OK


def test_option_and_counters(handle):
    L = pkg("_lib")
    lib = L.load()
    for v in (1, 1024, 65536):
        assert lib.aic_jpegdec_option(handle, b"launch_budget_mb", v) == L.OK
    for v in (0, -1, 65537):
        assert lib.aic_jpegdec_option(handle, b"launch_budget_mb", v) == L.ERR_INVALID and b"launch_budget_mb" in lib.aic_last_error()
    assert lib.aic_jpegdec_option(handle, b"quality", 1) == L.ERR_INVALID and b"quality" in lib.aic_last_error()
    assert lib.aic_jpegdec_option(handle, None, 1) == L.ERR_INVALID and lib.aic_jpegdec_option(None, b"launch_budget_mb", 1) == L.ERR_INVALID
    c = [C.c_int64(-1) for _ in range(4)]
    assert lib.aic_jpegdec_counters(handle, *(C.byref(x) for x in c)) == L.OK and [x.value for x in c] == [0, 0, 0, 0]
    assert lib.aic_jpegdec_counters(None, None, None, None, None) == L.ERR_INVALID and lib.aic_jpegdec_counters(handle, None, None, None, None) == L.OK


def test_decode_rejects_before_the_device(handle):
    L, J = pkg("_lib"), pkg("jpegdec")
    lib = L.load()
    f = E.encode(K.image("noise", 16, 16, 1), 85, 0, 420)
    buf, off = J.pack([f] * 4)
    out, st, rs = np.full((4, 16, 16, 3), 7, np.uint8), np.full(4, -9, np.int32), np.full(4, -9, np.int32)
    base = dict(h=handle, f=buf, fm=L.HOST, off=off, n=4, out=out, om=L.HOST, st=st, rs=rs)

    def rc(**kw):
        a = dict(base, **kw)
        return lib.aic_jpegdec_decode(a["h"], L.ptr(a["f"]), a["fm"], L.ptr(a["off"]), a["n"], L.ptr(a["out"]), a["om"], L.ptr(a["st"]), L.ptr(a["rs"]))
    down, huge = off.copy(), off.copy()
    down[2] = down[1] - 1
    huge[1:] += 64 << 20
    neg = off - 1
    for kw in (dict(n=5), dict(n=-1), dict(f=None), dict(off=None), dict(out=None), dict(st=None), dict(rs=None), dict(fm=2), dict(fm=-1), dict(om=2), dict(h=None),
               dict(off=down), dict(off=huge), dict(off=neg)):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert (out == 7).all() and (st == -9).all() and (rs == -9).all()
    assert rc(n=0, f=None, off=None, out=None, st=None, rs=None) == L.OK         # no images: nothing to do, on every machine
    coef = np.zeros((1, 6, 64), np.int16)
    for kw in (dict(n=5), dict(image=4), dict(image=-1), dict(out=None), dict(fm=3), dict(off=None), dict(f=None), dict(n=0, image=0)):
        a = dict(dict(f=buf, fm=L.HOST, off=off, n=4, image=0, out=coef), **kw)
        assert lib.aic_jpegdec_coefficients(handle, L.ptr(a["f"]), a["fm"], L.ptr(a["off"]), a["n"], a["image"], L.ptr(a["out"])) == L.ERR_INVALID, kw
    assert lib.aic_jpegdec_coefficients(None, L.ptr(buf), L.HOST, L.ptr(off), 4, 0, L.ptr(coef)) == L.ERR_INVALID
    assert lib.aic_pipeline_upload_jpeg(None, 0, L.ptr(buf), L.HOST, L.ptr(off), 4, L.ptr(st), L.ptr(rs)) == L.ERR_INVALID
    if L.device_count() == 0:                                                 # what passes the checks reaches the device
        assert rc() == L.ERR_NO_DEVICE and rc(om=L.DEVICE) == L.ERR_NO_DEVICE
        assert lib.aic_jpegdec_coefficients(handle, L.ptr(buf), L.HOST, L.ptr(off), 4, 0, L.ptr(coef)) == L.ERR_NO_DEVICE


def test_python_class_and_splitter_need_no_device(tmp_path):
    J, L = pkg("jpegdec"), pkg("_lib")
    for kw in (dict(max_images=0), dict(max_images=4097)):
        with pytest.raises(L.AicError) as ei:
            J.JpegDecoder(16, 16, **kw)
        assert ei.value.code == L.ERR_INVALID
    for hw in ((0, 16), (16, 16385)):
        with pytest.raises(L.AicError):
            J.JpegDecoder(*hw)
    d = J.JpegDecoder(16, 16, max_images=2)
    files = [E.encode(K.image("noise", 16, 16, k), 85, 0, 420) for k in range(3)]
    buf, off = J.pack(files)
    assert off.tolist() == [0, len(files[0]), len(files[0]) + len(files[1]), sum(map(len, files))] and buf.size == off[-1]
    with pytest.raises(ValueError):
        d.decode(files)                                                       # three images, max_images is 2
    for bad_buf, bad_off in ((buf.astype(np.int32), off[:3]), (buf.reshape(1, -1), off[:3]), (buf[:10], off[:3]), (buf, off[:1][:0])):
        with pytest.raises(ValueError):
            d.decode_packed(bad_buf, bad_off)
    for out in (np.zeros((2, 16, 16, 3), np.int32), np.zeros((1, 16, 16, 3), np.uint8), np.zeros((2, 16, 32, 3), np.uint8)[:, :, ::2]):
        with pytest.raises(ValueError):
            d.decode_packed(buf, off[:3], out=out)
    bgr, st, rs = d.decode([])
    assert bgr.shape == (0, 16, 16, 3) and st.size == 0 and d.counters() == dict(images=0, refused=0, bytes_in=0, bytes_out=0)
    d.option("launch_budget_mb", 8)
    with pytest.raises(L.AicError):
        d.option("launch_budget_mb", 0)
    d.close(), d.close()
    # the splitter: by the side file, and by walking SOI .. EOI (a comment that holds a marker, restart markers, stuffing)
    odd = K.splice(files[1], 0xFE, b"\xff\xd9\xff\xd8 inside a comment")
    clip = tmp_path / "clip.mjpeg"
    clip.write_bytes(files[0] + odd + files[2])
    want = [0, len(files[0]), len(files[0]) + len(odd), len(files[0]) + len(odd) + len(files[2])]
    b2, o2 = J.split_mjpeg(clip)
    assert o2.tolist() == want and b2.tobytes() == clip.read_bytes()
    (tmp_path / "clip.mjpeg.json").write_text(json.dumps(dict(offsets=want, frames=3)))
    assert J.split_mjpeg(str(clip))[1].tolist() == want
    (tmp_path / "clip.mjpeg.json").write_text(json.dumps(dict(offsets=[0, 5], frames=1)))    # a stale side file is not believed
    assert J.split_mjpeg(clip)[1].tolist() == want
    os.remove(tmp_path / "clip.mjpeg.json")
    clip.write_bytes(files[0] + files[1][:-40])
    assert J.split_mjpeg(clip)[1].tolist() == [0, len(files[0]), len(files[0]) + len(files[1]) - 40]       # the torn tail is a file of its own
    P = pkg("pipeline").TrackingPipeline
    assert callable(P.upload_jpeg) and callable(P.run_from_jpeg)


def test_host_half_and_the_shared_decoder_under_the_sanitizers_stand_alone(tmp_path):
    """jpegdec_host.cpp + jpeg_host.cpp + jpegdec_decode.hpp + tests/jpegdec_host_probe.cpp with the system g++ under
    -fsanitize=address,undefined, run as a program of its own over every case and 2 000 mutations, against a dump of the oracle's."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the probe builds jpegdec_host.cpp with the system compiler")
    cases = K.well_formed() + K.refused() + K.mutations()
    assert len(K.mutations()) == 2000
    K.dump(tmp_path / "cases.bin", cases)
    exe, csrc = str(tmp_path / "jpegdec_host_probe"), os.path.join(ROOT, "ai-camera_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",              # the runtimes inside the program: it runs as it is, whatever the environment preloads
                    os.path.join(csrc, "jpegdec_host.cpp"), os.path.join(csrc, "jpeg_host.cpp"), os.path.join(ROOT, "tests", "jpegdec_host_probe.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith(f"probe ok: {len(cases)} cases") and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_kernels_have_no_scratch_no_spills_and_a_small_lds_tile():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "jpegdec_" in k and "_kernel" in k}
    assert len(tab) == 4 and all(sum(n in k for k in tab) == 1 for n in ("markers", "entropy", "idct", "colour")), sorted(tab)
    for k, r in tab.items():             # as the encoder's kernels: 128 registers leave four waves a SIMD; the table set in LDS is 6240 bytes, the IDCT's workspace 9216
        assert not r["scratch"] and not r["vgpr_spills"] and r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 16 * 1024, (k, r)


def test_cli_parser_refuses_yuv_pixel_formats_for_a_motion_jpeg_source():
    cli = pkg("cli")
    assert cli.parse_arguments(["--input", "clip.mjpeg"]).input == "clip.mjpeg"
    assert cli.parse_arguments(["--inputs", "a.mjpeg,b.npy", "--tracker", "bytetrack"]).inputs == "a.mjpeg,b.npy"
    assert cli.parse_arguments(["--input", "clip.mjpeg", "--output_codec", "mjpeg"]).output_codec == "mjpeg"
    for fmt in ("nv12", "i420"):
        for src in (["--input", "clip.mjpeg"], ["--inputs", "raw:64x48:a.yuv,clip.mjpeg", "--tracker", "bytetrack"]):
            with pytest.raises(SystemExit):
                cli.parse_arguments(src + ["--pixel_format", fmt])
    with pytest.raises(SystemExit) as ei:
        cli.frame_source("no_such_clip.mjpeg")
    assert "not found" in str(ei.value)
