"""The zone / line counting stage (aic_zones_*) without a GPU: the symbols, every rejection that comes before the
device (create, set, reset and option never touch it; on a machine without a GPU anything that got past an update's checks would
answer AIC_ERR_NO_DEVICE instead), the --zones file of the CLI, the pipeline hook with nothing attached, and the kernels' budget."""
import ctypes as C
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_zones_{f}" for f in ("create", "destroy", "set", "update", "counters", "reset", "option"))
I32 = lambda *v: np.array(v, np.int32)        # noqa: E731


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert pkg().ZoneCounter is pkg("zones").ZoneCounter
    import src.tracker.zones as re_export
    assert re_export.ZoneCounter is pkg("zones").ZoneCounter


@pytest.mark.parametrize("args,word", [((0, 8, 70, 0), b"streams"), ((257, 8, 70, 0), b"streams"), ((2, 0, 70, 0), b"max_tracks"),
                                       ((2, 513, 70, 0), b"max_tracks"), ((2, 8, -1, 0), b"forget_after"), ((2, 8, 70, 2), b"anchor"),
                                       ((2, 8, 70, -1), b"anchor")])
def test_create_rejects(args, word):
    L = pkg("_lib")
    h = C.c_void_p()
    assert L.load().aic_zones_create(0, *args, C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()
    assert L.load().aic_zones_create(0, 2, 8, 70, 0, None) == L.ERR_INVALID
    assert L.load().aic_zones_create(-1, 2, 8, 70, 0, C.byref(h)) == L.ERR_INVALID and not h.value


@pytest.fixture()
def handle():
    """A counter of 2 streams: creating one touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    assert L.load().aic_zones_create(0, 2, 8, 70, 0, C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_zones_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    a = I32(0, 0)
    assert lib.aic_zones_set(None, 0, 0, None, None, 0, None) == L.ERR_INVALID
    assert lib.aic_zones_update(None, L.ptr(a), None, None, L.HOST, 4, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_zones_counters(None, 0, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_zones_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_zones_option(None, b"frames_per_launch", 1) == L.ERR_INVALID
    assert lib.aic_zones_destroy(None) == L.OK


def test_set_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    tri, m = I32(0, 0, 10, 0, 0, 10), 1 << 20
    line = I32(0, 0, 5, 5)

    def rc(stream, nz, nvert, xy, nl, lines):
        return lib.aic_zones_set(handle, stream, nz, L.ptr(nvert), L.ptr(xy), nl, L.ptr(lines))
    assert rc(0, 1, I32(3), tri, 1, line) == L.OK
    assert rc(0, 0, None, None, 0, None) == L.OK
    for stream in (-1, 2):
        assert rc(stream, 1, I32(3), tri, 0, None) == L.ERR_INVALID and b"stream" in lib.aic_last_error()
    assert rc(0, 33, I32(*[3] * 33), np.tile(tri, 33), 0, None) == L.ERR_INVALID and b"n_zones" in lib.aic_last_error()
    assert rc(0, -1, None, None, 0, None) == L.ERR_INVALID
    assert rc(0, 0, None, None, 33, np.tile(line, 33)) == L.ERR_INVALID and b"n_lines" in lib.aic_last_error()
    assert rc(0, 0, None, None, -1, None) == L.ERR_INVALID
    assert rc(0, 1, None, tri, 0, None) == L.ERR_INVALID and rc(0, 1, I32(3), None, 0, None) == L.ERR_INVALID
    assert rc(0, 0, None, None, 1, None) == L.ERR_INVALID
    for nv in (2, 33, 0, -3):
        assert rc(0, 1, I32(nv), np.tile(tri, 11), 0, None) == L.ERR_INVALID and b"vertices" in lib.aic_last_error(), nv
    assert rc(0, 1, I32(32), np.tile(tri, 11), 0, None) == L.OK
    for bad in (m + 1, -m - 1):
        assert rc(0, 1, I32(3), I32(0, 0, bad, 0, 0, 10), 0, None) == L.ERR_INVALID and b"2^20" in lib.aic_last_error()
        assert rc(0, 0, None, None, 1, I32(0, 0, 5, bad)) == L.ERR_INVALID and b"2^20" in lib.aic_last_error()
    assert rc(0, 1, I32(3), I32(-m, -m, m, -m, 0, m), 1, I32(-m, m, m, -m)) == L.OK


def test_update_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    fps, counts, rows = I32(1, 1), I32(1, 0), np.zeros((1, 6), np.int32)
    ne, ev, occ, st = np.zeros(2, np.int32), np.zeros((2, 4, 8), np.int32), np.zeros((2, 32), np.int32), np.zeros(2, np.int32)

    def rc(fps=fps, counts=counts, rows=rows, mem=L.HOST, cap=4, ne=ne, ev=ev, occ=occ, st=st):
        return lib.aic_zones_update(handle, L.ptr(fps), L.ptr(counts), L.ptr(rows), mem, cap, L.ptr(ne), L.ptr(ev), L.ptr(occ), L.ptr(st))
    for kw in (dict(fps=None), dict(counts=None), dict(rows=None), dict(ne=None), dict(ev=None), dict(occ=None), dict(mem=2), dict(mem=-1),
               dict(cap=-1), dict(cap=(1 << 16) + 1), dict(fps=I32(1, -1)), dict(counts=I32(1, -1))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=I32(513, 0), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY and b"512" in lib.aic_last_error()
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE, and NULL status / no rows / no frames are fine
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE
        assert rc(st=None) == L.ERR_NO_DEVICE
        assert rc(counts=I32(0, 0), rows=None) == L.ERR_NO_DEVICE
        assert rc(fps=I32(0, 0), counts=None, rows=None, ne=None, ev=None, occ=None) == L.ERR_NO_DEVICE
        assert rc(cap=0, ev=None) == L.ERR_NO_DEVICE


def test_reset_option_counters_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_zones_reset(handle, 0) == L.OK and lib.aic_zones_reset(handle, 1) == L.OK
    assert lib.aic_zones_reset(handle, 2) == L.ERR_INVALID and lib.aic_zones_reset(handle, -1) == L.ERR_INVALID
    assert lib.aic_zones_option(handle, b"frames_per_launch", 16) == L.OK and lib.aic_zones_option(handle, b"frames_per_launch", 0) == L.OK
    assert lib.aic_zones_option(handle, b"frames_per_launch", -1) == L.ERR_INVALID
    assert lib.aic_zones_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_zones_option(handle, None, 1) == L.ERR_INVALID
    a = [np.full(32, 9, np.int64) for _ in range(4)]
    assert lib.aic_zones_counters(handle, 1, *(L.ptr(x) for x in a)) == L.OK      # nothing counted yet: zeros, no device
    assert not any(x.any() for x in a)
    assert lib.aic_zones_counters(handle, 2, *(L.ptr(x) for x in a)) == L.ERR_INVALID
    assert lib.aic_zones_counters(handle, 0, None, None, None, None) == L.OK


def test_python_class_rejections_need_no_device():
    Z = pkg("zones")
    L = pkg("_lib")
    with pytest.raises(ValueError):
        Z.ZoneCounter(anchor="top")
    with pytest.raises(L.AicError) as ei:
        Z.ZoneCounter(streams=0)
    assert ei.value.code == L.ERR_INVALID
    zc = Z.ZoneCounter(streams=2, max_tracks=4)
    zc.set_zones(1, [[(0, 0), (10, 0), (0, 10)]], [[(0, 0), (5, 5)]])
    assert zc.n_zones == [0, 1] and zc.n_lines == [0, 1]
    for zones, lines in (([[(0, 0), (1, 1)]], []), ([[(0, 0), (1, 1), (0.5, 3)]], []), ([[(0, 0), (1, 1), (1 << 21, 3)]], []), ([], [[(0, 0)]]),
                         ([[(0, 0), (4, 0), (0, 4)]] * 33, [])):
        with pytest.raises(ValueError):
            zc.set_zones(0, zones, lines)
    with pytest.raises(ValueError):
        zc.update([[]])                                                      # one list for two streams
    with pytest.raises(ValueError):
        zc.update(np.zeros((3, 6), np.int32), counts=[2, 2], frames_per_stream=[1, 1])
    assert all(v.tolist() == [0] for v in zc.counters(1).values())
    if L.device_count() == 0:
        with pytest.raises(L.NoDeviceError):
            zc.update([[np.zeros((0, 6), np.int32)], []])
    zc.close()


def test_zones_file_parser(tmp_path):
    Z, cli = pkg("zones"), pkg("cli")
    one = {"cameras": [{"zones": [[[0, 0], [10, 0], [10, 10], [0, 10]]], "lines": [[[0, 5], [10, 5]]]}]}
    p = tmp_path / "z.json"
    p.write_text(json.dumps(one))
    got = Z.load_zones_file(str(p), 3)                                       # one entry serves every camera
    assert len(got) == 3 and all(len(z) == 1 and len(l) == 1 for z, l in got)
    assert got[2][0][0].dtype == np.int32 and got[2][0][0].tolist() == [[0, 0], [10, 0], [10, 10], [0, 10]] and got[0][1][0].tolist() == [[0, 5], [10, 5]]
    two = {"cameras": [one["cameras"][0], {"lines": []}]}
    got = Z.load_zones_file(two, 2)
    assert got[1] == ([], [])
    for bad, n in ((two, 3), ({}, 1), ({"cameras": []}, 1), ([1], 1), ({"cameras": [{"zone": []}]}, 1), ({"cameras": [{"zones": [[[0, 0], [1, 1]]]}]}, 1),
                   ({"cameras": [{"zones": [[[0, 0], [1, 1], [2.5, 0]]]}]}, 1), ({"cameras": [{"lines": [[[0, 0], [1, 1], [2, 2]]]}]}, 1),
                   ({"cameras": [{"lines": [[[0, 0], [1 << 21, 1]]]}]}, 1)):
        with pytest.raises(ValueError):
            Z.load_zones_file(bad, n)
    assert cli.parse_arguments(["--zones", str(p), "--input", "a.npy"]).zones == str(p)
    assert cli.parse_arguments(["--zones", str(p), "--inputs", "a.npy,b.npy", "--tracker", "ocsort"]).zones == str(p)
    assert cli.parse_arguments(["--input", "a.npy"]).zones is None


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_zones(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                                # nothing attached: nothing is computed, nothing is set
    assert TP._zones is None and TP.zone_events is None and TP.zone_occupancy is None and TP.zone_result is None
    with pytest.raises(RuntimeError):
        TP.zone_counters(type("P", (), dict(streams=2, _zones=None))())
    with pytest.raises(ValueError):
        TP.attach_zones(type("P", (), dict(streams=2))(), type("Z", (), dict(streams=3))())
    fake = type("P", (), dict(streams=2))()
    TP.attach_zones(fake, None)
    assert fake._zones is None and fake.zone_result is None


def test_new_kernels_have_no_scratch_and_no_spills():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "zones_" in k}
    for name in ("zones_classify_kernel", "zones_walk_kernel"):
        assert sum(name in k for k in tab) == 1, (name, sorted(tab))
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in tab.items():                                                 # a 512-thread block is 2 waves per SIMD: 256 registers each
        assert r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 40 * 1024, (k, r)
