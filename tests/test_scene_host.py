"""The scene-watch stage (aic_scene_*) without a GPU: the symbols, every rejection that comes before the device
(create, option and reset never touch it; on a machine without a GPU anything that got past an update's checks answers
AIC_ERR_NO_DEVICE instead), the Python class's own checks, the CLI flags, the pipeline hook with nothing attached, and the kernels'
budget."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import scene_oracle as SO
from conftest import ROOT, pkg

NEW = tuple(f"aic_scene_{f}" for f in ("config_default", "create", "destroy", "option", "reset", "update", "export"))


def config(**kw):
    L = pkg("_lib")
    cfg = L.SceneConfig()
    assert L.load().aic_scene_config_default(2, 72, 101, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_symbols_declared_exported_and_defaults():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    assert set(re.findall(r"\b(aic_scene_[a-z0-9_]+)\s*\(", hdr)) == set(NEW) == {n for n in L.EXPORTS if n.startswith("aic_scene_")}
    for name in NEW:
        getattr(lib, name)
    assert pkg().SceneWatch is pkg("scene").SceneWatch
    import src.tracker.scene as re_export
    assert re_export.SceneWatch is pkg("scene").SceneWatch
    cfg = config()
    assert (cfg.streams, cfg.frame_h, cfg.frame_w, cfg.cell) == (2, 72, 101, 8)
    assert lib.aic_scene_config_default(1, 1, 1, None) == L.ERR_INVALID
    assert pkg("scene").KINDS == SO.KINDS and pkg("scene").RECORD_FIELDS == SO.RECORD_FIELDS
    assert set(pkg("scene").OPTIONS) == set(SO.OPTIONS) | {"ticks_per_launch", "launch_budget_mb"}


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(cell=0), b"cell"), (dict(cell=2), b"cell"), (dict(cell=12), b"cell"), (dict(cell=32), b"cell"), (dict(frame_h=7), b"smaller"),
    (dict(frame_w=15, cell=16), b"smaller")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_scene_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_and_limits():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_scene_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_scene_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_scene_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    big = config(streams=256, frame_h=16384, frame_w=16384, cell=4)         # the largest: no device, no memory yet
    assert lib.aic_scene_create(0, C.byref(big), C.byref(h)) == L.OK and h.value
    assert lib.aic_scene_destroy(h) == L.OK


@pytest.fixture()
def handle():
    """Two streams of 72 x 101 at c = 8 (a 9 x 12 grid): creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config()
    assert L.load().aic_scene_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_scene_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_scene_option(None, b"thresh", 1) == L.ERR_INVALID
    assert lib.aic_scene_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_scene_update(None, None, L.HOST, 0, None, None, L.HOST, None, None, None) == L.ERR_INVALID
    assert lib.aic_scene_export(None, 0, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_scene_destroy(None) == L.OK


def test_every_option_range_and_reset_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert all(lib.aic_scene_reset(handle, s) == L.OK for s in (-1, 0, 1))
    assert lib.aic_scene_reset(handle, 2) == L.ERR_INVALID and lib.aic_scene_reset(handle, -2) == L.ERR_INVALID
    ranges = {k: (lo, hi) for k, (_, lo, hi) in SO.OPTIONS.items()}
    ranges.update(ticks_per_launch=(0, 65536), launch_budget_mb=(1, 65536))
    for key, (lo, hi) in ranges.items():
        default = SO.OPTIONS.get(key, (None,))[0]
        for v in (lo, hi):
            rc = lib.aic_scene_option(handle, key.encode(), v)
            assert rc == L.OK or key in ("learn_shift", "slow_extra"), (key, v)          # (their sum is bounded as well: below)
        for v in (lo - 1, hi + 1):
            assert lib.aic_scene_option(handle, key.encode(), v) == L.ERR_INVALID, (key, v)
            assert key.encode() in lib.aic_last_error()
        if default is not None:
            assert lib.aic_scene_option(handle, key.encode(), default) == L.OK
    assert lib.aic_scene_option(handle, b"learn_shift", 12) == L.ERR_INVALID and b"14" in lib.aic_last_error()       # 12 + 3
    assert lib.aic_scene_option(handle, b"slow_extra", 2) == L.OK and lib.aic_scene_option(handle, b"learn_shift", 12) == L.OK
    assert lib.aic_scene_option(handle, b"slow_extra", 3) == L.ERR_INVALID
    assert lib.aic_scene_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_scene_option(handle, None, 1) == L.ERR_INVALID
    bg, dv, pv, sc = [np.ones((9, 12), np.int32) for _ in range(3)] + [np.ones(16, np.int32)]
    assert lib.aic_scene_export(handle, 0, L.ptr(bg), L.ptr(dv), L.ptr(pv), L.ptr(sc)) == L.OK            # nothing seen yet: zeros, no device
    assert not bg.any() and not dv.any() and not pv.any() and not sc.any()
    assert lib.aic_scene_export(handle, 2, L.ptr(bg), L.ptr(dv), L.ptr(pv), L.ptr(sc)) == L.ERR_INVALID
    assert lib.aic_scene_export(handle, 0, None, L.ptr(dv), L.ptr(pv), L.ptr(sc)) == L.ERR_INVALID


def test_update_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    rec, masks, rm = np.zeros((1, 2, 16), np.int32), np.zeros((1, 2, 9, 12), np.uint8), np.zeros(1, np.int32)

    def rc(frames=frames, fmem=L.HOST, ticks=1, counts=counts, rows=rows, rmem=L.HOST, rec=rec, masks=masks, rm=rm):
        return lib.aic_scene_update(handle, L.ptr(frames), fmem, ticks, L.ptr(counts), L.ptr(rows), rmem, L.ptr(rec), L.ptr(masks), L.ptr(rm))
    for kw in (dict(frames=None), dict(rows=None), dict(rec=None), dict(rm=None), dict(fmem=2), dict(fmem=-1), dict(rmem=2), dict(rmem=-1),
               dict(ticks=-1), dict(ticks=65537), dict(counts=np.array([1, -1], np.int32)), dict(counts=None)):    # (row_motion without counts)
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32), rm=np.zeros(513, np.int32)) == L.ERR_CAPACITY
    assert b"512" in lib.aic_last_error()
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE; no rows, no masks and no ticks are fine
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE
        assert rc(masks=None) == L.ERR_NO_DEVICE
        assert rc(counts=None, rows=None, rm=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None, rm=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, frames=None, counts=None, rows=None, rec=None, masks=None, rm=None) == L.ERR_NO_DEVICE


def test_python_class_needs_no_device_until_update():
    SW, L = pkg("scene").SceneWatch, pkg("_lib")
    for kw in (dict(streams=0), dict(streams=257), dict(cell=5), dict(frame_hw=(4, 101)), dict(thresh=256), dict(hold=0), dict(warmup=0),
               dict(learn_shift=13), dict(slow_extra=9), dict(learn_shift=12), dict(min_neighbours=10), dict(gate_cells=0), dict(no_such_option=1)):
        a = dict(streams=2, frame_hw=(72, 101))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            SW(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    sw = SW(2, (72, 101), cell=4, hold=3, warmup=2)
    assert (sw.grid_h, sw.grid_w) == (18, 25)
    sw.set_option("thresh", 9), sw.reset(), sw.reset(1)
    with pytest.raises(L.AicError):
        sw.reset(2)
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        sw.update(frames[:, :1])                                             # one stream's frames for two
    with pytest.raises(ValueError):
        sw.update(np.zeros((1, 2, 72, 100, 3), np.uint8))
    with pytest.raises(ValueError):
        sw.update(frames, [[empty]])                                         # one row list for two streams
    with pytest.raises(ValueError):
        sw.update(frames, np.zeros((3, 6), np.int32), counts=[2, 2])
    with pytest.raises(ValueError):
        sw.update(frames, np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        sw.update(frames, [[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    e = sw.export(1)
    assert e["bg"].shape == (18, 25) and e["age"] == 0 and not e["scalars"].any()
    if L.device_count() == 0:
        for call in (lambda: sw.update(frames), lambda: sw.update(frames, [[empty, empty]], want_masks=True), lambda: sw.update(frames[:0])):
            with pytest.raises(L.NoDeviceError):
                call()
    sw.close()


def test_result_views_and_events():
    S = pkg("scene")
    rec = np.zeros((3, 2, 16), np.int32)
    rec[1, 1, 15] = S.DARK | S.FROZEN << 8
    rec[2, 0, 15] = S.SCENE
    rec[2, 0, 14] = S.SCENE | S.DEFOCUS
    rec[:, :, 2] = 1
    rec[0, 1, 5:9] = 8, 16, 24, 32
    res = S.SceneResult(rec, None, np.array([5, -1, 7], np.int32), np.array([0, 0, 2, 2, 2, 3, 3]))
    assert res.events() == [(1, 1, "dark", True), (1, 1, "frozen", False), (2, 0, "scene", True)]
    assert res.active.all() and res.alarms[2, 0] == 12 and S.alarm_names(res.alarms[2, 0]) == ["defocus", "scene"]
    assert res.motion_box[0, 1].tolist() == [8, 16, 24, 32] and res.rows_of(0, 1).tolist() == [5, -1] and res.rows_of(2, 0).tolist() == [7]
    with pytest.raises(AttributeError):
        res.no_such_field


def test_cli_flags():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--scene_watch", "--scene_cell", "16"])
    assert a.scene_watch and a.scene_cell == 16
    for tracker in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
        a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", tracker, "--scene_watch"])
        assert a.scene_watch and a.scene_cell is None
    a = cli.parse_arguments(["--input", "a.npy"])
    assert not a.scene_watch and a.scene_cell is None
    for bad in (["--scene_cell", "8"], ["--scene_watch", "--scene_cell", "5"], ["--scene_watch", "--scene_cell", "x"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + bad)


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_scene(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._scene_watch is None and TP.scene_result is None
    watch = type("W", (), dict(streams=3, frame_h=72, frame_w=101))()
    with pytest.raises(ValueError):
        TP.attach_scene_watch(type("P", (), dict(streams=2, frame_h=72, frame_w=101))(), watch)
    with pytest.raises(ValueError):
        TP.attach_scene_watch(type("P", (), dict(streams=3, frame_h=72, frame_w=100))(), watch)
    fake = type("P", (), dict(streams=3, frame_h=72, frame_w=101))()
    TP.attach_scene_watch(fake, watch)
    assert fake._scene_watch is watch and fake.scene_result is None
    TP.attach_scene_watch(fake, None)
    assert fake._scene_watch is None


def test_new_kernels_have_no_scratch_no_spills_and_no_float():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "scene_" in k}
    for name, n in (("scene_gray_kernel", 6), ("scene_model_kernel", 1), ("scene_stats_kernel", 1), ("scene_rows_kernel", 1), ("scene_walk_kernel", 1)):
        assert sum(name in k for k in tab) == n, (name, sorted(tab))
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in tab.items():
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] <= 4 * 1024, (k, r)
    src = open(os.path.join(ROOT, "ai-camera_amd", "csrc", "kernels_scene.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|half)\b|\d\.\d*f?\b", code)
