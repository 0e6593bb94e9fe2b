"""The left-objects stage (aic_left_*) without a GPU: the symbols, every rejection that comes before the device
(create, option and reset never touch it; on a machine without a GPU anything that got past an update's checks answers
AIC_ERR_NO_DEVICE instead), the Python class's own checks, the CLI flags, the pipeline hook with nothing attached, and the kernels'
budget."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import left_oracle as LO
from conftest import ROOT, pkg

NEW = tuple(f"aic_left_{f}" for f in ("config_default", "create", "destroy", "option", "reset", "update", "export"))


def config(**kw):
    L = pkg("_lib")
    cfg = L.LeftConfig()
    assert L.load().aic_left_config_default(2, 72, 101, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_symbols_declared_exported_and_defaults():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    assert set(re.findall(r"\b(aic_left_[a-z0-9_]+)\s*\(", hdr)) == set(NEW) == {n for n in L.EXPORTS if n.startswith("aic_left_")}
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().LeftObjects is pkg("leftobj").LeftObjects
    import src.tracker.leftobj as re_export
    assert re_export.LeftObjects is pkg("leftobj").LeftObjects
    cfg = config()
    assert (cfg.streams, cfg.frame_h, cfg.frame_w, cfg.cell, cfg.max_objects) == (2, 72, 101, 8, 32)
    assert lib.aic_left_config_default(1, 1, 1, None) == L.ERR_INVALID
    M = pkg("leftobj")
    assert (M.RECORD_FIELDS, M.OBJECT_FIELDS, M.EVENT_FIELDS) == (LO.RECORD_FIELDS, LO.OBJECT_FIELDS, LO.EVENT_FIELDS)
    assert set(M.OPTIONS) == set(LO.OPTIONS) | {"ticks_per_launch", "launch_budget_mb"}
    assert (M.APPEARED, M.RAISED, M.ENDED, M.LEFT, M.REMOVED) == (LO.APPEARED, LO.RAISED, LO.ENDED, LO.LEFT, LO.REMOVED)


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(cell=0), b"cell"), (dict(cell=2), b"cell"), (dict(cell=12), b"cell"), (dict(cell=32), b"cell"), (dict(frame_h=7), b"smaller"),
    (dict(frame_w=15, cell=16), b"smaller"), (dict(max_objects=0), b"max_objects"), (dict(max_objects=65), b"max_objects")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_left_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_and_the_grid_limit():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_left_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_left_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_left_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    for kw in (dict(frame_h=512, frame_w=1024, cell=4), dict(frame_h=720, frame_w=1280, cell=8), dict(streams=256, frame_h=2048, frame_w=4096, cell=16),
               dict(frame_h=515, frame_w=1027, cell=4, max_objects=64)):     # 32768 cells, 14400, 32768, 32768 with remainders: no device, no memory yet
        assert lib.aic_left_create(0, C.byref(config(**kw)), C.byref(h)) == L.OK and h.value, kw
        assert lib.aic_left_destroy(h) == L.OK
        h = C.c_void_p()
    for kw in (dict(frame_h=516, frame_w=1024, cell=4), dict(frame_h=720, frame_w=1280, cell=4), dict(frame_h=16384, frame_w=16384, cell=16)):
        assert lib.aic_left_create(0, C.byref(config(**kw)), C.byref(h)) == L.ERR_CAPACITY and not h.value, kw
        assert b"32768" in lib.aic_last_error()


@pytest.fixture()
def handle():
    """Two streams of 72 x 101 at c = 8 (a 9 x 12 grid): creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config()
    assert L.load().aic_left_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_left_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_left_option(None, b"thresh", 1) == L.ERR_INVALID
    assert lib.aic_left_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_left_update(None, None, L.HOST, 0, None, None, L.HOST, 0, None, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_left_export(None, 0, None, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_left_destroy(None) == L.OK


def export_args(L, grid=(9, 12), m=32, fill=1):
    return [np.full(grid, fill, np.int32) for _ in range(5)] + [np.full((m, 12), fill, np.int32), np.full(4, fill, np.int32)]


def test_every_option_range_and_reset_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    opt = lambda k, v: lib.aic_left_option(handle, k.encode(), v)
    assert all(lib.aic_left_reset(handle, s) == L.OK for s in (-1, 0, 1))
    assert lib.aic_left_reset(handle, 2) == L.ERR_INVALID and lib.aic_left_reset(handle, -2) == L.ERR_INVALID
    ranges = {k: (lo, hi) for k, (_, lo, hi) in LO.OPTIONS.items()}
    ranges.update(ticks_per_launch=(0, 65536), launch_budget_mb=(1, 65536))
    coupled = ("min_ticks", "absorb_ticks", "min_cells", "max_cells")
    for key, (lo, hi) in ranges.items():
        default = LO.OPTIONS.get(key, (None,))[0]
        for v in (lo, hi):
            assert opt(key, v) == L.OK or key in coupled, (key, v)            # (each pair is bounded together as well: below)
        for v in (lo - 1, hi + 1):
            assert opt(key, v) == L.ERR_INVALID, (key, v)
            assert key.encode() in lib.aic_last_error()
        if default is not None:
            assert opt(key, default) == L.OK
    # absorb_ticks in min_ticks + 1 .. 65535
    assert opt("absorb_ticks", 50) == L.ERR_INVALID and b"absorb_ticks" in lib.aic_last_error() and opt("absorb_ticks", 51) == L.OK
    assert opt("min_ticks", 51) == L.ERR_INVALID and opt("min_ticks", 50) == L.OK and opt("min_ticks", 1) == L.OK and opt("absorb_ticks", 2) == L.OK
    assert opt("absorb_ticks", 65535) == L.OK and opt("min_ticks", 65534) == L.OK and opt("min_ticks", 65535) == L.ERR_INVALID
    # max_cells in min_cells .. 32768
    assert opt("max_cells", 1) == L.ERR_INVALID and opt("max_cells", 2) == L.OK and opt("min_cells", 3) == L.ERR_INVALID
    assert opt("max_cells", 32768) == L.OK and opt("min_cells", 32768) == L.OK and opt("min_cells", 1) == L.OK and opt("max_cells", 1) == L.OK
    assert opt("nonsense", 1) == L.ERR_INVALID and lib.aic_left_option(handle, None, 1) == L.ERR_INVALID
    out = export_args(L)
    assert lib.aic_left_export(handle, 0, *(L.ptr(a) for a in out)) == L.OK                # nothing seen yet: zeros, no device
    assert not any(a.any() for a in out)
    assert lib.aic_left_export(handle, 2, *(L.ptr(a) for a in out)) == L.ERR_INVALID
    assert lib.aic_left_export(handle, 0, None, *(L.ptr(a) for a in out[1:])) == L.ERR_INVALID
    assert lib.aic_left_export(handle, 0, *(L.ptr(a) for a in out[:6]), None) == L.ERR_INVALID


def test_update_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    rec, obj, ev = np.zeros((1, 2, 8), np.int32), np.zeros((1, 2, 32, 12), np.int32), np.zeros((4, 12), np.int32)
    n, st = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cand, labels = np.zeros((1, 2, 9, 12), np.uint8), np.zeros((1, 2, 9, 12), np.int32)

    def rc(frames=frames, fmem=L.HOST, ticks=1, counts=counts, rows=rows, rmem=L.HOST, cap=4, rec=rec, obj=obj, ev=ev, n=n, st=st, cand=cand,
           labels=labels):
        return lib.aic_left_update(handle, L.ptr(frames), fmem, ticks, L.ptr(counts), L.ptr(rows), rmem, cap, L.ptr(rec), L.ptr(obj), L.ptr(ev),
                                   L.ptr(n), L.ptr(st), L.ptr(cand), L.ptr(labels))
    for kw in (dict(frames=None), dict(rows=None), dict(rec=None), dict(obj=None), dict(ev=None), dict(n=None), dict(fmem=2), dict(fmem=-1),
               dict(rmem=2), dict(rmem=-1), dict(ticks=-1), dict(ticks=65537), dict(cap=-1), dict(cap=(1 << 24) + 1),
               dict(counts=np.array([1, -1], np.int32))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY
    assert b"512" in lib.aic_last_error()
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE; no rows, no masks, no status and no ticks are fine
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE
        assert rc(cand=None, labels=None, st=None) == L.ERR_NO_DEVICE
        assert rc(counts=None, rows=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None) == L.ERR_NO_DEVICE
        assert rc(cap=0, ev=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, frames=None, counts=None, rows=None, rec=None, obj=None, cand=None, labels=None) == L.ERR_NO_DEVICE


def test_python_class_needs_no_device_until_update():
    LOb, L = pkg("leftobj").LeftObjects, pkg("_lib")
    for kw in (dict(streams=0), dict(streams=257), dict(cell=5), dict(frame_hw=(4, 101)), dict(max_objects=0), dict(max_objects=65), dict(thresh=0),
               dict(thresh=256), dict(fast_shift=9), dict(slow_shift=13), dict(warmup=0), dict(decay=65), dict(min_ticks=0), dict(min_ticks=9000),
               dict(absorb_ticks=50), dict(pad_cells=9), dict(min_cells=0), dict(max_cells=1), dict(alarm_hold=0), dict(gone_ticks=-1),
               dict(no_such_option=1)):
        a = dict(streams=2, frame_hw=(72, 101))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            LOb(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    with pytest.raises(L.AicError) as ei:
        LOb(1, (720, 1280), cell=4)
    assert ei.value.code == L.ERR_CAPACITY
    lo = LOb(2, (72, 101), cell=4, max_objects=5, alarm_hold=3, warmup=2)
    assert (lo.grid_h, lo.grid_w, lo.max_objects) == (18, 25, 5)
    lo.option("thresh", 9), lo.reset(), lo.reset(1)
    with pytest.raises(L.AicError):
        lo.reset(2)
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        lo.update(frames[:, :1])                                             # one stream's frames for two
    with pytest.raises(ValueError):
        lo.update(np.zeros((1, 2, 72, 100, 3), np.uint8))
    with pytest.raises(ValueError):
        lo.update(frames, [[empty]])                                         # one row list for two streams
    with pytest.raises(ValueError):
        lo.update(frames, np.zeros((3, 6), np.int32), counts=[2, 2])
    with pytest.raises(ValueError):
        lo.update(frames, np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        lo.update(frames, [[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    e = lo.export(1)
    assert e["fast"].shape == (18, 25) and e["slots"].shape == (5, 12) and e["age"] == 0 and e["uids"] == 0 and not e["scalars"].any()
    if L.device_count() == 0:
        for call in (lambda: lo.update(frames), lambda: lo.update(frames, [[empty, empty]], want_masks=True), lambda: lo.update(frames[:0])):
            with pytest.raises(L.NoDeviceError):
                call()
    lo.close()


def test_result_views_alarmed_and_prims():
    M = pkg("leftobj")
    rec = np.zeros((2, 2, 8), np.int32)
    rec[1, 1] = 40, 1, 6, 1, 2, 1, 0, 0
    obj = np.zeros((2, 2, 3, 12), np.int32)
    obj[1, 1, 0] = 7, M.LEFT, 1, 16, 24, 48, 40, 12, 10, 6, 30, 0
    obj[1, 1, 2] = 9, 0, 0, 64, 8, 72, 16, -1, 38, 2, 3, 0
    ev = np.array([[1, 1, M.RAISED, 7, M.LEFT, 16, 24, 48, 40, 12, 6, 40], [1, 0, M.ENDED, 3, M.REMOVED, 0, 0, 8, 8, -1, 1, 40]], np.int32)
    res = M.LeftResult(rec, obj, ev, 2)
    assert not res.overflow and res.n_alarmed[1, 1] == 1 and res.frame[1, 1] == 40 and res.n_objects.tolist() == [[0, 0], [0, 2]]
    assert res.alarmed(1, 1) == [dict(uid=7, kind="LEFT", box=[16, 24, 48, 40], owner=12, age=30)] and res.alarmed(0, 1) == []
    assert res.events_of(1, 1).tolist() == [ev[0].tolist()] and len(res.events_of(0, 0)) == 0
    assert M.LeftResult(rec, obj, ev[:1], 2).overflow
    prims, text = res.prims(1, 1).arrays()
    assert bytes(text) == b"LEFT 7 <- 12" and [p[0] for p in prims] == [0, 1, 2, 0]      # outline + label bar + text, then the plain outline
    assert prims[0][1:5].tolist() == [16, 24, 48, 40] and prims[3][1:5].tolist() == [64, 8, 72, 16]
    assert len(res.prims(0, 0).arrays()[0]) == 0
    with pytest.raises(AttributeError):
        res.no_such_field


def test_cli_flags():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--left_objects", "--left_cell", "16", "--left_after", "120"])
    assert a.left_objects and a.left_cell == 16 and a.left_after == 120
    for tracker in ("deepsort", "bytetrack", "ocsort", "botsort"):
        a = cli.parse_arguments(["--input", "a.npy", "--tracker", tracker, "--left_objects"])
        assert a.left_objects and a.left_cell is None and a.left_after is None
    for tracker in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
        a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", tracker, "--left_objects", "--scene_watch"])
        assert a.left_objects and a.scene_watch
    a = cli.parse_arguments(["--input", "a.npy"])
    assert not a.left_objects and a.left_cell is None and a.left_after is None
    for bad in (["--left_cell", "8"], ["--left_after", "50"], ["--left_objects", "--left_cell", "5"], ["--left_objects", "--left_cell", "x"],
                ["--left_objects", "--left_after", "0"], ["--left_objects", "--left_after", "65535"], ["--left_objects", "--left_after", "x"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + bad)


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_left(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._left_objects is None and TP.left_result is None
    stage = type("W", (), dict(streams=3, frame_h=72, frame_w=101))()
    with pytest.raises(ValueError):
        TP.attach_left_objects(type("P", (), dict(streams=2, frame_h=72, frame_w=101))(), stage)
    with pytest.raises(ValueError):
        TP.attach_left_objects(type("P", (), dict(streams=3, frame_h=72, frame_w=100))(), stage)
    fake = type("P", (), dict(streams=3, frame_h=72, frame_w=101))()
    TP.attach_left_objects(fake, stage, cap_events=9)
    assert fake._left_objects is stage and fake.left_result is None and fake.left_cap_events == 9
    TP.attach_left_objects(fake, None)
    assert fake._left_objects is None


def test_new_kernels_have_no_scratch_no_spills_and_no_float():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "left_" in k}
    for name in ("left_occupancy_kernel", "left_model_kernel", "left_blobs_kernel", "left_walk_kernel", "left_events_kernel"):
        assert sum(name in k for k in tab) == 1, (name, sorted(tab))
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in tab.items():
        assert r["vgpr"] + r["agpr"] <= 64 and r["lds"] <= 4 * 1024, (k, r)  # (static LDS; the blob kernel's labels are dynamic, 4 bytes per cell)
    src = open(os.path.join(ROOT, "ai-camera_amd", "csrc", "kernels_left.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|half)\b|\d\.\d*f?\b", code)
