"""The best-shot stage (aic_bestshot_*) without a GPU: the symbols, every rejection that comes before the device
(create, option and reset never touch it; on a machine without a GPU anything that got past an update's checks answers
AIC_ERR_NO_DEVICE instead), the Python class's own checks, the CLI flags, the pipeline hook with nothing attached, and the kernels'
budget."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_bestshot_{f}" for f in ("params", "create", "destroy", "option", "reset", "update", "flush", "export", "counters"))
FIELDS = ("streams", "frame_h", "frame_w", "thumb_w", "thumb_h", "max_tracks", "forget_after", "region", "head_q8", "pad", "min_w", "min_h")


def config(**kw):
    L = pkg("_lib")
    cfg = L.BestShotConfig()
    assert L.load().aic_bestshot_params(2, 72, 101, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_symbols_declared_exported_and_defaults():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert pkg().BestShots is pkg("bestshot").BestShots
    import src.tracker.bestshot as re_export
    assert re_export.BestShots is pkg("bestshot").BestShots
    cfg = config()
    assert [getattr(cfg, f) for f in FIELDS] == [2, 72, 101, 64, 128, 128, 70, 0, 64, 0, 8, 16]
    assert lib.aic_bestshot_params(1, 1, 1, None) == L.ERR_INVALID


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(thumb_w=8), b"thumb_w"), (dict(thumb_w=136), b"thumb_w"), (dict(thumb_w=60), b"thumb_w"), (dict(thumb_h=8), b"thumb_h"),
    (dict(thumb_h=264), b"thumb_h"), (dict(thumb_h=100), b"thumb_h"), (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=513), b"max_tracks"),
    (dict(forget_after=-1), b"forget_after"), (dict(region=2), b"region"), (dict(region=-1), b"region"), (dict(head_q8=0), b"head_q8"),
    (dict(head_q8=257), b"head_q8"), (dict(pad=-1), b"pad"), (dict(pad=65), b"pad"), (dict(min_w=0), b"min_w"), (dict(min_h=0), b"min_w")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_bestshot_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_and_limits():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_bestshot_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_bestshot_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_bestshot_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    big = config(streams=256, frame_h=16384, frame_w=16384, thumb_w=128, thumb_h=256, max_tracks=512, pad=64)      # the largest: no device, no memory yet
    assert lib.aic_bestshot_create(0, C.byref(big), C.byref(h)) == L.OK and h.value
    assert lib.aic_bestshot_destroy(h) == L.OK


@pytest.fixture()
def handle():
    """Two streams of 72 x 101 with 16 x 24 thumbnails: creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(thumb_w=16, thumb_h=24, max_tracks=8)
    assert L.load().aic_bestshot_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_bestshot_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_bestshot_option(None, b"ticks_per_launch", 1) == L.ERR_INVALID
    assert lib.aic_bestshot_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_bestshot_update(None, None, L.HOST, 0, None, None, L.HOST, 4, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_bestshot_flush(None, -1, 4, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_bestshot_export(None, 0, None, None, None) == L.ERR_INVALID
    assert lib.aic_bestshot_destroy(None) == L.OK


def test_option_and_reset_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_bestshot_reset(handle, 0) == L.OK and lib.aic_bestshot_reset(handle, 1) == L.OK
    assert lib.aic_bestshot_reset(handle, 2) == L.ERR_INVALID and lib.aic_bestshot_reset(handle, -1) == L.ERR_INVALID
    for key, good, bad in ((b"ticks_per_launch", (0, 1, 65536), (-1, 65537)), (b"launch_budget_mb", (1, 65536), (0, 65537))):
        assert all(lib.aic_bestshot_option(handle, key, v) == L.OK for v in good)
        assert all(lib.aic_bestshot_option(handle, key, v) == L.ERR_INVALID for v in bad)
    assert lib.aic_bestshot_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_bestshot_option(handle, None, 1) == L.ERR_INVALID
    assert lib.aic_bestshot_option(handle, b"stats", 1) == L.OK and lib.aic_bestshot_option(handle, b"stats", 2) == L.ERR_INVALID
    c = [C.c_int64(5) for _ in range(3)]
    assert lib.aic_bestshot_counters(handle, *(C.byref(x) for x in c)) == L.OK and [x.value for x in c] == [0, 0, 0]
    assert lib.aic_bestshot_counters(handle, None, None, None) == L.OK and lib.aic_bestshot_counters(None, None, None, None) == L.ERR_INVALID
    n, ev, th = C.c_int32(7), np.zeros((8, 16), np.int32), np.zeros((8, 24, 16, 3), np.uint8)
    assert lib.aic_bestshot_export(handle, 0, C.byref(n), L.ptr(ev), L.ptr(th)) == L.OK and n.value == 0      # nothing seen yet: no device
    assert lib.aic_bestshot_export(handle, 2, C.byref(n), L.ptr(ev), L.ptr(th)) == L.ERR_INVALID
    assert lib.aic_bestshot_export(handle, 0, None, L.ptr(ev), L.ptr(th)) == L.ERR_INVALID


def test_update_and_flush_reject_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    nf, ev, th, pend, st = np.zeros(2, np.int32), np.zeros((2, 4, 16), np.int32), np.zeros((2, 4, 24, 16, 3), np.uint8), np.zeros(2, np.int32), np.zeros(2, np.int32)

    def rc(frames=frames, fmem=L.HOST, ticks=1, counts=counts, rows=rows, rmem=L.HOST, cap=4, nf=nf, ev=ev, th=th, pend=pend, st=st):
        return lib.aic_bestshot_update(handle, L.ptr(frames), fmem, ticks, L.ptr(counts), L.ptr(rows), rmem, cap, L.ptr(nf), L.ptr(ev), L.ptr(th),
                                       L.ptr(pend), L.ptr(st))
    for kw in (dict(frames=None), dict(counts=None), dict(rows=None), dict(nf=None), dict(ev=None), dict(th=None), dict(pend=None), dict(fmem=2),
               dict(fmem=-1), dict(rmem=2), dict(rmem=-1), dict(cap=-1), dict(cap=4097), dict(ticks=-1), dict(ticks=65537),
               dict(counts=np.array([1, -1], np.int32))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY and b"512" in lib.aic_last_error()
    for kw in (dict(stream=2), dict(stream=-2), dict(cap=-1), dict(cap=4097), dict(nf=None), dict(pend=None), dict(ev=None), dict(th=None)):
        a = dict(stream=-1, cap=4, nf=nf, ev=ev, th=th, pend=pend)
        a.update(kw)
        assert lib.aic_bestshot_flush(handle, a["stream"], a["cap"], L.ptr(a["nf"]), L.ptr(a["ev"]), L.ptr(a["th"]), L.ptr(a["pend"]), L.ptr(st)) == L.ERR_INVALID, kw
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE; NULL status, no rows, no ticks and cap 0 are fine
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE
        assert rc(st=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, frames=None, counts=None, rows=None) == L.ERR_NO_DEVICE
        assert rc(cap=0, ev=None, th=None) == L.ERR_NO_DEVICE
        assert lib.aic_bestshot_flush(handle, -1, 4, L.ptr(nf), L.ptr(ev), L.ptr(th), L.ptr(pend), None) == L.ERR_NO_DEVICE


def test_python_class_rejections_need_no_device():
    B, L = pkg("bestshot"), pkg("_lib")
    with pytest.raises(ValueError):
        B.BestShots(1, (72, 101), region="feet")
    for kw in (dict(streams=0), dict(streams=257), dict(thumb=(20, 24)), dict(thumb=(16, 20)), dict(thumb=(136, 24)), dict(max_tracks=0)):
        a = dict(streams=2, frame_hw=(72, 101), thumb=(16, 24))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            B.BestShots(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    bs = B.BestShots(2, (72, 101), thumb=(16, 24), max_tracks=8)
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        bs.update(frames[:, :1], [[empty]])                                  # one stream's frames for two
    with pytest.raises(ValueError):
        bs.update(np.zeros((1, 2, 72, 100, 3), np.uint8), [[empty, empty]])
    with pytest.raises(ValueError):
        bs.update(frames, [[empty]])                                         # one row list for two streams
    with pytest.raises(ValueError):
        bs.update(frames, np.zeros((3, 6), np.int32), counts=[2, 2])
    with pytest.raises(ValueError):
        bs.update(frames, np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        bs.update(frames, [[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    ev, th = bs.export(1)
    assert ev.shape == (0, 16) and th.shape == (0, 24, 16, 3)
    bs.reset(1)
    if L.device_count() == 0:
        for call in (lambda: bs.update(frames, [[empty, empty]]), bs.drain, bs.flush, lambda: bs.update_tuples(frames, [[[], []]])):
            with pytest.raises(L.NoDeviceError):
                call()
    bs.close()


def test_ppm_writer(tmp_path):
    B = pkg("bestshot")
    t = np.arange(24 * 16 * 3, dtype=np.uint8).reshape(24, 16, 3)
    B.write_ppm(tmp_path / "a.ppm", t)
    raw = (tmp_path / "a.ppm").read_bytes()
    assert raw.startswith(b"P6\n16 24\n255\n") and raw[len(b"P6\n16 24\n255\n"):] == t[:, :, ::-1].tobytes()


def test_cli_flags():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--best_shots", "shots", "--best_shot_size", "32x64", "--best_shot_region", "head"])
    assert (a.best_shots, a.best_shot_wh, a.best_shot_region) == ("shots", (32, 64), "head")
    a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", "ocsort", "--best_shots", "shots"])
    assert (a.best_shots, a.best_shot_wh, a.best_shot_region) == ("shots", (64, 128), "box")
    assert cli.parse_arguments(["--input", "a.npy"]).best_shots is None
    for bad in (["--best_shot_size", "32x64"], ["--best_shot_region", "head"], ["--best_shots", "d", "--best_shot_size", "32"],
                ["--best_shots", "d", "--best_shot_size", "ax4"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + bad)


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_best_shots(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._best_shots is None and TP.best_shot_result is None
    shots = type("B", (), dict(streams=3, frame_h=72, frame_w=101))()
    with pytest.raises(ValueError):
        TP.attach_best_shots(type("P", (), dict(streams=2, frame_h=72, frame_w=101))(), shots)
    with pytest.raises(ValueError):
        TP.attach_best_shots(type("P", (), dict(streams=3, frame_h=72, frame_w=100))(), shots)
    fake = type("P", (), dict(streams=3, frame_h=72, frame_w=101))()
    TP.attach_best_shots(fake, shots, cap=4)
    assert fake._best_shots is shots and fake.best_shot_cap == 4 and fake.best_shot_result is None
    TP.attach_best_shots(fake, None)
    assert fake._best_shots is None


def test_new_kernels_have_no_scratch_and_no_spills():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "bestshot_" in k}
    for name in ("bestshot_score_kernel", "bestshot_walk_kernel"):
        assert sum(name in k for k in tab) == 1, (name, sorted(tab))
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in tab.items():                                                 # a 512-thread block is 2 waves per SIMD: 256 registers each
        assert r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 40 * 1024, (k, r)
