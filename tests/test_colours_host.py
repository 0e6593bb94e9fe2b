"""The clothing-colour stage (aic_colours_*) without a GPU: the symbols, every rejection that comes before the
device (create, option and reset never touch it; on a machine without a GPU anything that got past an update's checks answers
AIC_ERR_NO_DEVICE instead), the host's copy of the pixel rule against the oracle, the Python class's own checks, finals / matches, the
CLI flags, the pipeline hook with nothing attached, and the kernels' budget."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import colours_cases as CC
import colours_oracle as CO
from conftest import ROOT, pkg

NEW = tuple(f"aic_colours_{f}" for f in ("config_default", "create", "destroy", "option", "reset", "update", "flush", "export", "classify"))
FIELDS = ("streams", "frame_h", "frame_w", "max_tracks", "forget_after", "torso0", "torso1", "legs0", "legs1", "inset_q8", "min_w", "min_h", "max_cover_q8")


def config(**kw):
    L = pkg("_lib")
    cfg = L.ColoursConfig()
    assert L.load().aic_colours_config_default(2, 72, 101, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_symbols_declared_exported_and_defaults():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    assert set(re.findall(r"\b(aic_colours_[a-z0-9_]+)\s*\(", hdr)) == set(NEW) == {n for n in L.EXPORTS if n.startswith("aic_colours_")}
    for name in NEW:
        getattr(lib, name)
    assert lib.aic_abi_version() == 2
    assert pkg().TrackColours is pkg("colours").TrackColours
    import src.tracker.colours as re_export
    assert re_export.TrackColours is pkg("colours").TrackColours
    cfg = config()
    assert tuple(getattr(cfg, f) for f in FIELDS) == (2, 72, 101, 128, 70, 51, 128, 141, 230, 64, 4, 4, 64)
    assert tuple(n for n, _ in L.ColoursConfig._fields_) == FIELDS
    assert lib.aic_colours_config_default(1, 1, 1, None) == L.ERR_INVALID
    M = pkg("colours")
    assert (M.NAMES, M.EVENT_FIELDS, (M.LIVE, M.EXPIRED, M.FLUSHED)) == (CO.NAMES, CO.EVENT_FIELDS, (CO.LIVE, CO.EXPIRED, CO.FLUSHED))


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=513), b"max_tracks"), (dict(forget_after=-1), b"forget_after"),
    (dict(torso0=-1), b"torso_q8"), (dict(torso0=128), b"torso_q8"), (dict(torso1=257), b"torso_q8"), (dict(legs0=230), b"legs_q8"),
    (dict(legs1=257), b"legs_q8"), (dict(legs0=-1), b"legs_q8"), (dict(inset_q8=128), b"inset_q8"), (dict(inset_q8=-1), b"inset_q8"),
    (dict(min_w=0), b"min_w"), (dict(min_h=16385), b"min_h"), (dict(max_cover_q8=-1), b"max_cover_q8"), (dict(max_cover_q8=257), b"max_cover_q8")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_colours_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_and_the_largest():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_colours_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_colours_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_colours_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    big = config(streams=256, frame_h=16384, frame_w=16384, max_tracks=512, torso0=0, torso1=256, legs0=0, legs1=256, inset_q8=127, max_cover_q8=256)
    assert lib.aic_colours_create(0, C.byref(big), C.byref(h)) == L.OK and h.value      # the largest: no device, no memory yet
    assert lib.aic_colours_destroy(h) == L.OK


@pytest.fixture()
def handle():
    """Two streams of 72 x 101: creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(max_tracks=8)
    assert L.load().aic_colours_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_colours_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_colours_option(None, b"ticks_per_launch", 1) == L.ERR_INVALID
    assert lib.aic_colours_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_colours_update(None, None, L.HOST, 0, None, None, L.HOST, 4, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_colours_flush(None, -1, 4, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_colours_export(None, 0, None, None) == L.ERR_INVALID
    assert lib.aic_colours_destroy(None) == L.OK


def test_option_ranges_and_reset_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_colours_reset(handle, 0) == L.OK and lib.aic_colours_reset(handle, 1) == L.OK
    assert lib.aic_colours_reset(handle, 2) == L.ERR_INVALID and lib.aic_colours_reset(handle, -1) == L.ERR_INVALID
    for key, good, bad in ((b"ticks_per_launch", (0, 1, 65536), (-1, 65537)), (b"launch_budget_mb", (1, 65536), (0, 65537))):
        assert all(lib.aic_colours_option(handle, key, v) == L.OK for v in good)
        for v in bad:
            assert lib.aic_colours_option(handle, key, v) == L.ERR_INVALID and key in lib.aic_last_error()
    assert lib.aic_colours_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_colours_option(handle, None, 1) == L.ERR_INVALID
    n, ev = C.c_int32(7), np.zeros((8, 48), np.int32)
    assert lib.aic_colours_export(handle, 0, C.byref(n), L.ptr(ev)) == L.OK and n.value == 0      # nothing seen yet: no device
    assert lib.aic_colours_export(handle, 2, C.byref(n), L.ptr(ev)) == L.ERR_INVALID
    assert lib.aic_colours_export(handle, 0, None, L.ptr(ev)) == L.ERR_INVALID and lib.aic_colours_export(handle, 0, C.byref(n), None) == L.ERR_INVALID


def test_update_and_flush_reject_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    nf, ev, tags, pend, st = np.zeros(2, np.int32), np.zeros((2, 4, 48), np.int32), np.zeros((1, 4), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)

    def rc(frames=frames, fmem=L.HOST, ticks=1, counts=counts, rows=rows, rmem=L.HOST, cap=4, nf=nf, ev=ev, tags=tags, pend=pend, st=st):
        return lib.aic_colours_update(handle, L.ptr(frames), fmem, ticks, L.ptr(counts), L.ptr(rows), rmem, cap, L.ptr(nf), L.ptr(ev), L.ptr(tags),
                                      L.ptr(pend), L.ptr(st))
    for kw in (dict(frames=None), dict(counts=None), dict(rows=None), dict(nf=None), dict(ev=None), dict(pend=None), dict(fmem=2), dict(fmem=-1),
               dict(rmem=2), dict(rmem=-1), dict(cap=-1), dict(cap=4097), dict(ticks=-1), dict(ticks=65537), dict(counts=np.array([1, -1], np.int32))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY and b"512" in lib.aic_last_error()
    for kw in (dict(stream=2), dict(stream=-2), dict(cap=-1), dict(cap=4097), dict(nf=None), dict(pend=None), dict(ev=None)):
        a = dict(stream=-1, cap=4, nf=nf, ev=ev, pend=pend)
        a.update(kw)
        assert lib.aic_colours_flush(handle, a["stream"], a["cap"], L.ptr(a["nf"]), L.ptr(a["ev"]), L.ptr(a["pend"]), L.ptr(st)) == L.ERR_INVALID, kw
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE; NULL status and row_tags, no rows, no ticks and cap 0 are fine
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE
        assert rc(st=None, tags=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, frames=None, counts=None, rows=None) == L.ERR_NO_DEVICE
        assert rc(cap=0, ev=None) == L.ERR_NO_DEVICE
        assert lib.aic_colours_flush(handle, -1, 4, L.ptr(nf), L.ptr(ev), L.ptr(pend), None) == L.ERR_NO_DEVICE


def test_classify_equals_the_oracle():
    M, L = pkg("colours"), pkg("_lib")
    px = np.concatenate([np.random.default_rng(45).integers(0, 256, (1 << 16, 3)).astype(np.uint8), CC.threshold_set(),
                         np.array([p for ps in CC.PALETTE.values() for p in ps], np.uint8)])
    got = M.classify(px)
    assert got.dtype == np.uint8 and np.array_equal(got, CO.classify(px))
    assert set(got.tolist()) == set(range(12))
    assert M.classify(px.reshape(-1, 3)[:6].reshape(2, 3, 3)).shape == (2, 3) and M.classify(np.zeros((0, 3), np.uint8)).shape == (0,)
    lib = L.load()
    assert lib.aic_colours_classify(None, 1, None) == L.ERR_INVALID and lib.aic_colours_classify(None, -1, None) == L.ERR_INVALID
    assert lib.aic_colours_classify(None, 0, None) == L.OK
    with pytest.raises(ValueError):
        M.classify(np.zeros((4, 4), np.uint8))


def test_python_class_needs_no_device_until_update():
    M, L = pkg("colours"), pkg("_lib")
    for kw in (dict(streams=0), dict(streams=257), dict(max_tracks=0), dict(max_tracks=513), dict(torso_q8=(128, 51)), dict(legs_q8=(0, 257)),
               dict(inset_q8=128), dict(min_w=0), dict(max_cover_q8=257), dict(forget_after=-1), dict(frame_hw=(0, 101))):
        a = dict(streams=2, frame_hw=(72, 101))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            M.TrackColours(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    tc = M.TrackColours(2, (72, 101), max_tracks=8)
    frames = np.zeros((1, 2, 72, 101, 3), np.uint8)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        tc.update(frames[:, :1], [[empty]])                                  # one stream's frames for two
    with pytest.raises(ValueError):
        tc.update(np.zeros((1, 2, 72, 100, 3), np.uint8), [[empty, empty]])
    with pytest.raises(ValueError):
        tc.update(frames, [[empty]])                                         # one row list for two streams
    with pytest.raises(ValueError):
        tc.update(frames, np.zeros((3, 6), np.int32), counts=[2, 2])
    with pytest.raises(ValueError):
        tc.update(frames, np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        tc.update(frames, [[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    assert tc.export(1).shape == (0, 48)
    tc.option("ticks_per_launch", 3), tc.reset(1)
    with pytest.raises(L.AicError):
        tc.reset(2)
    if L.device_count() == 0:
        for call in (lambda: tc.update(frames, [[empty, empty]]), tc.drain, tc.flush, lambda: tc.update_tuples(frames, [[[], []]])):
            with pytest.raises(L.NoDeviceError):
                call()
    tc.close()


def test_finals_and_matches():
    M = pkg("colours")
    ev = np.zeros((2, 3, 48), np.int32)
    ev[1, 0, :14] = M.EXPIRED, 1, 7, 0, 3, 40, 30, 20, 18, CO.RED, CO.BLACK, CO.BLUE, -1, 5
    ev[1, 0, 16 + CO.RED], ev[1, 0, 16 + CO.BLACK], ev[1, 0, 16 + CO.WHITE] = 170, 60, 26
    ev[1, 0, 28 + CO.BLUE] = 250
    ev[0, 0, :14] = M.FLUSHED, 0, 9, -1, 0, 2, 3, 0, 0, -1, -1, -1, -1, 0
    res = M.ColourResult(np.array([1, 1], np.int32), ev, np.zeros((0, 4), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), {})
    f = M.finals(res)
    assert [e["id"] for e in f] == [9, 7] and f[0]["upper"] is None and f[0]["lower"] is None and f[0]["hist_upper"] == [0] * 12
    e = f[1]
    assert (e["upper"], e["upper_second"], e["lower"], e["lower_second"], e["slot"], e["samples_lower"]) == ("red", "black", "blue", None, 5, 18)
    assert M.matches(e, upper="red") and M.matches(e, upper="red", lower="blue") and M.matches(e, lower=("black", "blue")) and M.matches(e)
    assert not M.matches(e, upper="black")                                   # the second bin holds 60 < 64 ...
    assert M.matches(e, upper="black", min_share_q8=60) and M.matches(e, upper=("green", "black"), min_share_q8=60)      # ... and counts from 60 on
    assert not M.matches(e, upper="white", min_share_q8=1)                   # neither top nor second
    assert not M.matches(e, upper="red", lower="red") and not M.matches(e, upper="red", min_share_q8=171)
    assert not M.matches(f[0], upper="red") and M.matches(f[0])
    assert M.matches(ev[1, 0], upper="red")                                  # the 48 ints as they come
    with pytest.raises(ValueError):
        M.matches(e, upper="mauve")
    assert M.name_of(-1) is None and M.name_of(11) == "brown"


def test_cli_flags_and_the_parser_error():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--colours", "--colours_file", "worn.jsonl"])
    assert a.colours and a.colours_file == "worn.jsonl"
    for tracker in ("deepsort", "bytetrack", "ocsort", "botsort"):
        a = cli.parse_arguments(["--input", "a.npy", "--tracker", tracker, "--colours"])
        assert a.colours and a.colours_file is None
    for tracker in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
        a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", tracker, "--colours", "--scene_watch", "--colours_file", "w.jsonl"])
        assert a.colours and a.scene_watch and a.colours_file == "w.jsonl"
    a = cli.parse_arguments(["--input", "a.npy"])
    assert not a.colours and a.colours_file is None
    with pytest.raises(SystemExit):
        cli.parse_arguments(["--input", "a.npy", "--colours_file", "worn.jsonl"])


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_colours(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._colours is None and TP.colour_result is None
    stage = type("W", (), dict(streams=3, frame_h=72, frame_w=101))()
    with pytest.raises(ValueError):
        TP.attach_colours(type("P", (), dict(streams=2, frame_h=72, frame_w=101))(), stage)
    with pytest.raises(ValueError):
        TP.attach_colours(type("P", (), dict(streams=3, frame_h=72, frame_w=100))(), stage)
    fake = type("P", (), dict(streams=3, frame_h=72, frame_w=101))()
    TP.attach_colours(fake, stage, cap=9)
    assert fake._colours is stage and fake.colour_result is None and fake.colour_cap == 9
    TP.attach_colours(fake, None)
    assert fake._colours is None


def test_new_kernels_have_no_scratch_no_spills_and_no_float():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "colours_" in k}
    for name in ("colours_sample_kernel", "colours_walk_kernel"):
        assert sum(name in k for k in tab) == 1, (name, sorted(tab))
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in tab.items():                                                 # a 512-thread block is 2 waves per SIMD: 256 registers each
        assert r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 24 * 1024, (k, r)
    for f in ("kernels_colours.hip", "colours.hpp"):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "ai-camera_amd", "csrc", f)).read())
        assert not re.search(r"\b(float|double|half)\b|\d\.\d*f?\b", code), f
