"""The proximity stage (aic_prox_*) without a GPU: the header's prototypes against the ctypes declarations, every
rejection that comes before the device (create, option, reset and set_ground never touch it; on a machine without a GPU anything that got
past a call's checks answers AIC_ERR_NO_DEVICE instead), csrc/prox_math.hpp in a stand-alone sanitized program against the oracle, the
Python class's own checks, the pipeline hook with nothing attached, the CLI's argument errors, and the kernels' budget."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import prox_oracle as PO
from conftest import ROOT, pkg

NEW = tuple(f"aic_prox_{f}" for f in ("config_default", "create", "destroy", "option", "reset", "set_ground", "update", "flush", "export", "export_pairs"))
FIELDS = ("streams", "frame_h", "frame_w", "max_tracks", "forget_after", "metric", "near", "height_ratio_q8", "link_ticks", "unlink_ticks", "speed_shift",
          "still_speed", "run_speed")


def config(**kw):
    L = pkg("_lib")
    cfg = L.ProxConfig()
    assert L.load().aic_prox_config_default(2, 48, 64, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_prototypes_equal_the_declarations():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    protos = dict(re.findall(r"^int (aic_prox_[a-z0-9_]+)\(([^;]*)\);", hdr, re.M))
    assert set(protos) == set(NEW) == {n for n in L.EXPORTS if n.startswith("aic_prox_")}

    def kind(arg):
        arg = arg.strip()
        return "char*" if arg.startswith("const char*") else "ptr" if "*" in arg else "int"
    want = {C.c_int: "int", C.c_void_p: "ptr", C.c_char_p: "char*"}
    for name, args in protos.items():
        res, sig = L._SIGS[name]
        assert res is C.c_int and [kind(a) for a in args.replace("\n", " ").split(",")] == [want[t] for t in sig], name
        getattr(lib, name)
    M = pkg("proximity")
    assert pkg().Proximity is M.Proximity
    import src.tracker.proximity as re_export
    assert re_export.Proximity is M.Proximity
    cfg = config()
    d = PO.DEFAULTS
    assert tuple(getattr(cfg, f) for f in FIELDS) == (2, 48, 64) + tuple(d[f] for f in FIELDS[3:])
    assert tuple(n for n, _ in L.ProxConfig._fields_) == FIELDS
    assert re.search(r"int32_t " + r",\s+".join(FIELDS) + ";", hdr)                          # the struct in the header, field by field
    assert lib.aic_prox_config_default(1, 1, 1, None) == L.ERR_INVALID
    assert M.METRICS == dict(ground=PO.GROUND, body=PO.BODY) and (M.LINK, M.UNLINK) == (PO.LINK, PO.UNLINK)
    assert set(M.OPTIONS) == set(FIELDS[4:])


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=513), b"max_tracks"), (dict(forget_after=-1), b"forget_after"),
    (dict(forget_after=(1 << 24) + 1), b"forget_after"), (dict(metric=2), b"metric"), (dict(metric=-1), b"metric"), (dict(near=0), b"near"),
    (dict(near=4097), b"near"), (dict(metric=0, near=(1 << 24) + 1), b"near"), (dict(height_ratio_q8=255), b"height_ratio_q8"),
    (dict(height_ratio_q8=65537), b"height_ratio_q8"), (dict(link_ticks=0), b"link_ticks"), (dict(link_ticks=32768), b"link_ticks"),
    (dict(unlink_ticks=0), b"unlink_ticks"), (dict(unlink_ticks=32768), b"unlink_ticks"), (dict(speed_shift=-1), b"speed_shift"),
    (dict(speed_shift=13), b"speed_shift"), (dict(still_speed=-1), b"still_speed"), (dict(run_speed=(1 << 20) + 1), b"run_speed"),
    (dict(still_speed=71), b"still_speed")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_prox_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_and_the_largest():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_prox_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_prox_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_prox_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    big = config(streams=256, frame_h=16384, frame_w=16384, max_tracks=512, metric=0, near=1 << 24, link_ticks=32767, unlink_ticks=32767,
                 speed_shift=12, still_speed=1 << 20, run_speed=1 << 20, height_ratio_q8=1 << 16, forget_after=1 << 24)
    assert lib.aic_prox_create(0, C.byref(big), C.byref(h)) == L.OK and h.value             # no device, no memory yet
    assert lib.aic_prox_destroy(h) == L.OK


@pytest.fixture()
def handle():
    """Two streams of 48 x 64: creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(max_tracks=8)
    assert L.load().aic_prox_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_prox_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    H = np.array(PO.IDENTITY, np.int32)
    assert lib.aic_prox_option(None, b"near", 1) == L.ERR_INVALID and lib.aic_prox_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_prox_set_ground(None, 0, L.ptr(H), 0) == L.ERR_INVALID
    assert lib.aic_prox_update(None, 0, None, None, L.HOST, 4, 4, None, None, None, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_prox_flush(None, -1, 4, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_prox_export(None, 0, None, None) == L.ERR_INVALID and lib.aic_prox_export_pairs(None, 0, None, None) == L.ERR_INVALID
    assert lib.aic_prox_destroy(None) == L.OK


def test_options_reset_and_set_ground_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_prox_reset(handle, 0) == L.OK and lib.aic_prox_reset(handle, 1) == L.OK
    assert lib.aic_prox_reset(handle, 2) == L.ERR_INVALID and lib.aic_prox_reset(handle, -1) == L.ERR_INVALID
    for key, good, bad in ((b"forget_after", (0, 70, 1 << 24), (-1, (1 << 24) + 1)), (b"height_ratio_q8", (256, 1 << 16), (255, (1 << 16) + 1)),
                           (b"link_ticks", (1, 32767), (0, 32768)), (b"unlink_ticks", (1, 32767), (0, 32768)), (b"speed_shift", (0, 12), (-1, 13)),
                           (b"run_speed", (1 << 20, 70), (-1, (1 << 20) + 1, 4)), (b"still_speed", (0, 70), (-1, 71)), (b"near", (1, 4096), (0, 4097)),
                           (b"ticks_per_launch", (0, 1, 65536), (-1, 65537)), (b"launch_budget_mb", (1, 65536), (0, 65537))):
        assert all(lib.aic_prox_option(handle, key, v) == L.OK for v in good), key
        for v in bad:
            assert lib.aic_prox_option(handle, key, v) == L.ERR_INVALID, (key, v)
    # near's range follows the metric, in either order of the two options
    assert lib.aic_prox_option(handle, b"metric", 2) == L.ERR_INVALID and lib.aic_prox_option(handle, b"metric", 0) == L.OK
    assert lib.aic_prox_option(handle, b"near", 1 << 24) == L.OK and lib.aic_prox_option(handle, b"near", (1 << 24) + 1) == L.ERR_INVALID
    assert lib.aic_prox_option(handle, b"metric", 1) == L.ERR_INVALID and b"near" in lib.aic_last_error()      # 2^24 per mille is no body metric
    assert lib.aic_prox_option(handle, b"near", 700) == L.OK and lib.aic_prox_option(handle, b"metric", 1) == L.OK
    assert lib.aic_prox_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_prox_option(handle, None, 1) == L.ERR_INVALID
    H = np.array(PO.IDENTITY, np.int32)
    for stream, shift, ok in ((0, 0, True), (1, 14, True), (-1, 3, True), (2, 0, False), (-2, 0, False), (0, -1, False), (0, 15, False)):
        assert (lib.aic_prox_set_ground(handle, stream, L.ptr(H), shift) == L.OK) == ok, (stream, shift)
    assert lib.aic_prox_set_ground(handle, 0, None, 0) == L.ERR_INVALID
    for k in range(9):
        for v, ok in ((1 << 30, True), (-(1 << 30), True), ((1 << 30) + 1, False), (-(1 << 30) - 1, False)):
            Hk = H.copy()
            Hk[k] = v
            assert (lib.aic_prox_set_ground(handle, 0, L.ptr(Hk), 0) == L.OK) == ok, (k, v)
    n, ev, pairs = C.c_int32(7), np.zeros((8, 16), np.int32), np.zeros((28, 6), np.int32)
    assert lib.aic_prox_export(handle, 0, C.byref(n), L.ptr(ev)) == L.OK and n.value == 0         # nothing seen yet: no device
    n = C.c_int32(7)
    assert lib.aic_prox_export_pairs(handle, 1, C.byref(n), L.ptr(pairs)) == L.OK and n.value == 0
    for f, buf in ((lib.aic_prox_export, ev), (lib.aic_prox_export_pairs, pairs)):
        assert f(handle, 2, C.byref(n), L.ptr(buf)) == L.ERR_INVALID and f(handle, -1, C.byref(n), L.ptr(buf)) == L.ERR_INVALID
        assert f(handle, 0, None, L.ptr(buf)) == L.ERR_INVALID and f(handle, 0, C.byref(n), None) == L.ERR_INVALID


def test_every_call_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    nf, ev, pend, st = np.zeros(2, np.int32), np.zeros((2, 4, 16), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    recs, tags, npe, pe = np.zeros((2, 16), np.int32), np.zeros((1, 8), np.int32), np.zeros(2, np.int32), np.zeros((2, 4, 8), np.int32)

    def rc(ticks=1, counts=counts, rows=rows, rmem=L.HOST, cap=4, cap_pairs=4, nf=nf, ev=ev, pend=pend, st=st, recs=recs, tags=tags, npe=npe, pe=pe):
        return lib.aic_prox_update(handle, ticks, L.ptr(counts), L.ptr(rows), rmem, cap, cap_pairs, L.ptr(nf), L.ptr(ev), L.ptr(pend), L.ptr(st),
                                   L.ptr(recs), L.ptr(tags), L.ptr(npe), L.ptr(pe))
    for kw in (dict(counts=None), dict(rows=None), dict(nf=None), dict(ev=None), dict(pend=None), dict(recs=None), dict(tags=None), dict(npe=None),
               dict(pe=None), dict(rmem=2), dict(rmem=-1), dict(cap=-1), dict(cap=4097), dict(cap_pairs=-1), dict(cap_pairs=4097), dict(ticks=-1),
               dict(ticks=65537), dict(counts=np.array([1, -1], np.int32))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY and b"512" in lib.aic_last_error()
    for kw in (dict(stream=2), dict(stream=-2), dict(cap=-1), dict(cap=4097), dict(nf=None), dict(pend=None), dict(ev=None)):
        a = dict(stream=-1, cap=4, nf=nf, ev=ev, pend=pend)
        a.update(kw)
        assert lib.aic_prox_flush(handle, a["stream"], a["cap"], L.ptr(a["nf"]), L.ptr(a["ev"]), L.ptr(a["pend"]), L.ptr(st)) == L.ERR_INVALID, kw
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE and rc(st=None) == L.ERR_NO_DEVICE and rc(cap_pairs=0, pe=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None, tags=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, counts=None, rows=None, recs=None, tags=None, npe=None, pe=None) == L.ERR_NO_DEVICE and rc(cap=0, ev=None) == L.ERR_NO_DEVICE
        assert lib.aic_prox_flush(handle, -1, 4, L.ptr(nf), L.ptr(ev), L.ptr(pend), None) == L.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------- prox_math.hpp, stand-alone
@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the proximity host test builds tests/prox_probe.cpp with the system compiler")
    exe = str(tmp_path_factory.mktemp("prox") / "prox_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "prox_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def lines(printed, key):
    return [ln[len(key) + 1:] for ln in printed if ln.startswith(key + " ") or ln == key]


def test_probe_isqrt_floor_division_and_placement_equal_the_oracle(printed):
    (isq,) = lines(printed, "isq")
    pairs = [tuple(int(x) for x in t.split(":")) for t in isq.split()]
    assert len(pairs) > 500 and {p[0] for p in pairs} >= {0, 1, (1 << 61) - 1, 1 << 61, (1 << 61) + 1, (1 << 30) ** 2 - 1}
    for v, r in pairs:
        assert r == PO.isqrt(v), v
    (fdiv,) = lines(printed, "fdiv")
    trip = [tuple(int(x) for x in t.split(":")) for t in fdiv.split()]
    assert len(trip) == 66 and any(a < 0 and a % b for a, b, _ in trip)
    for a, b, q in trip:
        assert q == a // b, (a, b)
    maps = [((1024, 0, 0, 0, 1024, 0, 0, -1, 40), 14), ((2, 0, 0, 0, 2, 0, 0, 0, 1), 0), ((-(1 << 30), 1 << 30, 12345, 7, -9, 1 << 30, 3, 5, -100), 3)]
    seen = set()
    for ln in lines(printed, "plc"):
        m, *rest = ln.split()
        H, shift = maps[int(m)]
        for t in rest:
            fx, fy, ok, gx, gy = (int(x) for x in t.split(":"))
            assert (bool(ok), gx, gy) == PO.place(PO.GROUND, H, shift, fx, fy), (m, fx, fy)
            seen.add((int(m), ok))
    assert seen == {(0, 0), (0, 1), (1, 1), (2, 0)}                               # (the third map's quotients all lie beyond 2^24 or behind it)


def test_probe_near_distance_speed_and_judgement_equal_the_oracle(printed):
    for metric in (0, 1):
        (near,) = lines(printed, f"near {metric}")
        want = [int(PO.near_rule(metric, 13 if metric == 0 else 700, 384, (0, 0, ha), (dx, dy, hb)))
                for ha in (10, 20, 30, 31) for hb in (20, 30) for dx in range(-30, 31) for dy in (0, 5, 12, 13, 14)]
        assert [int(x) for x in near.split()] == want and 0 < sum(want) < len(want)
        (dst,) = lines(printed, f"dst {metric}")
        for t in dst.split():
            ha, dx, dy, d = (int(x) for x in t.split(":"))
            assert d == PO.distance(metric, (0, 0, ha), (dx, dy, 20)), t
        (mov,) = lines(printed, f"mov {metric}")
        for t in mov.split():
            hc, dx, dy, d = (int(x) for x in t.split(":"))
            assert d == PO.moved(metric, dx, dy, hc), t
    seq = ((100, 1), (0, 1), (7, 2), (1 << 25, 1), (1 << 30, 1), (0, 1), (0, 3), (5, 1), (1000, 7), (0, 1), (0, 1), (0, 1))
    for shift in (0, 1, 2, 12):
        (spd,) = lines(printed, f"spd {shift}")
        v, gait, want = 0, 0, []
        for mv, dt in seq:
            speed = min(mv // dt, PO.SPEED_MAX)
            v = speed << 8 if gait == 0 else v + (((speed << 8) - v) >> shift)
            gait = PO.gait_of(v, 5, 70)
            want.append(f"{v}:{gait}")
        assert spd.split() == want and max(int(t.split(":")[0]) for t in want) <= PO.SAT
    (jdg,) = lines(printed, "jdg")
    e, want = [0, 0, 0, 0], []
    for f, c in enumerate("1101110100111001"):
        kind = 0
        if c == "1":
            e[1], e[2] = min(e[1] + 1, PO.ON_MAX), 0
            if not e[0] and e[1] >= 3:
                e[0], e[3], kind = 1, f, PO.LINK
        else:
            e[2], e[1] = min(e[2] + 1, PO.ON_MAX), 0
            if e[0] and e[2] >= 2:
                e[0], kind = 0, PO.UNLINK
        want.append(f"{kind}:{e[0]}:{e[1]}:{e[2]}:{e[3]}")
    got = jdg.split()
    assert got[:16] == want and {t.split(":")[0] for t in want} == {"0", "1", "2"}
    assert [t.split(":")[1:4] for t in got[16:19]] == [["1", "32767", "0"]] * 3 and [t.split(":")[1:4] for t in got[19:]] == [["0", "0", "32767"]] * 3
    (idx,) = lines(printed, "idx")
    assert idx.split() == ["2:1", "3:1", "128:1", "512:1"]


# ---------------------------------------------------------------------------------------------------- the Python class
def test_python_class_needs_no_device_until_a_call_that_computes():
    M, L = pkg("proximity"), pkg("_lib")
    for kw in (dict(streams=0), dict(streams=257), dict(max_tracks=0), dict(max_tracks=513), dict(near=0), dict(near=4097), dict(forget_after=-1),
               dict(frame_hw=(0, 64)), dict(link_ticks=0), dict(still_speed=80)):
        a = dict(streams=2, frame_hw=(48, 64))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            M.Proximity(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    with pytest.raises(ValueError):
        M.Proximity(2, (48, 64), metric="feet")
    with pytest.raises(ValueError):
        M.Proximity(2, (48, 64), metric="ground")                           # near is in ground units: there is no default
    px = M.Proximity(2, (48, 64), max_tracks=8)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        px.update([[empty]])                                                 # one row list for two streams
    with pytest.raises(ValueError):
        px.update(np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        px.update([[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    with pytest.raises(ValueError):
        px.set_ground([1, 0, 0, 0, 1, 0, 0, 0])
    with pytest.raises(ValueError):
        px.set_ground([1 << 31, 0, 0, 0, 1, 0, 0, 0, 1])
    with pytest.raises(ValueError):
        px.option("metric", "feet")
    px.set_ground(PO.IDENTITY), px.set_ground([2, 0, 0, 0, 2, 0, 0, 0, 1], 3, stream=1), px.option("link_ticks", 5), px.option("ticks_per_launch", 3)
    px.option("metric", "ground"), px.option("near", 100000), px.reset(1)
    assert px.export(1).shape == (0, 16) and px.export_pairs(0).shape == (0, 6)
    with pytest.raises(L.AicError):
        px.reset(2)
    if L.device_count() == 0:
        for call in (lambda: px.update([[empty, empty]]), px.drain, px.flush, lambda: px.update_tuples([[[], []]])):
            with pytest.raises(L.NoDeviceError):
                call()
    px.close()


def test_result_slices_parties_and_pairs():
    M = pkg("proximity")
    tags = np.array([[20, 20, -1, 0, 3, 2, 1, 31], [0, 0, -1, 0, -1, 0, 0, 1], [24, 20, 512, 2, 3, 2, 1, 15], [90, 80, -1, 0, 9, 1, 0, 31],
                     [10, 10, -1, 0, 5, 1, 0, 31]], np.int32)
    pe = np.zeros((2, 1, 2, 8), np.int32)
    pe[1, 0, 0] = M.LINK, 1, 3, 7, 0, 300, 2, 0
    pe[1, 0, 1] = M.UNLINK, 1, 5, 9, 4, 1250, 2, 0                           # three events, room for two
    recs = np.zeros((2, 1, 16), np.int32)
    recs[0, 0, :10] = 0, 3, 3, 1, 2, 1, 1, 1, 2, 2
    res = M.ProximityResult(np.zeros(1, np.int32), np.zeros((1, 2, 16), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32), recs, tags,
                            np.array([[0], [3]], np.int32), pe, {}, np.array([[4], [1]], np.int32), np.array([7, 7, 3, 9, 5], np.int32))
    assert res.parties(0, 0) == [[3, 7], [9]] and res.parties(1, 0) == [[5]]
    assert res.tags(1, 0).tolist() == [tags[4].tolist()] and res.record(0, 0)["n_units"] == 2 and res.record(0, 0)["largest_party"] == 2
    assert res.pairs() == [dict(kind="link", frame=1, ids=(3, 7), duration=0, distance=300, ticks=2, stream=0),
                           dict(kind="unlink", frame=1, ids=(5, 9), duration=4, distance=1250, ticks=2, stream=0)]
    assert res.pairs(0, 0) == [] and res.ended() == []


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_proximity(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._prox is None and TP.proximity_result is None
    stage = type("W", (), dict(streams=3, frame_h=48, frame_w=64))()
    with pytest.raises(ValueError):
        TP.attach_proximity(type("P", (), dict(streams=2, frame_h=48, frame_w=64))(), stage)
    with pytest.raises(ValueError):
        TP.attach_proximity(type("P", (), dict(streams=3, frame_h=48, frame_w=60))(), stage)
    fake = type("P", (), dict(streams=3, frame_h=48, frame_w=64))()
    TP.attach_proximity(fake, stage, cap=9, cap_pairs=5)
    assert fake._prox is stage and fake.proximity_result is None and (fake.proximity_cap, fake.proximity_cap_pairs) == (9, 5)
    TP.attach_proximity(fake, None)
    assert fake._prox is None


# ---------------------------------------------------------------------------------------------------- the kernels' budget
RECORDED = {  # DESIGN.md sections 48, 49 and the stages' own sections: (VGPRs, static LDS bytes); scratch and spills 0 everywhere
    "colours_sample_kernel": (35, 1236), "colours_walk_kernel": (76, 20512), "bestshot_score_kernel": (36, 32), "bestshot_walk_kernel": (71, 32800),
    "zones_classify_kernel": (18, 8448), "zones_walk_kernel": (92, 27168), "scene_model_kernel": (16, 0), "scene_stats_kernel": (29, 2624),
    "scene_rows_kernel": (36, 0), "scene_walk_kernel": (48, 0), "scene_gray_kernel<4, 1>": (16, 768), "scene_gray_kernel<8, 1>": (28, 768),
    "scene_gray_kernel<16, 1>": (52, 768), "scene_gray_kernel<4, 4>": (29, 3072), "scene_gray_kernel<8, 4>": (44, 3072),
    "scene_gray_kernel<16, 4>": (62, 3072), "left_occupancy_kernel": (20, 0), "left_model_kernel": (26, 0), "left_blobs_kernel": (32, 3600),
    "left_walk_kernel": (64, 0), "left_events_kernel": (29, 0), "heat_walk_kernel": (77, 40992)}


def test_prox_kernel_has_no_scratch_and_the_other_stages_keep_their_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so")
    prox = {k: r for k, r in table.items() if re.search(r"\d+prox_[a-z]+_kernel", k)}
    assert len(prox) == 1 and "16prox_walk_kernel" in next(iter(prox)), sorted(prox)
    (r,) = prox.values()
    assert not r["scratch"] and not r["vgpr_spills"] and not r.get("sgpr_spills", 0), r
    assert r["vgpr"] + r["agpr"] <= 128, r                                   # a 512-thread block is 2 waves per SIMD: 256 registers each
    assert 64 * 1024 < r["lds"] <= 160 * 1024, r                             # two bit matrices of 32 KiB and the tables: one block per CU
    others = {k: r for k, r in table.items() if re.search(r"\d+(colours|bestshot|zones|scene|left)_[a-z]+_kernel|\d+heat_walk_kernel", k)}
    assert len(others) == len(RECORDED), sorted(others)
    for name, (vgpr, lds) in RECORDED.items():                               # the symbols as the compiler mangles them: <length><name>[I Li<n>E .. E]
        base, _, targs = name.partition("<")
        want = f"{len(base)}{base}" + ("I" + "".join(f"Li{int(t)}E" for t in targs.rstrip(">").split(",")) + "E" if targs else "E")
        hit = [r for k, r in others.items() if want in k]
        assert len(hit) == 1, (name, want, sorted(others))
        r = hit[0]
        assert (r["vgpr"], r["lds"], r["scratch"], r["vgpr_spills"], r["agpr"]) == (vgpr, lds, 0, 0, 0), (name, r)


def test_prox_kernel_source_has_no_floating_point():
    src = open(os.path.join(ROOT, "ai-camera_amd", "csrc", "kernels_prox.hip")).read() + open(os.path.join(ROOT, "ai-camera_amd", "csrc", "prox_math.hpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|half|__half|sqrtf?|rsqrtf?)\b", code)


def test_cli_flags_and_the_parser_errors():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--proximity", "--ground", "g.json", "--near", "1500", "--proximity_file", "p.jsonl"])
    assert (a.proximity, a.ground, a.near, a.proximity_file) == (True, "g.json", 1500, "p.jsonl")
    for tracker in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
        a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", tracker, "--proximity", "--near", "900", "--heat_maps", "maps"])
        assert a.proximity and a.near == 900 and a.ground is None and a.proximity_file is None
    a = cli.parse_arguments(["--input", "a.npy"])
    assert not a.proximity and a.ground is None and a.near is None and a.proximity_file is None
    for flags in (["--ground", "g.json"], ["--near", "700"], ["--proximity_file", "p.jsonl"], ["--proximity", "--near", "0"],
                  ["--proximity", "--near", "4097"], ["--proximity", "--ground", "g.json"], ["--proximity", "--ground", "g.json", "--near", str((1 << 24) + 1)]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + flags)
