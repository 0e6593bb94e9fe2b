"""The heat-map stage (aic_heat_*) without a GPU: the header's prototypes against the ctypes declarations, every
rejection that comes before the device (create, option, reset, set_lut and the import's range check never touch it; on a machine without
a GPU anything that got past a call's checks answers AIC_ERR_NO_DEVICE instead), csrc/heat_math.hpp in a stand-alone sanitized program
against the oracle, the Python class's own checks, the pipeline hook with nothing attached, and the kernels' budget."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import heat_oracle as HO
from conftest import ROOT, pkg

NEW = tuple(f"aic_heat_{f}" for f in ("config_default", "create", "destroy", "option", "reset", "update", "flush", "export", "decay", "export_layers",
                                      "import_layers", "set_lut", "lut", "render"))
FIELDS = ("streams", "frame_h", "frame_w", "cell", "max_tracks", "forget_after", "anchor", "min_move")


def config(**kw):
    L = pkg("_lib")
    cfg = L.HeatConfig()
    assert L.load().aic_heat_config_default(2, 37, 61, C.byref(cfg)) == L.OK
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_header_prototypes_equal_the_declarations():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    protos = dict(re.findall(r"^int (aic_heat_[a-z0-9_]+)\(([^;]*)\);", hdr, re.M))
    assert set(protos) == set(NEW) == {n for n in L.EXPORTS if n.startswith("aic_heat_")}

    def kind(arg):
        arg = arg.strip()
        return "char*" if arg.startswith("const char*") else "ptr" if "*" in arg else "int"
    want = {C.c_int: "int", C.c_void_p: "ptr", C.c_char_p: "char*"}
    for name, args in protos.items():
        res, sig = L._SIGS[name]
        assert res is C.c_int and [kind(a) for a in args.replace("\n", " ").split(",")] == [want[t] for t in sig], name
        getattr(lib, name)
    M = pkg("heatmap")
    assert pkg().HeatMaps is M.HeatMaps
    import src.tracker.heatmap as re_export
    assert re_export.HeatMaps is M.HeatMaps
    cfg = config()
    assert tuple(getattr(cfg, f) for f in FIELDS) == (2, 37, 61, 16, 128, 70, 0, 4)
    assert tuple(n for n, _ in L.HeatConfig._fields_) == FIELDS
    assert lib.aic_heat_config_default(1, 1, 1, None) == L.ERR_INVALID
    assert (M.LAYERS, M.EVENT_FIELDS, (M.LIVE, M.EXPIRED, M.FLUSHED)) == (HO.LAYERS, HO.EVENT_FIELDS, (HO.LIVE, HO.EXPIRED, HO.FLUSHED))
    assert (M.ANCHORS, M.SCALES) == (dict(foot=HO.FOOT, centre=HO.CENTRE), dict(linear=HO.LINEAR, log=HO.LOG))


@pytest.mark.parametrize("kw,word", [
    (dict(streams=0), b"streams"), (dict(streams=257), b"streams"), (dict(frame_h=0), b"16384"), (dict(frame_w=16385), b"16384"),
    (dict(cell=0), b"cell"), (dict(cell=12), b"cell"), (dict(cell=64), b"cell"), (dict(max_tracks=0), b"max_tracks"), (dict(max_tracks=513), b"max_tracks"),
    (dict(forget_after=-1), b"forget_after"), (dict(anchor=2), b"anchor"), (dict(anchor=-1), b"anchor"), (dict(min_move=0), b"min_move"),
    (dict(min_move=(1 << 20) + 1), b"min_move")])
def test_create_rejects(kw, word):
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(**kw)
    assert L.load().aic_heat_create(0, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_create_null_capacity_and_the_largest():
    L = pkg("_lib")
    lib = L.load()
    h = C.c_void_p()
    cfg = config()
    assert lib.aic_heat_create(0, C.byref(cfg), None) == L.ERR_INVALID
    assert lib.aic_heat_create(0, None, C.byref(h)) == L.ERR_INVALID and not h.value
    assert lib.aic_heat_create(-1, C.byref(cfg), C.byref(h)) == L.ERR_INVALID and not h.value
    # 32768 cells is the most: 2048 x 4096 at cell 16 is exactly that, one more cell column is refused as left objects refuses it
    big = config(streams=256, frame_h=2048, frame_w=4096, cell=16, max_tracks=512)
    assert lib.aic_heat_create(0, C.byref(big), C.byref(h)) == L.OK and h.value          # no device, no memory yet
    assert lib.aic_heat_destroy(h) == L.OK
    h = C.c_void_p()
    over = config(frame_h=2048, frame_w=4097, cell=16)
    assert lib.aic_heat_create(0, C.byref(over), C.byref(h)) == L.ERR_CAPACITY and not h.value and b"32768" in lib.aic_last_error()
    assert lib.aic_heat_create(0, C.byref(config(frame_h=16384, frame_w=16384, cell=32)), C.byref(h)) == L.ERR_CAPACITY and not h.value


@pytest.fixture()
def handle():
    """Two streams of 37 x 61: creating it touches no device, so this works on every machine."""
    L = pkg("_lib")
    h = C.c_void_p()
    cfg = config(max_tracks=8)
    assert L.load().aic_heat_create(0, C.byref(cfg), C.byref(h)) == L.OK and h.value
    yield h
    assert L.load().aic_heat_destroy(h) == L.OK


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    lut = np.zeros((256, 3), np.uint8)
    assert lib.aic_heat_option(None, b"floor", 1) == L.ERR_INVALID and lib.aic_heat_reset(None, 0) == L.ERR_INVALID
    assert lib.aic_heat_update(None, 0, None, None, L.HOST, 4, None, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_heat_flush(None, -1, 4, None, None, None, None) == L.ERR_INVALID
    assert lib.aic_heat_export(None, 0, None, None) == L.ERR_INVALID and lib.aic_heat_decay(None, -1, 1, 1) == L.ERR_INVALID
    assert lib.aic_heat_export_layers(None, 0, 1, None) == L.ERR_INVALID and lib.aic_heat_import_layers(None, 0, 1, None) == L.ERR_INVALID
    assert lib.aic_heat_set_lut(None, L.ptr(lut)) == L.ERR_INVALID and lib.aic_heat_render(None, None, 0, L.HOST, None, 0) == L.ERR_INVALID
    assert lib.aic_heat_lut(None) == L.ERR_INVALID and lib.aic_heat_destroy(None) == L.OK


def test_options_reset_set_lut_and_the_default_table_without_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    assert lib.aic_heat_reset(handle, 0) == L.OK and lib.aic_heat_reset(handle, 1) == L.OK
    assert lib.aic_heat_reset(handle, 2) == L.ERR_INVALID and lib.aic_heat_reset(handle, -1) == L.ERR_INVALID
    for key, good, bad in ((b"scale", (0, 1), (-1, 2)), (b"alpha_q8", (0, 160, 256), (-1, 257)), (b"floor", (0, 8, 255), (-1, 256)),
                           (b"chunk_frames", (0, 1, 65536), (-1, 65537)), (b"ticks_per_launch", (0, 1, 65536), (-1, 65537)),
                           (b"launch_budget_mb", (1, 65536), (0, 65537))):
        assert all(lib.aic_heat_option(handle, key, v) == L.OK for v in good), key
        for v in bad:
            assert lib.aic_heat_option(handle, key, v) == L.ERR_INVALID and key in lib.aic_last_error()
    assert lib.aic_heat_option(handle, b"nonsense", 1) == L.ERR_INVALID and lib.aic_heat_option(handle, None, 1) == L.ERR_INVALID
    lut = np.zeros((256, 3), np.uint8)
    assert lib.aic_heat_lut(L.ptr(lut)) == L.OK and np.array_equal(lut, HO.default_lut())
    assert lib.aic_heat_set_lut(handle, L.ptr(lut)) == L.OK and lib.aic_heat_set_lut(handle, None) == L.ERR_INVALID
    n, ev = C.c_int32(7), np.zeros((8, 16), np.int32)
    assert lib.aic_heat_export(handle, 0, C.byref(n), L.ptr(ev)) == L.OK and n.value == 0         # nothing seen yet: no device
    assert lib.aic_heat_export(handle, 2, C.byref(n), L.ptr(ev)) == L.ERR_INVALID
    assert lib.aic_heat_export(handle, 0, None, L.ptr(ev)) == L.ERR_INVALID and lib.aic_heat_export(handle, 0, C.byref(n), None) == L.ERR_INVALID


def test_every_call_rejects_before_the_device(handle):
    L = pkg("_lib")
    lib = L.load()
    counts, rows = np.array([1, 0], np.int32), np.zeros((1, 6), np.int32)
    nf, ev, tags, pend, st = np.zeros(2, np.int32), np.zeros((2, 4, 16), np.int32), np.zeros((1, 4), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)

    def rc(ticks=1, counts=counts, rows=rows, rmem=L.HOST, cap=4, nf=nf, ev=ev, tags=tags, pend=pend, st=st):
        return lib.aic_heat_update(handle, ticks, L.ptr(counts), L.ptr(rows), rmem, cap, L.ptr(nf), L.ptr(ev), L.ptr(tags), L.ptr(pend), L.ptr(st))
    for kw in (dict(counts=None), dict(rows=None), dict(nf=None), dict(ev=None), dict(pend=None), dict(rmem=2), dict(rmem=-1), dict(cap=-1),
               dict(cap=4097), dict(ticks=-1), dict(ticks=65537), dict(counts=np.array([1, -1], np.int32))):
        assert rc(**kw) == L.ERR_INVALID, kw
    assert rc(counts=np.array([513, 0], np.int32), rows=np.zeros((513, 6), np.int32)) == L.ERR_CAPACITY and b"512" in lib.aic_last_error()
    for kw in (dict(stream=2), dict(stream=-2), dict(cap=-1), dict(cap=4097), dict(nf=None), dict(pend=None), dict(ev=None)):
        a = dict(stream=-1, cap=4, nf=nf, ev=ev, pend=pend)
        a.update(kw)
        assert lib.aic_heat_flush(handle, a["stream"], a["cap"], L.ptr(a["nf"]), L.ptr(a["ev"]), L.ptr(a["pend"]), L.ptr(st)) == L.ERR_INVALID, kw
    GH, GW = 3, 4                                                            # 37 x 61 at cell 16
    lay = np.zeros((12, GH, GW), np.int32)
    for stream, mask, shift in ((2, 1, 1), (-2, 1, 1), (0, 0, 1), (0, 1 << 12, 1), (0, -1, 1), (0, 1, 0), (0, 1, 32)):
        assert lib.aic_heat_decay(handle, stream, mask, shift) == L.ERR_INVALID, (stream, mask, shift)
    for stream, mask, p in ((2, 1, lay), (-1, 1, lay), (0, 0, lay), (0, 1 << 12, lay), (0, 1, None)):
        assert lib.aic_heat_export_layers(handle, stream, mask, L.ptr(p)) == L.ERR_INVALID, (stream, mask)
        assert lib.aic_heat_import_layers(handle, stream, mask, L.ptr(p)) == L.ERR_INVALID, (stream, mask)
    for bad in (-1, (1 << 30) + 1):                                          # the range check comes before the device
        lay[11, GH - 1, GW - 1] = bad
        assert lib.aic_heat_import_layers(handle, 0, 0xFFF, L.ptr(lay)) == L.ERR_INVALID and b"2^30" in lib.aic_last_error()
        assert lib.aic_heat_import_layers(handle, 0, 1 << 11, L.ptr(lay[11:])) == L.ERR_INVALID
    lay[11, GH - 1, GW - 1] = 1 << 30
    frames = np.zeros((2, 37, 61, 3), np.uint8)
    cams = np.array([0, 1], np.int32)
    for kw in (dict(n=-1), dict(n=65537), dict(mem=2), dict(mem=-1), dict(layer=-1), dict(layer=12), dict(frames=None),
               dict(cams=np.array([0, 2], np.int32)), dict(cams=np.array([-1, 0], np.int32))):
        a = dict(frames=frames, n=2, mem=L.HOST, cams=cams, layer=1)
        a.update(kw)
        assert lib.aic_heat_render(handle, L.ptr(a["frames"]), a["n"], a["mem"], L.ptr(a["cams"]), a["layer"]) == L.ERR_INVALID, kw
    # what passes the checks reaches the device: no GPU here -> AIC_ERR_NO_DEVICE
    if L.device_count() == 0:
        assert rc() == L.ERR_NO_DEVICE and rc(st=None, tags=None) == L.ERR_NO_DEVICE
        assert rc(counts=np.array([0, 0], np.int32), rows=None) == L.ERR_NO_DEVICE
        assert rc(ticks=0, counts=None, rows=None) == L.ERR_NO_DEVICE and rc(cap=0, ev=None) == L.ERR_NO_DEVICE
        assert lib.aic_heat_flush(handle, -1, 4, L.ptr(nf), L.ptr(ev), L.ptr(pend), None) == L.ERR_NO_DEVICE
        assert lib.aic_heat_decay(handle, -1, 0xFFF, 31) == L.ERR_NO_DEVICE
        assert lib.aic_heat_export_layers(handle, 0, 0xFFF, L.ptr(lay)) == L.ERR_NO_DEVICE
        assert lib.aic_heat_import_layers(handle, 0, 0xFFF, L.ptr(lay)) == L.ERR_NO_DEVICE
        assert lib.aic_heat_render(handle, L.ptr(frames), 2, L.HOST, None, 0) == L.ERR_NO_DEVICE
        assert lib.aic_heat_render(handle, None, 0, L.HOST, None, 0) == L.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------- heat_math.hpp, stand-alone
@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the heat host test builds tests/heat_probe.cpp with the system compiler")
    exe = str(tmp_path_factory.mktemp("heat") / "heat_probe")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "heat_probe.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def lines(printed, key):
    return [ln[len(key) + 1:] for ln in printed if ln.startswith(key + " ") or ln == key]


def test_probe_octants_logs_and_levels_equal_the_oracle(printed):
    (octs,) = lines(printed, "oct")
    want = "".join(str(HO.octant(dx, dy)) for dy in range(-40, 41) for dx in range(-40, 41) if dx or dy)
    assert octs == want and set(octs) == set("01234567")
    (logs,) = lines(printed, "log")
    pairs = [tuple(int(x) for x in t.split(":")) for t in logs.split()]
    assert len(pairs) > 2100 and {p[0] for p in pairs} >= {0, 1, (1 << 30) - 1, 1 << 30, (1 << 29) + 1}
    for v, u in pairs:
        assert u == HO.log_q8(v), v
    seen = 0
    for ln in lines(printed, "lev"):
        scale, M, *rest = ln.split()
        for t in rest:
            v, q = (int(x) for x in t.split(":"))
            assert q == HO.level(v, int(M), int(scale)) and 0 <= q <= HO.Q_MAX, ln
            seen += 1
    assert seen == 2 * 11 * 6
    (sat,) = lines(printed, "sat")
    assert sat == f"{1 << 30} {1 << 30} 11"


def grid_q(cell, r, c):
    return ((((r * 7919 + c * 104729 + cell * 31) * 2654435761) & 0xFFFFFFFF) >> 8) % (HO.Q_MAX + 1)


def test_probe_bilinear_lut_anchor_and_blend_equal_the_oracle(printed):
    H, W = 37, 61
    bil = lines(printed, "bil")
    assert [int(ln.split()[0]) for ln in bil] == [4, 8, 16, 32]
    for ln in bil:
        cell, *vals = (int(x) for x in ln.split())
        GH, GW = -(-H // cell), -(-W // cell)
        q = np.array([[grid_q(cell, r, c) for c in range(GW)] for r in range(GH)])
        assert np.array_equal(np.array(vals).reshape(H, W), HO.bilinear(q, H, W, cell)), cell
    (lut,) = lines(printed, "lut")
    assert np.array_equal(np.array(lut.split(), int).reshape(256, 3), HO.default_lut())
    anc = [[int(x) for x in ln.split()] for ln in lines(printed, "anc")]
    assert len(anc) == 18
    for anchor, x1, y1, x2, y2, fx, fy in anc:
        o = HO.HeatOracle((H, W), anchor=anchor)
        assert (fx, fy) == o.anchor_of([x1, y1, x2, y2]), (anchor, x1, y1, x2, y2)
    (bld,) = lines(printed, "bld")
    want = [(i * (256 - a) + l * a + 128) >> 8 for a in (0, 1, 128, 160, 255, 256) for i in (0, 1, 127, 128, 254, 255) for l in (0, 1, 127, 128, 254, 255)]
    assert [int(x) for x in bld.split()] == want and max(want) == 255 and min(want) == 0


# ---------------------------------------------------------------------------------------------------- the Python class
def test_python_class_needs_no_device_until_a_call_that_computes():
    M, L = pkg("heatmap"), pkg("_lib")
    for kw in (dict(streams=0), dict(streams=257), dict(max_tracks=0), dict(max_tracks=513), dict(cell=5), dict(min_move=0), dict(forget_after=-1),
               dict(frame_hw=(0, 61))):
        a = dict(streams=2, frame_hw=(37, 61))
        a.update(kw)
        with pytest.raises(L.AicError) as ei:
            M.HeatMaps(**a)
        assert ei.value.code == L.ERR_INVALID, kw
    with pytest.raises(L.AicError) as ei:
        M.HeatMaps(1, (16384, 16384))
    assert ei.value.code == L.ERR_CAPACITY
    with pytest.raises(ValueError):
        M.HeatMaps(2, (37, 61), anchor="head")
    hm = M.HeatMaps(2, (37, 61), max_tracks=8)
    assert (hm.grid_h, hm.grid_w) == (3, 4)
    empty = np.zeros((0, 6), np.int32)
    with pytest.raises(ValueError):
        hm.update([[empty]])                                                 # one row list for two streams
    with pytest.raises(ValueError):
        hm.update(np.zeros((3, 6), np.int32), counts=[2, 2])
    with pytest.raises(ValueError):
        hm.update(np.zeros((3, 6), np.int32), counts=[3])
    with pytest.raises(L.AicError) as ei:
        hm.update([[np.zeros((513, 6), np.int32), empty]])
    assert ei.value.code == L.ERR_CAPACITY
    for bad in (dict(dwell=np.zeros((3, 5), np.int32)), dict(dwell=np.zeros((3, 4), np.float32)), dict(dwell=np.full((3, 4), -1)),
                dict(dwell=np.full((3, 4), (1 << 30) + 1)), dict(heat=np.zeros((3, 4), np.int32)), {}):
        with pytest.raises(ValueError):
            hm.load_layers(0, bad)
    with pytest.raises(ValueError):
        hm.layers(0, ["footfall"])
    with pytest.raises(ValueError):
        hm.render(np.zeros((2, 37, 60, 3), np.uint8))
    with pytest.raises(ValueError):
        hm.render(np.zeros((2, 37, 61, 3), np.uint8), cameras=[0])
    with pytest.raises(ValueError):
        hm.render(np.zeros((2, 37, 61, 3), np.uint8), layer="heat")
    with pytest.raises(ValueError):
        hm.set_colour_table(np.zeros((255, 3), np.uint8))
    with pytest.raises(ValueError):
        hm.option("scale", "cubic")
    hm.set_colour_table(hm.colour_table()), hm.option("scale", "linear"), hm.option("alpha_q8", 200), hm.option("ticks_per_launch", 3), hm.reset(1)
    assert np.array_equal(M.colour_table(), HO.default_lut()) and hm.export(1).shape == (0, 16)
    assert M.layer_mask() == 0xFFF and M.layer_mask(["dwell", 11]) == 0b100000000010 and M.layer_index("dir3") == 7
    with pytest.raises(L.AicError):
        hm.reset(2)
    if L.device_count() == 0:
        for call in (lambda: hm.update([[empty, empty]]), hm.drain, hm.flush, lambda: hm.update_tuples([[[], []]]), lambda: hm.layers(0), hm.decay,
                     lambda: hm.load_layers(0, dict(dwell=np.zeros((3, 4), np.int32))), lambda: hm.render(np.zeros((2, 37, 61, 3), np.uint8)), hm.images):
            with pytest.raises(L.NoDeviceError):
                call()
    hm.close()


def test_paths_and_event_dict():
    M = pkg("heatmap")
    ev = np.zeros((2, 2, 16), np.int32)
    ev[1, 0] = M.EXPIRED, 1, 7, 0, 3, 40, 30, 5, 20, 30, 100, 90, 160, 9, 25, 14
    ev[0, 0] = M.FLUSHED, 0, 9, -1, 0, 0, 1, 1, 8, 8, 8, 8, 0, 0, 0, 0
    res = M.HeatResult(np.array([1, 1], np.int32), ev, np.zeros((0, 4), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), {})
    p = M.paths(res)
    assert [d["id"] for d in p] == [9, 7] and p[0]["why"] == "flushed" and p[0]["straightness"] is None and p[0]["length"] == 0
    d = p[1]
    assert (d["start"], d["end"], d["length"], d["cells"], d["last_cell"], d["moving"]) == ((10.0, 15.0), (50.0, 45.0), 80.0, 5, 14, 25)
    assert d["straightness"] == 0.5 and M.event_dict(ev[1, 0])["max_step"] == 9


def test_pipeline_hook_does_nothing_unless_attached():
    TP = pkg("pipeline").TrackingPipeline
    fake = TP.__new__(TP)                                                    # no engines, no handle: only the hook is under test
    fake.streams = 2
    fake._feed_heat(np.ones(4, np.int32), np.ones((4, 3, 6), np.int32))
    assert vars(fake) == {"streams": 2}                                      # nothing attached: nothing is computed, nothing is set
    assert TP._heat is None and TP.heat_result is None
    stage = type("W", (), dict(streams=3, frame_h=37, frame_w=61))()
    with pytest.raises(ValueError):
        TP.attach_heat_maps(type("P", (), dict(streams=2, frame_h=37, frame_w=61))(), stage)
    with pytest.raises(ValueError):
        TP.attach_heat_maps(type("P", (), dict(streams=3, frame_h=37, frame_w=60))(), stage)
    fake = type("P", (), dict(streams=3, frame_h=37, frame_w=61))()
    TP.attach_heat_maps(fake, stage, cap=9)
    assert fake._heat is stage and fake.heat_result is None and fake.heat_cap == 9
    TP.attach_heat_maps(fake, None)
    assert fake._heat is None


# ---------------------------------------------------------------------------------------------------- the kernels' budget
RECORDED = {  # DESIGN.md section 48 and the stages' own sections: (VGPRs, static LDS bytes); scratch and spills 0 everywhere
    "colours_sample_kernel": (35, 1236), "colours_walk_kernel": (76, 20512), "bestshot_score_kernel": (36, 32), "bestshot_walk_kernel": (71, 32800),
    "zones_classify_kernel": (18, 8448), "zones_walk_kernel": (92, 27168), "scene_model_kernel": (16, 0), "scene_stats_kernel": (29, 2624),
    "scene_rows_kernel": (36, 0), "scene_walk_kernel": (48, 0), "scene_gray_kernel<4, 1>": (16, 768), "scene_gray_kernel<8, 1>": (28, 768),
    "scene_gray_kernel<16, 1>": (52, 768), "scene_gray_kernel<4, 4>": (29, 3072), "scene_gray_kernel<8, 4>": (44, 3072),
    "scene_gray_kernel<16, 4>": (62, 3072), "left_occupancy_kernel": (20, 0), "left_model_kernel": (26, 0), "left_blobs_kernel": (32, 3600),
    "left_walk_kernel": (64, 0), "left_events_kernel": (29, 0)}


def test_heat_kernels_have_no_scratch_and_the_other_stages_keep_their_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    table = kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so")
    heat = {k: r for k, r in table.items() if re.search(r"\d+heat_[a-z]+_kernel", k)}
    for name in ("heat_walk_kernel", "heat_decay_kernel", "heat_levels_kernel", "heat_render_kernel"):
        assert sum(f"{len(name)}{name}" in k for k in heat) == 1, (name, sorted(heat))
    assert len(heat) == 4
    bad = {k: r for k, r in heat.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    for k, r in heat.items():                                                # a 512-thread block is 2 waves per SIMD: 256 registers each
        assert r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 48 * 1024, (k, r)
    others = {k: r for k, r in table.items() if re.search(r"\d+(colours|bestshot|zones|scene|left)_[a-z]+_kernel", k)}
    assert len(others) == len(RECORDED), sorted(others)
    for name, (vgpr, lds) in RECORDED.items():                               # the symbols as the compiler mangles them: <length><name>[I Li<n>E .. E]
        base, _, targs = name.partition("<")
        want = f"{len(base)}{base}" + ("I" + "".join(f"Li{int(t)}E" for t in targs.rstrip(">").split(",")) + "E" if targs else "E")
        hit = [r for k, r in others.items() if want in k]
        assert len(hit) == 1, (name, want, sorted(others))
        r = hit[0]
        assert (r["vgpr"], r["lds"], r["scratch"], r["vgpr_spills"], r["agpr"]) == (vgpr, lds, 0, 0, 0), (name, r)


def test_cli_flags_and_the_parser_errors():
    cli = pkg("cli")
    a = cli.parse_arguments(["--input", "a.npy", "--heat_maps", "maps", "--heat_cell", "8", "--heat_layer", "dir3", "--heat_paths", "p.jsonl", "--heat_overlay"])
    assert (a.heat_maps, a.heat_cell, a.heat_layer, a.heat_paths, a.heat_overlay) == ("maps", 8, "dir3", "p.jsonl", True)
    for tracker in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
        a = cli.parse_arguments(["--inputs", "a.npy,b.npy", "--tracker", tracker, "--heat_maps", "maps", "--colours"])
        assert a.heat_maps == "maps" and a.colours and a.heat_cell is None and a.heat_layer is None and not a.heat_overlay
    a = cli.parse_arguments(["--input", "a.npy"])
    assert a.heat_maps is None and a.heat_paths is None and not a.heat_overlay
    for flags in (["--heat_cell", "8"], ["--heat_layer", "dwell"], ["--heat_paths", "p.jsonl"], ["--heat_overlay"], ["--heat_maps", "maps", "--heat_layer", "heat"],
                  ["--heat_maps", "maps", "--heat_cell", "5"]):
        with pytest.raises(SystemExit):
            cli.parse_arguments(["--input", "a.npy"] + flags)
    assert cli.HEAT_LAYERS == pkg("heatmap").LAYERS
