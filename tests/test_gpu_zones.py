"""Zone entries, dwell and line crossings on the device (csrc/kernels_zones.hip) against tests/zones_oracle.py:
exact integer arithmetic on both sides, so everything -- events, n_events, occupancy, counters, status -- is np.array_equal.  Each
case is the smallest shape that can break; tests/test_zones_oracle.py shows through the oracle alone that the seeded scenes emit every
kind of event."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import zones_cases as ZC
import zones_oracle as ZO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

EMPTY = np.zeros((0, 6), np.int32)


def counter(geo, **kw):
    zc = pkg("zones").ZoneCounter(streams=len(geo), **kw)
    for s, (zs, ls) in enumerate(geo):
        zc.set_zones(s, zs, ls)
    return zc


def same_result(got, want, what=""):
    for name, g, w in zip(("n_events", "events", "occupancy", "status"), got[:4], want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g[:4] if g.ndim > 1 else g, w[:4] if w.ndim > 1 else w)


def same_counters(zc, oracles, what=""):
    for s, o in enumerate(oracles):
        c = zc.counters(s)
        for name, w in zip(("zone_in", "zone_out", "line_pos", "line_neg"), o.counters()):
            assert c[name].dtype == np.int64 and np.array_equal(c[name], w), (what, s, name, c[name], w)


def check(geo, calls, cap=64, options=(), **kw):
    """calls: per call frames[s] for every stream.  The device against one oracle per stream, call by call; returns (counter, oracles,
    the results)."""
    zc, oracles = counter(geo, **kw), ZC.oracles_for(geo, **kw)
    for key, v in options:
        zc.option(key, v)
    res = []
    for i, frames in enumerate(calls):
        got = zc.update(frames, cap_events=cap)
        same_result(got, ZO.run_bank(oracles, frames, cap), i)
        same_counters(zc, oracles, i)
        res.append(got)
    return zc, oracles, res


def frames_at(paths, **kw):
    """paths[i] = the anchor of id i + 1 per frame (None = not seen) -> one stream's frames."""
    out = []
    for f in range(len(paths[0])):
        seen = [(p[f], i + 1) for i, p in enumerate(paths) if p[f] is not None]
        out.append(ZC.rows_at([p for p, _ in seen], ids=[i for _, i in seen], **kw))
    return out


def test_inside_rule_on_vertices_edges_and_negative_coordinates():
    tri = [(-40, -30), (20, -30), (-40, 30)]                                 # a slanted edge through (-10, 0)
    star = ZC.star32(0, 0, 90, 35)
    pts = [(-40, -30), (20, -30), (-40, 30),                                 # the triangle's vertices
           (-10, -30), (-40, 0), (-10, 0), (-11, 0), (-9, 0), (-39, -29), (-41, -30), (-10, -31),   # on / beside its edges
           star[0], star[1], star[16], star[31], (0, 0), (89, 0), (91, 0), (-60, -60), (34, 7), (35, 7), (36, 7)]
    frames = [ZC.rows_at(pts)] + [ZC.rows_at(pts[::-1]), np.array([[x - 2, y - 9, x + 1, y, i + 1, 0] for i, (x, y) in enumerate(pts)], np.int32)]
    for anchor in ("bottom", "centre"):
        _, oracles, res = check([([tri, star, tri[::-1]], [])], [[frames]], cap=128, anchor=anchor)
        assert 0 < res[0].occupancy[0, 0] < len(pts) and 0 < res[0].occupancy[0, 1] < len(pts)
        assert res[0].occupancy[0, 0] != res[0].occupancy[0, 2]             # the winding decides the boundary points


def test_int64_cross_products():
    """Vertices, lines and boxes at +-2^20: doubled differences reach 2^22, the products 2^44.  The zone's bottom edge rises ONE pixel over
    2^21, so the answer one pixel above / on it changes under int32 or fp32 arithmetic."""
    m = 1 << 20
    poly = [(-m, -m), (m, -m + 1), (m, m), (-m, m - 1)]
    pts = [(m - 1, -m + 1), (m - 1, -m), (-m + 1, m - 1), (-m + 1, m), (0, 0), (m - 1, -m + 1), (-m + 1, m - 1), (m - 1, m - 1), (-m + 1, -m + 1)]
    frames = [np.array([[x - 1, y, x + 1, y, 1, 0], [x - 1, y - 1, x + 1, y, 2, 0], [m, -m, m, m, 3, 0], [m + 1, 0, m + 1, 0, 4, 0]], np.int32) for x, y in pts]
    lines = [((-m, -m), (m, m)), ((m, -m), (-m, m)), ((-m, 1), (m, 0))]
    _, oracles, res = check([([poly], lines)], [[frames]], cap=16)
    assert res[0].occupancy[:5, 0].tolist()[:4] == [2, 0, 2, 0]              # as worked by hand in tests/test_zones_oracle.py (id 3, 4 outside / ignored)
    assert ZC.kinds_seen(res[0].events) >= {(ZO.ENTER, 0), (ZO.EXIT, 0), (ZO.CROSS, 1), (ZO.CROSS, -1)}


def test_lines_endpoints_collinear_zero_moves_and_the_forget_gap():
    line = [((0, 0), (10, 0))]
    paths = [[(0, -5), (0, 5), (0, -5)], [(10, -5), (10, 5), (10, -5)],      # through A, through B: half-open
             [(2, 0), (8, 0), (8, 0)], [(-5, 0), (15, 0), (-5, 0)],          # collinear, zero move
             [(5, -5), (5, 5), (5, -5)], [(5, -5), (5, 0), (5, 5)]]          # both directions; stopping on the line
    _, oracles, res = check([(ZC.GEOMETRY[1][0], line)], [[frames_at(paths)]])
    assert oracles[0].line_pos == [3] and oracles[0].line_neg == [2]
    # seen again after a gap of forget_after: still the same track, it crosses; after forget_after + 1: LOST (it was in the zone), then a
    # first sighting without a crossing
    for gap, kinds in ((3, [ZO.EXIT, ZO.CROSS]), (4, [ZO.LOST])):
        frames = [ZC.rows_at([(5, 5)])] + [EMPTY] * (gap - 1) + [ZC.rows_at([(5, -5)])]
        _, oracles, res = check([([ZC.SQUARE], line)], [[frames]], forget_after=3)
        assert res[0].events[gap, :2, 0].tolist() == (kinds + [0])[:2] and oracles[0].line_neg == [gap == 3]


def test_slots_reuse_capacity_stop_and_reset():
    geo = [([ZC.SQUARE], []), ([ZC.SQUARE], [])]
    inside = (5, 5)
    s0 = [ZC.rows_at([inside] * 2, ids=[11, 12]), ZC.rows_at([inside], ids=[12]), ZC.rows_at([inside] * 2, ids=[12, 13]),      # 11 expires at frame 2, 13 takes slot 0
          ZC.rows_at([inside] * 2, ids=[13, 12]), ZC.rows_at([inside] * 3, ids=[12, 13, 14]), ZC.rows_at([inside], ids=[12])]     # frame 4: a third live id
    s1 = [ZC.rows_at([inside] * 2, ids=[1, 2])] * 6
    zc, oracles, res = check(geo, [[s0, s1]], max_tracks=2, forget_after=1)
    r = res[0]
    assert r.status.tolist() == [ZO.ERR_CAPACITY, 0] and r.n_events[:6].tolist() == [2, 0, 2, 0, 0, 0] and r.n_events[6:].sum() == 2
    assert r.events[2, :2, 0].tolist() == [ZO.LOST, ZO.ENTER] and r.events[2, :2, 2].tolist() == [11, 13]
    assert 0 in zc.failed and 1 not in zc.failed
    L = pkg("_lib")
    with pytest.raises(L.AicError) as ei:                                    # a set while the stream is stopped
        zc.set_zones(0, [ZC.SQUARE], [])
    assert ei.value.code == L.ERR_INVALID
    again = [[ZC.rows_at([inside], ids=[12])], [ZC.rows_at([inside], ids=[1])]]
    same_result(zc.update(again, cap_events=64), ZO.run_bank(oracles, again, 64), "stopped")     # nothing for stream 0, stream 1 goes on
    same_counters(zc, oracles)
    zc.reset(0), oracles[0].reset()
    assert not zc.failed and not any(v.any() for v in zc.counters(0).values())
    got = zc.update(again, cap_events=64)
    same_result(got, ZO.run_bank(oracles, again, 64), "after reset")
    assert got.status.tolist() == [0, 0] and got.events[0, 0, :5].tolist() == [ZO.ENTER, 0, 12, 0, 0]
    same_counters(zc, oracles)
    # a full table whose slots all expire in the frame makes room for as many new ids in that frame
    check([([ZC.SQUARE], [])], [[[ZC.rows_at([inside] * 2, ids=[1, 2]), ZC.rows_at([inside] * 2, ids=[3, 4])]]], max_tracks=2, forget_after=0)


def test_duplicates_empty_frames_512_rows_and_513_rejected():
    geo = [(ZC.GEOMETRY[0][0], ZC.LINES)]
    rng = np.random.default_rng(5)
    far = (1 << 20) + 1
    dup = np.array([ZC.box(60, 60) + [4, 0], ZC.box(300, 300) + [4, 1], [far, 0, far, 5, 9, 0], ZC.box(30, 30) + [9, 0], ZC.box(61, 60) + [4, 2]], np.int32)
    ids = rng.permutation(np.arange(1, 257)).repeat(2)                       # 512 rows, every id twice
    full = [np.array([ZC.box(int(x), int(y), 3, 12) + [int(i), int(i) % 5] for (x, y), i in zip(rng.integers(-30, 230, (512, 2)), ids)], np.int32)
            for _ in range(3)]
    frames = [dup, EMPTY, dup[::-1], EMPTY, EMPTY] + full + [EMPTY]
    zc, oracles, res = check(geo, [[frames]], cap=1024, forget_after=2)
    assert res[0].occupancy[5].sum() > 0 and res[0].n_events[5:8].min() > 32
    L = pkg("_lib")
    with pytest.raises(L.AicError) as ei:
        zc.update([[full[0], np.zeros((513, 6), np.int32)]])
    assert ei.value.code == L.ERR_CAPACITY
    same_result(zc.update([[full[1]]], cap_events=1024), ZO.run_bank(oracles, [[full[1]]], 1024), "after the rejected call")   # nothing was staged


def test_event_cap_truncates_the_list_only():
    pts = [(5, 5)] * 5
    frames = [ZC.rows_at(pts), ZC.rows_at([(50, 50)] * 5)]
    _, oracles, res = check([([ZC.SQUARE], [])], [[frames]], cap=1)
    assert res[0].n_events.tolist() == [5, 5] and res[0].events.shape == (2, 1, 8) and res[0].events[1, 0, :3].tolist() == [ZO.EXIT, 0, 1]
    assert oracles[0].zone_in == [5] and oracles[0].zone_out == [5]
    check([([ZC.SQUARE], [])], [[frames]], cap=0)


def test_bank_of_256_streams_one_frame():
    geo, frames = ZC.bank_scene(256, 2, seed=2)
    zc, oracles, res = check(geo, [[f[:1] for f in frames], [f[1:] for f in frames]], forget_after=3)
    assert res[1].n_events.sum() > 0


@pytest.mark.parametrize("options", [(), (("frames_per_launch", 1),), (("frames_per_launch", 16),)])
def test_bank_equals_singles_on_any_split(options):
    geo, frames = ZC.bank_scene(3, 20, seed=1)
    whole = [frames[0], [], frames[2]]                                       # stream 1 is handed no frame at all
    zc, oracles, res = check(geo, [whole], options=options, forget_after=3)
    assert ZC.kinds_seen(res[0].events) == ZC.ALL_KINDS
    split, _, parts = check(geo, [[f[a:b] for f in whole] for a, b in ((0, 1), (1, 17), (17, 20))], options=options, forget_after=3)
    for s in (0, 2):                                                         # the bank's stream s == a single-stream object
        one = counter([geo[s]], forget_after=3)
        got = one.update([frames[s]], cap_events=64)
        lo = 0 if s == 0 else 20
        assert np.array_equal(got.events, res[0].events[lo:lo + 20]) and np.array_equal(got.occupancy, res[0].occupancy[lo:lo + 20])
        assert np.array_equal(np.concatenate([p.events[p.frames_per_stream[:s].sum():][:p.frames_per_stream[s]] for p in parts]), got.events)
        for k, v in one.counters(0).items():
            assert np.array_equal(v, zc.counters(s)[k]) and np.array_equal(v, split.counters(s)[k])


def test_host_rows_equal_device_rows():
    geo, frames = ZC.bank_scene(3, 6, seed=3)
    flat = [r for f in frames for r in f]
    counts, fps = [len(r) for r in flat], [len(f) for f in frames]
    rows = np.concatenate(flat)
    a, b, c = (counter(geo, forget_after=3) for _ in range(3))
    ra = a.update(frames, cap_events=32)
    rb = b.update(torch.from_numpy(rows).cuda(), counts=counts, frames_per_stream=fps, cap_events=32)
    rc = c.update(rows, counts=counts, frames_per_stream=fps, cap_events=32)
    assert ra.n_events.sum() > 0
    same_result(rb, ra[:4], "device")
    same_result(rc, ra[:4], "flat host")
    for s in range(3):
        for k, v in a.counters(s).items():
            assert np.array_equal(v, b.counters(s)[k]) and np.array_equal(v, c.counters(s)[k])


def test_no_zones_or_no_lines():
    _, frames = ZC.bank_scene(2, 12, seed=4)
    _, oracles, res = check([([], ZC.LINES), (ZC.GEOMETRY[0][0], []), ([], [])], [[frames[0], frames[1], frames[0]]], forget_after=3)
    assert oracles[0].line_pos != [0, 0] and sum(oracles[1].zone_in) > 0 and res[0].n_events[24:].sum() == 0


# ---------------------------------------------------------------------------------------------------- end to end
def _tuples_to_rows(tracks):
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    return np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks], np.int32).reshape(-1, 6)


def test_pipeline_attach_zones_end_to_end():
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, Scene = pkg("pipeline").TrackingPipeline, pkg("synthetic").Scene
    S, T = 2, 40
    scenes = [Scene(seed=61 + s, n_targets=6, conf_range=(0.8, 0.95), speed=9.0, gaps=[(0, 10, 16), (1, 5, 30)]) for s in range(S)]
    planted = [scenes[i % S].detections(i // S)[:3] for i in range(S * T)]   # tick-major: slot t * S + s
    geo = [([[(300, 150), (900, 150), (900, 600), (300, 600)]], [((640, 0), (640, 720))]) for _ in range(S)]

    def run(zc):
        pipe = TP(ypath, None, (720, 1280), batch=8, ring_frames=S * T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=S,
                  track_buffer=3)
        pipe.upload(0, np.zeros((S * T, 720, 1280, 3), np.uint8))
        pipe.inject(0, planted)
        if zc is not None:
            pipe.attach_zones(zc)
        out = []
        for lo in (0, 16):                                                   # two run calls: the counter's state carries over
            out += pipe.run(lo, 16 if lo == 0 else S * T - 16)[0]
        state = (pipe.zone_events, pipe.zone_occupancy, pipe.zone_counters() if zc is not None else None, pipe.zone_result)
        pipe.close()
        return out, state

    plain, none = run(None)
    assert none == (None, None, None, None)
    zc = counter(geo, forget_after=5)
    tracks, (events, occ, counters, res) = run(zc)
    assert tracks == plain                                                   # the tracks are untouched
    oracles = ZC.oracles_for(geo, forget_after=5)
    per_stream = [[_tuples_to_rows(tracks[t * S + s]) for t in range(T)] for s in range(S)]
    ZO.run_bank(oracles, [f[:8] for f in per_stream], 256)
    want = ZO.run_bank(oracles, [f[8:] for f in per_stream], 256)           # the second run call is what the pipeline still shows
    same_result(res, want, "pipeline")
    assert want[0].sum() > 0 and want[2].sum() > 0 and sum(o.line_pos[0] + o.line_neg[0] for o in oracles) > 0
    for s in range(S):
        assert len(events[s]) == T - 8 and np.array_equal(occ[s], want[2][s * (T - 8):(s + 1) * (T - 8)])
        for name, w in zip(("zone_in", "zone_out", "line_pos", "line_neg"), oracles[s].counters()):
            assert np.array_equal(counters[s][name], w), (s, name)
        assert sum(oracles[s].zone_in) > 0
    zc.close()


def test_update_tuples_from_deepsort():
    engines = pkg("engine_file").ensure_seeded_engines(ROOT)
    Scene = pkg("synthetic").Scene
    sc = Scene(seed=71, n_targets=5, width=640, height=360, w_range=(30.0, 50.0), h_range=(60.0, 100.0), y_range=(20.0, 200.0), speed=8.0,
               conf_range=(0.8, 0.95))
    trk = pkg("deepsort_tracker").DeepSORT(reid_model_path=engines[1], device=0)
    geo = [([[(150, 80), (500, 80), (500, 330), (150, 330)]], [((320, 0), (320, 360))])]
    zc, oracle = counter(geo, forget_after=5), ZC.oracles_for(geo, forget_after=5)[0]
    n_ev = 0
    for f in range(12):
        b, c, k, _ = sc.detections(f)
        tracks = trk.update(b, c, k, sc.render(f))
        got = zc.update_tuples([[tracks]])
        same_result(got, ZO.run_bank([oracle], [[_tuples_to_rows(tracks)]], 256), f)
        n_ev += int(got.n_events.sum())
    same_counters(zc, [oracle])
    assert n_ev > 0


def test_cli_zones_lines(tmp_path):
    import json
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    zfile = tmp_path / "zones.json"
    zfile.write_text(json.dumps({"cameras": [{"zones": [[[100, 50], [540, 50], [540, 330], [100, 330]], [[0, 0], [320, 0], [0, 360]]],
                                              "lines": [[[320, 0], [320, 360]]]}]}))
    srcs = ["synthetic:640x360:6:16:1", "synthetic:640x360:4:16:2"]
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--zones", str(zfile)]
    assert cli.main(["--inputs", ",".join(srcs), "--batch", "8", "--output_dir", str(tmp_path / "both")] + common) == 0    # one entry serves both cameras
    assert cli.main(["--input", srcs[0], "--output_dir", str(tmp_path / "one")] + common) == 0                            # frame by frame: update_tuples
    assert cli.main(["--input", srcs[0], "--batch", "8", "--output_dir", str(tmp_path / "batched")] + common) == 0
    files = sorted((tmp_path / "both").glob("*.jsonl")) + list((tmp_path / "one").glob("*.jsonl")) + list((tmp_path / "batched").glob("*.jsonl"))
    assert len(files) == 4
    for path in files:
        lines = [json.loads(l) for l in path.read_text().splitlines()]
        assert len(lines) == 16
        last = None
        for l in lines:
            z = l["zones"]
            assert set(z) == {"occupancy", "zone_in", "zone_out", "line_pos", "line_neg", "events"}
            assert len(z["occupancy"]) == len(z["zone_in"]) == len(z["zone_out"]) == 2 and len(z["line_pos"]) == len(z["line_neg"]) == 1
            assert all(o <= len(l["tracks"]) for o in z["occupancy"])
            assert all(e["kind"] in ("enter", "exit", "lost", "cross") and e["frame"] == l["frame"] for e in z["events"])
            total = z["zone_in"] + z["zone_out"] + z["line_pos"] + z["line_neg"]
            assert last is None or all(a >= b for a, b in zip(total, last))      # cumulative
            last = total
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps({"cameras": [{}, {}, {}]}))                    # three entries for two sources
    assert cli.main(["--inputs", ",".join(srcs), "--batch", "8", "--output_dir", str(tmp_path / "bad"), "--yolo_engine", ypath, "--tracker", "bytetrack",
                     "--zones", str(bad)]) == 1
