"""Left objects on the device (csrc/kernels_left.hip) against tests/left_oracle.py: integer arithmetic on both
sides, so everything -- records, objects, events, cand, labels, the exported planes, slots and scalars -- is np.array_equal.  Each case
is the smallest shape that can break; tests/test_left_oracle.py shows through the oracle alone what the planted scenes do."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import left_cases as LC
import left_oracle as LO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

_REF = {}
NAMES = ("records", "objects", "events", "cand", "labels")
EXPORTS = ("fast", "slow", "still", "last_id", "last_tick", "slots", "scalars")


def reference(cs):
    """(records, objects, events, cand, labels, [export per stream]) of the oracle over the whole case, computed once per case name."""
    if cs["name"] not in _REF:
        o = LC.oracles_for(cs)
        _REF[cs["name"]] = LO.run(o, cs["frames"], cs["rows"]) + ([x.export() for x in o],)
    return _REF[cs["name"]]


def stage_for(cs, streams=None, options=()):
    lo = pkg("leftobj").LeftObjects(streams or cs["frames"].shape[1], cs["hw"], cs["cell"], cs["max_objects"], **cs["options"])
    for k, v in options:
        lo.option(k, v)
    return lo


def differ(name, g, w, what):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError((what, name, len(bad), "differences, the first at", bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def same_export(lo, exports, what="", streams=None):
    for s in streams if streams is not None else range(len(exports)):
        e = lo.export(s)
        for name, w in zip(EXPORTS, exports[s]):
            differ(f"export {name} of stream {s}", e[name], w, what)


def feed(lo, cs, cuts=None, device=False, offset=0, cap_events=4096):
    """The case through the device in calls of `cuts` ticks; returns (records, objects, events, cand, labels) of all calls joined, the
    events' tick counted over the whole case."""
    frames, rows = cs["frames"], cs["rows"]
    T = len(frames)
    out, lo_t = [[] for _ in NAMES], 0
    for n in cuts or [T]:
        fr = frames[lo_t:lo_t + n]
        r = None if rows is None else rows[lo_t:lo_t + n]
        if device:
            raw = torch.zeros(fr.size + offset + 16, dtype=torch.uint8, device="cuda")
            raw[offset:offset + fr.size] = torch.from_numpy(fr.reshape(-1)).cuda()
            fr_d = raw[offset:offset + fr.size].view(fr.shape)
            assert fr_d.data_ptr() % 16 == offset
            if r is not None:
                flat = [x for tick in r for x in tick]
                counts = torch.tensor([len(x) for x in flat], dtype=torch.int32).cuda()
                allrows = torch.from_numpy(np.concatenate(flat + [np.zeros((0, 6), np.int32)])).cuda().contiguous()
                res = lo.update(fr_d, allrows, counts, cap_events=cap_events, want_masks=True)
            else:
                res = lo.update(fr_d, cap_events=cap_events, want_masks=True)
        else:
            res = lo.update(fr, r, cap_events=cap_events, want_masks=True)
        assert not res.overflow and res.n_events == len(res.events)
        ev = res.events.copy()
        ev[:, 0] += lo_t
        for acc, x in zip(out, (res.records, res.objects, ev, res.cand, res.labels)):
            acc.append(x)
        lo_t += n
    assert lo_t == T
    return tuple(np.concatenate(x) for x in out)


def check(cs, what=None, **kw):
    lo = stage_for(cs, options=kw.pop("options", ()))
    got = feed(lo, cs, **kw)
    want = reference(cs)
    for name, g, w in zip(NAMES, got, want):
        differ(name, g, w, what or cs["name"])
    same_export(lo, want[5], what or cs["name"])
    return lo, got


SHAPES = [("12x12 c4: a 3 x 3 grid", (12, 12), 4, 1), ("4x64 c4: a 1 x 16 grid", (4, 64), 4, 1), ("64x96 c8", (64, 96), 8, 1),
          ("132x260 c4: a 33 x 65 grid", (132, 260), 4, 1), ("48x53 c16: 3 W = 159", (48, 53), 16, 1), ("three streams", (64, 96), 8, 3)]


def shape_case(i, **kw):
    name, hw, cell, S = SHAPES[i]
    return LC.seeded(name, hw, cell, streams=S, ticks=40, seed=40 + i, **kw)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_shapes_host_frames(i):
    cs = shape_case(i)
    _, got = check(cs)
    if i in (2, 3, 5):                                                       # the seeded scene did reach the paths of a tick
        ev = got[2]
        assert set(ev[:, 2]) == {1, 2, 3} and got[0][..., 2].any() and (got[1][..., 7] >= 0).any()


@pytest.mark.parametrize("i,offset", [(0, 0), (2, 0), (3, 3), (4, 3), (5, 0), (5, 3)], ids=str)
def test_shapes_device_frames_and_rows_any_alignment(i, offset):
    check(shape_case(i), device=True, offset=offset)


@pytest.mark.parametrize("c", (4, 8, 16))
def test_component_scenes(c):
    for cs in LC.component_cases(c):
        _, got = check(cs)
        assert got[3][-1].any()


def test_largest_grid_spiral():
    """32768 cells (128 x 256 at c = 4): the labels and areas fill 128 KiB of LDS, and the last label is 32768 as a u16."""
    m = np.zeros((128, 256), bool)
    m[:33, :33][np.pad(LC.spiral(17), 8)] = True
    m[127, 200:] = True                                                      # a blob whose label is 127 * 256 + 200, its last cell 32767
    check(LC.pattern("largest grid", m, 4))


PLANTED = [LC.bag, LC.mirror, LC.owner_carried, LC.df_edge, LC.ds_edge, LC.jump, LC.absorb, LC.no_decay, lambda: LC.no_decay(2)]


@pytest.mark.parametrize("k", range(len(PLANTED)))
def test_planted_scenes(k):
    cs = PLANTED[k]()
    _, got = check(cs)
    if cs["name"] == "the mirror":
        assert [(e[2], e[4]) for e in got[2]] == [(LO.APPEARED, 0), (LO.RAISED, LO.REMOVED)]
    if cs["name"].startswith("owner carried"):
        assert [(e[2], e[4], e[9]) for e in got[2]] == [(LO.APPEARED, 0, 12), (LO.RAISED, LO.LEFT, 12)]


def test_bank_equals_single_stream_handles():
    cs = shape_case(5)
    S = cs["frames"].shape[1]
    bank = feed(stage_for(cs), cs)
    for s in range(S):
        one = dict(cs, frames=np.ascontiguousarray(cs["frames"][:, s:s + 1]), rows=[[tick[s]] for tick in cs["rows"]])
        got = feed(stage_for(one), one)
        for k in (0, 1, 3, 4):
            differ(NAMES[k], got[k][:, 0], bank[k][:, s], ("single", s))
        ev = bank[2][bank[2][:, 1] == s].copy()
        ev[:, 1] = 0
        differ("events", got[2], ev, ("single", s))


def test_one_call_equals_several():
    check(shape_case(5), cuts=[1, 7, 32])


@pytest.mark.parametrize("options", [(("ticks_per_launch", 1),), (("ticks_per_launch", 3),), (("launch_budget_mb", 1),)], ids=str)
@pytest.mark.parametrize("device", (False, True))
def test_launch_cuts_change_nothing(options, device):
    check(shape_case(5), options=options, device=device)                    # 55 KB per tick: 1 MiB of staged host frames is 18 ticks


def test_reset_one_stream_of_three():
    cs = shape_case(5)
    lo = stage_for(cs)
    first = dict(cs, frames=cs["frames"][:20], rows=cs["rows"][:20])
    rest = dict(cs, frames=cs["frames"][20:], rows=cs["rows"][20:])
    feed(lo, first)
    lo.reset(1)
    e = lo.export(1)
    assert not any(e[k].any() for k in EXPORTS) and lo.export(0)["age"] == 20
    got = feed(lo, rest)
    want = reference(cs)
    for s in (0, 2):
        for k in (0, 1, 3, 4):
            differ(NAMES[k], got[k][:, s], want[k][20:, s], ("undisturbed", s))
        ev = want[2][(want[2][:, 1] == s) & (want[2][:, 0] >= 20)].copy()
        ev[:, 0] -= 20
        differ("events", got[2][got[2][:, 1] == s], ev, ("undisturbed", s))
    same_export(lo, want[5], "undisturbed", streams=(0, 2))
    o = LC.oracles_for(cs)[1]                                                # stream 1 starts again at age 0, its uids at 1
    evs = [np.zeros((0, 12), np.int32)]
    for t in range(20):
        rec, obj, ev, cand, labels = o.tick(rest["frames"][t, 1], rest["rows"][t][1], t, 1)
        evs.append(ev)
        for name, g, w in zip(("records", "objects", "cand", "labels"), (got[0], got[1], got[3], got[4]), (rec, obj, cand, labels)):
            differ(name, g[t, 1], w, ("restarted", t))
    differ("events", got[2][got[2][:, 1] == 1], np.concatenate(evs), "restarted")
    assert got[0][0, 1, 0] == 0
    same_export(lo, [None, o.export()], "restarted", streams=(1,))


def test_event_overflow_reports_and_loses_no_state():
    cs = shape_case(5)
    want = reference(cs)
    lo = stage_for(cs)
    res = lo.update(cs["frames"], cs["rows"], cap_events=2)
    assert res.overflow and res.n_events == len(want[2]) > 2
    differ("events", res.events, want[2][:2], "the first two")
    differ("records", res.records, want[0], "overflow")
    differ("objects", res.objects, want[1], "overflow")
    same_export(lo, want[5], "overflow")
    L = pkg("_lib")
    lo2 = stage_for(cs)                                                      # without a status word the call itself reports it
    rec, obj, ev, n = np.zeros((40, 3, 8), np.int32), np.zeros((40, 3, 32, 12), np.int32), np.zeros((2, 12), np.int32), np.zeros(1, np.int32)
    rc = L.load().aic_left_update(lo2._h, L.ptr(cs["frames"]), L.HOST, 40, None, None, L.HOST, 2, L.ptr(rec), L.ptr(obj), L.ptr(ev), L.ptr(n), None,
                                  None, None)
    assert rc == L.ERR_CAPACITY and n[0] > 2 and lo2.export(0)["age"] == 40


def test_no_ticks_is_no_change():
    cs = shape_case(2)
    lo, _ = check(cs)
    res = lo.update(cs["frames"][:0])
    assert res.records.shape == (0, 1, 8) and len(res.events) == 0
    same_export(lo, reference(cs)[5], "after an empty call")


def _rows_of(tracks):
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    return np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks], np.int64).reshape(-1, 6).astype(np.int32)


def test_pipeline_attach_left_objects_end_to_end():
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, Scene, LOb = pkg("pipeline").TrackingPipeline, pkg("synthetic").Scene, pkg("leftobj").LeftObjects
    S, T, H, W = 2, 12, 360, 640
    scenes = [Scene(seed=81 + s, n_targets=5, width=W, height=H, w_range=(30.0, 50.0), h_range=(60.0, 100.0), y_range=(20.0, 200.0), speed=8.0,
                    conf_range=(0.8, 0.95)) for s in range(S)]
    frames = np.stack([scenes[i % S].render(i // S) for i in range(S * T)])  # tick-major: slot t * S + s
    frames[4 * S:, 320:352, 40:88] = 255                                     # a parcel appears in both cameras at tick 4 and stays
    planted = [scenes[i % S].detections(i // S)[:3] for i in range(S * T)]
    kw = dict(cell=8, warmup=2, min_ticks=2, alarm_hold=2, fast_shift=1)
    calls = ((0, 8), (8, S * T - 8))

    def run(lo):
        pipe = TP(ypath, None, (H, W), batch=8, ring_frames=S * T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=S,
                  track_buffer=3)
        pipe.upload(0, frames)
        pipe.inject(0, planted)
        if lo is not None:
            pipe.attach_left_objects(lo)
        out, results = [], []
        for lo_f, n in calls:                                                # two run calls: the stage's state carries over
            out += pipe.run(lo_f, n)[0]
            results.append(pipe.left_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    tracks, results = run(LOb(S, (H, W), **kw))
    assert tracks == plain                                                   # the tracks are untouched
    direct = LOb(S, (H, W), **kw)
    oracles = [LO.LeftOracle((H, W), **kw) for _ in range(S)]
    for (lo_f, n), got in zip(calls, results):
        fr = frames[lo_f:lo_f + n].reshape(n // S, S, H, W, 3)
        rows = [[_rows_of(tracks[lo_f + t * S + s]) for s in range(S)] for t in range(n // S)]
        ref = direct.update(fr, rows)
        want = LO.run(oracles, fr, rows)
        for name, g, r, w in zip(NAMES[:3], (got.records, got.objects, got.events), (ref.records, ref.objects, ref.events), want[:3]):
            differ(name, g, r, ("pipeline against update", lo_f))
            differ(name, g, w, ("pipeline against the oracle", lo_f))
    assert results[1].n_alarmed.any() and len(results[1].events)


def test_cli_left_objects(tmp_path, capsys):
    import json
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    srcs = ["synthetic:640x360:6:24:1", "synthetic:640x360:4:24:2"]
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--left_objects", "--left_cell", "16", "--left_after", "2", "--draw_zones", "--zones"]
    zones = tmp_path / "zones.json"
    zones.write_text(json.dumps({"cameras": [{"zones": [[[10, 10], [300, 10], [300, 300], [10, 300]]]}]}))
    for argv, name, n_lines in ((["--inputs", ",".join(srcs), "--batch", "8"], "both", 48), (["--input", srcs[0]], "one", 24)):
        out = tmp_path / name
        assert cli.main(argv + common + [str(zones), "--output_dir", str(out)]) == 0
        lines = [json.loads(l) for f in sorted(out.glob("*.jsonl")) for l in f.read_text().splitlines()]
        assert len(lines) == n_lines
        for l in lines:
            assert isinstance(l["left_objects"], list) and all(set(o) == {"uid", "kind", "box", "owner", "age"} for o in l["left_objects"])
        events = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith('{"left_object"')]
        assert all(e["left_object"] in ("appeared", "raised", "ended") and e["frame"] >= 16 for e in events)   # ready from age 16
