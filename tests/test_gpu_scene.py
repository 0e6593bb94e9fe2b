"""Scene watch on the device (csrc/kernels_scene.hip) against tests/scene_oracle.py: integer arithmetic on both
sides, so everything -- records, masks, row_motion, the exported bg / dev / prev planes and scalars -- is np.array_equal.  Each case is
the smallest shape that can break; tests/test_scene_oracle.py shows through the oracle alone what the planted scenes do."""
import json

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import scene_cases as SC
import scene_oracle as SO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

_REF = {}


def reference(cs):
    """(records, masks, row_motion, [export per stream]) of the oracle over the whole case, computed once per case name."""
    if cs["name"] not in _REF:
        o = SC.oracles_for(cs)
        _REF[cs["name"]] = SO.run(o, cs["frames"], cs["rows"]) + ([x.export() for x in o],)
    return _REF[cs["name"]]


def watch_for(cs, streams=None, options=()):
    sw = pkg("scene").SceneWatch(streams or cs["frames"].shape[1], cs["hw"], cs["cell"], **cs["options"])
    for k, v in options:
        sw.set_option(k, v)
    return sw


def differ(name, g, w, what):
    assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError((what, name, len(bad), "differences, the first at", bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def same_export(sw, exports, what="", streams=None):
    for s in streams if streams is not None else range(len(exports)):
        e = sw.export(s)
        for name, w in zip(("bg", "dev", "prev", "scalars"), exports[s]):
            differ(f"export {name} of stream {s}", e[name], w, what)


def feed(sw, cs, cuts=None, device=False, offset=0):
    """The case through the device in calls of `cuts` ticks; returns (records, masks, row_motion) of all calls joined."""
    frames, rows = cs["frames"], cs["rows"]
    T = len(frames)
    recs, masks, rm, lo = [], [], [], 0
    for n in cuts or [T]:
        fr = frames[lo:lo + n]
        r = None if rows is None else rows[lo:lo + n]
        if device:
            raw = torch.zeros(fr.size + offset + 16, dtype=torch.uint8, device="cuda")
            raw[offset:offset + fr.size] = torch.from_numpy(fr.reshape(-1)).cuda()
            fr_d = raw[offset:offset + fr.size].view(fr.shape)
            assert fr_d.data_ptr() % 16 == offset
            if r is not None:
                flat = [x for tick in r for x in tick]
                counts = torch.tensor([len(x) for x in flat], dtype=torch.int32).cuda()
                allrows = torch.from_numpy(np.concatenate(flat + [np.zeros((0, 6), np.int32)])).cuda().contiguous()
                res = sw.update(fr_d, allrows, counts, want_masks=True)
            else:
                res = sw.update(fr_d, want_masks=True)
        else:
            res = sw.update(fr, r, want_masks=True)
        recs.append(res.records), masks.append(res.masks)
        if res.row_motion is not None:
            rm.append(res.row_motion)
        lo += n
    assert lo == T
    return np.concatenate(recs), np.concatenate(masks), np.concatenate(rm) if rm else np.zeros(0, np.int32)


def check(cs, what=None, **kw):
    sw = watch_for(cs, options=kw.pop("options", ()))
    got = feed(sw, cs, **kw)
    want = reference(cs)
    for name, g, w in zip(("records", "masks", "row_motion"), got, want):
        differ(name, g, w, what or cs["name"])
    same_export(sw, want[3], what or cs["name"])
    return sw, got


SHAPES = [("37x53 c4: 3 W = 159, no aligned load", (37, 53), 4, 1, 40), ("64x96 c8: every row 16-byte aligned", (64, 96), 8, 1, 40),
          ("48x80 c16", (48, 80), 16, 1, 40), ("8x200 c8: one cell row, no interior", (8, 200), 8, 1, 40),
          ("16x2100 c4: 525 cells wide", (16, 2100), 4, 1, 40), ("three streams", (16, 24), 8, 3, 40), ("256 streams", (16, 24), 8, 256, 20),
          ("one tick", (64, 96), 8, 1, 1), ("two ticks", (37, 53), 4, 3, 2), ("80x272 c4: two tile rows, two tile columns", (80, 272), 4, 1, 10)]


def shape_case(i):
    name, hw, cell, S, T = SHAPES[i]
    return SC.seeded(name, hw, cell, streams=S, ticks=T, seed=20 + i)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=[s[0] for s in SHAPES])
def test_shapes_host_frames(i):
    cs = shape_case(i)
    _, got = check(cs)
    if cs["frames"].shape[0] == 40:                                          # the seeded scene did reach every branch of a tick
        recs = got[0]
        assert recs[..., 15].any() and (recs[..., 15] >> 8).any() and recs[..., 3].any() and (recs[..., 2] == 0).any()


@pytest.mark.parametrize("i", (0, 1, 2, 4, 5), ids=[SHAPES[i][0] for i in (0, 1, 2, 4, 5)])
@pytest.mark.parametrize("offset", (0, 3))
def test_shapes_device_frames_and_rows_any_alignment(i, offset):
    check(shape_case(i), device=True, offset=offset)


PLANTED = [lambda: SC.noise_mover(2), lambda: SC.noise_mover(6), lambda: SC.noise_mover(12), SC.threshold_edge, SC.floor_shift, lambda: SC.cleanup(3),
           lambda: SC.cleanup(2), lambda: SC.alarm_scene("dark"), lambda: SC.alarm_scene("defocus"), lambda: SC.alarm_scene("frozen"),
           lambda: SC.alarm_scene("scene"), SC.gate_scene]


@pytest.mark.parametrize("k", range(len(PLANTED)))
def test_planted_scenes(k):
    cs = PLANTED[k]()
    sw, got = check(cs)
    if "sigma" in cs:                                                        # what test_scene_oracle.py asserts of the oracle, of the device
        assert not got[1][20:60].any() and (got[0][60:, 0, 3] >= 21).all()
    if cs["name"].startswith("alarm"):
        res = pkg("scene").SceneResult(got[0], None, None, None)
        assert (12, 0, cs["kind"], True) in res.events()


def test_bank_equals_single_stream_handles():
    cs = shape_case(5)
    S = cs["frames"].shape[1]
    bank = feed(watch_for(cs), cs)
    off = np.concatenate([[0], np.cumsum([len(r) for tick in cs["rows"] for r in tick])])
    for s in range(S):
        one = dict(cs, frames=np.ascontiguousarray(cs["frames"][:, s:s + 1]), rows=[[tick[s]] for tick in cs["rows"]])
        recs, masks, rm = feed(watch_for(one), one)
        differ("records", recs[:, 0], bank[0][:, s], ("single", s))
        differ("masks", masks[:, 0], bank[1][:, s], ("single", s))
        want = np.concatenate([bank[2][off[t * S + s]:off[t * S + s + 1]] for t in range(len(recs))])
        differ("row_motion", rm, want, ("single", s))


@pytest.mark.parametrize("cuts", [(1, 7, 32), (39, 1), (1,) * 5 + (35,)], ids=str)
def test_one_call_equals_several(cuts):
    check(shape_case(5), cuts=list(cuts))


@pytest.mark.parametrize("options", [(("ticks_per_launch", 1),), (("ticks_per_launch", 5),), (("launch_budget_mb", 1),)], ids=str)
@pytest.mark.parametrize("device", (False, True))
def test_launch_cuts_change_nothing(options, device):
    cs = SC.seeded("launch cuts", (64, 96), 8, streams=3, ticks=40, seed=7)  # 55 KB per tick: 1 MiB of staged host frames is 18 ticks
    check(cs, options=options, device=device)


def test_reset_one_stream_of_three():
    cs = shape_case(5)
    sw = watch_for(cs)
    first = dict(cs, frames=cs["frames"][:20], rows=cs["rows"][:20])
    rest = dict(cs, frames=cs["frames"][20:], rows=cs["rows"][20:])
    feed(sw, first)
    sw.reset(1)
    assert sw.export(1)["scalars"].tolist() == [0] * 16 and sw.export(0)["age"] == 20
    got = feed(sw, rest)
    want = reference(cs)
    for s in (0, 2):
        differ("records", got[0][:, s], want[0][20:, s], ("undisturbed", s))
        differ("masks", got[1][:, s], want[1][20:, s], ("undisturbed", s))
    same_export(sw, want[3], "undisturbed", streams=(0, 2))
    o = SC.oracles_for(cs)[1]                                                # stream 1 starts again at age 0
    for t in range(20):
        rec, mask, _ = o.tick(rest["frames"][t, 1])
        differ("records", got[0][t, 1], rec, ("restarted", t))
        differ("masks", got[1][t, 1], mask, ("restarted", t))
    assert got[0][0, 1, 0] == 0
    same_export(sw, [None, o.export()], "restarted", streams=(1,))
    sw.reset()
    assert all(sw.export(s)["scalars"].tolist() == [0] * 16 for s in range(3))


def test_rows_none_0_512_and_513():
    L = pkg("_lib")
    base = SC.seeded("rows", (48, 80), 8, streams=2, ticks=10, seed=9, with_rows=False, options=dict(warmup=1))
    rng = np.random.default_rng(5)
    full = [[SC.rows_for(rng, base["hw"], 512 if (t + s) % 2 else 0) for s in range(2)] for t in range(10)]
    cs = dict(base, name="rows 0 and 512", rows=full)
    sw, got = check(cs)
    assert len(got[2]) == 512 * 10 and (got[2] > 0).any() and (got[2] == 0).any() and (got[2] == -1).any()
    check(cs, "device rows", device=True)
    plain = feed(watch_for(base), base)                                      # no rows at all: the same records, no row_motion
    differ("records", plain[0], got[0], "without rows")
    assert len(plain[2]) == 0
    before = [sw.export(s) for s in range(2)]
    over = [[SC.rows_for(rng, base["hw"], 513 if (t, s) == (5, 1) else 1) for s in range(2)] for t in range(10)]
    with pytest.raises(L.AicError) as ei:
        sw.update(base["frames"], over)
    assert ei.value.code == L.ERR_CAPACITY
    for s in range(2):                                                       # rejected before anything was staged: nothing moved
        assert all(np.array_equal(before[s][k], sw.export(s)[k]) for k in ("bg", "dev", "prev", "scalars"))


def test_no_ticks_is_no_change():
    cs = shape_case(7)
    sw, _ = check(cs)
    res = sw.update(cs["frames"][:0])
    assert res.records.shape == (0, 1, 16) and res.events() == []
    same_export(sw, reference(cs)[3], "after an empty call")


def _rows_of(tracks):
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    return np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks], np.int64).reshape(-1, 6).astype(np.int32)


def test_pipeline_attach_scene_watch_end_to_end():
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, Scene, SW = pkg("pipeline").TrackingPipeline, pkg("synthetic").Scene, pkg("scene").SceneWatch
    S, T, H, W = 2, 12, 360, 640
    scenes = [Scene(seed=81 + s, n_targets=5, width=W, height=H, w_range=(30.0, 50.0), h_range=(60.0, 100.0), y_range=(20.0, 200.0), speed=8.0,
                    conf_range=(0.8, 0.95)) for s in range(S)]
    frames = np.stack([scenes[i % S].render(i // S) for i in range(S * T)])  # tick-major: slot t * S + s
    planted = [scenes[i % S].detections(i // S)[:3] for i in range(S * T)]
    kw = dict(cell=8, warmup=3, hold=2)
    calls = ((0, 8), (8, S * T - 8))

    def run(sw):
        pipe = TP(ypath, None, (H, W), batch=8, ring_frames=S * T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=S,
                  track_buffer=3)
        pipe.upload(0, frames)
        pipe.inject(0, planted)
        if sw is not None:
            pipe.attach_scene_watch(sw)
        out, results = [], []
        for lo, n in calls:                                                  # two run calls: the stage's state carries over
            out += pipe.run(lo, n)[0]
            results.append(pipe.scene_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    tracks, results = run(SW(S, (H, W), **kw))
    assert tracks == plain                                                   # the tracks are untouched
    direct = SW(S, (H, W), **kw)
    oracles = [SO.SceneOracle((H, W), **kw) for _ in range(S)]
    for (lo, n), got in zip(calls, results):
        fr = frames[lo:lo + n].reshape(n // S, S, H, W, 3)
        rows = [[_rows_of(tracks[lo + t * S + s]) for s in range(S)] for t in range(n // S)]
        ref = direct.update(fr, rows)
        want = SO.run(oracles, fr, rows)
        differ("records", got.records, ref.records, ("pipeline against update", lo))
        differ("row_motion", got.row_motion, ref.row_motion, ("pipeline against update", lo))
        differ("records", got.records, want[0], ("pipeline against the oracle", lo))
        differ("row_motion", got.row_motion, want[2], ("pipeline against the oracle", lo))
    assert results[1].n_moving.any() and sum(len(r.row_motion) for r in results) > 0 and (results[1].row_motion > 0).any()


def test_cli_scene_watch(tmp_path):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    srcs = ["synthetic:640x360:6:12:1", "synthetic:640x360:4:12:2"]
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--scene_watch", "--scene_cell", "16"]
    for argv, name, n_lines in ((["--inputs", ",".join(srcs), "--batch", "8"], "both", 24), (["--input", srcs[0]], "one", 12)):
        out = tmp_path / name
        assert cli.main(argv + common + ["--output_dir", str(out)]) == 0
        lines = [json.loads(l) for f in sorted(out.glob("*.jsonl")) for l in f.read_text().splitlines()]
        assert len(lines) == n_lines
        for l in lines:
            sc = l["scene"]
            assert set(sc) == {"active", "moving_cells", "motion_box", "alarms"} and sc["alarms"] == [] and len(sc["motion_box"]) == 4
            assert sc["active"] is True and sc["moving_cells"] == 0          # 12 frames: still warming up
            assert len(l["moving"]) == len(l["tracks"]) and all(-1 <= m <= 256 for m in l["moving"])
