"""Best shots on the device (csrc/kernels_bestshot.hip) against tests/bestshot_oracle.py: integer arithmetic on
both sides, so everything -- events, thumbnails, n_final, pending, status -- is np.array_equal, call by call.  Each case is the
smallest shape that can break; tests/test_bestshot_oracle.py shows through the oracle alone that the seeded cases reach every branch."""
import json

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import bestshot_cases as BC
import bestshot_oracle as BO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

NAMES = ("n_final", "events", "thumbs", "pending", "status")
SMALL = dict(thumb=(16, 24), min_w=8, min_h=16)


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got[:5], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError((what, name, "first difference at", bad.tolist(), g[tuple(bad)], w[tuple(bad)],
                                  got[1][bad[0], :2] if name != "thumbs" else None, want[1][bad[0], :2] if name != "thumbs" else None))


def shots_for(case, options=()):
    bs = pkg("bestshot").BestShots(case["streams"], case["hw"], **case["kw"])
    for k, v in options:
        bs.option(k, v)
    return bs


def check(case, options=()):
    """The device against one oracle per stream, call by call; returns (BestShots, oracles, the device's results)."""
    bs, oracles, res = shots_for(case, options), BC.oracles_for(case), []
    for i, (frames, rows) in enumerate(case["calls"]):
        got = bs.update(frames, rows, cap=case["cap"])
        same(got, BO.run_bank(oracles, frames, rows, case["cap"]), (case["name"], "call", i))
        res.append(got)
    return bs, oracles, res


def same_export(bs, oracles, what=""):
    for s, o in enumerate(oracles):
        ev, th = bs.export(s)
        want = o.export()
        assert len(ev) == len(want), (what, s, len(ev), len(want))
        for k, (e, t) in enumerate(want):
            assert np.array_equal(ev[k], e) and np.array_equal(th[k], t), (what, s, k, ev[k], e)


def finals_of(results):
    """[(event bytes, thumbnail bytes)] over a list of results: what came out, whichever call it came out of."""
    out = []
    for r in results:
        for s, n in enumerate(r[0]):
            out += [(r[1][s, k].tobytes(), r[2][s, k].tobytes()) for k in range(int(n))]
    return out


def one_frame(hw, rows, kw, seed=0, cap=16, name="frame"):
    return BC.simple_case(name, hw, kw, cap, [[rows]], seed=seed)


@pytest.mark.parametrize("case", BC.CASES, ids=[c["name"] for c in BC.CASES])
def test_seeded_cases(case):
    bs, oracles, res = check(case)
    same_export(bs, oracles, case["name"])
    same(bs.flush(cap=3), BO.flush_bank(oracles, 3), (case["name"], "flush at cap 3"))       # the rest stays pending ...
    same(bs.drain(cap=16), BO.run_bank(oracles, np.zeros((0,)), [], 16), (case["name"], "drain"))      # ... and a drain fetches it
    same_export(bs, oracles, case["name"])


def test_largest_thumbnails():
    rows = [BC.row(10, 20, 150, 270, 1), BC.row(60, 100, 139, 199, 2), BC.row(-20, -30, 100, 120, 3), BC.row(5, 5, 40, 90, 4)]
    case = one_frame((300, 200), rows, dict(thumb=(128, 256), max_tracks=4), seed=11, name="128x256 thumbnails")
    bs, oracles, res = check(case)
    same(bs.flush(), BO.flush_bank(oracles, 4), "flush")
    assert res[0].n_final.tolist() == [0]


def test_clipping_outside_tiny_inverted_and_out_of_bound_rows():
    H, W, far = 72, 101, (1 << 20) + 1
    rows = [BC.row(-6, 20, 20, 30, 1), BC.row(W - 12, 20, 20, 30, 2), BC.row(30, -9, 20, 30, 3), BC.row(60, H - 17, 20, 30, 4),      # four edges
            BC.row(-30, -40, 20, 30, 5), BC.row(W, 10, 20, 30, 6), BC.row(10, H, 20, 30, 7),                                         # wholly outside
            BC.row(50, 50, 1, 1, 8), [40, 40, 30, 60, 9, 0], [40, 40, 60, 30, 10, 0], [far, 0, far + 9, 20, 11, 0], [0, -far, 9, 20, 12, 0],
            BC.row(-5, -5, W + 10, H + 10, 13), BC.row(0, 0, W, H, 14)]                                                            # the whole frame, clipped and not
    case = one_frame((H, W), rows, dict(max_tracks=16, **SMALL), seed=12, name="edges")
    bs, oracles, _ = check(case)
    ev, _ = bs.export(0)
    assert ev[:, 2].tolist() == [1, 2, 3, 4, 8, 13, 14] and ev[:, 7].tolist() == [1, 1, 1, 1, 0, 1, 1]
    same_export(bs, oracles)


@pytest.mark.parametrize("kw", [dict(region="head", pad=3), dict(region="head", head_q8=256, pad=0), dict(region="box", pad=64),
                                dict(region="head", head_q8=1, pad=5, min_h=4)])
def test_regions_and_pad(kw):
    rows = [BC.row(20, 10, 24, 50, 1), BC.row(2, 30, 24, 40, 2), BC.row(70, 1, 28, 60, 3), BC.row(40, 40, 30, 31, 4)]
    bs, oracles, _ = check(one_frame((72, 101), rows, dict(max_tracks=8, **dict(SMALL, **kw)), seed=13, name=str(kw)))
    same_export(bs, oracles)
    assert bs.export(0)[0][:, 7].sum() >= 2


def test_upsampling_and_uneven_windows():
    sizes = [(5, 9), (16, 24), (17, 25), (23, 47), (15, 23), (31, 5), (1, 70), (99, 1)]
    rows = [BC.row(1 + (7 * i) % 60, 1 + (5 * i) % 20, w, h, i + 1) for i, (w, h) in enumerate(sizes)]
    bs, oracles, _ = check(one_frame((72, 101), rows, dict(max_tracks=8, thumb=(16, 24), min_w=1, min_h=1), seed=14, name="windows"))
    same_export(bs, oracles)
    assert bs.export(0)[0][:, 7].tolist() == [1] * 8


def test_duplicate_ids_and_the_occluder_tie():
    a, b = BC.row(10, 10, 20, 30, 1), BC.row(14, 10, 20, 30, 2)              # equal feet: the earlier row stands in front
    lower = BC.row(12, 20, 20, 30, 3)
    ticks = [[[a, b, BC.row(60, 5, 20, 30, 1), lower, BC.row(70, 30, 20, 30, 2)]], [[b, a, lower]], [[lower, BC.row(60, 5, 30, 40, 3), b]]]
    case = BC.simple_case("ties", (72, 101), dict(max_tracks=8, **SMALL), 16, ticks, seed=15)
    bs, oracles, _ = check(case)
    same_export(bs, oracles)
    ev, _ = bs.export(0)
    assert ev[:, 6].tolist() == [2, 3, 3]                                     # sightings: the duplicates never counted


def test_512_rows_and_513_rejected():
    rng = np.random.default_rng(16)
    ids = rng.permutation(np.arange(1, 257)).repeat(2)                       # 512 rows, every id twice
    rows = [BC.row(int(x), int(y), int(w), int(h), int(i)) for (x, y), (w, h), i in
            zip(rng.integers(-10, 90, (512, 2)), rng.integers(1, 30, (512, 2)), ids)]
    case = BC.simple_case("512 rows", (72, 101), dict(max_tracks=256, forget_after=1, **SMALL), 8, [[rows], [rows[::-1]], [[]], [[]]], seed=16)
    bs, oracles, res = check(case)
    assert res[0].n_final.tolist() == [8] and res[0].pending[0] > 200 and res[0].status.tolist() == [0]
    L = pkg("_lib")
    with pytest.raises(L.AicError) as ei:
        bs.update(case["calls"][0][0][:1], [[np.zeros((513, 6), np.int32)]])
    assert ei.value.code == L.ERR_CAPACITY
    same(bs.drain(cap=300), BO.run_bank(oracles, np.zeros((0,)), [], 300), "after the rejected call")      # nothing was staged
    same_export(bs, oracles)


def test_empty_frames_no_ticks_and_immediate_expiry():
    a, b = BC.row(10, 10, 20, 30, 1), BC.row(50, 10, 20, 30, 2)
    case = BC.simple_case("forget_after 0", (72, 101), dict(max_tracks=4, forget_after=0, **SMALL), 16, [[[a, b]], [[]], [[a]], [[]], [[]]], seed=17)
    bs, oracles, res = check(case)
    assert res[0].n_final.tolist() == [3] and res[0].events[0, :3, 2].tolist() == [1, 2, 1] and res[0].events[0, :3, 0].tolist() == [BO.EXPIRED] * 3
    none = bs.update(case["calls"][0][0][:0], [], cap=16)                    # ticks = 0, nothing pending
    same(none, BO.run_bank(oracles, np.zeros((0,)), [], 16), "ticks = 0")
    assert none.n_final.tolist() == [0]
    same(bs.update(case["calls"][0][0][:1], [[BC.EMPTY]], cap=0), BO.run_bank(oracles, case["calls"][0][0][:1], [[BC.EMPTY]], 0), "cap = 0")


def test_small_cap_defers_and_loses_nothing():
    case = BC.scripted_case("cap 1", (72, 101), 2, 13, [(0, 13)], cap=1, seed=5, max_tracks=8, forget_after=1, **SMALL)
    bs, oracles, res = check(case)
    assert res[0].pending.sum() > 0
    tail = []
    while True:
        r = bs.drain(cap=1)
        same(r, BO.run_bank(oracles, np.zeros((0,)), [], 1), "drain")
        tail.append(r)
        if not r.pending.sum():
            break
    tail.append(bs.flush())
    big = dict(case, cap=64)
    bs2, _, res2 = check(big)
    assert res2[0].pending.sum() == 0
    strip = lambda fin: sorted((e[:14 * 4], t) for e, t in fin)             # noqa: E731 -- (the slot may differ: slots were freed later)
    got, want = finals_of(res + tail), finals_of(res2 + [bs2.flush()])
    assert len(got) == len(want) > 6 and strip(got) == strip(want)


def test_capacity_stop_then_export_flush_and_reset():
    a, b, c = BC.row(2, 4, 20, 30, 1), BC.row(30, 4, 20, 30, 2), BC.row(60, 4, 20, 30, 3)
    case = BC.simple_case("max_tracks 2", (72, 101), dict(max_tracks=2, **SMALL), 4, [[[a, b], [a]], [[a, b, c], [a, b]], [[a], [a]]], seed=4)
    bs, oracles, res = check(case)
    L = pkg("_lib")
    assert res[0].status.tolist() == [L.ERR_CAPACITY, 0] and 0 in bs.failed and 1 not in bs.failed and res[0].failed == bs.failed
    same_export(bs, oracles, "stopped")                                      # the shots can be rescued
    frames, rows = case["calls"][0][0][:1], [[BC.rows_of(a), BC.rows_of(a)]]
    same(bs.update(frames, rows, cap=4), BO.run_bank(oracles, frames, rows, 4), "stopped: nothing for stream 0, stream 1 goes on")
    same(bs.flush(0, cap=4), BO.flush_bank(oracles, 4, stream=0), "flush of the stopped stream")
    bs.reset(0), oracles[0].reset()
    assert not bs.failed and bs.export(0)[0].shape == (0, 16)
    got = bs.update(frames, rows, cap=4)
    same(got, BO.run_bank(oracles, frames, rows, 4), "after reset")
    assert got.status.tolist() == [0, 0]
    same_export(bs, oracles, "after reset")
    # a full table whose slots all expire in the tick makes room for as many new ids -- while the output list has room for them
    for cap in (4, 1):
        check(BC.simple_case(f"turnover at cap {cap}", (72, 101), dict(max_tracks=2, forget_after=0, **SMALL), cap, [[[a, b]], [[]], [[c, a]]], seed=6))


def test_bank_equals_singles_and_any_split():
    case = BC.scripted_case("bank of 3", (72, 101), 3, 13, [(0, 13)], seed=7, max_tracks=8, forget_after=2, **SMALL)
    bs, oracles, res = check(case)
    frames, rows = case["calls"][0]
    res = res + [bs.flush()]
    per_stream = lambda results, s: [x for r in results for x in finals_of([(r[0][s:s + 1], r[1][s:s + 1], r[2][s:s + 1])])]      # noqa: E731
    assert sum(len(per_stream(res, s)) for s in range(3)) > 6
    for s in range(3):                                                       # the bank's stream s == a single-stream handle
        one = pkg("bestshot").BestShots(1, case["hw"], **case["kw"])
        got = one.update(np.ascontiguousarray(frames[:, s:s + 1]), [[r[s]] for r in rows], cap=16)
        ev = got.events[0].copy()
        ev[:got.n_final[0], 1] = s
        assert got.n_final[0] == res[0].n_final[s] and np.array_equal(ev, res[0].events[s]) and np.array_equal(got.thumbs[0], res[0].thumbs[s])
    for splits in ([(0, 3), (3, 6), (6, 13)], [(t, t + 1) for t in range(13)], [(0, 0), (0, 6), (6, 6), (6, 13)]):
        parts = dict(case, calls=[(np.ascontiguousarray(frames[a:b]), rows[a:b]) for a, b in splits])
        bs2, _, res2 = check(parts)
        res2 = res2 + [bs2.flush()]
        for s in range(3):                                                   # the same sequence of finals, stream by stream
            assert per_stream(res2, s) == per_stream(res, s), (splits, s)


def test_six_ticks_split_three_ways():
    case = BC.scripted_case("six ticks", (72, 101), 1, 12, [(6, 12)], seed=8, max_tracks=8, forget_after=0, **SMALL)
    frames, rows = case["calls"][0]
    runs = []
    for splits in ([(0, 6)], [(0, 3), (3, 6)], [(t, t + 1) for t in range(6)]):
        bs, _, res = check(dict(case, calls=[(np.ascontiguousarray(frames[a:b]), rows[a:b]) for a, b in splits]))
        runs.append(finals_of(res + [bs.flush()]))
    assert runs[0] == runs[1] == runs[2] and len(runs[0]) > 3


def test_bank_of_256_streams():
    rng = np.random.default_rng(9)
    S, T = 256, 3
    frames = rng.integers(0, 256, (T, S, 32, 32, 3)).astype(np.uint8)
    rows = [[BC.rows_of(*[BC.row(int(x), int(y), 12, 20, int(i)) for (x, y), i in zip(rng.integers(-4, 24, (2, 2)), rng.choice(5, 2, replace=False))])
             for _ in range(S)] for _ in range(T)]
    case = dict(name="256 streams", hw=(32, 32), streams=S, kw=dict(thumb=(16, 16), max_tracks=4, forget_after=0), cap=4, calls=[(frames, rows)])
    bs, oracles, res = check(case)
    assert res[0].n_final.sum() > 256 and res[0].events[:, :, 7].sum() > 256
    same(bs.flush(), BO.flush_bank(oracles, 4), "flush")


def test_host_and_device_memory_are_the_same():
    case = BC.scripted_case("memory", (72, 101), 2, 12, [(0, 12)], seed=10, max_tracks=8, forget_after=2, **SMALL)
    frames, rows = case["calls"][0]
    flat = np.concatenate([r for tick in rows for r in tick])
    counts = np.array([len(r) for tick in rows for r in tick], np.int32)
    a, b, c, d = (shots_for(case) for _ in range(4))
    ra = a.update(frames, rows, cap=16)
    rb = b.update(torch.from_numpy(frames).cuda(), torch.from_numpy(flat).cuda(), counts=torch.from_numpy(counts).cuda(), cap=16)
    rc = c.update(frames, flat, counts=counts, cap=16)
    rd = d.update(torch.from_numpy(frames).cuda(), torch.from_numpy(flat).cuda(), counts=counts.tolist(), cap=16)
    assert ra.n_final.sum() > 2
    for r, what in ((rb, "device"), (rc, "flat host"), (rd, "device rows, host counts")):
        same(r, ra[:5], what)
    fa = a.flush()
    for x, what in ((b, "device"), (c, "flat host"), (d, "device rows, host counts")):
        same(x.flush(), fa[:5], ("flush", what))


@pytest.mark.parametrize("options", [(("ticks_per_launch", 1),), (("ticks_per_launch", 5),), (("launch_budget_mb", 1),)])
def test_launch_chunking(options):
    case = BC.scripted_case("chunks", (72, 101), 2, 13, [(0, 13)], seed=1, max_tracks=8, forget_after=2, **SMALL)
    bs, oracles, res = check(case, options)
    plain, _, res0 = check(case)
    same(res[0], res0[0][:5], options)
    same(bs.flush(), plain.flush()[:5], "flush")


# ---------------------------------------------------------------------------------------------------- end to end
def _tuples_to_rows(tracks):
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    return np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tracks], np.int32).reshape(-1, 6)


def test_pipeline_attach_best_shots_end_to_end():
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, Scene, B = pkg("pipeline").TrackingPipeline, pkg("synthetic").Scene, pkg("bestshot")
    S, T, H, W = 2, 16, 360, 640
    scenes = [Scene(seed=81 + s, n_targets=5, width=W, height=H, w_range=(30.0, 50.0), h_range=(60.0, 100.0), y_range=(20.0, 200.0), speed=8.0,
                    conf_range=(0.8, 0.95), gaps=[(0, 4, 16), (1, 6, 16)]) for s in range(S)]
    frames = np.stack([scenes[i % S].render(i // S) for i in range(S * T)])  # tick-major: slot t * S + s
    planted = [scenes[i % S].detections(i // S)[:3] for i in range(S * T)]
    kw = dict(thumb=(32, 64), max_tracks=16, forget_after=2)

    def run(bs):
        pipe = TP(ypath, None, (H, W), batch=8, ring_frames=S * T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=S,
                  track_buffer=3)
        pipe.upload(0, frames)
        pipe.inject(0, planted)
        if bs is not None:
            pipe.attach_best_shots(bs)
        out, results = [], []
        for lo, n in ((0, 16), (16, S * T - 16)):                            # two run calls: the stage's state carries over
            out += pipe.run(lo, n)[0]
            results.append(pipe.best_shot_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    bs = B.BestShots(S, (H, W), **kw)
    tracks, results = run(bs)
    assert tracks == plain                                                   # the tracks are untouched
    direct = B.BestShots(S, (H, W), **kw)
    oracles = [BO.BestShotOracle((H, W), stream=s, **kw) for s in range(S)]
    for (lo, n), got in zip(((0, 16), (16, S * T - 16)), results):
        fr = frames[lo:lo + n].reshape(n // S, S, H, W, 3)
        rows = [[_tuples_to_rows(tracks[lo + t * S + s]) for s in range(S)] for t in range(n // S)]
        same(got, direct.update(fr, rows, cap=16)[:5], ("pipeline against update", lo))
        same(got, BO.run_bank(oracles, fr, rows, 16), ("pipeline against the oracle", lo))
    last = bs.flush()
    same(last, direct.flush()[:5], "flush")
    assert sum(int(r.n_final.sum()) for r in results) + int(last.n_final.sum()) > 2 and last.events[:, :, 7].sum() > 0
    # a host call hands its own array over: the same result from run_from_host
    pipe = TP(ypath, None, (H, W), batch=8, ring_frames=S * T, max_persons=64, dtype="fp16", tracker="bytetrack", streams=S)
    again = B.BestShots(S, (H, W), **kw)
    pipe.attach_best_shots(again)
    nt, rows, _ = pipe.run_raw_from_host(np.ascontiguousarray(frames[:8]))
    got = pipe.best_shot_result
    ref = B.BestShots(S, (H, W), **kw)
    same(got, ref.update(frames[:8].reshape(4, S, H, W, 3), [[rows[t * S + s, :nt[t * S + s]] for s in range(S)] for t in range(4)], cap=16)[:5],
         "run_raw_from_host")
    pipe.close()


def test_update_tuples():
    B = pkg("bestshot")
    frame = BC.texture(np.random.default_rng(3), 72, 101)[None, None]
    cls = pkg("config").CLASSES[0]
    bs, ref = B.BestShots(1, (72, 101), **SMALL), B.BestShots(1, (72, 101), **SMALL)
    bs.update_tuples(frame, [[[(10, 10, 29, 39, 7, cls, 0.9), (50, 10, 69, 39, 8, "no such class", 0.8)]]])
    ref.update(frame, [[BC.rows_of([10, 10, 29, 39, 7, 0], [50, 10, 69, 39, 8, -1])]])
    a, b = bs.export(0), ref.export(0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][:, 3].tolist() == [0, -1]


def test_cli_best_shots(tmp_path, monkeypatch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli, B = pkg("cli"), pkg("bestshot")
    seen = []
    real = B.finals
    monkeypatch.setattr(B, "finals", lambda result: seen.append(real(result)) or seen[-1])
    srcs = ["synthetic:640x360:6:16:1", "synthetic:640x360:4:16:2"]
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--best_shot_size", "32x64", "--no_save"]
    class Planted:
        """The scene's own boxes in place of the seeded detector's: the frame-by-frame run then has tracks to show."""

        def __init__(self, **kw):
            self.scene, self.i = pkg("synthetic").Scene(seed=1, n_targets=6, width=640, height=360, conf_range=(0.8, 0.95)), 0

        def detect(self, frame):
            self.i += 1
            return self.scene.detections(self.i - 1)

    runs = ((["--inputs", ",".join(srcs), "--batch", "8"], "both"), (["--input", srcs[0]], "one"), (["--input", srcs[0], "--batch", "8"], "batched"),
            (["--input", srcs[0]], "planted"))
    for argv, name in runs:
        del seen[:]
        if name == "planted":
            monkeypatch.setattr(cli, "YOLODetector", Planted)
        out = tmp_path / name
        assert cli.main(argv + common + ["--best_shots", str(out)]) == 0
        finals = [f for batch in seen for f in batch]
        lines = [json.loads(l) for l in (out / "index.jsonl").read_text().splitlines()]
        assert len(lines) == len(finals)
        shown = [(ev, th) for ev, th in finals if ev["has_shot"]]
        files = sorted(p.name for p in out.glob("*.ppm"))
        assert files == sorted(l["file"] for l in lines if l["file"]) and len(files) == len(shown)
        for ev, th in shown:
            raw = (out / f"cam{ev['stream']}_id{ev['id']}_f{ev['best_frame']}.ppm").read_bytes()
            head = b"P6\n32 64\n255\n"
            assert raw.startswith(head) and raw[len(head):] == th[:, :, ::-1].tobytes()
        for l, (ev, _) in zip(lines, finals):
            assert l["reason"] in ("expired", "flushed") and all(l[k] == ev[k] for k in ("stream", "id", "cls", "best_frame", "score", "sightings"))
        print(name, "finals", len(finals), "files", len(files))
        assert name != "planted" or len(files) >= 3
