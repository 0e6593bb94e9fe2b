"""Clothing colours on the device (csrc/kernels_colours.hip) against tests/colours_oracle.py: integer arithmetic
on both sides, so everything -- n_final, events, row_tags, pending, status -- is np.array_equal, call by call.  Each case is the smallest
shape that can break; tests/test_colours_oracle.py shows through the oracle alone that the seeded cases reach every branch."""
import json

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import colours_cases as CC
import colours_oracle as CO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

NAMES = ("n_final", "events", "row_tags", "pending", "status")
NO_FRAMES = np.zeros((0,))


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got[:5], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError((what, name, "first difference at", bad.tolist(), g[tuple(bad)], w[tuple(bad)], g[tuple(bad[:-1])], w[tuple(bad[:-1])]))


def stage_for(case, options=()):
    tc = pkg("colours").TrackColours(case["streams"], case["hw"], **case["kw"])
    for k, v in options:
        tc.option(k, v)
    return tc


def check(case, options=()):
    """The device against one oracle per stream, call by call; returns (TrackColours, oracles, the device's results)."""
    tc, oracles, res = stage_for(case, options), CC.oracles_for(case), []
    for i, (frames, rows) in enumerate(case["calls"]):
        got = tc.update(frames, rows, cap=case["cap"])
        same(got, CO.run_bank(oracles, frames, rows, case["cap"]), (case["name"], "call", i))
        res.append(got)
    return tc, oracles, res


def same_export(tc, oracles, what=""):
    for s, o in enumerate(oracles):
        ev, want = tc.export(s), o.export()
        assert len(ev) == len(want), (what, s, len(ev), len(want))
        for k, e in enumerate(want):
            assert np.array_equal(ev[k], e), (what, s, k, ev[k], e)


def finals_of(results, s=None):
    """[event bytes] over a list of results: what came out, whichever call it came out of."""
    return [r[1][q, k].tobytes() for r in results for q, n in enumerate(r[0]) if s in (None, q) for k in range(int(n))]


def one_frame(hw, rows, kw, seed=0, cap=16, name="frame", frames=None):
    return CC.simple_case(name, hw, kw, cap, [[rows]], seed=seed, frames=frames)


# ---------------------------------------------------------------------------------------------------- pixels
@pytest.mark.parametrize("hw", [(48, 64), (37, 61)], ids=["48x64", "37x61 (3 W % 4 != 0)"])
def test_pixels_threshold_set_and_noise_at_every_alignment(hw):
    """Tiles of at most 256 pixels a part over frames that hold the whole threshold set: one pixel named wrongly changes a share.  The
    tiles start at every x1 mod 4 and have widths 13..16, so rows of 1, 2, 3 and 4 pixels in the last item of a pixel row occur."""
    frames = CC.pixel_frames(hw, seed=31, ticks=4)
    assert len(CC.threshold_set()) <= len(frames) * hw[0] * hw[1] * 3 // 4
    ticks = [[CC.tiles(hw, 13 + (t + x0) % 4, 16, x0=x0 if t < 4 else 0, y0=0)] for t, x0 in zip(range(len(frames)), [0, 1, 2, 3] * len(frames))]
    case = CC.simple_case(f"pixels {hw}", hw, dict(CC.PIXEL_KW, forget_after=0), 512, ticks, frames=frames)
    tc, oracles, res = check(case)
    assert oracles[0].log["sampled"] >= 80 and oracles[0].log["covered"] == 0
    same(tc.flush(cap=512), CO.flush_bank(oracles, 512), "flush")


def test_pixels_one_wide_whole_frame_and_outside():
    hw = (37, 61)
    frames = CC.pixel_frames(hw, seed=32)[:1]
    rows = [CC.row(17, 3, 1, 30, 1), CC.row(0, 0, 61, 37, 2), CC.row(-3, -2, 70, 45, 3), CC.row(70, 5, 10, 10, 4), CC.row(5, -30, 10, 20, 5),
            CC.row(58, 30, 9, 9, 6), CC.row(1, 1, 2, 2, 7), CC.row(2, 5, 3, 9, 8), CC.row(3, 9, 5, 1, 9)]
    for kw in (dict(CC.PIXEL_KW), dict(max_tracks=16, min_w=1, min_h=1), dict(max_tracks=16)):
        tc, oracles, _ = check(one_frame(hw, rows, kw, frames=frames, name=str(kw)))
        same_export(tc, oracles, str(kw))
        assert tc.export(0)[:, 2].tolist() == [1, 2, 3, 6, 7, 8, 9]           # the two boxes outside the frame are not counted


# ---------------------------------------------------------------------------------------------------- rows
def test_0_1_512_rows_and_513_rejected():
    rng = np.random.default_rng(16)
    ids = rng.permutation(np.arange(1, 257)).repeat(2)                       # 512 rows, every id twice
    rows = [CC.row(int(x), int(y), int(w), int(h), int(i)) for (x, y), (w, h), i in
            zip(rng.integers(-10, 90, (512, 2)), rng.integers(1, 30, (512, 2)), ids)]
    case = CC.simple_case("512 rows", (72, 101), dict(max_tracks=256, forget_after=1, max_cover_q8=230, min_w=1, min_h=1), 8, [[rows], [rows[::-1]], [[]], [rows[:1]], [[]], [[]]],
                          seed=16)
    tc, oracles, res = check(case)
    assert res[0].n_final.tolist() == [8] and res[0].pending[0] > 200 and res[0].status.tolist() == [0] and res[0].row_tags.shape == (1025, 4)
    assert oracles[0].log["covered"] > 50 and oracles[0].log["sampled"] > 50
    L = pkg("_lib")
    with pytest.raises(L.AicError) as ei:
        tc.update(case["calls"][0][0][:1], [[np.zeros((513, 6), np.int32)]])
    assert ei.value.code == L.ERR_CAPACITY
    same(tc.drain(cap=300), CO.run_bank(oracles, NO_FRAMES, [], 300), "after the rejected call")      # nothing was staged
    same_export(tc, oracles)


def test_duplicate_ids_invalid_rows_between_and_the_occluder_tie():
    far = (1 << 20) + 1
    a, b = CC.row(10, 10, 20, 40, 1), CC.row(14, 10, 20, 40, 2)              # equal feet: the earlier row stands in front
    lower = CC.row(12, 20, 20, 40, 3)
    bad = [[40, 40, 30, 60, 9, 0], [far, 0, far + 9, 20, 1, 0], [0, -far, 9, 20, 2, 0]]
    ticks = [[[a, bad[0], b, CC.row(60, 5, 20, 40, 1), bad[1], lower, CC.row(70, 30, 20, 30, 2)]], [[bad[2], b, a, lower]],
             [[lower, bad[1], CC.row(60, 5, 30, 40, 3), b]]]
    case = CC.simple_case("ties", (72, 101), dict(max_tracks=8, max_cover_q8=100), 16, ticks, seed=15)
    tc, oracles, res = check(case)
    same_export(tc, oracles)
    ev = tc.export(0)
    assert ev[:, 2].tolist() == [1, 2, 3] and ev[:, 6].tolist() == [2, 3, 3]  # sightings: the duplicates and the invalid rows never counted
    assert (res[0].row_tags[[1, 3, 4, 6]] == -1).all() and oracles[0].log["covered"] >= 2


# ---------------------------------------------------------------------------------------------------- memory
def test_host_and_device_memory_at_byte_offset_3_are_the_same():
    case = CC.scripted_case("memory", (61, 61), 2, 12, [(0, 12)], seed=10, big=(14, 30), max_tracks=8, forget_after=2)
    frames, rows = case["calls"][0]
    flat = np.concatenate([r for tick in rows for r in tick])
    counts = np.array([len(r) for tick in rows for r in tick], np.int32)
    a, b, c, d = (stage_for(case) for _ in range(4))
    ra = a.update(frames, rows, cap=16)
    same(ra, CO.run_bank(CC.oracles_for(case), frames, rows, 16), "host")
    raw = torch.zeros(frames.size + 3, dtype=torch.uint8, device="cuda")
    raw[3:] = torch.from_numpy(frames.reshape(-1)).cuda()
    dev_frames = raw[3:].view(frames.shape)                                  # device memory at byte offset 3
    assert dev_frames.data_ptr() % 4 == 3
    rb = b.update(dev_frames, torch.from_numpy(flat).cuda(), counts=torch.from_numpy(counts).cuda(), cap=16)
    rc = c.update(frames, flat, counts=counts, cap=16)
    rd = d.update(dev_frames, torch.from_numpy(flat).cuda(), counts=counts.tolist(), cap=16)
    assert ra.n_final.sum() > 2
    for r, what in ((rb, "device"), (rc, "flat host"), (rd, "device rows, host counts")):
        same(r, ra[:5], what)
    fa = a.flush()
    for x, what in ((b, "device"), (c, "flat host"), (d, "device rows, host counts")):
        same(x.flush(), fa[:5], ("flush", what))


# ---------------------------------------------------------------------------------------------------- equivalences
def test_bank_of_3_equals_three_single_stream_handles():
    case = CC.scripted_case("bank of 3", (72, 101), 3, 13, [(0, 13)], seed=7, max_tracks=8, forget_after=2)
    tc, oracles, res = check(case)
    frames, rows = case["calls"][0]
    last = tc.flush()
    assert len(finals_of(res + [last])) > 6
    counts = np.array([[len(r) for r in tick] for tick in rows])
    off = np.concatenate([[0], np.cumsum(counts.reshape(-1))])
    for s in range(3):
        one = pkg("colours").TrackColours(1, case["hw"], **case["kw"])
        got = one.update(np.ascontiguousarray(frames[:, s:s + 1]), [[r[s]] for r in rows], cap=16)
        ev = got.events[0].copy()
        ev[:got.n_final[0], 1] = s
        assert got.n_final[0] == res[0].n_final[s] and np.array_equal(ev, res[0].events[s])
        tags = np.concatenate([res[0].row_tags[off[t * 3 + s]:off[t * 3 + s + 1]] for t in range(13)])
        assert np.array_equal(got.row_tags, tags), s
        fl = one.flush()
        ev = fl.events[0].copy()
        ev[:fl.n_final[0], 1] = s
        assert np.array_equal(ev, last.events[s])


def test_one_40_tick_call_equals_calls_of_1_7_and_32_ticks():
    case = CC.scripted_case("40 ticks", (72, 101), 2, 40, [(0, 40)], seed=8, max_tracks=8, forget_after=3)
    tc, oracles, res = check(case)
    frames, rows = case["calls"][0]
    whole = res + [tc.flush()]
    parts = dict(case, calls=[(np.ascontiguousarray(frames[a:b]), rows[a:b]) for a, b in ((0, 1), (1, 8), (8, 40))])
    tc2, _, res2 = check(parts)
    split = res2 + [tc2.flush()]
    for s in range(2):
        assert finals_of(split, s) == finals_of(whole, s) and len(finals_of(whole, s)) > 3
    assert np.array_equal(np.concatenate([r.row_tags for r in res2]), res[0].row_tags)


@pytest.mark.parametrize("options", [(("ticks_per_launch", 1),), (("ticks_per_launch", 3),), (("launch_budget_mb", 1),)])
def test_launch_chunking(options):
    case = CC.scripted_case("chunks", (360, 640) if options[0][0] == "launch_budget_mb" else (72, 101), 2, 13, [(0, 13)], seed=1, max_tracks=8,
                            forget_after=2)                                  # (two frames of 360 x 640 are 1.3 MB: one tick per launch)
    tc, oracles, res = check(case, options)
    plain = stage_for(case)
    same(res[0], plain.update(*case["calls"][0], cap=case["cap"])[:5], options)
    same(tc.flush(), plain.flush()[:5], "flush")


def test_reset_of_one_stream_of_three():
    case = CC.scripted_case("reset", (72, 101), 3, 12, [(0, 6), (6, 12)], seed=9, max_tracks=8, forget_after=2)
    tc, oracles = stage_for(case), CC.oracles_for(case)
    other = stage_for(case)                                                  # the same bank, never reset
    f0, r0 = case["calls"][0]
    f1, r1 = case["calls"][1]
    same(tc.update(f0, r0), CO.run_bank(oracles, f0, r0, 16), "before")
    other.update(f0, r0)
    tc.reset(1), oracles[1].reset()
    assert len(tc.export(1)) == 0
    got, ref = tc.update(f1, r1), other.update(f1, r1)
    same(got, CO.run_bank(oracles, f1, r1, 16), "after")
    for s in (0, 2):                                                         # the others: bit-identical to the bank that was not reset
        assert np.array_equal(got.events[s], ref.events[s]) and got.n_final[s] == ref.n_final[s]
        assert np.array_equal(tc.export(s), other.export(s))
    assert tc.export(1)[:, 4].min() == 0 and tc.export(1)[:, 5].max() == 5   # stream 1 counts its frames from 0 again
    same_export(tc, oracles)


# ---------------------------------------------------------------------------------------------------- life cycle
@pytest.mark.parametrize("case", CC.CASES, ids=[c["name"] for c in CC.CASES])
def test_seeded_cases(case):
    tc, oracles, res = check(case)
    same_export(tc, oracles, case["name"])
    same(tc.flush(cap=3), CO.flush_bank(oracles, 3), (case["name"], "flush at cap 3"))       # the rest stays pending ...
    same(tc.drain(cap=16), CO.run_bank(oracles, NO_FRAMES, [], 16), (case["name"], "drain"))  # ... and a drain fetches it
    same_export(tc, oracles, case["name"])


def test_expiry_inside_a_launch_slot_reuse_cap_1_and_drain():
    a, b, c = CC.row(2, 4, 20, 40, 1), CC.row(30, 4, 20, 40, 2), CC.row(60, 4, 20, 40, 3)
    case = CC.simple_case("forget_after 0", (72, 101), dict(max_tracks=4, forget_after=0), 16, [[[a, b]], [[]], [[a]], [[c]], [[]]], seed=17)
    tc, oracles, res = check(case)
    assert res[0].n_final.tolist() == [4] and res[0].events[0, :4, 2].tolist() == [1, 2, 1, 3] and res[0].events[0, :4, 0].tolist() == [CO.EXPIRED] * 4
    assert res[0].events[0, :4, 13].tolist() == [0, 1, 0, 0] and oracles[0].log["reused_in_call"] >= 2      # a slot reused in the tick it was freed
    none = tc.update(case["calls"][0][0][:0], [], cap=16)                    # ticks = 0, nothing pending
    same(none, CO.run_bank(oracles, NO_FRAMES, [], 16), "ticks = 0")
    same(tc.update(case["calls"][0][0][:1], [[CC.EMPTY]], cap=0), CO.run_bank(oracles, case["calls"][0][0][:1], [[CC.EMPTY]], 0), "cap = 0")
    case = CC.scripted_case("cap 1", (72, 101), 2, 13, [(0, 13)], cap=1, seed=5, max_tracks=8, forget_after=1)
    tc, oracles, res = check(case)
    assert res[0].pending.sum() > 0
    tail = []
    while True:
        r = tc.drain(cap=1)
        same(r, CO.run_bank(oracles, NO_FRAMES, [], 1), "drain")
        tail.append(r)
        if not r.pending.sum():
            break
    tail.append(tc.flush())
    tc2, _, res2 = check(dict(case, cap=64))
    assert res2[0].pending.sum() == 0
    strip = lambda fin: sorted(e[:13 * 4] + e[16 * 4:] for e in fin)        # noqa: E731 -- (the slot may differ: slots were freed later)
    got, want = finals_of(res + tail), finals_of(res2 + [tc2.flush()])
    assert len(got) == len(want) > 6 and strip(got) == strip(want)


def test_capacity_stop_rescue_and_max_tracks_1_and_512():
    a, b, c = CC.row(2, 4, 20, 40, 1), CC.row(30, 4, 20, 40, 2), CC.row(60, 4, 20, 40, 3)
    case = CC.simple_case("max_tracks 2", (72, 101), dict(max_tracks=2), 4, [[[a, b], [a]], [[a, b, c], [a, b]], [[a], [a]]], seed=4)
    tc, oracles, res = check(case)
    L = pkg("_lib")
    assert res[0].status.tolist() == [L.ERR_CAPACITY, 0] and 0 in tc.failed and 1 not in tc.failed and res[0].failed == tc.failed
    same_export(tc, oracles, "stopped")                                      # what it had can be rescued
    frames, rows = case["calls"][0][0][:1], [[CC.rows_of(a), CC.rows_of(a)]]
    same(tc.update(frames, rows, cap=4), CO.run_bank(oracles, frames, rows, 4), "stopped: nothing for stream 0, stream 1 goes on")
    same(tc.flush(0, cap=4), CO.flush_bank(oracles, 4, stream=0), "flush of the stopped stream")
    tc.reset(0), oracles[0].reset()
    assert not tc.failed and tc.export(0).shape == (0, 48)
    got = tc.update(frames, rows, cap=4)
    same(got, CO.run_bank(oracles, frames, rows, 4), "after reset")
    assert got.status.tolist() == [0, 0]
    for cap in (4, 1):                                                       # a full table whose slots all expire makes room -- while the list has room
        check(CC.simple_case(f"turnover at cap {cap}", (72, 101), dict(max_tracks=2, forget_after=0), cap, [[[a, b]], [[]], [[c, a]]], seed=6))
    tc, oracles, res = check(CC.simple_case("max_tracks 1", (72, 101), dict(max_tracks=1, forget_after=0), 4, [[[a]], [[b]], [[b]], [[a, b]]], seed=7))
    assert res[0].status.tolist() == [L.ERR_CAPACITY] and res[0].n_final.tolist() == [2]   # (forget_after 0: b expires at every tick and comes back)
    rows = CC.tiles((72, 101), 4, 6)[:300]
    tc, oracles, res = check(CC.simple_case("max_tracks 512", (72, 101), dict(max_tracks=512, forget_after=0, min_w=1, min_h=1), 512,
                                            [[rows], [[]], [rows[100:]]], seed=8))
    assert res[0].n_final.tolist() == [300] and len(tc.export(0)) == 200
    same_export(tc, oracles)


# ---------------------------------------------------------------------------------------------------- end to end
def test_update_tuples():
    M = pkg("colours")
    frame = CC.texture(np.random.default_rng(3), 72, 101)[None, None]
    cls = pkg("config").CLASSES[0]
    tc, ref = M.TrackColours(1, (72, 101)), M.TrackColours(1, (72, 101))
    got = tc.update_tuples(frame, [[[(10, 10, 29, 49, 7, cls, 0.9), (50, 10, 69, 49, 8, "no such class", 0.8)]]])
    want = ref.update(frame, [[CC.rows_of([10, 10, 29, 49, 7, 0], [50, 10, 69, 49, 8, -1])]])
    assert np.array_equal(got.row_tags, want.row_tags) and np.array_equal(tc.export(0), ref.export(0)) and tc.export(0)[:, 3].tolist() == [0, -1]


def test_planted_scene_through_the_pipeline_hook():
    """The red-over-blue walker of tests/colours_cases.py, its boxes injected into a tiny pipeline run: attach_colours hands the run's
    frames and tracks over, and the walker's track ends as RED over BLUE."""
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, M = pkg("pipeline").TrackingPipeline, pkg("colours")
    frames, rows = CC.planted_scene()
    T, H, W = len(frames), frames.shape[2], frames.shape[3]
    planted = [(r[0][:, :4].astype(np.float32) + np.array([0, 0, 1, 1], np.float32), np.full(len(r[0]), 0.9, np.float32), np.zeros(len(r[0]), np.int32))
               for r in rows]

    def run(stage):
        pipe = TP(ypath, None, (H, W), batch=4, ring_frames=T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=1, track_buffer=3)
        pipe.upload(0, frames[:, 0])
        pipe.inject(0, planted)
        if stage is not None:
            pipe.attach_colours(stage)
        out, results = [], []
        for lo, n in ((0, 8), (8, T - 8)):                                   # two run calls: the stage's state carries over
            out += pipe.run(lo, n)[0]
            results.append(pipe.colour_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    stage = M.TrackColours(1, (H, W))
    tracks, results = run(stage)
    assert tracks == plain and sum(len(t) for t in tracks) >= T              # the tracks are untouched
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    to_rows = lambda tr: np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tr], np.int32).reshape(-1, 6)      # noqa: E731
    oracle = CO.ColoursOracle((H, W))
    for (lo, n), got in zip(((0, 8), (8, T - 8)), results):
        fr = frames[lo:lo + n]
        same(got, CO.run_bank([oracle], fr, [[to_rows(tracks[lo + t])] for t in range(n)], 16), ("pipeline against the oracle", lo))
    last = stage.flush()
    same(last, CO.flush_bank([oracle], 128), "flush")
    evs = M.finals(last)
    walker = max(evs, key=lambda e: e["sightings"])
    assert (walker["upper"], walker["lower"]) == ("red", "blue") and walker["hist_upper"][CO.RED] >= 200 and walker["hist_lower"][CO.BLUE] >= 200
    assert M.matches(walker, upper="red", lower=("blue", "black")) and not M.matches(walker, upper="green")


def test_cli_colours_both_paths(tmp_path, monkeypatch):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli, M = pkg("cli"), pkg("colours")
    srcs = ["synthetic:640x360:6:16:1", "synthetic:640x360:4:16:2"]
    common = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--output_dir", str(tmp_path)]

    class Planted:
        """The scene's own boxes in place of the seeded detector's: the frame-by-frame run then has tracks to show."""

        def __init__(self, **kw):
            self.scene, self.i = pkg("synthetic").Scene(seed=1, n_targets=6, width=640, height=360, conf_range=(0.8, 0.95)), 0

        def detect(self, frame):
            self.i += 1
            return self.scene.detections(self.i - 1)

    monkeypatch.setattr(cli, "YOLODetector", Planted)
    for argv, name in ((["--inputs", ",".join(srcs), "--batch", "8"], "both"), (["--input", srcs[0]], "planted")):
        for f in tmp_path.glob("*.jsonl"):
            f.unlink()
        out = tmp_path / f"{name}_colours.out"
        assert cli.main(argv + common + ["--colours", "--colours_file", str(out)]) == 0
        lines = [json.loads(l) for f in sorted(tmp_path.glob("*_tracked_*.jsonl")) for l in f.read_text().splitlines()]
        assert lines and all("colours" in l and len(l["colours"]) == len(l["tracks"]) for l in lines)
        named = [c for l in lines for pair in l["colours"] for c in pair]
        assert all(c is None or c in M.NAMES for c in named)
        ended = [json.loads(l) for l in out.read_text().splitlines()]
        assert all(e["reason"] in ("expired", "flushed") and len(e["hist_upper"]) == 12 and e["upper"] in M.NAMES + (None,) for e in ended)
        print(name, "lines", len(lines), "named", sum(c is not None for c in named), "ended", len(ended))
        if name == "planted":
            assert sum(c is not None for c in named) > 10 and len(ended) >= 3
