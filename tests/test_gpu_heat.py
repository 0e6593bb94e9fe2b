"""Heat maps on the device (csrc/kernels_heat.hip) against tests/heat_oracle.py: integer arithmetic on both sides, so
everything -- n_final, events, row_tags, pending, status, all twelve layers after every call, every rendered byte -- is np.array_equal.
Each case is the smallest shape that can break; tests/test_heat_oracle.py shows through the oracle alone that the seeded cases reach
every branch."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import colours_cases as CC
import colours_oracle as CO
import heat_cases as HC
import heat_oracle as HO
import slot_life_scene as SL
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

NAMES = ("n_final", "events", "row_tags", "pending", "status")


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got[:5], want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError((what, name, "first difference at", bad.tolist(), g[tuple(bad)], w[tuple(bad)], g[tuple(bad[:-1])], w[tuple(bad[:-1])]))


def device_layers(hm, s):
    lay = hm.layers(s)
    return np.stack([lay[n] for n in HO.LAYERS])


def same_layers(hm, oracles, what=""):
    for s, o in enumerate(oracles):
        got = device_layers(hm, s)
        if not np.array_equal(got, o.layers):
            bad = np.argwhere(got != o.layers)[0]
            raise AssertionError((what, "stream", s, "layer", HO.LAYERS[bad[0]], "cell", bad[1:].tolist(), got[tuple(bad)], o.layers[tuple(bad)]))


def stage_for(case, options=()):
    kw = dict(case["kw"])
    kw["anchor"] = "centre" if kw["anchor"] == HO.CENTRE else "foot"
    hm = pkg("heatmap").HeatMaps(case["streams"], case["hw"], **kw)
    for k, v in options:
        hm.option(k, v)
    return hm


def names_of(mask):
    return [HO.LAYERS[l] for l in range(12) if mask >> l & 1]


def apply(hm, op, cap):
    """One op of a case on the device -> a HeatResult or None."""
    kind = op[0]
    if kind == "update":
        return hm.update(op[1], cap=cap)
    if kind == "drain":
        return hm.drain(cap=cap)
    if kind == "flush":
        return hm.flush(op[1], cap=cap)
    if kind == "reset":
        hm.reset(op[1])
    elif kind == "import":
        hm.load_layers(op[1], dict(zip(names_of(op[2]), op[3])))
    elif kind == "decay":
        hm.decay(op[3], stream=op[1], names=names_of(op[2]))
    return None


def check(case, options=()):
    """The device against one oracle per stream, op by op, the layers after every op; returns (HeatMaps, oracles, the device's results)."""
    hm, oracles, res = stage_for(case, options), HC.oracles_for(case), []
    for i, op in enumerate(case["ops"]):
        got, want = apply(hm, op, case["cap"]), HC.run_op(oracles, op, case["cap"])
        if want is not None:
            same(got, want, (case["name"], op[0], i))
            res.append(got)
        same_layers(hm, oracles, (case["name"], op[0], i))
    return hm, oracles, res


def same_export(hm, oracles, what=""):
    for s, o in enumerate(oracles):
        ev, want = hm.export(s), o.export()
        assert len(ev) == len(want), (what, s, len(ev), len(want))
        for k, e in enumerate(want):
            assert np.array_equal(ev[k], e), (what, s, k, ev[k], e)


# ---------------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("case", HC.seeded_cases(), ids=lambda c: c["name"])
def test_seeded_cases_call_by_call(case):
    hm, oracles, res = check(case)
    same_export(hm, oracles, case["name"])
    if case["name"].startswith("crowd1-"):                                   # stream 2's five ids do not fit four slots: it stops alone
        assert res[0][4].tolist() == [0, 0, HO.ERR_CAPACITY] and 2 in res[0].failed and res[1][4][2] == HO.ERR_CAPACITY
        assert res[1][0][:2].sum() + res[1][3][:2].sum() > 0                 # the others run on: tracks end or wait
    if case["name"] == "contention":
        lay = device_layers(hm, 0)
        assert lay[HO.STARTS, 1, 2] == 512 and lay[HO.VISITS, 1, 2] == 512 and lay[HO.DWELL, 1, 2] == 1024 and lay[HO.DIR0 + 0, 1, 2] == 512
        assert lay[HO.ENDS, 1, 2] == 512
    if case["name"] == "saturation":
        lay = device_layers(hm, 0)
        assert (lay[:4, 2, 3] == HO.SAT).all() and lay[HO.DIR0 + 1, 2, 3] == HO.SAT and lay[HO.DIR0 + 2, 2, 3] == HO.SAT - 3
    hm.close()


def test_513_rows_is_a_capacity_error_before_staging():
    L = pkg("_lib")
    hm = pkg("heatmap").HeatMaps(1, (48, 64), max_tracks=4)
    with pytest.raises(L.AicError) as ei:
        hm.update([[np.zeros((513, 6), np.int32)]])
    assert ei.value.code == L.ERR_CAPACITY
    got = hm.update([[HC.rows_array([HC.person(10, 10, 1)])]])             # nothing was staged, nothing stopped
    assert got.status.tolist() == [0] and got.row_tags.tolist() == [[0, 1, 0, -1]]
    hm.close()


def test_capacity_stop_leaves_the_tick_out_of_the_layers():
    case = dict(name="stop", streams=2, hw=(48, 64), kw=dict(cell=8, max_tracks=2, forget_after=5, anchor=HO.FOOT, min_move=4), cap=4, ops=[])
    two = HC.rows_array([HC.person(10, 10, 1), HC.person(30, 30, 2)])
    three = HC.rows_array([HC.person(12, 10, 1), HC.person(50, 40, 3), HC.person(33, 30, 2)])
    case["ops"] = [("update", [[two, two], [three, two], [two, two]])]
    hm, oracles, res = check(case)
    assert res[0].status.tolist() == [HO.ERR_CAPACITY, 0]
    lay0, lay1 = device_layers(hm, 0), device_layers(hm, 1)
    assert lay0[HO.DWELL].sum() == 2 and lay0[HO.DIR0:].sum() == 0 and lay1[HO.DWELL].sum() == 6     # one tick of stream 0, three of stream 1
    assert res[0].row_tags[4:7].tolist() == [[-1, 0, 0, -1]] * 3             # the rows of the tick it stopped at
    hm.reset(0), oracles[0].reset()
    same(hm.update([[two, two]], cap=4), HO.run_bank(oracles, [[two, two]], 4), "after the reset")
    same_layers(hm, oracles, "after the reset")
    hm.close()


def test_ends_follow_the_drain():
    hm = pkg("heatmap").HeatMaps(1, (48, 64), cell=8, max_tracks=4, forget_after=0)
    o = HO.HeatOracle((48, 64), cell=8, max_tracks=4, forget_after=0)
    a = HC.rows_array([HC.person(10, 10, 1), HC.person(30, 30, 2)])
    got = hm.update([[a], [HC.EMPTY]], cap=1)
    same(got, HO.run_bank([o], [[a], [HC.EMPTY]], 1), "two end, one is handed over")
    assert got.n_final.tolist() == [1] and got.pending.tolist() == [1] and device_layers(hm, 0)[HO.ENDS].sum() == 1
    got = hm.drain(cap=1)
    same(got, HO.run_bank([o], [], 1), "the drain")
    ends = device_layers(hm, 0)[HO.ENDS]
    assert got.pending.tolist() == [0] and ends.sum() == 2 and ends[1, 1] == 1 and ends[3, 3] == 1
    same_layers(hm, [o])
    hm.close()


@pytest.mark.parametrize("options", [(("ticks_per_launch", 1),), (("ticks_per_launch", 0),), (("ticks_per_launch", 5), ("launch_budget_mb", 1))])
def test_launch_options_give_the_same_results(options):
    hm, _, _ = check(HC.crowd_case(1, (48, 64), 16, 3, (3, 4, 5)), options)
    hm.close()


def test_the_same_ticks_in_one_call_and_in_two():
    one = HC.crowd_case(3, (37, 61), 16, 1, (4,), cap=16, split=(12, 0), extra_ops=False)
    two = HC.crowd_case(3, (37, 61), 16, 1, (4,), cap=16, split=(7, 5), extra_ops=False)
    (ha, _, ra), (hb, _, rb) = check(one), check(two)
    assert np.array_equal(device_layers(ha, 0), device_layers(hb, 0))
    events = lambda res: [r.events[0, k].tobytes() for r in res for k in range(int(r.n_final[0]))]      # noqa: E731
    assert events(ra) == events(rb) and len(events(ra)) > 4
    assert np.array_equal(np.concatenate([r.row_tags for r in ra]), np.concatenate([r.row_tags for r in rb]))
    ha.close(), hb.close()


def test_rows_and_counts_from_device_memory():
    case = HC.crowd_case(1, (48, 64), 16, 3, (3, 4, 5))
    rows = case["ops"][0][1]
    IO = pkg("_bank_io")
    flat, counts = IO.flat_rows(rows, len(rows), 3)
    host, dev = stage_for(case), stage_for(case)
    a = host.update(flat, counts=counts, cap=2)
    b = dev.update(torch.from_numpy(flat).cuda(), counts=torch.from_numpy(counts).cuda(), cap=2)
    c = host.update(rows, cap=2)
    same(b, a[:5], "device rows against host rows")
    assert a.row_tags.shape == c.row_tags.shape
    oracles = HC.oracles_for(case)
    same(a, HO.run_bank(oracles, rows, 2), "flat host rows against the oracle")
    same_layers(dev, oracles, "device rows")
    host.close(), dev.close()


def test_round_trip_into_a_second_stage_that_continues_identically():
    case = HC.crowd_case(2, (37, 61), 8, 3, (4, 5, 2), cap=16, forget_after=2, extra_ops=False)
    a, oracles, _ = check(case)                                              # ends with a flush and a drain: the tables are empty
    b = stage_for(case)
    for s in range(3):
        if s != 1:
            b.load_layers(s, a.layers(s))
        else:
            b.load_layers(s, a.layers(s, ["dwell", "dir7"]))                 # a masked import: two layers only
    for s in range(3):
        want = device_layers(a, s)
        if s == 1:
            want = np.where(np.isin(np.arange(12), [1, 11])[:, None, None], want, 0)
            a.decay(31, stream=1, names=[l for l in HO.LAYERS if l not in ("dwell", "dir7")])
            oracles[1].decay(0xFFF & ~0b100000000010, 31)
        assert np.array_equal(device_layers(b, s), want), s
    a.reset(1), b.reset(1), oracles[1].reset()                               # stream 1 had stopped: a reset puts it back, in both
    more = HC.crowd_case(7, (37, 61), 8, 3, (4, 3, 2), cap=16, forget_after=2, extra_ops=False)
    def no_frames(res):                                                      # the second stage counts its ticks from 0: first_frame, last_seen apart
        ev = res[1].copy()
        ev[:, :, 4:6] = 0
        return (res[0], ev) + tuple(res[2:5])
    for op in more["ops"]:
        ga, gb, want = apply(a, op, 16), apply(b, op, 16), HC.run_op(oracles, op, 16)
        same(ga, want, ("first stage", op[0])), same(no_frames(gb), no_frames(want), ("second stage", op[0]))
    same_layers(a, oracles, "first stage"), same_layers(b, oracles, "second stage")
    a.close(), b.close()


def test_reset_then_import_then_update_in_call_order():
    hm = pkg("heatmap").HeatMaps(2, (37, 61), cell=16, max_tracks=4)
    oracles = [HO.HeatOracle((37, 61), cell=16, max_tracks=4, stream=s) for s in range(2)]
    rows = [[HC.rows_array([HC.person(10, 10, 1)]), HC.rows_array([HC.person(40, 30, 2)])]]
    same(hm.update(rows), HO.run_bank(oracles, rows, 16))
    planted = np.full((1, 3, 4), 77, np.int32)
    hm.reset(0), oracles[0].reset()
    hm.load_layers(0, dict(visits=planted[0])), oracles[0].import_layers(1, planted)       # behind the reset: it survives it
    hm.load_layers(1, dict(ends=planted[0])), oracles[1].import_layers(8, planted)
    hm.reset(1), oracles[1].reset()                                          # in front of the reset: it does not
    same(hm.update(rows), HO.run_bank(oracles, rows, 16))
    same_layers(hm, oracles)
    assert device_layers(hm, 0)[HO.VISITS, 0, 0] == 78 and device_layers(hm, 1)[HO.ENDS].sum() == 0
    hm.close()


def test_slot_life_scene_gives_the_colour_oracles_life_cycle():
    """tests/slot_life_scene.py through this stage: one life cycle (slot_walk.hpp), so the seven shared event ints, n_final, pending and
    status equal the colour oracle's on the same scene."""
    hm = pkg("heatmap").HeatMaps(SL.STREAMS, SL.HW, cell=8, max_tracks=SL.MAX_TRACKS, forget_after=SL.FORGET_AFTER)
    colour = [CO.ColoursOracle(SL.HW, stream=s, **SL.CL_KW) for s in range(SL.STREAMS)]
    heat = [HO.HeatOracle(SL.HW, cell=8, max_tracks=SL.MAX_TRACKS, forget_after=SL.FORGET_AFTER, stream=s) for s in range(SL.STREAMS)]
    for i, (frames, rows) in enumerate(SL.calls()):
        got, want = hm.update(rows, cap=SL.CAP), CO.run_bank(colour, frames, rows, SL.CAP)
        same(got, HO.run_bank(heat, rows, SL.CAP), ("the heat oracle", i))
        assert np.array_equal(got.n_final, want[0]) and np.array_equal(got.pending, want[3]) and np.array_equal(got.status, want[4]), i
        assert np.array_equal(got.events[:, :, :SL.HEAD], want[1][:, :, :SL.HEAD]), i
    assert got.status.tolist() == [0, 0, SL.ERR_CAPACITY] and got.pending.max() >= 1
    for s in range(SL.STREAMS):
        ev, want = hm.export(s), colour[s].export()
        assert len(ev) == len(want) and all(np.array_equal(a[:SL.HEAD], b[:SL.HEAD]) for a, b in zip(ev, want)), s
    hm.close()


# ---------------------------------------------------------------------------------------------------- render
def planted_stage(hw, cell, streams=3, seed=0, peak=1000):
    hm = pkg("heatmap").HeatMaps(streams, hw, cell=cell, max_tracks=4)
    lays = [HC.blob_layers(hw, cell, seed + s, peak) for s in range(streams)]
    for s, lay in enumerate(lays):
        hm.load_layers(s, dict(zip(HO.LAYERS, lay)))
    return hm, lays


def frames_of(n, hw, seed=49):
    return np.random.default_rng(seed).integers(0, 256, (n,) + tuple(hw) + (3,), dtype=np.uint8)


def same_pixels(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, len(bad), "bytes differ; first at", bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.mark.parametrize("scale", ["linear", "log"])
@pytest.mark.parametrize("hw,cell", [((37, 61), 4), ((37, 61), 8), ((37, 61), 16), ((37, 61), 32), ((20, 150), 8)])
def test_render_every_pixel(hw, cell, scale):
    """Five frames in one bank; a 37 x 61 frame is 6 771 bytes, so frame 1 starts at an odd byte.  20 x 150: a band of more than 256 items."""
    hm, lays = planted_stage(hw, cell)
    hm.option("scale", scale)
    frames = frames_of(5, hw)
    cams = [2, 0, 0, 2, 0]                                                   # repeats, and camera 1 is missing
    for alpha, floor in ((160, 8), (0, 8), (256, 8), (160, 0), (160, 255), (256, 0), (99, 100)):
        hm.option("alpha_q8", alpha), hm.option("floor", floor)
        kw = dict(scale=HO.LINEAR if scale == "linear" else HO.LOG, alpha_q8=alpha, floor=floor)
        for layer in ("dwell", "dir7") if (alpha, floor) == (160, 8) else ("dwell",):
            l = HO.LAYERS.index(layer)
            want = HO.render(frames, cams, lambda c: lays[c], l, hw[0], hw[1], cell, **kw)
            got = hm.render(frames, cameras=cams, layer=layer)
            assert got is not frames
            same_pixels(got, want, (hw, cell, scale, alpha, floor, layer, "host frames"))
            if alpha == 0:
                assert np.array_equal(got, frames)
            if (alpha, floor) == (160, 8):
                assert (want != frames).any() and (want == frames).any()
                dev = torch.from_numpy(frames).cuda()
                assert hm.render(dev, cameras=cams, layer=layer) is dev
                same_pixels(dev, want, (hw, cell, scale, "device frames"))
                want3 = HO.render(frames[:3], [0, 1, 2], lambda c: lays[c], l, hw[0], hw[1], cell, **kw)
                same_pixels(hm.render(frames[:3], layer=layer), want3, (hw, cell, scale, "cameras None"))
    hm.close()


def test_render_at_odd_addresses_and_in_chunks():
    hw, cell = (37, 61), 8
    hm, lays = planted_stage(hw, cell)
    frames = frames_of(4, hw, seed=5)
    cams = [1, 2, 0, 1]
    want = HO.render(frames, cams, lambda c: lays[c], HO.DWELL, hw[0], hw[1], cell)
    for chunk in (1, 3, 0):
        hm.option("chunk_frames", chunk)
        same_pixels(hm.render(frames, cameras=cams), want, ("host", chunk))
        dev = torch.from_numpy(frames).cuda()
        hm.render(dev, cameras=cams)
        same_pixels(dev, want, ("device", chunk))
    # a bank that starts at every byte offset of a dword, with guard bytes around it that must stay as they are
    n = frames.size
    for off in (1, 2, 3, 5):
        buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[off:off + n].view(4, hw[0], hw[1], 3)
        view.copy_(torch.from_numpy(frames))
        assert view.data_ptr() % 4 == off % 4
        hm.render(view, cameras=cams)
        same_pixels(view, want, ("offset", off))
        guard = buf.cpu().numpy()
        assert (guard[:off] == 0xA5).all() and (guard[off + n:] == 0xA5).all(), off
    hm.close()


def test_render_edge_layers_and_a_custom_table():
    hw, cell = (37, 61), 8
    M = pkg("heatmap")
    hm = M.HeatMaps(2, hw, cell=cell, max_tracks=4)
    o = HO.HeatOracle(hw, cell=cell)
    frames = frames_of(2, hw, seed=9)
    same_pixels(hm.render(frames), frames, "all-zero layers leave the bytes untouched")
    dev = torch.from_numpy(frames).cuda()
    hm.render(dev)
    same_pixels(dev, frames, "all-zero layers, device frames")
    one = np.zeros((12, o.GH, o.GW), np.int32)
    one[HO.DWELL, 2, 5] = 1                                                  # a single cell, M = 1
    big = np.zeros((12, o.GH, o.GW), np.int32)
    big[HO.DWELL] = np.random.default_rng(3).integers(0, 1 << 30, (o.GH, o.GW))
    big[HO.DWELL, 0, 0], big[HO.DWELL, 4, 7] = 1 << 30, (1 << 30) - 1        # a layer that holds 2^30
    hm.load_layers(0, dict(dwell=one[HO.DWELL])), hm.load_layers(1, dict(dwell=big[HO.DWELL]))
    lays = [one, big]
    table = np.random.default_rng(4).integers(0, 256, (256, 3), dtype=np.uint8)
    for scale in ("log", "linear"):
        hm.option("scale", scale)
        kw = dict(scale=HO.LOG if scale == "log" else HO.LINEAR)
        want = HO.render(frames, [0, 1], lambda c: lays[c], HO.DWELL, hw[0], hw[1], cell, **kw)
        same_pixels(hm.render(frames), want, (scale, "M = 1 and 2^30"))
        assert (want[0] != frames[0]).any() and (want[0, :8] == frames[0, :8]).all()      # only around the one cell
        hm.set_colour_table(table)
        same_pixels(hm.render(frames), HO.render(frames, [0, 1], lambda c: lays[c], HO.DWELL, hw[0], hw[1], cell, lut=table, **kw), (scale, "custom table"))
        hm.set_colour_table(M.colour_table())
    img = hm.images([1, 0], layer="dwell")
    want = HO.render(np.zeros_like(frames), [1, 0], lambda c: lays[c], HO.DWELL, hw[0], hw[1], cell, scale=HO.LINEAR, alpha_q8=256)
    same_pixels(img, want, "images")
    same_pixels(hm.render(frames), HO.render(frames, [0, 1], lambda c: lays[c], HO.DWELL, hw[0], hw[1], cell, scale=HO.LINEAR), "alpha is put back")
    hm.close()


# ---------------------------------------------------------------------------------------------------- pipeline
def test_planted_scene_through_the_pipeline_hook():
    """The walker of tests/colours_cases.py, its boxes injected into the tiny pipeline run tests/test_gpu_colours.py uses: attach_heat_maps
    hands the run's tracks over; heat_result and the layers equal a stage fed the same rows by hand, and the tracks are unchanged."""
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, M = pkg("pipeline").TrackingPipeline, pkg("heatmap")
    frames, rows = CC.planted_scene()
    T, H, W = len(frames), frames.shape[2], frames.shape[3]
    planted = [(r[0][:, :4].astype(np.float32) + np.array([0, 0, 1, 1], np.float32), np.full(len(r[0]), 0.9, np.float32), np.zeros(len(r[0]), np.int32))
               for r in rows]

    def run(stage):
        pipe = TP(ypath, None, (H, W), batch=4, ring_frames=T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=1, track_buffer=3)
        pipe.upload(0, frames[:, 0])
        pipe.inject(0, planted)
        if stage is not None:
            pipe.attach_heat_maps(stage)
        out, results = [], []
        for lo, n in ((0, 8), (8, T - 8)):                                   # two run calls: the stage's state carries over
            out += pipe.run(lo, n)[0]
            results.append(pipe.heat_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    stage = M.HeatMaps(1, (H, W))
    tracks, results = run(stage)
    assert tracks == plain and sum(len(t) for t in tracks) >= T              # the tracks are untouched
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    to_rows = lambda tr: np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tr], np.int32).reshape(-1, 6)      # noqa: E731
    by_hand, oracle = M.HeatMaps(1, (H, W)), HO.HeatOracle((H, W))
    for (lo, n), got in zip(((0, 8), (8, T - 8)), results):
        fed = [[to_rows(tracks[lo + t])] for t in range(n)]
        same(got, by_hand.update(fed)[:5], ("pipeline against a stage fed by hand", lo))
        same(got, HO.run_bank([oracle], fed, 16), ("pipeline against the oracle", lo))
    assert np.array_equal(device_layers(stage, 0), device_layers(by_hand, 0))
    same_layers(stage, [oracle])
    last = stage.flush()
    same(last, HO.flush_bank([oracle], 128), "flush")
    walker = max(M.paths(last), key=lambda e: e["sightings"])
    assert walker["sightings"] >= T // 2 and device_layers(stage, 0)[HO.DWELL].sum() >= T
    stage.close(), by_hand.close()


def test_cli_heat_maps_both_paths(tmp_path, monkeypatch):
    import json
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli, M = pkg("cli"), pkg("heatmap")
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
    for argv, name, cams in ((["--inputs", ",".join(srcs), "--batch", "8"], "both", 2), (["--input", srcs[0]], "planted", 1)):
        d, out = tmp_path / f"{name}_heat", tmp_path / f"{name}_paths.jsonl"
        assert cli.main(argv + common + ["--heat_maps", str(d), "--heat_cell", "8", "--heat_layer", "visits", "--heat_paths", str(out), "--heat_overlay"]) == 0
        for c in range(cams):
            lay = np.load(d / f"cam{c}_layers.npy")
            assert lay.shape == (12, 45, 80) and lay.dtype == np.int32 and lay.min() >= 0
            assert lay[HO.VISITS].sum() >= lay[HO.STARTS].sum() == lay[HO.ENDS].sum()          # the flush at the end handed every track over
            jpg = (d / f"cam{c}_visits.jpg").read_bytes()
            assert jpg[:2] == b"\xff\xd8" and jpg[-2:] == b"\xff\xd9"
        ended = [json.loads(l) for l in out.read_text().splitlines()] if out.exists() else []
        assert all(e["why"] in ("expired", "flushed") and e["cells"] >= 1 and len(e["start"]) == 2 for e in ended)
        assert len(ended) == sum(int(np.load(d / f"cam{c}_layers.npy")[HO.ENDS].sum()) for c in range(cams))
        if name == "planted":
            assert len(ended) >= 3 and np.load(d / "cam0_layers.npy")[HO.DWELL].sum() > 10
