"""Proximity on the device (csrc/kernels_prox.hip) against tests/prox_oracle.py: integer arithmetic on both sides, so
everything -- n_final, events, pending, status, records, row tags, pair events with their true counts, and after every call the exported
slots and the exported pair table -- is np.array_equal.  Each case is the smallest shape that can break (frames of 48 x 64: none is read);
tests/test_prox_oracle.py shows through the oracle alone that the seeded cases reach every branch."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import poison_scenarios as P
import prox_cases as PC
import prox_oracle as PO
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

NAMES = ("n_final", "events", "pending", "status", "records", "row_tags", "n_pair_events", "pair_events")


def flat(res):
    """A ProximityResult as the oracle packs a call."""
    return (res.n_final, res.events, res.pending, res.status, res.records.reshape(-1, 16), res.row_tags, res.n_pair_events.reshape(-1),
            res.pair_events.reshape(res.n_pair_events.size, res.pair_events.shape[2], 8))


def same(got, want, what=""):
    got = flat(got) if hasattr(got, "records") else got
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[0]
            raise AssertionError((what, name, "first difference at", bad.tolist(), g[tuple(bad)], w[tuple(bad)], g[tuple(bad[:-1])], w[tuple(bad[:-1])]))


def stage_for(case, options=(), streams=None):
    kw = dict(case["kw"])
    kw["metric"] = "ground" if kw["metric"] == PO.GROUND else "body"
    px = pkg("proximity").Proximity(case["streams"] if streams is None else streams, case["hw"], **kw)
    for k, v in options:
        px.option(k, v)
    return px


def apply(px, op, cap, cap_pairs):
    """One op of a case on the device -> a ProximityResult or None."""
    kind = op[0]
    if kind == "update":
        return px.update(op[1], cap=cap, cap_pairs=cap_pairs)
    if kind == "drain":
        return px.drain(cap=cap)
    if kind == "flush":
        return px.flush(op[1], cap=cap)
    if kind == "reset":
        px.reset(op[1])
    elif kind == "option":
        px.option(op[1], op[2])
    elif kind == "ground":
        px.set_ground(op[2], op[3], stream=op[1])
    return None


def same_state(px, oracles, what=""):
    for s, o in enumerate(oracles):
        ev, want = px.export(s), o.export()
        assert len(ev) == len(want), (what, "export", s, len(ev), len(want))
        for k, e in enumerate(want):
            assert np.array_equal(ev[k], e), (what, "export", s, k, ev[k], e)
        got, wantp = px.export_pairs(s), o.export_pairs()
        assert got.shape == wantp.shape and np.array_equal(got, wantp), (what, "export_pairs", s, got[:8], wantp[:8])


def check(case, options=()):
    """The device against one oracle per stream, op by op, the state after every op; returns (Proximity, oracles, the device's results)."""
    px, oracles, res = stage_for(case, options), PC.oracles_for(case), []
    for i, op in enumerate(case["ops"]):
        got, want = apply(px, op, case["cap"], case["cap_pairs"]), PC.run_op(oracles, op, case["cap"], case["cap_pairs"])
        if want is not None:
            same(got, want, (case["name"], op[0], i))
            res.append(got)
        same_state(px, oracles, (case["name"], op[0], i))
    return px, oracles, res


# ---------------------------------------------------------------------------------------------------- the seeded cases
@pytest.mark.parametrize("case", PC.seeded_cases(), ids=lambda c: c["name"])
def test_seeded_cases_call_by_call(case):
    px, oracles, res = check(case)
    if case["name"] == "pair":
        kinds = [(e["kind"], e["frame"], e["ids"]) for r in res for e in r.pairs()]
        assert kinds == [("link", 2, (1, 2)), ("unlink", 6, (1, 2)), ("link", 11, (1, 4))]
        assert res[0].parties(2, 0) == [[1, 2], [3]] and res[0].parties(3, 0) == [[1], [3]]
    if case["name"] == "path":
        r = res[0]
        assert r.record(0, 0)["largest_near"] == 512 and r.record(0, 0)["largest_party"] == 512 and r.record(0, 0)["n_link"] == 511
        assert r.record(1, 0)["largest_near"] == 256 and r.record(1, 0)["n_parties"] == 2
        assert int(r.n_pair_events[0, 0]) == 511 and len(r.pairs(0, 0)) == 511
    if case["name"] == "cliques":
        assert res[0].record(1, 0)["largest_party"] == 8 and res[1].record(3, 0)["largest_party"] == 4 and res[1].record(2, 0)["n_unlink"] == 1
    if case["name"] == "truncation":
        assert int(res[0].n_pair_events[0, 0]) == 15 and (res[0].pair_events[0, 0, :, 0] == PO.LINK).all() and len(res[0].pairs(0, 0)) == 4
    if case["name"].startswith("crowd1-"):                                   # stream 2's five ids do not fit four slots: it stops alone
        assert res[0].status.tolist() == [0, 0, PO.ERR_CAPACITY] and 2 in res[0].failed
    if case["name"] == "long":
        assert px.export_pairs(0).tolist() == [[1, 2, 1, 32767, 0, 1]]
    px.close()


def test_513_rows_is_a_capacity_error_before_staging():
    L = pkg("_lib")
    px = pkg("proximity").Proximity(1, PC.HW, max_tracks=4)
    with pytest.raises(L.AicError) as ei:
        px.update([[np.zeros((513, 6), np.int32)]])
    assert ei.value.code == L.ERR_CAPACITY
    got = px.update([[PC.rows_array([PC.person(10, 10, 1)])]])             # nothing was staged, nothing stopped
    assert got.status.tolist() == [0] and got.row_tags.tolist() == [[20, 20, -1, 0, 1, 1, 0, 1 | 2 | 4 | 8 | 16]]
    px.close()


# ---------------------------------------------------------------------------------------------------- the same ticks, cut differently
CROWD = dict(seed=7, streams=3, ids=(4, 3, 4), ticks=40, cap=16, cap_pairs=8, extra_ops=False, forget_after=2)


def crowd_rows():
    return [op[1] for op in PC.crowd_case(split=(40, 0), **CROWD)["ops"] if op[0] == "update"][0]


def run_cut(rows, cuts, options=(), device_rows=False):
    """The 40 ticks in calls of `cuts` ticks -> (the concatenated outputs that do not depend on the cut, exports, pair tables)."""
    case = PC.crowd_case(split=(40, 0), **CROWD)
    px = stage_for(case, options)
    IO = pkg("_bank_io")
    recs, tags, npe, pe, ended = [], [], [], [], []
    lo = 0
    for n in cuts:
        part = rows[lo:lo + n]
        if device_rows:
            fl, counts = IO.flat_rows(part, n, 3)
            r = px.update(torch.from_numpy(fl).cuda(), counts=torch.from_numpy(counts).cuda(), cap=16, cap_pairs=8)
        else:
            r = px.update(part, cap=16, cap_pairs=8)
        recs.append(r.records), tags.append(r.row_tags), npe.append(r.n_pair_events), pe.append(r.pair_events)
        ended += [r.events[s, k].tobytes() for s in range(3) for k in range(int(r.n_final[s]))]
        lo += n
    state = [px.export(s) for s in range(3)], [px.export_pairs(s) for s in range(3)]
    px.close()
    return (np.concatenate(recs), np.concatenate(tags), np.concatenate(npe), np.concatenate(pe)), sorted(ended), state


def same_runs(a, b, what):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y), what
    assert a[1] == b[1], what
    for x, y in zip(a[2][0] + a[2][1], b[2][0] + b[2][1]):
        assert np.array_equal(x, y), what


def test_one_call_of_40_ticks_equals_calls_of_1_7_and_32_and_any_launch_cut():
    rows = crowd_rows()
    one = run_cut(rows, (40,))
    assert one[0][2].sum() > 4 and len(one[1]) > 2                           # pairs linked and unlinked, tracks ended
    same_runs(one, run_cut(rows, (1, 7, 32)), "calls of 1, 7 and 32 ticks")
    for options in ((("ticks_per_launch", 1),), (("ticks_per_launch", 7),), (("ticks_per_launch", 0), ("launch_budget_mb", 1))):
        same_runs(one, run_cut(rows, (40,), options), options)
    same_runs(one, run_cut(rows, (40,), device_rows=True), "rows and counts in device memory")
    same_runs(one, run_cut(rows, (1, 7, 32), (("ticks_per_launch", 5),), device_rows=True), "device rows, cut twice")
    # and the oracle, on the whole call
    case = PC.crowd_case(split=(40, 0), **CROWD)
    px, oracles = stage_for(case), PC.oracles_for(case)
    same(px.update(rows, cap=16, cap_pairs=8), PO.run_bank(oracles, rows, 16, 8), "40 ticks against the oracle")
    same_state(px, oracles)
    px.close()


def test_a_bank_of_three_equals_three_single_handles():
    case = PC.crowd_case(split=(12, 0), seed=9, streams=3, ids=(4, 5, 3), cap=2, cap_pairs=4, extra_ops=False)
    rows = case["ops"][0][1]
    bank = stage_for(case).update(rows, cap=2, cap_pairs=4)
    for s in range(3):
        one = stage_for(case, streams=1)
        r = one.update([[t[s]] for t in rows], cap=2, cap_pairs=4)
        assert np.array_equal(r.records[:, 0], bank.records[:, s]) and np.array_equal(r.n_pair_events[:, 0], bank.n_pair_events[:, s]), s
        assert np.array_equal(r.pair_events[:, 0], bank.pair_events[:, s]), s
        assert (r.n_final[0], r.pending[0], r.status[0]) == (bank.n_final[s], bank.pending[s], bank.status[s]), s
        n = int(r.n_final[0])
        a, b = r.events[0, :n].copy(), bank.events[s, :n].copy()
        a[:, 1] = b[:, 1] = 0                                                # (the stream's own number)
        assert np.array_equal(a, b), s
        for t in range(12):
            assert np.array_equal(r.tags(t, 0), bank.tags(t, s)), (s, t)
        one.close()


def test_reset_of_one_stream_of_three_and_set_ground_between_calls():
    case = PC.crowd_case(split=(12, 0), seed=11, streams=3, ids=(4, 4, 3), cap=16, cap_pairs=8, extra_ops=False, forget_after=2, link_ticks=1)
    rows = case["ops"][0][1]
    px, oracles = stage_for(case), PC.oracles_for(case)
    same(px.update(rows[:5], cap=16, cap_pairs=8), PO.run_bank(oracles, rows[:5], 16, 8), "before the reset")
    assert len(px.export_pairs(1)) > 0                                       # there is pair state to forget
    px.reset(1), oracles[1].reset()
    assert len(px.export_pairs(1)) == 0 and len(px.export(1)) == 0           # a pending reset already shows nothing
    same_state(px, oracles, "a pending reset")
    same(px.update(rows[5:8], cap=16, cap_pairs=8), PO.run_bank(oracles, rows[5:8], 16, 8), "after the reset")
    same_state(px, oracles, "after the reset")
    assert [o.frame for o in oracles] == [8, 3, 8]                                 # stream 1 counts its ticks anew
    # the ground map of one stream changes between calls; the metric with it
    px.option("metric", "ground"), px.option("near", 6)
    px.set_ground(PC.GROUND_H, PC.GROUND_SHIFT, stream=2), px.set_ground(PC.DOUBLED, 0, stream=0)
    for o in oracles:
        o.option("metric", PO.GROUND), o.option("near", 6)
    oracles[2].set_ground(PC.GROUND_H, PC.GROUND_SHIFT), oracles[0].set_ground(PC.DOUBLED, 0)
    same(px.update(rows[8:], cap=16, cap_pairs=8), PO.run_bank(oracles, rows[8:], 16, 8), "after set_ground")
    same_state(px, oracles, "after set_ground")
    px.close()


# ---------------------------------------------------------------------------------------------------- poisoned allocations
HIP_ERROR_WORDS = ("AicError", "hipError", "HIP error", "illegal memory access", "Memory access fault", "HSA_STATUS_ERROR")
CHILD_LIMIT_S = 90


def run_child(out_dir, mode):
    """One child under `timeout` (the discipline of tests/test_gpu_poison.py): a signal, a time limit or a HIP error ends the session."""
    env = {k: v for k, v in os.environ.items() if k != "AICAM_POISON_ALLOC"}
    env["AICAM_POISON_ALLOC"] = mode
    t0 = time.perf_counter()
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.join(ROOT, "tests", "prox_poison.py"), str(out_dir), mode]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    tail = (r.stdout[-300:] + r.stderr[-1500:])
    print(f"poison child prox / {mode}: {time.perf_counter() - t0:.1f} s, status {r.returncode}")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or any(w in tail for w in HIP_ERROR_WORDS):
        pytest.exit(f"poison child prox / {mode} ended with status {r.returncode} (a signal, its {CHILD_LIMIT_S} s limit or a HIP error); "
                    f"stopping, nothing more is started on this device:\n{tail}", returncode=1)
    assert r.returncode == 0, f"child prox / {mode} failed:\n{tail}"
    return P.load_recording(str(out_dir), mode)


def test_outputs_do_not_depend_on_what_memory_held(gpu, tmp_path):
    assert "AICAM_POISON_ALLOC" not in os.environ, "this process must not run under the hook: the children get it, one value each"
    recs = {}
    for mode in P.MODES:                                                     # one child at a time
        recs[mode] = run_child(tmp_path, mode)
        assert P.probe_shows(mode, recs[mode]), (mode, {k: recs[mode][k] for k in P.PROBE_KEYS})
    assert len(recs["zero"]) > 40 and any(k.endswith("_pairs0") and len(v) for k, v in recs["zero"].items())
    strip = lambda r: {k: v for k, v in r.items() if k not in P.PROBE_KEYS}                  # noqa: E731
    findings = {tag: P.compare(strip(recs["zero"]), strip(recs[tag])) for tag in ("big", "nan")}
    assert not any(findings.values()), "outputs that depend on what memory held: " + "; ".join(
        f"{tag}: {k} {what} at {idx}" for tag, f in findings.items() for k, what, idx in f[:8])


# ---------------------------------------------------------------------------------------------------- pipeline and CLI
def test_planted_scene_through_the_pipeline_hook():
    """The walker of tests/colours_cases.py, its boxes injected into the tiny pipeline run tests/test_gpu_heat.py uses: attach_proximity
    hands the run's tracks over; proximity_result equals a stage fed the same rows by hand and the oracle, and the tracks are unchanged."""
    import colours_cases as CC
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    TP, M = pkg("pipeline").TrackingPipeline, pkg("proximity")
    frames, rows = CC.planted_scene()
    T, H, W = len(frames), frames.shape[2], frames.shape[3]
    planted = [(r[0][:, :4].astype(np.float32) + np.array([0, 0, 1, 1], np.float32), np.full(len(r[0]), 0.9, np.float32), np.zeros(len(r[0]), np.int32))
               for r in rows]
    kw = dict(near=4000, link_ticks=2, unlink_ticks=2, height_ratio_q8=1024)

    def run(stage):
        pipe = TP(ypath, None, (H, W), batch=4, ring_frames=T, max_persons=64, dtype="fp16", inject=True, tracker="bytetrack", streams=1, track_buffer=3)
        pipe.upload(0, frames[:, 0])
        pipe.inject(0, planted)
        if stage is not None:
            pipe.attach_proximity(stage, cap=16, cap_pairs=8)
        out, results = [], []
        for lo, n in ((0, 8), (8, T - 8)):                                   # two run calls: the stage's state carries over
            out += pipe.run(lo, n)[0]
            results.append(pipe.proximity_result)
        pipe.close()
        return out, results

    plain, none = run(None)
    assert none == [None, None]
    stage = M.Proximity(1, (H, W), **kw)
    tracks, results = run(stage)
    assert tracks == plain and sum(len(t) for t in tracks) >= T              # the tracks are untouched
    ids = {n: i for i, n in enumerate(pkg("config").CLASSES)}
    to_rows = lambda tr: np.array([[t[0], t[1], t[2], t[3], t[4], ids.get(t[5], -1)] for t in tr], np.int32).reshape(-1, 6)      # noqa: E731
    by_hand, oracle = M.Proximity(1, (H, W), **kw), PO.ProxOracle((H, W), **kw)
    for (lo, n), got in zip(((0, 8), (8, T - 8)), results):
        fed = [[to_rows(tracks[lo + t])] for t in range(n)]
        same(got, flat(by_hand.update(fed, cap=16, cap_pairs=8)), ("pipeline against a stage fed by hand", lo))
        same(got, PO.run_bank([oracle], fed, 16, 8), ("pipeline against the oracle", lo))
    same_state(stage, [oracle], "pipeline")
    last = stage.flush()
    same(last, PO.flush_bank([oracle], stage.max_tracks), "flush")
    assert max(e["sightings"] for e in last.ended()) >= T // 2
    stage.close(), by_hand.close()


def test_cli_proximity_on_three_cameras_adds_only_its_keys(tmp_path, capsys):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli = pkg("cli")
    srcs = ["synthetic:640x360:6:16:1", "synthetic:640x360:4:16:2", "synthetic:640x360:5:16:3"]
    common = ["--inputs", ",".join(srcs), "--batch", "12", "--yolo_engine", ypath, "--tracker", "bytetrack"]
    ground = tmp_path / "ground.json"
    ground.write_text(json.dumps([dict(H=[2, 0, 0, 0, 2, 0, 0, 0, 1], shift=0), dict(H=[1, 0, 0, 0, 1, 0, 0, 0, 1]),
                                  dict(pixels=[[0, 0], [640, 0], [0, 360], [640, 360], [320, 180]], ground=[[0, 0], [64, 0], [0, 36], [64, 36], [32, 18]])]))
    runs = {}
    for name, extra in (("plain", []), ("prox", ["--proximity", "--proximity_file", str(tmp_path / "ended.jsonl")]),
                        ("ground", ["--proximity", "--ground", str(ground), "--near", "40"])):
        d = tmp_path / name
        assert cli.main(common + ["--output_dir", str(d)] + extra) == 0
        files = sorted(d.glob("*.jsonl"), key=lambda p: p.name[-8:])
        assert len(files) == 3
        runs[name] = [[json.loads(l) for l in f.read_text().splitlines()] for f in files]
    capsys.readouterr()
    new = {"parties", "units", "speed"}
    for name in ("prox", "ground"):
        for cam, (with_, without) in enumerate(zip(runs[name], runs["plain"])):
            assert len(with_) == len(without) == 16
            for a, b in zip(with_, without):
                assert set(a) - set(b) == new and {k: v for k, v in a.items() if k not in new} == b, (name, cam)
                assert len(a["speed"]) == len(a["tracks"]) and a["units"] == len(a["parties"])
                assert sorted(i for p in a["parties"] for i in p) == sorted(t[4] for t in a["tracks"]) or name == "ground"
    ended = [json.loads(l) for l in (tmp_path / "ended.jsonl").read_text().splitlines()] if (tmp_path / "ended.jsonl").exists() else []
    assert all(e["why"] in ("expired", "flushed") and e["sightings"] >= 1 for e in ended)
