"""The OC-SORT kernel (csrc/kernels_ocsort.hip) on the planted scenes of tests/ocsort_edge_cases.py: an IoU on the threshold at each of
the three stages, tied optima, scores on every band edge, the OCM term at its end points, every exit of the observation lookup, a
reused slot with a stale ring, non-finite and shrinking predictions, the life-cycle edges, output coordinates on k + 0.5, the capacity
boundary and stage-1 problems on the kernel's own switches (64/65, 128/129, the 8428-float LDS arena).  OCSort replays every scene
under the four (lsap_fast, epoch_frames) configurations in the scene's ragged calls, OCSortBank replays them as streams; rows, scores,
the whole export (filter mean and covariance included) and every counter are np.array_equal to the NumPy oracle's: nothing is
compared with a tolerance.

tests/test_ocsort_edge_cases.py (CPU) shows that the oracle alone reaches the edge each scene is named for."""
import numpy as np
import pytest

import ocsort_edge_cases as E
from conftest import pkg
from test_gpu_ocsort import compare_export

pytestmark = pytest.mark.gpu

SCENE_IDS = [sc.id for sc in E.SCENES]


class Snapshot:
    """The oracle's export after one frame, with the face compare_export reads."""

    def __init__(self, rec):
        self.rec = rec

    def export(self):
        return self.rec["export"]


def single(sid, lsap_fast, epoch_frames):
    dev = pkg("ocsort").OCSort(**E.scene_of(sid).params)
    dev.option("lsap_fast", lsap_fast)
    dev.option("epoch_frames", epoch_frames)
    return dev


def same_rows(got, trace, first, where):
    for i, (rows, conf) in enumerate(got):
        rec = trace[first + i]
        assert np.array_equal(rows, rec["rows"]), (where, rec["frame"], rows, rec["rows"])
        assert np.array_equal(conf, rec["conf"]), (where, rec["frame"], conf, rec["conf"])


def check_counters(c, ora, where):
    assert c == {k: ora.stats[k] for k in c} and set(c) == set(ora.stats), (where, c, ora.stats)


@pytest.mark.parametrize("sid", SCENE_IDS)
def test_single_tracker_on_every_scene(sid):
    L = pkg("_lib")
    sc = E.scene_of(sid)
    for lsap_fast, epoch_frames in E.CONFIGS:
        where = (sid, lsap_fast, epoch_frames)
        trace, ora = E.oracle_trace(sid, bool(lsap_fast))
        dev = single(sid, lsap_fast, epoch_frames)
        f = 0
        for part in E.chunked(sid):
            same_rows(dev.update_batch_arrays(part), trace, f, where)
            f += len(part)
            compare_export(dev, Snapshot(trace[f - 1]))           # every key of OCSort.KEYS after every call
        assert f == len(trace)
        check_counters(dev.counters(), ora, where)
        if sc.overflow is not None:                               # one slot short: the tracker stops, as test_capacity_error_raises expects
            with pytest.raises(L.AicError) as ei:
                dev.update_batch_arrays([sc.overflow])
            assert ei.value.code == L.ERR_CAPACITY, where
            with pytest.raises(L.AicError):
                dev.update_batch_arrays([sc.frames[0]])
            with pytest.raises(L.AicError):
                dev.export()
        dev.close()


def test_every_scene_is_run():
    """The parametrised ids are exactly SCENES: no scene is skipped, xfailed or left out."""
    marks = {m.name for m in getattr(test_single_tracker_on_every_scene, "pytestmark", [])}
    assert marks == {"parametrize"}
    ids = [m.args[1] for m in test_single_tracker_on_every_scene.pytestmark if m.name == "parametrize"]
    assert ids == [SCENE_IDS] and sorted(SCENE_IDS) == sorted(sc.id for sc in E.SCENES) and len(set(SCENE_IDS)) == len(E.SCENES)
    assert sorted({sid for g in groups() for sid in g}) == sorted(SCENE_IDS)


# ------------------------------------------------------------------------------------------------------------------ banks
class Stream:
    """One stream of a bank with the face compare_export reads."""

    def __init__(self, bank, s):
        self.bank, self.s = bank, s

    def export(self):
        return self.bank.export(self.s)


def groups():
    """The scenes by parameter set: a bank has one.  A scene alone with its parameters runs as two streams, under different plans."""
    out = {}
    for sc in E.SCENES:
        out.setdefault(repr(sorted(sc.params.items())), []).append(sc.id)
    return [g * 2 if len(g) == 1 else g for g in out.values()]


def single_run(sid, lsap_fast, epoch_frames):
    dev = single(sid, lsap_fast, epoch_frames)
    for part in E.chunked(sid):
        dev.update_batch_arrays(part)
    state = (dev.export(), dev.counters())                       # OC-SORT's counters hold no clocks
    dev.close()
    return state


@pytest.mark.parametrize("g", groups(), ids=lambda g: g[0] + f"+{len(g) - 1}")
def test_banks_of_scenes_equal_the_single_trackers(g):
    L = pkg("_lib")
    lsap_fast, epoch_frames = 1, 0
    S, sc0 = len(g), E.scene_of(g[0])
    bk = pkg("ocsort").OCSortBank(S, **sc0.params)
    bk.option("lsap_fast", lsap_fast)
    bk.option("epoch_frames", epoch_frames)
    frames = [E.scene_of(sid).frames for sid in g]
    plan = E.bank_plan([len(fr) for fr in frames])
    assert any(0 in call for call in plan) and (S > 2 or [c[0] for c in plan] != [c[1] for c in plan])      # ragged, and some call leaves a stream out
    pos = [0] * S
    for call in plan:
        res = bk.update_arrays([frames[s][pos[s]:pos[s] + call[s]] for s in range(S)])
        for s in range(S):
            same_rows(res[s], E.oracle_trace(g[s])[0], pos[s], (g[s], "stream", s))
            pos[s] += call[s]
    for s, sid in enumerate(g):
        trace, ora = E.oracle_trace(sid)
        assert pos[s] == len(trace)
        compare_export(Stream(bk, s), ora)
        check_counters(bk.counters(s), ora, (sid, "stream", s))
        exp, cnt = single_run(sid, lsap_fast, epoch_frames)      # the stream is the single tracker, bit for bit
        got = bk.export(s)
        assert got.keys() == exp.keys()
        for key in exp:
            assert np.array_equal(np.asarray(got[key]), np.asarray(exp[key])), (sid, s, key)
        assert bk.counters(s) == cnt, (sid, s)
    if sc0.overflow is not None:                                 # stream 0 comes one slot short and stops alone
        res = bk.update_arrays([[sc0.overflow]] + [[]] * (S - 1))
        assert res[0] is None and list(bk.failed) == [0] and res[1] == []
        with pytest.raises(L.AicError):
            bk.export(0)
        res = bk.update_arrays([[]] + [[E.scene_of(g[1]).frames[-1]]] + [[]] * (S - 2))       # stream 1 carries on
        more, _ = E.oracle_trace(g[1], True, extra=(E.scene_of(g[1]).frames[-1],))
        same_rows(res[1], more, len(more) - 1, (g[1], "after the overflow of stream 0"))
        compare_export(Stream(bk, 1), Snapshot(more[-1]))
    bk.close()


def test_a_bank_holds_an_overflow_scene():
    assert sum(E.scene_of(g[0]).overflow is not None for g in groups()) >= 1 and max(len(g) for g in groups()) >= 8
