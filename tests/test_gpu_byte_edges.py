"""The BYTE skeleton (csrc/byte_epoch.hpp) on the planted scenes of tests/byte_edge_cases.py: duplicate removal with every outcome of its
age comparison, costs on, below and above a threshold, tied optima at all three stages, scores on every band edge, slot reuse, empty and
low-only frames, the lost timeout and the capacity boundary.  ByteTrack and BoT-SORT replay every scene through their public classes,
alone under the four (lsap_fast, epoch_frames) configurations and as banks; rows and scores are np.array_equal to the NumPy oracles'
frame by frame, the exports are compared as tests/test_gpu_bytetrack.py and tests/test_gpu_botsort.py compare theirs, and the counters
must show the oracle's problems: an equality or a tie has to go through the LSAP, a unique optimum through the read-off.

tests/test_byte_edge_cases.py (CPU) shows that the scenes reach these edges and that an exact comparison of ByteTrack is sound on them."""
import numpy as np
import pytest

import byte_edge_cases as E
from conftest import pkg
from test_gpu_botsort import compare_export as compare_botsort
from test_gpu_bytetrack import compare_export as compare_bytetrack

pytestmark = pytest.mark.gpu

_EXPECTED = {}
CLOCKS = ("cost_cycles", "kernel_cycles")


def expected(kind, sid):
    """The oracle's trace of the scene, once: its final state and the figures the device's counters must show."""
    if (kind, sid) not in _EXPECTED:
        trace, ora = E.oracle_trace(kind, sid)
        problems = [p for rec in trace for p in rec["problems"]]
        _EXPECTED[kind, sid] = dict(trace=trace, ora=ora, n_problems=len(problems), max_side=max([sum(p["cost"].shape) for p in problems] + [0]),
                                    n_read_off=sum(E.read_off(p["cost"], p["th"]) for p in problems))
    return _EXPECTED[kind, sid]


def single(kind, sid):
    sc = E.scene_of(sid)
    return pkg(kind).BYTETracker(**sc.params(kind)) if kind == "bytetrack" else pkg(kind).BoTSORT(**sc.params(kind))


def same_rows(got, trace, first, where):
    for i, (rows, conf) in enumerate(got):
        rec = trace[first + i]
        assert np.array_equal(rows, rec["rows"]), (where, rec["frame"], rows, rec["rows"])
        assert np.array_equal(conf, rec["conf"]), (where, rec["frame"], conf, rec["conf"])


def check_counters(c, want, lsap_fast, where):
    """n_fast + n_lsap = the oracle's non-empty problems; with the read-off on, n_fast = the problems whose OWN matrix satisfies read_off
    (BoT-SORT's matrices are the oracle's bit for bit; ByteTrack's are, or keep MARGIN_COST to the threshold: the same entries lie below)."""
    assert c["n_fast"] + c["n_lsap"] == want["n_problems"], (where, c, want["n_problems"])
    assert c["max_side"] == want["max_side"], (where, c, want["max_side"])
    assert c["n_fast"] == (want["n_read_off"] if lsap_fast else 0), (where, c, want["n_read_off"])


def compare_state(kind, dev, ora):
    (compare_bytetrack if kind == "bytetrack" else compare_botsort)(dev, ora)


@pytest.mark.parametrize("sid", [sc.id for sc in E.SCENES])
@pytest.mark.parametrize("kind", E.KINDS)
def test_single_tracker_on_every_scene(kind, sid):
    L = pkg("_lib")
    want = expected(kind, sid)
    for lsap_fast, epoch_frames in E.CONFIGS:
        where = (kind, sid, lsap_fast, epoch_frames)
        dev = single(kind, sid)
        dev.option("lsap_fast", lsap_fast)
        dev.option("epoch_frames", epoch_frames)
        f = 0
        for part in E.chunked(sid, kind):
            same_rows(dev.update_batch_arrays(part), want["trace"], f, where)
            f += len(part)
        compare_state(kind, dev, want["ora"])
        check_counters(dev.counters(), want, lsap_fast, where)
        if E.scene_of(sid).overflow is not None:                  # one slot short: the tracker stops
            with pytest.raises(L.AicError) as ei:
                dev.update_batch_arrays([E.overflow_of(sid, kind)])
            assert ei.value.code == L.ERR_CAPACITY, where
        dev.close()


# ------------------------------------------------------------------------------------------------------------------ banks
class Stream:
    """One stream of a bank with the face compare_export reads."""

    def __init__(self, bank, s):
        self.bank, self.s, self.feature_dim = bank, s, getattr(bank, "feature_dim", None)

    def export(self):
        return self.bank.export(self.s)

    def counters(self):
        return self.bank.counters(self.s)


def groups(kind):
    """The scenes by parameter set: a bank has one.  A scene alone with its parameters runs as two streams, under different plans."""
    out = {}
    for sc in E.SCENES:
        out.setdefault(repr(sorted(sc.params(kind).items())), []).append(sc.id)
    return [g * 2 if len(g) == 1 else g for g in out.values()]


def single_run(kind, sid, lsap_fast, epoch_frames):
    dev = single(kind, sid)
    dev.option("lsap_fast", lsap_fast)
    dev.option("epoch_frames", epoch_frames)
    for part in E.chunked(sid, kind):
        dev.update_batch_arrays(part)
    state = (dev.export(), {k: v for k, v in dev.counters().items() if k not in CLOCKS})
    dev.close()
    return state


@pytest.mark.parametrize("kind", E.KINDS)
def test_banks_of_scenes_equal_the_single_trackers(kind):
    L = pkg("_lib")
    lsap_fast, epoch_frames = 1, 0
    gs = groups(kind)
    assert sorted({sid for g in gs for sid in g}) == sorted(sc.id for sc in E.SCENES) and max(len(g) for g in gs) >= 10
    for g in gs:
        S, sc0 = len(g), E.scene_of(g[0])
        bk = pkg(kind).BYTETrackerBank(S, **sc0.params(kind)) if kind == "bytetrack" else pkg(kind).BoTSORTBank(S, **sc0.params(kind))
        bk.option("lsap_fast", lsap_fast)
        bk.option("epoch_frames", epoch_frames)
        frames = [E.frames_of(sid, kind) for sid in g]
        plan = E.bank_plan([len(fr) for fr in frames])
        assert any(0 in call for call in plan) and (S > 2 or [c[0] for c in plan] != [c[1] for c in plan])
        pos = [0] * S
        for call in plan:
            res = bk.update_arrays([frames[s][pos[s]:pos[s] + call[s]] for s in range(S)])
            for s in range(S):
                same_rows(res[s], expected(kind, g[s])["trace"], pos[s], (kind, g[s], "stream", s))
                pos[s] += call[s]
        for s, sid in enumerate(g):
            want = expected(kind, sid)
            compare_state(kind, Stream(bk, s), want["ora"])
            check_counters(bk.counters(s), want, lsap_fast, (kind, sid, "stream", s))
            exp, cnt = single_run(kind, sid, lsap_fast, epoch_frames)          # the stream is the single tracker, bit for bit
            got = bk.export(s)
            assert got.keys() == exp.keys()
            for key in exp:
                assert np.array_equal(np.asarray(got[key]), np.asarray(exp[key])), (kind, sid, s, key)
            assert {k: v for k, v in bk.counters(s).items() if k not in CLOCKS} == cnt, (kind, sid, s)
        if sc0.overflow is not None:                             # stream 0 comes one slot short and stops alone
            res = bk.update_arrays([[E.overflow_of(g[0], kind)]] + [[]] * (S - 1))
            assert res[0] is None and list(bk.failed) == [0] and res[1] == []
            with pytest.raises(L.AicError):
                bk.export(0)
            compare_state(kind, Stream(bk, 1), expected(kind, g[1])["ora"])
        bk.close()
