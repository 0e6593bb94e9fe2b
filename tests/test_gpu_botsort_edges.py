"""What BoT-SORT adds to the BYTE skeleton (BsVariant of csrc/kernels_botsort.hip, csrc/kf8wh_math.hpp, botsort_normalize_kernel) on the
planted scenes of tests/botsort_edge_cases.py: the proximity veto and the appearance gate on their thresholds, an appearance distance
equal to the IoU distance, the clamp, first feature against smoothed update, the has_feat life cycle, the one needed dot product on the
64-pair group boundaries of cost_pass, the warp before the costs, and features that do not normalise to finite values.  Every scene runs
through the public BoTSORT class under the four (lsap_fast, epoch_frames) configurations and as a stream of a BoTSORTBank; rows and
scores are np.array_equal to the oracle's frame by frame, the export (Kalman state, has_feat, smooth_feat) and n_appearance as
tests/test_gpu_botsort.py compares them, the counters as tests/test_gpu_byte_edges.py does.  No tolerance anywhere.

tests/test_botsort_edge_cases.py (CPU) shows that the scenes reach these edges."""
import numpy as np
import pytest

import botsort_edge_cases as B
from conftest import pkg
from test_gpu_botsort import compare_export, frames_of as random_frames, run_pair, scene
from test_gpu_byte_edges import CLOCKS, Stream, check_counters, same_rows

pytestmark = pytest.mark.gpu

_EXPECTED = {}
GROUPS = B.groups()


def expected(sid, sign=1):
    """The oracle's trace of the scene, once: its final state and the figures the device's counters must show."""
    if (sid, sign) not in _EXPECTED:
        trace, ora = B.oracle_trace(sid, sign)
        problems = [p for rec in trace for p in rec["problems"]]
        _EXPECTED[sid, sign] = dict(trace=trace, ora=ora, n_problems=len(problems), max_side=max([sum(p["cost"].shape) for p in problems] + [0]),
                                    n_read_off=sum(B.read_off(p["cost"], p["th"]) for p in problems))
    return _EXPECTED[sid, sign]


def single(sid, lsap_fast, epoch_frames):
    dev = pkg("botsort").BoTSORT(**B.scene_of(sid).params())
    dev.option("lsap_fast", lsap_fast)
    dev.option("epoch_frames", epoch_frames)
    return dev


@pytest.mark.parametrize("sid", [sc.id for sc in B.SCENES])
def test_single_tracker_on_every_scene(sid):
    want = expected(sid)
    for lsap_fast, epoch_frames in B.CONFIGS:
        where = (sid, lsap_fast, epoch_frames)
        dev = single(sid, lsap_fast, epoch_frames)
        f = 0
        for part in B.chunked(sid):
            same_rows(dev.update_batch_arrays(part), want["trace"], f, where)
            f += len(part)
        compare_export(dev, want["ora"])
        check_counters(dev.counters(), want, lsap_fast, where)
        dev.close()


def single_run(sid, sign, lsap_fast, epoch_frames):
    dev = single(sid, lsap_fast, epoch_frames)
    for part in B.chunked(sid, sign):
        dev.update_batch_arrays(part)
    state = (dev.export(), {k: v for k, v in dev.counters().items() if k not in CLOCKS})
    dev.close()
    return state


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=[f"{g[0]}-x{len(g)}" for g in GROUPS])
def test_banks_of_scenes_equal_the_single_trackers(g):
    """Streams of one parameter set under bank_plan's ragged calls; odd streams take every feature negated, so that two neighbours never
    hold the same vector at the same slot index: a stream that read its neighbour's smoothed features would see every distance change."""
    lsap_fast, epoch_frames = 1, 0
    g = GROUPS[g]
    S, signs = len(g), [1 - 2 * (s % 2) for s in range(len(g))]
    bk = pkg("botsort").BoTSORTBank(S, **B.scene_of(g[0]).params())
    bk.option("lsap_fast", lsap_fast)
    bk.option("epoch_frames", epoch_frames)
    frames = [B.frames_of(sid, sg) for sid, sg in zip(g, signs)]
    plan = B.bank_plan([len(fr) for fr in frames])
    assert any(0 in call for call in plan) and (S > 2 or [c[0] for c in plan] != [c[1] for c in plan])
    pos = [0] * S
    for call in plan:
        res = bk.update_arrays([frames[s][pos[s]:pos[s] + call[s]] for s in range(S)])
        for s in range(S):
            same_rows(res[s], expected(g[s], signs[s])["trace"], pos[s], (g[s], "stream", s))
            pos[s] += call[s]
    for s, sid in enumerate(g):
        want = expected(sid, signs[s])
        compare_export(Stream(bk, s), want["ora"])
        check_counters(bk.counters(s), want, lsap_fast, (sid, "stream", s))
        exp, cnt = single_run(sid, signs[s], lsap_fast, epoch_frames)           # the stream is the single tracker, bit for bit
        got = bk.export(s)
        assert got.keys() == exp.keys()
        for key in exp:
            assert np.array_equal(np.asarray(got[key]), np.asarray(exp[key])), (sid, s, key)
        assert {k: v for k, v in bk.counters(s).items() if k not in CLOCKS} == cnt, (sid, s)
    bk.close()


# one lane of one pass; the last lane partial; exactly one pass; one pass and a lane; four and sixteen passes of wave_dot, feat_update_wave
# and the normalise kernel (256 elements a pass, 4 a lane)
@pytest.mark.parametrize("dim", [4, 252, 256, 260, 1024, 4096])
def test_feature_dims(dim):
    dets = random_frames(scene(n=6, frames=80, seed=9), 20, dim=dim)
    dev, ora = run_pair(dets, chunk=7, feature_dim=dim)
    assert dev.counters()["n_appearance"] == ora.n_appearance > 0, "the scene does not exercise the appearance term"
    assert dev.export()["has_feat"].all()
    dev.close()
