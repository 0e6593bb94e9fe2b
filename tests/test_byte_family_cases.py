"""The scenes of tests/byte_family_cases.py through the NumPy oracles alone: together they reach every regime of the extended
assignment's side for both trackers, and the long small scene sees every life-cycle event.  This is what entitles
tests/test_gpu_byte_family_pinned.py to call its replay a test of every path of the BYTE skeleton (csrc/byte_epoch.hpp)."""
import pytest

import byte_family_cases as C

_RUNS = {}


def oracle(kind, sid):
    if (kind, sid) not in _RUNS:
        _RUNS[kind, sid] = C.oracle_run(kind, sid)
    return _RUNS[kind, sid]


@pytest.mark.parametrize("kind", C.KINDS)
def test_scenes_reach_every_regime_of_the_assignment(kind):
    seen = set()
    for fs in C.SCENES:
        sides, _, _ = oracle(kind, fs.id)
        assert (len(sides), max(sides)) == C.PROMISED[kind][fs.id], fs.id
        seen |= {C.regime(kind, s) for s in sides}
    assert seen == set(C.REGIMES), sorted(set(C.REGIMES) - seen)
    assert C.ARENA_SIDE[kind] < 128 and max(p[1] for p in C.PROMISED[kind].values()) <= 512


@pytest.mark.parametrize("kind", C.KINDS)
def test_long_small_scene_sees_every_life_cycle_event(kind):
    fs = C.SCENES[0]
    assert fs.long and fs.n == 12 and C.PARAMS[kind]["track_buffer"] == 5
    _, events, n_appearance = oracle(kind, fs.id)
    assert events == set(C.EVENTS), sorted(set(C.EVENTS) - events)
    if kind == "botsort":
        assert n_appearance >= 1, "no pair won by appearance"
        assert sum(w is not None for w in fs.warps()) > 0 and sum(w is None for w in fs.warps()) > 0


def test_bank_plan_covers_its_scenes():
    for s, sid in enumerate(C.BANK):
        assert sum(call[s] for call in C.BANK_PLAN) == C.scene_of(sid).frames
    assert any(0 in call for call in C.BANK_PLAN)                 # a stream without a frame in a call
