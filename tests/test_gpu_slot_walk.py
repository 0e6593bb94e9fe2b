"""The slot walk on the device (csrc/slot_walk.hpp): bestshot_walk_kernel and colours_walk_kernel are two variants
of ONE life cycle, so on tests/slot_life_scene.py BestShots and TrackColours must give the same n_final, pending, status, event heads
and slots after every call -- and each must still equal its own oracle, bit for bit.  tests/test_slot_life_cycle.py pins on the CPU that
the two oracles agree on this scene."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import bestshot_oracle as BO
import colours_oracle as CO
import slot_life_scene as SL
from conftest import pkg

pytestmark = pytest.mark.gpu

NO_FRAMES = np.zeros((0,))


def equals(got, want, what):
    for k, (g, w) in enumerate(zip(got[:5], want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "output", k, g, w)


def test_one_scene_gives_both_stages_the_same_life_cycle():
    bs = pkg("bestshot").BestShots(SL.STREAMS, SL.HW, **SL.BS_KW)
    tc = pkg("colours").TrackColours(SL.STREAMS, SL.HW, **SL.CL_KW)
    bo = [BO.BestShotOracle(SL.HW, stream=s, **SL.BS_KW) for s in range(SL.STREAMS)]
    co = [CO.ColoursOracle(SL.HW, stream=s, **SL.CL_KW) for s in range(SL.STREAMS)]

    def exports(what):
        for s in range(SL.STREAMS):
            b_ev, c_ev = bs.export(s)[0], tc.export(s)
            SL.same_export_heads(b_ev, c_ev, (what, "export", s))
            assert len(b_ev) == len(bo[s].export()) and all(np.array_equal(g, w) for g, w in zip(c_ev, co[s].export())), (what, "export", s)

    for i, (frames, rows) in enumerate(SL.calls()):
        if i == 1:                                                           # not an all-stopped bank, and not an all-running one
            assert sorted(bs.failed) == sorted(tc.failed) == [2]
        b, c = bs.update(frames, rows, cap=SL.CAP), tc.update(frames, rows, cap=SL.CAP)
        SL.same_life(b, c, ("call", i))
        equals(b, BO.run_bank(bo, frames, rows, SL.CAP), ("best shots, call", i))
        equals(c, CO.run_bank(co, frames, rows, SL.CAP), ("colours, call", i))
        assert b.status.tolist() == [0, 0, SL.ERR_CAPACITY], (i, b.status)
        exports(("call", i))
    assert b.n_final.tolist() == [1, 1, 0] and b.pending.tolist() == [1, 1, 0]          # cap = 1: one handed over, one waits
    b, c = bs.flush(cap=SL.CAP), tc.flush(cap=SL.CAP)
    SL.same_life(b, c, "flush")
    equals(b, BO.flush_bank(bo, SL.CAP), "best shots, flush")
    equals(c, CO.flush_bank(co, SL.CAP), "colours, flush")
    exports("flush")
    b, c = bs.drain(cap=16), tc.drain(cap=16)
    SL.same_life(b, c, "drain")
    equals(b, BO.run_bank(bo, NO_FRAMES, [], 16), "best shots, drain")
    equals(c, CO.run_bank(co, NO_FRAMES, [], 16), "colours, drain")
    assert not b.pending.any() and b.n_final.tolist() == [2, 3, 0]
    exports("drain")
