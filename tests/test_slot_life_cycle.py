"""The two stages that walk a slot table run one life cycle (csrc/slot_walk.hpp): on tests/slot_life_scene.py the best-shot oracle and the
colour oracle must give the same n_final, pending, status, event heads and slots after every call.  CPU only: this pins the agreement
of the two specifications that tests/test_gpu_slot_walk.py holds the device to."""
import numpy as np

import bestshot_oracle as BO
import colours_oracle as CO
import slot_life_scene as SL

NO_FRAMES = np.zeros((0,))


def test_both_oracles_agree_on_the_life_cycle_call_by_call():
    assert SL.ERR_CAPACITY == BO.ERR_CAPACITY == CO.ERR_CAPACITY
    bo = [BO.BestShotOracle(SL.HW, stream=s, **SL.BS_KW) for s in range(SL.STREAMS)]
    co = [CO.ColoursOracle(SL.HW, stream=s, **SL.CL_KW) for s in range(SL.STREAMS)]
    seen = []
    for i, (frames, rows) in enumerate(SL.calls()):
        if i == 1:                                                           # not an all-stopped bank, and not an all-running one
            assert [o.status for o in bo] == [0, 0, SL.ERR_CAPACITY]
        b, c = BO.run_bank(bo, frames, rows, SL.CAP), CO.run_bank(co, frames, rows, SL.CAP)
        SL.same_life(b, c, ("call", i))
        seen.append((b[0].tolist(), b[3].tolist(), b[4].tolist()))
    # streams 0 and 1 deliver under cap = 1 and end with one track waiting; stream 2 stopped in the first call and delivers nothing
    E = SL.ERR_CAPACITY
    assert seen == [([1, 1, 0], [0, 0, 0], [0, 0, E]), ([0, 0, 0], [0, 0, 0], [0, 0, E]), ([1, 1, 0], [1, 1, 0], [0, 0, E])]
    assert bo[0].log["reused_in_call"] >= 1 and co[0].log["reused_in_call"] >= 1          # a returning id took the slot its old track left
    for s in range(SL.STREAMS):
        SL.same_export_heads([e for e, _ in bo[s].export()], co[s].export(), ("export", s))
    b, c = BO.flush_bank(bo, SL.CAP), CO.flush_bank(co, SL.CAP)
    SL.same_life(b, c, "flush")
    assert b[0].tolist() == [1, 1, 0] and b[3].tolist() == [2, 3, 0]         # the waiting track first; the live ones now wait
    b, c = BO.run_bank(bo, NO_FRAMES, [], 16), CO.run_bank(co, NO_FRAMES, [], 16)
    SL.same_life(b, c, "drain")
    assert b[0].tolist() == [2, 3, 0] and not b[3].any()
    for s in range(SL.STREAMS):
        SL.same_export_heads([e for e, _ in bo[s].export()], co[s].export(), ("export at the end", s))


def test_the_scene_has_what_it_says():
    frames, rows = SL.scene()
    assert frames.shape == (14, 3, 48, 64, 3) and [len(rows[0][s]) for s in range(3)] == [3, 4, 5]
    for t in range(SL.TICKS):
        for s in range(SL.STREAMS):
            r = rows[t][s]
            inside = r[r[:, 4] != 999]
            assert (inside[:, 0] >= 0).all() and (inside[:, 1] >= 0).all() and (inside[:, 2] < 64).all() and (inside[:, 3] < 48).all()
            assert ((inside[:, 2] - inside[:, 0] + 1 == 20) & (inside[:, 3] - inside[:, 1] + 1 == 32)).all()
            assert (100 * s + 1 in r[:, 4]) == (t % 5 not in (2, 3))
    r = rows[3][0]
    assert (r[:, 4] == 999).sum() == 1 and (r[:, 4] == r[0, 4]).sum() == 2 and r[1, 0] >= 64 and r[1, 1] >= 48
