"""One scene for both stages that walk a slot table (csrc/slot_walk.hpp): best shots and clothing colours run ONE
life cycle, so the same frames and rows must give both the same life-cycle answers.  tests/test_slot_life_cycle.py pins that on the two
oracles, tests/test_gpu_slot_walk.py on the device.

3 streams of 48 x 64 frames, 14 ticks; max_tracks = 4, forget_after = 1, cap = 1.  Stream s has 3 + s ids.  Id 1 of every stream comes
and goes with a period of 5 ticks, away at ticks 2 3, 7 8, 12 13: with forget_after = 1 the second tick away ends its track, and it comes
back as a new one into the slot that became free; the other ids stay.  With cap = 1 a call hands over one ENDED track a stream: the
third call ends two, so one waits in its slot (pending 1).  Stream 2's five ids do not fit four slots: it stops with AIC_ERR_CAPACITY in
the first call, while streams 0 and 1 run to the end.  Boxes are 20 x 32 pixels inside the frame, so both stages count the same rows
(region "box", pad 0: both flag NONEMPTY on the clipped whole box).  Tick 3 carries a duplicate id and a row wholly outside the frame on
every stream."""
import numpy as np

STREAMS, HW, TICKS = 3, (48, 64), 14
MAX_TRACKS, FORGET_AFTER, CAP = 4, 1, 1
CALLS = (5, 1, 8)                                                            # ticks per call
BS_KW = dict(thumb=(16, 16), max_tracks=MAX_TRACKS, forget_after=FORGET_AFTER, region="box", pad=0)
CL_KW = dict(max_tracks=MAX_TRACKS, forget_after=FORGET_AFTER)
ERR_CAPACITY = -5
HEAD = 7                                                                     # reason, stream, id, cls, first_frame, last_seen, sightings
BS_SLOT, CL_SLOT = 14, 13                                                    # where an event names its slot


def box(j, tick):
    x, y = 2 + 8 * j + tick % 3, 3 + 2 * j
    return [x, y, x + 19, y + 31]


def rows_of(stream, tick):
    rows = [box(j, tick) + [100 * stream + j, j % 2] for j in range(3 + stream) if not (j == 1 and tick % 5 in (2, 3))]
    if tick == 3:
        rows.insert(1, [70, 50, 90, 60, 999, 0])                            # wholly outside the frame: counted by neither
        rows.append(rows[0][:4] + [rows[0][4], 1])                          # its id again: only the first row of an id counts
    return np.array(rows, np.int32).reshape(-1, 6)


def scene():
    """(frames uint8 [TICKS, STREAMS, H, W, 3], rows[tick][stream] = [n, 6] int32)"""
    frames = np.random.default_rng(48).integers(0, 256, (TICKS, STREAMS) + HW + (3,), dtype=np.uint8)
    return frames, [[rows_of(s, t) for s in range(STREAMS)] for t in range(TICKS)]


def calls():
    """[(frames, rows)] of the scene cut into CALLS."""
    frames, rows = scene()
    out, lo = [], 0
    for n in CALLS:
        out.append((frames[lo:lo + n], rows[lo:lo + n]))
        lo += n
    assert lo == TICKS
    return out


def same_life(bs, cl, what):
    """bs, cl: (n_final, events, x, pending, status) of one call of each stage."""
    assert np.array_equal(bs[0], cl[0]), (what, "n_final", bs[0], cl[0])
    assert np.array_equal(bs[3], cl[3]), (what, "pending", bs[3], cl[3])
    assert np.array_equal(bs[4], cl[4]), (what, "status", bs[4], cl[4])
    assert np.array_equal(bs[1][:, :, :HEAD], cl[1][:, :, :HEAD]), (what, "events", bs[1][:, :, :HEAD], cl[1][:, :, :HEAD])
    assert np.array_equal(bs[1][:, :, BS_SLOT], cl[1][:, :, CL_SLOT]), (what, "slots", bs[1][:, :, BS_SLOT], cl[1][:, :, CL_SLOT])


def same_export_heads(bs_events, cl_events, what):
    """export() of one stream of each stage: the same slots hold the same tracks."""
    assert len(bs_events) == len(cl_events), (what, len(bs_events), len(cl_events))
    for b, c in zip(bs_events, cl_events):
        assert np.array_equal(b[:HEAD], c[:HEAD]) and b[BS_SLOT] == c[CL_SLOT], (what, b, c)
