"""The cases of tests/call_history_cases.py are what they claim (no GPU): a patch is 192 bytes inside its box and changes the box's
crop, every history ends in a recorded call, and the clip of history (j) changes only inside the mover's boxes."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import call_history_cases as H                                          # noqa: E402
from oracle import image_oracle as I                                    # noqa: E402

PAIRS = [("A", f"A{k}", H.PATCHES[k], H.BOX, H.HW) for k in range(H.N_PATCH)] + \
        [("C", f"C{k}", H.BIG_PATCHES[k], H.BIG_BOX, H.BIG_HW) for k in range(H.N_PATCH_BIG)]


def test_case_counts_and_boxes():
    assert len(H.PATCHES) == len(set(H.PATCHES)) == 8 and len(H.BIG_PATCHES) == len(set(H.BIG_PATCHES)) == 2
    for box, boxes in ((H.BOX, H.BOXES), (H.BIG_BOX, H.BIG_BOXES)):
        x1, y1, x2, y2 = box
        assert x2 - x1 >= 40 and y2 - y1 >= 80 and tuple(boxes[0]) == box
    assert H.frame("A").shape == H.HW + (3,) and H.frame("C").shape == H.BIG_HW + (3,)
    assert H.BOX[2] <= H.HW[1] and H.BOX[3] <= H.HW[0] and H.BIG_BOX[2] <= H.BIG_HW[1] and H.BIG_BOX[3] <= H.BIG_HW[0]


@pytest.mark.parametrize("a,b,pos,box,hw", PAIRS, ids=[p[1] for p in PAIRS])
def test_b_is_a_with_one_patch_inside_the_box(a, b, pos, box, hw):
    A, B = H.frame(a), H.frame(b)
    assert A.shape == B.shape == hw + (3,) and A.dtype == B.dtype == np.uint8
    diff = A != B
    assert diff.sum() == H.PATCH * H.PATCH * 3 == 192
    ys, xs, _ = np.nonzero(diff)
    x, y = pos
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (y, y + H.PATCH - 1, x, x + H.PATCH - 1)
    assert np.array_equal((A ^ B)[diff], np.full(192, 0x80, np.uint8))
    assert box[0] <= x and x + H.PATCH <= box[2] and box[1] <= y and y + H.PATCH <= box[3]


@pytest.mark.parametrize("a,b,pos,box,hw", PAIRS, ids=[p[1] for p in PAIRS])
def test_the_box_crop_differs(a, b, pos, box, hw):
    """So the embeddings of row 0 have something to differ by; the other boxes' crops are the same."""
    boxes = H.boxes_of(b)
    ca, va = I.crops_to_batch(H.frame(a), boxes)
    cb, vb = I.crops_to_batch(H.frame(b), boxes)
    assert va.tolist() == vb.tolist() == [1, 1, 1, 0]
    assert not np.array_equal(ca[0], cb[0]) and np.abs(ca[0] - cb[0]).max() > 0.5
    assert np.array_equal(ca[1:], cb[1:])


def test_equal_bytes_other_geometry():
    assert H.frame("AT").shape == (H.HW[1], H.HW[0], 3) and H.frame("AT").tobytes() == H.frame("A").tobytes()
    _, v = I.crops_to_batch(H.frame("AT"), H.BOXES_T)
    assert v.tolist() == [1, 1, 1, 0]


def test_every_history_ends_in_a_recorded_call():
    ids = set(H.HISTORIES)
    assert {"b", "d", "e", "f", "g", "h", "i"} <= ids and sum(i[0] == "a" for i in ids) == 10 and sum(i[0] == "c" and i[-3:] != "ref" for i in ids) == 10
    for hid, calls in H.HISTORIES.items():
        assert len(calls) >= 2 and calls[-1][0] in ("detect", "embed"), hid
        engines = {c[1] for c in calls}
        assert engines <= {"Y", "R", "R2"} and len(engines) >= 2, hid        # another engine's call stands before the recorded one
        closed = set()
        for c in calls:
            assert c[1] not in closed, hid
            assert (c[0] == "detect") == (c[1] == "Y") or c[0] == "close", hid
            if c[0] == "close":
                closed.add(c[1])
            else:
                for n in (c[2] if isinstance(c[2], list) else [c[2]]):
                    H.frame(n.rstrip("+"))
        f, boxes = H.recorded_frame(hid)
        assert f.ndim == 3 and boxes.shape == (4, 4)
    for hid, ref in H.PATCH_CASES:                                           # same call, frames one patch apart
        a, b = H.recorded_call(hid), H.recorded_call(ref)
        assert a[0] == b[0] and (H.recorded_frame(hid)[0] != H.recorded_frame(ref)[0]).sum() == 192, hid
    for hid in H.EMBED_OF_A:
        assert H.recorded_call(hid)[0] == "embed" and H.recorded_frame(hid)[0] is H.frame("A")
    assert set(H.ORACLE_CASES) <= ids and all(H.recorded_call(h)[0] == "embed" for h in H.ORACLE_CASES)


def test_clip_changes_only_inside_the_movers_boxes():
    fr = H.clip()
    assert fr.shape == (H.J_FRAMES + 1,) + H.HW + (3,)
    for f in range(H.J_FRAMES):
        ys, xs, _ = np.nonzero(fr[f] != fr[f + 1])
        assert len(ys) > 0
        for g in (f, f + 1):                                                  # both positions lie in both frames' boxes: the boxes overlap
            x, y = H.mover_pos(g)
            assert 0 <= x and x + H.MOVER <= H.HW[1] and 0 <= y and y + H.MOVER <= H.HW[0]
        x1 = min(H.mover_box(f)[0], H.mover_box(f + 1)[0])
        y1 = min(H.mover_box(f)[1], H.mover_box(f + 1)[1])
        x2 = max(H.mover_box(f)[2], H.mover_box(f + 1)[2])
        y2 = max(H.mover_box(f)[3], H.mover_box(f + 1)[3])
        assert x1 <= xs.min() and xs.max() < x2 and y1 <= ys.min() and ys.max() < y2
        inside = np.zeros(H.HW, bool)
        for g in (f, f + 1):
            x, y = H.mover_pos(g)
            inside[y:y + H.MOVER, x:x + H.MOVER] = True
        assert not (fr[f] != fr[f + 1]).any(2)[~inside].any()
        boxes, conf, cls = H.planted(f)
        bx = H.mover_box(f)
        assert tuple(boxes[0]) == bx and bx[2] - bx[0] >= 40 and bx[3] - bx[1] >= 80
        x, y = H.mover_pos(f)
        assert bx[0] <= x and x + H.MOVER <= bx[2] and bx[1] <= y and y + H.MOVER <= bx[3]
        crops_f, v = I.crops_to_batch(fr[f], boxes)
        crops_n, _ = I.crops_to_batch(fr[f + 1], boxes)
        assert v.tolist() == [1, 1] and not np.array_equal(crops_f[0], crops_n[0]) and np.array_equal(crops_f[1], crops_n[1])
