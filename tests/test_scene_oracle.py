"""tests/scene_oracle.py, the specification of the scene-watch stage, on the planted scenes of
tests/scene_cases.py: what the rules are meant to do, shown without a GPU.  tests/test_gpu_scene.py holds the device to the same oracle
on the same scenes, bit for bit."""
import numpy as np
import pytest

import gmc_oracle
import scene_cases as SC
import scene_oracle as SO

F = {n: i for i, n in enumerate(SO.RECORD_FIELDS)}


def run(cs):
    """(records [ticks, 16], masks [ticks, Hc, Wc], the oracle) of a one-stream case."""
    o = SC.oracles_for(cs)
    recs, masks, _ = SO.run(o, cs["frames"], cs["rows"])
    return recs[:, 0], masks[:, 0], o[0]


@pytest.fixture(scope="module", params=(2, 6, 12))
def noise_run(request):
    cs = SC.noise_mover(request.param)
    return (cs,) + run(cs)


def test_noise_alone_moves_nothing(noise_run):
    cs, recs, masks, _ = noise_run
    assert recs[20:60, F["ready"]].all()
    assert recs[20:60, F["n_raw"]].sum() == 0 and recs[20:60, F["n_moving"]].sum() == 0
    assert not masks[20:60].any()
    assert (recs[20:60, F["x0"]:F["y1"] + 1] == -1).all()


def test_mover_is_found_on_every_tick(noise_run):
    """Tolerance, stated: a cell the block covers only in part may stay below the threshold, and the cells it has left stay raw until
    they are re-learned (a raw cell learns slowly).  So the clean box reaches to within one cell (8 px) INSIDE each edge of the block,
    and lies within one cell OUTSIDE of everything the block has swept so far; and every cell the block covers whole is moving."""
    cs, recs, masks, _ = noise_run
    c = cs["cell"]
    sx0 = SC.mover_box(SC.MOVER_FROM)[0]
    for t in range(SC.MOVER_FROM, len(recs)):
        bx0, by0, bx1, by1 = SC.mover_box(t)
        x0, y0, x1, y1 = recs[t, F["x0"]:F["y1"] + 1]
        assert x0 <= bx0 + c and y0 <= by0 + c and x1 >= bx1 - c and y1 >= by1 - c, (t, (x0, y0, x1, y1), (bx0, by0, bx1, by1))
        assert x0 >= sx0 - c and y0 >= by0 - c and x1 <= bx1 + c and y1 <= by1 + c, (t, (x0, y0, x1, y1), (bx0, by0, bx1, by1))
        whole = masks[t, -(-by0 // c):by1 // c, -(-bx0 // c):bx1 // c]
        assert whole.size >= 3 * 7 and (whole & 1).all(), t
        assert recs[t, F["n_moving"]] >= whole.size and recs[t, F["active"]] == 1


def test_threshold_edge():
    cs = SC.threshold_edge()
    o = SC.oracles_for(cs)[0]
    o.tick(cs["frames"][0, 0]), o.tick(cs["frames"][1, 0])
    bg, dev = o.bg.copy(), o.dev.copy()
    thr = np.maximum(o.o["thresh"] << 8, (dev * o.o["noise_k_q4"]) >> 4)
    d = np.abs(256 * 106 - bg)
    assert d[1, 1] == thr[1, 1] + 1 and d[1, 3] == thr[1, 3]
    rec, mask, _ = o.tick(cs["frames"][2, 0])
    assert mask[1, 1] == 3 and mask[1, 3] == 0 and rec[F["n_raw"]] == 1


def test_floor_shift_reaches_the_level_exactly():
    cs = SC.floor_shift()
    recs, _, o = run(cs)
    assert (o.bg == 256 * 50).all()
    b = 256 * 100                                                            # the same walk with a shift that truncates toward zero
    for _ in range(len(recs)):
        b += int((256 * 50 - b) / 4)
    assert b == 256 * 50 + 3


def test_cleanup_isolated_cell_and_a_row_at_the_corner():
    """Read by the rule itself: with min_neighbours = 3 the middle of a row of three has three raw cells around it and stays, its two
    ends have two and go (at a corner nothing outside the grid helps); with min_neighbours = 2 all three stay.  The isolated cell is raw
    and never clean."""
    for k, row in ((3, [0, 1, 0]), (2, [1, 1, 1])):
        cs = SC.cleanup(k)
        recs, masks, _ = run(cs)
        m = masks[3]
        assert m[3, 4] == 2
        assert (m[0, :3] >> 1).tolist() == [1, 1, 1] and (m[0, :3] & 1).tolist() == row
        assert recs[3, F["n_raw"]] == 4 and recs[3, F["n_moving"]] == sum(row)
        assert not masks[:3].any()


def test_alarm_dark_raises_and_clears():
    recs, _, _ = run(SC.alarm_scene("dark"))
    dark = lambda field: recs[:, F[field]] & (SO.DARK | SO.DARK << 8)        # (lights off also blurs and changes the scene: other bits)
    assert dark("edges")[12] == SO.DARK and dark("alarms")[12:22].all()      # ticks 10, 11, 12: hold = 3
    assert dark("edges")[22] == SO.DARK << 8 and not dark("alarms")[22:].any()
    assert not recs[:12, F["alarms"]].any() and np.count_nonzero(dark("edges")) == 2


def test_alarm_defocus_holds_and_the_reference_is_frozen():
    recs, _, _ = run(SC.alarm_scene("defocus"))
    assert recs[9, F["ref_q8"]] >= 512
    assert recs[12, F["edges"]] & SO.DEFOCUS
    assert (recs[12:110, F["alarms"]] & SO.DEFOCUS).all()
    assert (recs[10:110, F["ref_q8"]] == recs[9, F["ref_q8"]]).all()
    assert (recs[10:110, F["sharp"]] == 0).all()


def test_alarm_frozen():
    recs, _, _ = run(SC.alarm_scene("frozen"))
    assert (recs[10:20, F["cond"]] & SO.FROZEN).all() and not (recs[:10, F["cond"]] & SO.FROZEN).any()
    assert recs[12, F["edges"]] == SO.FROZEN and recs[22, F["edges"]] == SO.FROZEN << 8


def test_alarm_scene_change_clears_by_itself():
    recs, _, _ = run(SC.alarm_scene("scene"))
    assert recs[12, F["edges"]] & SO.SCENE
    cleared = np.nonzero(recs[:, F["edges"]] & (SO.SCENE << 8))[0]
    assert len(cleared) == 1 and cleared[0] > 12
    assert not (recs[cleared[0]:, F["alarms"]] & SO.SCENE).any() and recs[-1, F["n_changed"]] == 0


def test_gate_drops_after_the_hold_and_rises_at_once():
    recs, _, _ = run(SC.gate_scene())
    busy = recs[:, F["n_moving"]] >= 4
    (a0, b0), (a1, b1) = SC.GATE_BUSY
    assert busy.tolist() == [a0 <= t < b0 or a1 <= t < b1 for t in range(len(recs))]
    active = recs[:, F["active"]]
    last = b0 - 1
    assert active[:4].all() and not active[a0 - 1]                           # forced while not ready; idle since create by tick 5
    assert active[a0:last + SC.GATE_HOLD + 1].all() and not active[last + SC.GATE_HOLD + 1:a1].any()
    assert active[a1:b1 + SC.GATE_HOLD].all() and not active[b1 + SC.GATE_HOLD:].any()


def test_row_motion():
    clean = np.zeros((6, 8), bool)
    clean[2:4, 2:6] = True                                                   # 8 of 48 cells, c = 4: pixels 8..23 x 8..15
    rows = [[8, 8, 23, 15], [-100, -100, 1000, 1000], [40, 0, 50, 10], [20, 8, 10, 15], [0, 0, (1 << 20) + 1, 5], [9, 9, 9, 9], [0, 0, 0, 0],
            [6, 6, 9, 9], [0, 0, 1 << 20, 1 << 20], [-(1 << 20) - 1, 0, 5, 5], [0, -5, 31, -1]]
    rows = np.array([r + [1, 0] for r in rows], np.int32)
    assert SO.row_motion(rows, clean, 4).tolist() == [256, 256 * 8 // 48, -1, -1, -1, 256, 0, 64, 256 * 8 // 48, -1, -1]
    assert SO.row_motion(np.zeros((0, 6), np.int32), clean, 4).shape == (0,)


@pytest.mark.parametrize("hw", [(37, 53), (64, 96), (4, 4)])
def test_gray_is_the_camera_motion_gray_at_cell_4(hw):
    img = np.random.default_rng(1).integers(0, 256, hw + (3,)).astype(np.uint8)
    assert np.array_equal(SO.gray(img, 4), gmc_oracle.gray_level(img, 4))
    for c in (4, 8, 16):
        if min(hw) >= c:
            v = np.random.default_rng(2).integers(0, 256, (hw[0] // c, hw[1] // c))
            assert np.array_equal(SO.gray(SC.paint(v, c, hw), c), v)                       # a uniform cell (v, v, v) has level v


def test_record_and_export_layout():
    cs = SC.seeded("layout", (16, 24), 8, ticks=8)
    o = SC.oracles_for(cs)[0]
    assert o.export()[3].tolist() == [0] * 16
    recs, _, rm = SO.run([o], cs["frames"], cs["rows"])
    assert recs[:, 0, F["frame"]].tolist() == list(range(8)) and recs[:, 0, F["ready"]].tolist() == [0] * 4 + [1] * 4
    assert len(rm) == sum(len(r[0]) for r in cs["rows"])
    bg, dev, prev, sc = o.export()
    assert bg.dtype == np.int32 and bg.shape == (2, 3) and sc[0] == 8 and np.array_equal(prev, SO.gray(cs["frames"][-1, 0], 8))
    o.reset()
    assert o.export()[3].tolist() == [0] * 16 and not o.export()[0].any()
