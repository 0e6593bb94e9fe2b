"""The camera-motion specification (tests/gmc_oracle.py) on PanningScene: accuracy against the known similarity, every rule of its
steps 3, 4 and 6 hit at least once (asserted through stats), and what the estimate buys BoT-SORT (tests/botsort_oracle.py).

The accuracy bound is s / 2 px at every frame corner: the error of integer matching with no sub-pixel step at all (half a gray pixel);
a refinement that does worse than none is a bug.  For a pan by whole gray pixels the estimate is exact."""
import numpy as np
import pytest

import gmc_oracle as G
from botsort_oracle import BoTSORT as Oracle
from conftest import pkg

H, W = 360, 640


def _scene(**kw):
    kw.setdefault("n_targets", 0)
    kw.setdefault("pad", 128)
    return pkg("synthetic").PanningScene(seed=1, **kw)


def _estimate(sc, s, boxes=None, f=2):
    return G.estimate(sc.render(f - 1), sc.render(f), boxes, s)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("pan,rot,zoom", [((8, -4), 0, 1), ((5.3, 2.7), 0, 1), ((0, 0), 0, 1), ((2, 1), 0.5, 1.01), ((-3, 2), 1.0, 1.01),
                                          ((16, 0), 0, 1)])
def test_accuracy(s, pan, rot, zoom):
    sc = _scene(pan=pan, rot_deg=rot, zoom=zoom)
    w, st = _estimate(sc, s)
    if max(abs(p) for p in pan) >= 8 * s:
        # 16 px at s = 2 is 8 gray pixels: the border of the search square, which rule 4 discards (the range is |d| < 8 s)
        assert st["ok"] == 0 and st["border"] == st["blocks"] and np.array_equal(w, G.IDENTITY)
        return
    err = G.corner_error(w, sc.true_warp(2), H, W)
    print(f"s={s} pan={pan} rot={rot} zoom={zoom}: corner error {err:.4f} px, {st}")
    assert st["ok"] == 1 and st["inliers"] == st["kept"] == st["blocks"] == (36 if s == 4 else 190)
    assert err <= s / 2
    if rot == 0 and zoom == 1 and all(float(p) % s == 0 for p in pan):
        assert err == 0.0 and np.array_equal(w, sc.true_warp(2).astype(np.float32))


def test_person_box_removes_its_blocks():
    sc = _scene(pan=(4, 0))
    box = np.array([[8 * 4 + 1, 8 * 4 + 1, 8 * 4 + 60, 8 * 4 + 60]], np.float32)     # inside block (0, 0) of the s = 4 grid
    w0, st0 = _estimate(sc, 4)
    w1, st1 = _estimate(sc, 4, box)
    assert st0["masked"] == 0 and st1["masked"] == 1 and st1["kept"] == st0["kept"] - 1 and st1["ok"] == 1
    edge = np.array([[0, 0, 32, 32]], np.float32)                 # touches the block's corner without intersecting it
    assert _estimate(sc, 4, edge)[1]["masked"] == 0
    assert _estimate(sc, 4, np.array([[0, 0, W, H]], np.float32))[1]["masked"] == 36


def test_independent_movers_unmasked():
    """Rectangles with their own texture and motion touch about 30 % of the blocks (11 of 36); no box is passed.  The bound still holds."""
    sc = pkg("synthetic").PanningScene(seed=2, pan=(8, 4), n_targets=2, w_range=(60.0, 90.0), h_range=(70.0, 100.0), speed=9.0, pad=128)
    a, b = sc.render(1), sc.render(2)
    boxes = sc.boxes_at(2)
    covered = G.estimate(a, b, boxes, 4)[1]["masked"]
    assert 0.25 * 36 <= covered <= 0.4 * 36, covered
    w, st = G.estimate(a, b, None, 4)
    print(f"{covered} of 36 blocks under a mover: {st}, corner error {G.corner_error(w, sc.true_warp(2), H, W):.4f}")
    assert st["ok"] == 1 and st["masked"] == 0 and st["inliers"] < st["start"] == st["kept"]   # the residual gate of step 6 alone removed blocks
    assert G.corner_error(w, sc.true_warp(2), H, W) <= 4 / 2


def test_identity_cases():
    sc = _scene(pan=(4, 0))
    flat = np.full((H, W, 3), 90, np.uint8)
    w, st = G.estimate(flat, flat, None, 4)
    assert st["ok"] == 0 and st["flat"] == st["blocks"] == 36 and st["kept"] == 0 and np.array_equal(w, G.IDENTITY)
    w, st = G.estimate(None, sc.render(0), None, 4)                # a first frame
    assert st["ok"] == 0 and st["blocks"] == 36 and st["kept"] == 0 and np.array_equal(w, G.IDENTITY)
    w, st = _estimate(_scene(pan=(40, 0)), 4)                      # 10 gray pixels: outside the search
    assert st["ok"] == 0 and st["border"] > 0 and np.array_equal(w, G.IDENTITY)
    # too few blocks left for a fit (min_inliers): a frame of one block
    small = _scene(pan=(4, 0), width=128, height=128)
    w, st = G.estimate(small.render(1), small.render(2), None, 4)
    assert st["blocks"] == 1 and st["kept"] == 1 and st["ok"] == 0 and np.array_equal(w, G.IDENTITY)


def test_start_gate_through_stats():
    """A pasted region that moves 5 gray pixels against the background: its blocks fall outside the 4-pixel gate around the median."""
    syn = pkg("synthetic")
    bg = np.floor(syn._smooth_noise(np.random.default_rng(5), H + 64, W + 64) + 0.5).astype(np.uint8)
    fg = np.floor(syn._smooth_noise(np.random.default_rng(6), 120, 200, cells=(16, 8, 4)) + 0.5).astype(np.uint8)
    prev, cur = bg[32:32 + H, 32:32 + W].copy(), bg[28:28 + H, 24:24 + W].copy()      # the background moves by (8, 4)
    prev[100:220, 200:400] = fg
    cur[104:224, 228:428] = fg                                                       # the region by (28, 4): 5 gray pixels apart in x
    w, st = G.estimate(prev, cur, None, 4)
    print(st)
    assert st["ok"] == 1 and st["start"] < st["kept"] and st["inliers"] <= st["start"]
    assert G.corner_error(w, [[1, 0, 8], [0, 1, 4]], H, W) <= 4 / 2


def test_degenerate_fit_through_stats():
    """V <= 0 needs fewer than two distinct block centres: one block and min_inliers = 1."""
    small = _scene(pan=(4, 0), width=128, height=128)
    w, st = G.estimate(small.render(1), small.render(2), None, 4, min_inliers=1)
    assert st["kept"] == st["start"] == st["inliers"] == 1 and st["degenerate"] == 1 and st["ok"] == 0 and np.array_equal(w, G.IDENTITY)
    w, st = G.estimate(small.render(1), small.render(2), None, 4)
    assert st["degenerate"] == 0 and st["ok"] == 0 and st["inliers"] == 0          # min_inliers = 8 stops it before the fit


def test_start_gate_and_rounds():
    """Step 6 on planted displacements: the median gate drops far outliers before the first fit, the residual gate the near ones."""
    ii, jj = np.meshgrid(np.arange(9), np.arange(4))
    px, py = (16 * (8 + 16 * ii.ravel()) + 120).astype(np.int64), (16 * (8 + 16 * jj.ravel()) + 120).astype(np.int64)
    dx, dy = np.full(36, 32, np.int64), np.full(36, -16, np.int64)
    dx[:5] += 100                                                  # beyond the start gate
    dx[5:9] += 40                                                  # inside it, beyond the residual gate once the fit has settled
    ok, (a, b, tx, ty), n, rounds = G.fit_similarity(px, py, dx, dy)
    assert ok == 1 and rounds == 3 and n == 27 and a == 1.0 and b == 0.0 and tx == 32.0 and ty == -16.0
    ok, _, n, _ = G.fit_similarity(px[:7], py[:7], dx[:7], dy[:7])
    assert ok == 0 and n == 0
    dx2 = np.arange(36, dtype=np.int64) * 200                       # no agreement at all
    ok, _, n, rounds = G.fit_similarity(px, py, dx2, dy)
    assert ok == 0 and n < 8 and rounds == 0


def tie_frames(s, gh=64, gw=80, shift=2):
    """Two frames whose gray levels have period 4 along x and no period along y, the second shifted by `shift` gray pixels in x: the
    candidates dx = shift - 8, shift - 4, shift, shift + 4 at dy = 0 all have SAD 0.  With shift = 2 the first in (dy, dx) order is
    dx = -6, interior; a rule that took the last minimum would give +6, the smallest |dx| +-2."""
    rows = np.random.default_rng(9).permutation(gh) * 2                              # distinct per row: dy != 0 never ties
    pat = np.array([0, 60, 120, 30])

    def level(sh):
        return (rows[:, None] + pat[(np.arange(gw)[None, :] - sh) % 4]).astype(np.uint8)

    def frame(g):                                                                    # B = G = R: the gray level is g exactly
        return np.repeat(np.repeat(np.repeat(g, s, 0), s, 1)[:, :, None], 3, 2)

    return np.stack([frame(level(0)), frame(level(shift))])


@pytest.mark.parametrize("s", [2, 4])
def test_ties_go_to_the_first_candidate(s):
    frames = tie_frames(s)
    assert np.array_equal(G.gray_level(frames[0], s)[:, :8] - G.gray_level(frames[0], s)[:, :1], np.tile([0, 60, 120, 30], 2)[None] * np.ones((64, 1), int))
    w, st = G.estimate(frames[0], frames[1], None, s)
    assert st["ok"] == 1 and st["border"] == st["flat"] == 0 and st["inliers"] == st["blocks"] == 12
    assert np.array_equal(w, np.array([[1, 0, -6 * s], [0, 1, 0]], np.float32))
    # the same pattern unshifted: the first of the tied minima (dx = -8) lies on the border of the search square
    w, st = G.estimate(frames[0], frames[0], None, s)
    assert st["border"] == st["blocks"] and st["ok"] == 0


# ------------------------------------------------------------------------------------------------------------------- the payoff
PAYOFF = dict(seed=3, pan=(12, 0), n_targets=6, reverse_at=15, pad=256)
GAP = (15, 24)


def payoff_scene():
    """Persons stand still in the world, the camera pans 12 px per frame for 40 frames and sweeps back from frame 15 on, while the
    detections are missing for 10 frames: a constant-velocity filter coasts the wrong way through the gap."""
    return pkg("synthetic").PanningScene(gaps=[(t, *GAP) for t in range(PAYOFF["n_targets"])], **PAYOFF)


def payoff_ids(sc, warps, n=40):
    ora, ids = Oracle(with_reid=False), []
    for f in range(n):
        b, c, k, ident = sc.detections(f)
        rows, _ = Oracle.rows(ora.update_xyxy(b, c, k, None, warps[f]))
        ids.append(dict(zip(map(tuple, rows[:, :4].tolist()), rows[:, 4].tolist())))
    return ids


def payoff_warps(sc, n=40):
    est, warps = G.Stream(4), []
    for f in range(n):
        warps.append(est.apply(sc.render(f), sc.detections(f)[0])[0])
    return warps


def test_payoff_quality():
    """MOTA, IDF1 and ID switches of the oracle tracker on the payoff scene without a warp and with the estimated one."""
    mm = pkg("mot_metrics")
    sc, n = payoff_scene(), 40
    gt = mm.scene_ground_truth(sc, n)
    res = {}
    for name, ws in (("none", [None] * n), ("estimated", payoff_warps(sc, n))):
        ora, outs = Oracle(with_reid=False), []
        for f in range(n):
            b, c, k, _ = sc.detections(f)
            outs.append([tuple(r[:5]) for r in Oracle.rows(ora.update_xyxy(b, c, k, None, ws[f]))[0].tolist()])
        res[name] = mm.evaluate(gt, outs)
        print(name, {k: round(v, 4) if isinstance(v, float) else v for k, v in res[name].items()})
    assert res["estimated"]["idsw"] == 0 and res["none"]["idsw"] > 0
    assert res["estimated"]["idf1"] > res["none"]["idf1"] and res["estimated"]["mota"] > res["none"]["mota"]


def test_payoff_ids_survive_the_gap_with_the_estimated_warp():
    sc, n = payoff_scene(), 40
    est, warps = G.Stream(4), []
    for f in range(n):
        w, st = est.apply(sc.render(f), sc.detections(f)[0])
        assert st["ok"] == (f > 0), (f, st)
        assert G.corner_error(w, sc.true_warp(f), H, W) <= 2.0
        warps.append(w)
    true = [None] + [sc.true_warp(f).astype(np.float32) for f in range(1, n)]
    before, after = GAP[0] - 1, GAP[1] + 1
    runs = {name: payoff_ids(sc, ws) for name, ws in (("none", [None] * n), ("estimated", warps), ("true", true))}
    seen = set(runs["none"][before].values())
    assert len(seen) >= 2
    for name in ("estimated", "true"):
        assert set(runs[name][before].values()) == seen
        assert seen <= set(runs[name][after].values()) and max(runs[name][n - 1].values()) <= PAYOFF["n_targets"], name
    assert not (seen & set(runs["none"][after].values())), "the no-warp run kept its ids: the scene shows nothing"
