"""The tiled renderer on the GPU (aic_render_frames, csrc/kernels_render.hip) against its executable
specification tests/render_oracle.py: every frame of every case np.array_equal.

Shapes for the 64 x 32 tile: 2 x 64 x 128 (exact tiles, dword loads), 3 x 70 x 131 (partial tiles right and bottom, 3 W % 4 != 0 -> byte
path, the last 32-cell 6 rows tall), 1 x 33 x 65 (one extra row and column of tiles holding one pixel row / column)."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import render_oracle as RO
from conftest import pkg

SHAPES = [(2, 64, 128), (3, 70, 131), (1, 33, 65)]
MASKS = {0: [[(-20, 10), (100, 4), (60, 30), (120, 60), (30, 66), (45, 35)]],                     # concave, over several tiles, a vertex outside
         1: [[(5, 5), (40, 5), (40, 20), (5, 20)], [(70, 40), (90, 69), (50, 60)]]}


def frames_of(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


def rows_for(F, H, W, seed=1):
    """Per frame: straddling the tile borders and every frame edge (negative coordinates too), fully outside, one pixel, overlapping,
    an inverted row (dropped); the middle frame of three is empty."""
    rng = np.random.default_rng(seed)
    per = []
    for f in range(F):
        if F == 3 and f == 1:
            per.append(np.zeros((0, 6), np.int32))
            continue
        r = [(50, 20, 80, 45, 1, 0), (60, 28, 70, 36, 2, 0),                  # across the tile corner at (64, 32), overlapping
             (-15, -9, 6, 7, 3, 0), (W - 5, H - 4, W + 30, H + 9, 4, 2),      # the top-left and bottom-right frame corners
             (-40, 10, -3, 30, 5, 0), (W, 0, W + 10, 10, 6, 0), (0, H, 10, H + 5, 7, 0), (10, -30, 20, -1, 8, 0),      # fully outside
             (33, 17, 33, 17, 9, 1), (W - 1, H - 1, W - 1, H - 1, 10, 0),      # one pixel
             (20, 25, 10, 30, 11, 0),                                           # x2 < x1: dropped
             (5, H - 12, 30, H + 3, 12, 77), (W - 20, -3, W + 2, 12, 13, -1)]   # bottom and right edges; classes outside 0..63
        for k in range(4):
            x, y = int(rng.integers(-10, W)), int(rng.integers(-10, H))
            r.append((x, y, x + int(rng.integers(0, 40)), y + int(rng.integers(0, 30)), 20 + k, int(rng.integers(0, 3))))
        per.append(np.array(r, np.int32))
    return np.concatenate(per), np.array([len(p) for p in per], np.int32)


def prims_for(F, H, W):
    V = pkg("visualization")
    out = []
    for f in range(F):
        pl = V.PrimList()
        pl.fill(40, 10, 90, 40, (10, 20, 30))
        pl.outline(30 + f, 8, 100, 50, (0, 255, 0))
        pl.put_text(50, 26, "Id:7 ~x", 2, (255, 255, 255))                     # across the tile border at x = 64 and y = 32
        pl.put_text(-7, H - 10, "edge|", 3, (1, 2, 3))
        pl.segment(3, 3, W + 5, H - 2, 3, (200, 0, 0))                          # across every tile
        pl.segment(70, -4, 60, H + 4, 1, (0, 0, 200))
        pl.segment(W - 1, 5, 0, 15, 8, (7, 7, 7))
        pl.segment(20, 20, 20, 20, 4, (9, 9, 9))                                # A == B: nothing
        pl.outline(62, 30, 66, 34, (255, 0, 255))
        out.append(pl)
    return out


def oracle_call(frames, rows=None, counts=None, prims=None, cameras=None, masks=None, n_cameras=1, **kw):
    lists = None if prims is None else [None if p is None else p.arrays() for p in prims]
    return RO.render(frames, rows, counts, lists, cameras, masks, n_cameras, **kw)


@pytest.fixture(scope="module")
def R(gpu):
    return pkg("render")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("style,cell", [("mosaic", 4), ("mosaic", 8), ("mosaic", 16), ("mosaic", 32), ("fill", 16)])
@pytest.mark.parametrize("redact", ["box", "head"])
def test_redaction_styles_modes_and_cells(R, shape, style, cell, redact):
    F, H, W = shape
    fr = frames_of(shape)
    rows, counts = rows_for(F, H, W)
    kw = dict(redact=redact, style=style, cell=cell, fill_color=(3, 200, 77), pad=2 if redact == "box" else 0, head_q8=96)
    r = R.Renderer(**kw)
    got = r.render(fr.copy(), rows, counts)
    r.close()
    exp = oracle_call(fr, rows, counts, **dict(kw, fill_color=3 | 200 << 8 | 77 << 16))
    assert (got != fr).any() and np.array_equal(got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_everything_at_once_two_cameras(R, shape):
    """Rows, primitives (text and segments across tile borders) and two cameras with different masks, `cameras` given explicitly."""
    F, H, W = shape
    fr = frames_of(shape, 3)
    rows, counts = rows_for(F, H, W, 4)
    prims = prims_for(F, H, W)
    cams = np.array([1, 0, 1][:F], np.int32)
    r = R.Renderer(cameras=2, redact="box", style="mosaic", cell=8, classes={0, 2}, mask_color=(9, 8, 7), pad=1)
    for c, polys in MASKS.items():
        r.set_masks(c, polys)
    got = r.render(fr.copy(), rows, counts, prims, cams)
    exp = oracle_call(fr, rows, counts, prims, cams, MASKS, 2, redact="box", style="mosaic", cell=8, classes={0, 2}, mask_color=9 | 8 << 8 | 7 << 16, pad=1)
    assert np.array_equal(got, exp)
    # the default camera order f % cameras, and masks alone
    got = r.render(fr.copy())
    exp = oracle_call(fr, masks=MASKS, n_cameras=2, mask_color=9 | 8 << 8 | 7 << 16)
    assert np.array_equal(got, exp) and (got != fr).any()
    # F frames in one call equal F calls of one frame; chunk_frames = 1 equals unchunked
    whole = r.render(fr.copy(), rows, counts, prims, cams)
    off = np.concatenate([[0], np.cumsum(counts)])
    single = np.stack([r.render(fr[f:f + 1].copy(), rows[off[f]:off[f + 1]], counts[f:f + 1], prims[f:f + 1], cams[f:f + 1])[0] for f in range(F)])
    assert np.array_equal(whole, single)
    r.option("chunk_frames", 1)
    assert np.array_equal(r.render(fr.copy(), rows, counts, prims, cams), whole)
    r.close()


@pytest.mark.gpu
def test_512_rows_and_1500_primitives_in_one_tile(R):
    """The limits, all landing in one tile: 512 rectangles, and 1500 primitives of which the later paint over the earlier."""
    V = pkg("visualization")
    shape = (3, 70, 131)
    fr = frames_of(shape, 5)
    rng = np.random.default_rng(6)
    x, y = rng.integers(64, 100, 512), rng.integers(32, 60, 512)
    rows512 = np.stack([x, y, x + rng.integers(0, 6, 512), y + rng.integers(0, 5, 512), np.arange(512), np.zeros(512, int)], 1).astype(np.int32)
    rows = np.concatenate([rows512, rows512[:3]])
    counts = np.array([512, 0, 3], np.int32)
    pl = V.PrimList()
    for i in range(1500):
        k = i % 4
        px, py = 64 + int(rng.integers(0, 50)), 32 + int(rng.integers(0, 25))
        color = (i & 255, (i >> 8) & 255, (i * 7) & 255)
        if k == 0:
            pl.fill(px, py, px + int(rng.integers(0, 12)), py + int(rng.integers(0, 8)), color)
        elif k == 1:
            pl.outline(px, py, px + int(rng.integers(0, 12)), py + int(rng.integers(0, 8)), color)
        elif k == 2:
            pl.put_text(px, py, "ab"[i % 2], 1, color)
        else:
            pl.segment(px, py, px + int(rng.integers(-9, 10)), py + int(rng.integers(-9, 10)), 1 + i % 8, color)
    prims = [None, pl, pl]
    r = R.Renderer(redact="box", style="mosaic", cell=4)
    got = r.render(fr.copy(), rows, counts, prims)
    r.close()
    assert np.array_equal(got, oracle_call(fr, rows, counts, prims, redact="box", style="mosaic", cell=4))


@pytest.mark.gpu
def test_device_tensor_overlay_equivalence_and_nothing_to_draw(R):
    V = pkg("visualization")
    shape = (3, 70, 131)
    F, H, W = shape
    fr = frames_of(shape, 8)
    rows, counts = rows_for(F, H, W, 9)
    prims = prims_for(F, H, W)
    r = R.Renderer(redact="head", style="mosaic", cell=16, head_q8=128)
    host = r.render(fr.copy(), rows, counts, prims)
    dev = torch.from_numpy(fr.copy()).cuda()
    assert r.render(dev, rows, counts, prims) is dev
    assert np.array_equal(dev.cpu().numpy(), host)
    # an odd base address on the dword-capable width: the byte path must give the same
    shape2 = (2, 64, 128)
    fr2 = frames_of(shape2, 10)
    rows2, counts2 = rows_for(2, 64, 128, 11)
    exp2 = oracle_call(fr2, rows2, counts2, redact="head", style="mosaic", cell=16, head_q8=128)
    buf = torch.zeros(fr2.size + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + fr2.size].view(2, 64, 128, 3)
    view.copy_(torch.from_numpy(fr2).cuda())
    r.render(view, rows2, counts2)
    assert np.array_equal(view.cpu().numpy(), exp2) and int(buf[0]) == 0 and int(buf[1 + fr2.size:].sum()) == 0
    r.close()
    # redact off, no masks, kinds 0..2: every frame equals the existing overlay kernel on that frame
    r = R.Renderer()
    lists = []
    for f in range(F):
        pl = V.PrimList()
        V.track_prims(pl, [(10 + 9 * f, 20, 80, 60, 3, "person", 0.91), (60, 5, 125, 40, 12, "car")])
        V.info_prims(pl, ["AICamera", f"frame {f}"])
        lists.append(pl)
    got = r.render(fr.copy(), prims=lists)
    for f in range(F):
        assert np.array_equal(got[f], V.render(fr[f].copy(), lists[f]))
    # nothing to draw: the array stays equal to its copy
    same = r.render(fr.copy())
    assert np.array_equal(same, fr)
    same = r.render(fr.copy(), np.zeros((0, 6), np.int32), np.zeros(F, np.int32), [V.PrimList() for _ in range(F)])
    assert np.array_equal(same, fr)
    r.close()


@pytest.mark.gpu
def test_offsets_past_2_31_bytes(R):
    """3 frames of 16384 x 16384 on the device are 2.4 GB: the last frame lies past 2^31 bytes and its last tile row past 2^31 + 2^29.  No
    oracle at this size: zero frames, a fill rectangle in the last frame's corner, a segment and a one-pixel box in its first rows."""
    V = pkg("visualization")
    n = 16384
    t = torch.zeros((3, n, n, 3), dtype=torch.uint8, device="cuda")
    rows = np.array([(n - 100, n - 40, n + 5, n + 5, 1, 0), (7, 0, 7, 0, 2, 0)], np.int32)
    pl = V.PrimList()
    pl.segment(64, 2, 191, 2, 1, (1, 2, 3))
    r = R.Renderer(redact="box", style="fill", fill_color=(11, 12, 13))
    r.render(t, rows, np.array([0, 0, 2], np.int32), [None, None, pl])
    r.close()
    assert int(torch.count_nonzero(t[:2])) == 0
    last = t[2]
    assert int(torch.count_nonzero(last)) == (100 * 40 + 1 + 128) * 3
    assert last[n - 40:, n - 100:].reshape(-1, 3).unique(dim=0).tolist() == [[11, 12, 13]]
    assert last[0, 7].tolist() == [11, 12, 13] and last[2, 64:192].reshape(-1, 3).unique(dim=0).tolist() == [[1, 2, 3]]
