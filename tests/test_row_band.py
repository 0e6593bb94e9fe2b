"""The row-band planner (ai-camera_amd/csrc/row_band.cpp) on the CPU: built with the system g++ beside a test-only probe
(tests/row_band_probe.cpp), no hipcc, no GPU.

A letterboxed 16:9 frame carries the picture in rows [top, top + unpad_h) of the 640 x 640 input; the planner says which rows of every
op's output can depend on it.  The fp32 oracle (oracle/nets_oracle.EngineOracle) runs seeded YOLOv8n on two inputs that agree outside
the picture rows: every row in which an op's output differs must lie inside the planner's band of that op.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import pkg
from oracle import image_oracle as I, nets_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-camera_amd", "csrc")
OP_CONV, OP_SPPF_POOL = 1, 2

# (frame h, frame w): 16:9 (top 140), 4:3 (top 80), odd padding (top 139, bottom 140), portrait (borders left / right: "full")
GEOMETRIES = [(720, 1280), (960, 1280), (722, 1280), (1280, 720)]
# DESIGN: rows of ops 0 - 13 that depend on a 1280 x 720 frame
BANDS_720P = [(70, 250), (35, 125), (35, 125), (34, 126), (33, 127), (33, 127), (16, 64), (16, 64), (15, 65), (14, 66), (13, 67), (12, 68),
              (12, 68), (6, 34)]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the planner test builds row_band.cpp with the system compiler")
    so = str(tmp_path_factory.mktemp("row_band") / "librowband.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", os.path.join(CSRC, "row_band.cpp"),
                    os.path.join(ROOT, "tests", "row_band_probe.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def net():
    ef = pkg("engine_file")
    return N.EngineOracle(ef.serialize(ef.build_yolov8("n", calibrate=False)))


def iarr(v):
    a = np.ascontiguousarray(v, np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def planner_ops(eo):
    """The engine file's op list as the engine hands it to the planner (Model::plan_bands)."""
    rows = []
    for o in eo.ops:
        typ, sb, sc, cin, db, dc, cout, kh, kw, st, pad, act, rb, rc, rmode, wi = o[:16]
        conv = int(typ == OP_CONV and kh == kw and not eo.buffers[sb][3] and not eo.buffers[db][3])
        rows.append([conv, sb, sc, 8 if (typ == OP_CONV and cin == 3) else cin, db, dc, cout * (3 if typ == OP_SPPF_POOL else 1), kh, st, pad, rb if (typ == OP_CONV and rmode) else -1, rc])
    return rows


def bands_of(probe, eo, h, w):
    _, (unpad_h, unpad_w), _, (top, _, left, _) = I.letterbox_geometry(h, w, (eo.in_h, eo.in_w))
    ops, pops = iarr(planner_ops(eo))
    bh, pbh = iarr([b[0] for b in eo.buffers])
    out, pout = iarr(np.zeros((len(eo.ops), 3)))
    probe.probe_row_bands(len(eo.ops), pops, len(bh), pbh, int(top), int(unpad_h), int(left != 0 or unpad_w != eo.in_w), pout)
    return out, int(top), int(unpad_h)


@pytest.mark.parametrize("hw", GEOMETRIES, ids=lambda hw: f"{hw[1]}x{hw[0]}")
def test_rows_that_differ_lie_inside_the_band(probe, net, hw):
    eo = net
    bands, top, unpad_h = bands_of(probe, eo, *hw)
    g = torch.Generator().manual_seed(7)
    x = torch.full((2, 3, eo.in_h, eo.in_w), 114.0 / 255.0)
    _, (uh, uw), _, (t, _, left, _) = I.letterbox_geometry(hw[0], hw[1], (eo.in_h, eo.in_w))
    x[:, :, t:t + uh, left:left + uw] = torch.rand(2, 3, uh, uw, generator=g)          # two frames: same borders, other pictures

    # an op's output as it stood when the op had run: the final buffers, and for a slice a later op overwrites the list up to that op
    last = {}
    for i, o in enumerate(eo.ops):
        for j in [j for j, (b, c0, cn) in last.items() if b == o[4] and c0 < o[5] + o[6] and o[5] < c0 + cn]:
            last.pop(j)
        last[i] = (o[4], o[5], o[6] * (3 if o[0] == OP_SPPF_POOL else 1))
    all_ops = eo.ops
    final = eo.run(x)
    checked = 0
    for i, o in enumerate(all_ops):
        if o[0] != OP_CONV:
            continue
        if i in last:
            bufs = final
        else:
            eo.ops = all_ops[:i + 1]
            try:
                bufs = eo.run(x)
            finally:
                eo.ops = all_ops
        y = bufs[o[4]][:, o[5]:o[5] + o[6]]
        rows = torch.nonzero((y[0] != y[1]).any(0).any(1)).flatten().tolist()
        full, lo, hi = (int(v) for v in bands[i])
        if full:
            assert (lo, hi) == (0, y.shape[2] - 1), (i, lo, hi)
        assert all(lo <= r <= hi for r in rows), (i, (lo, hi), rows[:3], rows[-3:])
        checked += 1
    assert checked == sum(o[0] == OP_CONV for o in all_ops)
    if hw == (720, 1280):
        assert (top, unpad_h) == (140, 360)
        assert [(int(b[1]), int(b[2])) for b in bands[:14]] == BANDS_720P
        assert not bands[:14, 0].any()
        assert bands[19, 0] == 1 and bands[20:, 0].all()          # 6.c2f.cv2 would save 3 rows of 40: full, and every op behind it
    if hw == (1280, 720):
        assert bands[:, 0].all()                                  # portrait: out of scope


# ---------------------------------------------------------------------------------------------------------------------------------
def large_batch_steps(eo, exact_patch=True):
    """YOLOv8n's launches at 32 frames and more, as the engine plans them (Model::row_plan): the fused stem, 1.conv on the 16-channel
    kernel, 2.c2f as one kernel, 3.conv with 4.c2f.cv1 in its epilogue, the 4.c2f.m* convs on the patch kernel's 16 x 16 tiles,
    4.c2f.cv2 on the streaming 1x1; everything behind them without a window form."""
    ops = eo.ops
    steps, reads = [], []

    def add(first, n_ops, th, exact, halo=None):
        o, l = ops[first], ops[first + n_ops - 1]
        k, st, pad = o[7], o[9], o[10]
        lo, hi = halo if halo else (pad, k - 1 - pad)
        rd = [] if first == 0 else [[o[1], o[2], o[3], int(th == 0), st, lo, hi]]
        for q in ops[first:first + n_ops]:
            if q[0] == OP_CONV and q[14] and n_ops != 4:
                rd.append([q[12], q[13], q[6], int(th == 0), 1, 0, 0])
        steps.append([first + n_ops - 1, l[4], l[5], l[6] * (3 if l[0] == OP_SPPF_POOL else 1), eo.buffers[l[4]][0], th, int(exact), len(rd)])
        reads.extend(rd)

    add(0, 1, 8, False)
    add(1, 1, 8, False)
    add(2, 4, 8, False, halo=(2, 2))
    add(6, 2, 8, False)
    for i in (8, 9, 10, 11):
        add(i, 1, 16, exact_patch)
    add(12, 1, 1, True)
    for i in range(13, len(ops)):
        add(i, 1, 0, False)
    return steps, reads


def windows_of(probe, steps, reads, bands):
    s, ps = iarr(steps)
    r, pr = iarr(reads)
    b, pb = iarr(bands)
    out, pout = iarr(np.zeros((len(steps), 2)))
    probe.probe_row_windows(len(steps), ps, pr, len(bands), pb, pout)
    return out


def tile_window(probe, y0, rows, th, ho):
    out, pout = iarr([0, 0])
    probe.probe_tile_window(y0, rows, th, ho, pout)
    return int(out[0]), int(out[1])


def computed_rows(probe, step, win):
    _, _, _, _, ho, th, exact, _ = step
    y0, rows = int(win[0]), int(win[1])
    if rows == 0:
        return 0, ho - 1
    if exact:
        return y0, y0 + rows - 1
    org, tiles = tile_window(probe, y0, rows, th, ho)
    return org, min(org + tiles * th, ho) - 1


@pytest.mark.parametrize("hw", GEOMETRIES[:3], ids=lambda hw: f"{hw[1]}x{hw[0]}")
@pytest.mark.parametrize("exact_patch", [True, False], ids=["exact", "whole-tiles"])
def test_writers_of_a_shared_scratch_cover_their_readers(probe, net, hw, exact_patch):
    """The bottleneck scratch of a C2f with two bottlenecks has two writers (m0.cv1 and m1.cv1) and no persistent rows: each writer's
    window contains every row its reader reads for what the reader computes.  Every windowed launch covers its own band."""
    eo = net
    bands, _, _ = bands_of(probe, eo, *hw)
    steps, reads = large_batch_steps(eo, exact_patch)
    win = windows_of(probe, steps, reads, bands)
    shared = {}
    for si, s in enumerate(steps):
        shared.setdefault((s[1], s[2], s[3]), []).append(si)
    shared = {k: v for k, v in shared.items() if len(v) > 1}
    assert sorted(len(v) for v in shared.values()) == [2, 2], shared          # the 80 x 80 and the 40 x 40 level's scratch
    ri = np.cumsum([0] + [s[7] for s in steps])
    n_checked = 0
    for (buf, c0, cn), writers in shared.items():
        for wi, w in enumerate(writers):
            nxt = writers[wi + 1] if wi + 1 < len(writers) else len(steps)
            wlo, whi = computed_rows(probe, steps[w], win[w])
            if steps[w][6] and win[w][1]:                                     # exact: what it STORES
                wlo, whi = int(win[w][0]), int(win[w][0] + win[w][1] - 1)
            for r in range(w + 1, nxt):
                for rd in reads[ri[r]:ri[r + 1]]:
                    if rd[0] != buf or not (rd[1] < c0 + cn and c0 < rd[1] + rd[2]):
                        continue
                    a, b = computed_rows(probe, steps[r], win[r])
                    lo, hi = (0, steps[w][4] - 1) if rd[3] else (max(a * rd[4] - rd[5], 0), min(b * rd[4] + rd[6], steps[w][4] - 1))
                    assert wlo <= lo and hi <= whi, (hw, w, r, (wlo, whi), (lo, hi))
                    n_checked += 1
    assert n_checked == 4
    n_win = 0
    for si, s in enumerate(steps):
        full, lo, hi = (int(v) for v in bands[s[0]])
        a, b = computed_rows(probe, s, win[si])
        assert a <= lo and hi <= b, (si, (a, b), (lo, hi))
        n_win += int(win[si][1] > 0)
        if win[si][1]:
            assert s[5] > 0 and not full
    # the stem, 1.conv, 2.c2f, 3.conv + 4.c2f.cv1, 4.c2f.cv2 and the two bottlenecks' second convs always; their first convs where the
    # hull of their readers' rows still leaves a tile row out
    # (1280 x 960: the picture fills 75 % of the input; the 80 x 80 level's bottleneck convs need all five tile rows and run full)
    assert n_win >= (5 if hw == (960, 1280) else 7), win[:10]
    if exact_patch and hw == (720, 1280):
        assert [tuple(int(v) for v in w) for w in win[:10]] == [(70, 181), (35, 91), (33, 95), (16, 49), (13, 55), (14, 53), (11, 59), (12, 57),
                                                                 (12, 57), (0, 0)]


def test_tile_windows_stay_inside_the_map(probe):
    """Every tile height the kernels use: 8 (origin clamped so that the last tile ends inside the map), 16 with an unaligned origin."""
    for th, ho in ((8, 320), (8, 160), (8, 80), (16, 80), (16, 40), (1, 80)):
        full_tiles = -(-ho // th)
        assert tile_window(probe, 0, 0, th, ho) == (0, full_tiles)
        for y0 in range(ho):
            for rows in range(1, ho - y0 + 1):
                org, tiles = tile_window(probe, y0, rows, th, ho)
                assert 0 <= org <= y0 and 1 <= tiles <= full_tiles
                assert org + tiles * th >= y0 + rows                      # covers the window
                assert org + tiles * th <= max(ho, full_tiles * th)
                if ho % th == 0:
                    assert org + tiles * th <= ho                         # the last tile ends inside the map
                assert tiles == min(-(-rows // th), full_tiles)
                if org < y0:
                    assert org == max(0, ho - tiles * th)                 # moved only as far as the clamp needs
    assert tile_window(probe, 12, 57, 16, 80) == (12, 4)                  # 4.c2f.m1.cv2 at 1280 x 720: unaligned, 4 of 5 tile rows
    assert tile_window(probe, 70, 181, 8, 320) == (70, 23)                # the stem: 23 of 40
    assert tile_window(probe, 60, 20, 16, 80) == (48, 2)                  # clamped
