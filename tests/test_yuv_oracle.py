"""tests/yuv_oracle.py, the specification of the YUV <-> BGR conversions, checked against itself: the coefficient
tables against their derivation from the standards' constants, the range end points, gray, the int32 head room and the round trip."""
from fractions import Fraction

import numpy as np
import pytest

import yuv_oracle as Y

LITERALS = {
    (Y.BT601, Y.LIMITED): ([1220945, 1673555, -852458, -410793, 2115221], [269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897]),
    (Y.BT601, Y.FULL): ([1048576, 1470104, -748826, -360853, 1858077], [313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262]),
    (Y.BT709, Y.LIMITED): ([1220945, 1879825, -558796, -223607, 2215014], [191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230]),
    (Y.BT709, Y.FULL): ([1048576, 1651297, -490864, -196424, 1945738], [222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074]),
}
# the largest |decode(encode(rgb)) - rgb| over flat 2x2 blocks of the 64^3 lattice below, as the oracle itself produces it (measured with this
# file; limited range quantises 256 levels into 220 / 225, full range only rounds)
ROUND_TRIP_MAX = {(Y.BT601, Y.LIMITED): 2, (Y.BT601, Y.FULL): 1, (Y.BT709, Y.LIMITED): 2, (Y.BT709, Y.FULL): 1}


def test_tables_equal_the_literals_and_their_derivation():
    assert Y.SETS == tuple(LITERALS) and (Y.BGR24, Y.NV12, Y.I420) == (0, 1, 2)
    for key, (dec, enc) in LITERALS.items():
        d, e, yo = Y.coeffs(*key)
        assert (d, e, yo) == (dec, enc, 16 if key[1] == Y.LIMITED else 0), key
        assert Y.derive(*key) == (dec, enc, yo), key                         # Fractions -> * 2^20 -> half away from zero
    assert [Y._round_half_away(Fraction(n, 2)) for n in (1, -1, 3, -3, 2, -2, 0)] == [1, -1, 2, -2, 1, -1, 0]
    # an independent spot check of the derivation: BT.601 limited, V -> R is 2 * (1 - 0.299) * 255 / 224
    assert LITERALS[(Y.BT601, Y.LIMITED)][0][1] == round(2 * (1 - 0.299) * 255 / 224 * 2 ** 20)


@pytest.mark.parametrize("matrix", (Y.BT601, Y.BT709))
def test_limited_range_end_points(matrix):
    assert [int(c[0]) for c in Y.decode_pixels([16], [128], [128], matrix, Y.LIMITED)] == [0, 0, 0]
    assert [int(c[0]) for c in Y.decode_pixels([235], [128], [128], matrix, Y.LIMITED)] == [255, 255, 255]
    assert int(Y.encode_luma([0], [0], [0], matrix, Y.LIMITED)[0]) == 16 and int(Y.encode_luma([255], [255], [255], matrix, Y.LIMITED)[0]) == 235


@pytest.mark.parametrize("matrix", (Y.BT601, Y.BT709))
def test_full_range_gray_is_exact(matrix):
    g = np.arange(256)
    y = Y.encode_luma(g, g, g, matrix, Y.FULL)
    u, v = Y.encode_chroma(4 * g, 4 * g, 4 * g, matrix, Y.FULL)
    assert np.array_equal(y, g) and (u == 128).all() and (v == 128).all()
    for c in Y.decode_pixels(y, u, v, matrix, Y.FULL):
        assert np.array_equal(c, g)


@pytest.mark.parametrize("key", Y.SETS)
def test_no_int32_overflow_at_the_corners(key):
    """_fits asserts on every product and partial sum; the extremes of every input reach the largest magnitudes."""
    ext = np.array([0, 255])
    y, u, v = (a.ravel() for a in np.meshgrid(ext, ext, ext, indexing="ij"))
    Y.decode_pixels(y, u, v, *key)
    Y.encode_luma(y, u, v, *key)
    Y.encode_chroma(4 * y, 4 * u, 4 * v, *key)
    with pytest.raises(AssertionError):
        Y._fits(np.array([2 ** 30]), np.array([2 ** 30]))
    with pytest.raises(AssertionError):
        Y._fits(np.array([-2 ** 31]))


@pytest.mark.parametrize("key", Y.SETS)
def test_round_trip_on_the_rgb_lattice(key):
    lv = np.round(np.linspace(0, 255, 64)).astype(np.int64)                  # 64 levels, 0 and 255 among them
    r, g, b = (a.ravel() for a in np.meshgrid(lv, lv, lv, indexing="ij"))
    y = Y.encode_luma(r, g, b, *key)
    u, v = Y.encode_chroma(4 * r, 4 * g, 4 * b, *key)                        # a flat 2x2 block: the sums are four times the pixel
    back = Y.decode_pixels(y, u, v, *key)
    err = max(int(np.abs(c.astype(np.int64) - a).max()) for c, a in zip(back, (r, g, b)))
    print("round trip", key, "max error", err)
    assert err == ROUND_TRIP_MAX[key], (key, err)


def test_frame_layouts_and_rejections():
    rng = np.random.default_rng(1)
    bgr = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    nv, i4 = Y.encode(bgr, Y.NV12), Y.encode(bgr, Y.I420)
    assert nv.shape == i4.shape == (2, 6, 6) and np.array_equal(nv[:, :4], i4[:, :4])
    uv = nv[:, 4:].reshape(2, 2, 3, 2)                                       # [n, chroma row, block, (U, V)]
    planes = i4[:, 4:].reshape(2, 2, 2, 3)                                   # [n, (U, V), chroma row, block]
    assert np.array_equal(uv[..., 0], planes[:, 0]) and np.array_equal(uv[..., 1], planes[:, 1])
    assert np.array_equal(Y.decode(nv, Y.NV12), Y.decode(i4, Y.I420))
    # the block's chroma comes from the sums of its four pixels; luma is per pixel
    b0 = bgr[0, :2, :2].astype(np.int64).reshape(4, 3).sum(0)
    u, v = Y.encode_chroma(b0[2], b0[1], b0[0])
    assert (int(u), int(v)) == (int(uv[0, 0, 0, 0]), int(uv[0, 0, 0, 1]))
    # pitched: only the bytes inside w are written, and decode reads the same pixels back
    out = np.full(Y.buffer_bytes(Y.I420, 2, 4, 6, 10, 80), 0xA5, np.uint8)
    assert out.size == 80 + 60 and Y.encode(bgr, Y.I420, 10, 80, out=out) is out
    assert (out == 0xA5).sum() >= out.size - 2 * 36 and np.array_equal(Y.decode(out, Y.I420, (4, 6), 10, 80, n=2), Y.decode(i4, Y.I420))
    assert (Y.frame_bytes(Y.BGR24, 4, 6), Y.frame_bytes(Y.NV12, 4, 6), Y.frame_bytes(Y.I420, 4, 6)) == (72, 36, 36)
    for bad in (dict(fmt=Y.BGR24), dict(h=3), dict(w=5), dict(h=0), dict(w=16386), dict(pitch=4), dict(fmt=Y.I420, pitch=7), dict(frame_stride=35)):
        a = dict(dict(fmt=Y.NV12, h=4, w=6, pitch=0, frame_stride=0), **bad)
        with pytest.raises(ValueError):
            Y.check_layout(**a)
    assert Y.check_layout(Y.NV12, 4, 6, 7, 0) == (7, 42)                      # an odd pitch is legal for NV12
