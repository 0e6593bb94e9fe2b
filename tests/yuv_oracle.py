"""The 4:2:0 YUV <-> BGR24 specification of aic_frames_to_bgr / aic_frames_from_bgr and of the pipeline's unpack stage (DESIGN.md
section 33), in NumPy, integers only.  The device must equal it bit for bit in both directions.

Formats: NV12 = Y plane of h rows of `pitch` bytes, then h/2 rows of `pitch` bytes of interleaved U,V; I420 = Y plane h x pitch, then a U
plane of h/2 rows of pitch/2 bytes, then a V plane of the same shape.  pitch = 0 and frame_stride = 0 mean tight.

The coefficients are the standards' exact fractions (BT.601: Kr 0.299, Kb 0.114; BT.709: Kr 0.2126, Kb 0.0722; limited range: luma
offset 16, luma span 219, chroma span 224; full range: 0, 255, 255) times 2^20, rounded half away from zero.  All arithmetic is int32,
`>>` is the arithmetic (floor) shift, chroma is replicated on decode and taken from the 2x2 block's sums on encode."""
from fractions import Fraction

import numpy as np

BGR24, NV12, I420 = 0, 1, 2
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
SHIFT = 20
MAX_SIDE = 16384

_K = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}
_RANGE = {LIMITED: (16, 219, 224), FULL: (0, 255, 255)}


def _round_half_away(q):
    n = (abs(q) * 2 + 1) // 2                      # floor(|q| + 1/2): exact on Fractions
    return int(n) if q >= 0 else -int(n)


def derive(matrix, rng):
    """(dec[5] = cy cvr cvg cug cub, enc[9] = yr yg yb ur ug ub vr vg vb, y_offset) from the constants above, as exact fractions."""
    kr, kb = _K[matrix]
    kg = 1 - kr - kb
    yo, ys, cs = _RANGE[rng]
    one = 1 << SHIFT
    sy, sc = Fraction(255, ys), Fraction(255, cs)
    dec = [sy, 2 * (1 - kr) * sc, -2 * (1 - kr) * kr / kg * sc, -2 * (1 - kb) * kb / kg * sc, 2 * (1 - kb) * sc]
    ey, ec = Fraction(ys, 255), Fraction(cs, 255)
    enc = [kr * ey, kg * ey, kb * ey,
           -kr / (2 * (1 - kb)) * ec, -kg / (2 * (1 - kb)) * ec, Fraction(1, 2) * ec,
           Fraction(1, 2) * ec, -kg / (2 * (1 - kr)) * ec, -kb / (2 * (1 - kr)) * ec]
    return [_round_half_away(c * one) for c in dec], [_round_half_away(c * one) for c in enc], yo


# (matrix, range) -> (dec, enc): the literals csrc/yuv.hpp carries; tests/test_yuv_oracle.py checks derive() against them
TABLES = {
    (BT601, LIMITED): ((1220945, 1673555, -852458, -410793, 2115221),
                       (269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897)),
    (BT601, FULL): ((1048576, 1470104, -748826, -360853, 1858077),
                    (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262)),
    (BT709, LIMITED): ((1220945, 1879825, -558796, -223607, 2215014),
                       (191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230)),
    (BT709, FULL): ((1048576, 1651297, -490864, -196424, 1945738),
                    (222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074)),
}
SETS = tuple(TABLES)


def coeffs(matrix=BT601, rng=LIMITED):
    dec, enc = TABLES[(matrix, rng)]
    return list(dec), list(enc), _RANGE[rng][0]


def _fits(*terms):
    """Every term and every partial sum stays below 2^31 in magnitude (the device computes in int32)."""
    acc = np.zeros_like(np.asarray(terms[0], np.int64))
    for t in terms:
        t = np.asarray(t, np.int64)
        assert (np.abs(t) < 2 ** 31).all(), "int32 overflow in a product"
        acc = acc + t
        assert (np.abs(acc) < 2 ** 31).all(), "int32 overflow in a sum"
    return acc.astype(np.int32)


def _clamp8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def decode_pixels(y, u, v, matrix=BT601, rng=LIMITED):
    """y, u, v: integer arrays of one shape (chroma already replicated) -> (r, g, b) uint8."""
    (cy, cvr, cvg, cug, cub), _, yo = coeffs(matrix, rng)
    c, d, e = np.asarray(y, np.int64) - yo, np.asarray(u, np.int64) - 128, np.asarray(v, np.int64) - 128
    half = 1 << (SHIFT - 1)
    r = _fits(cy * c, cvr * e, half) >> SHIFT
    g = _fits(cy * c, cvg * e, cug * d, half) >> SHIFT
    b = _fits(cy * c, cub * d, half) >> SHIFT
    return _clamp8(r), _clamp8(g), _clamp8(b)


def encode_luma(r, g, b, matrix=BT601, rng=LIMITED):
    _, (yr, yg, yb, *_), yo = coeffs(matrix, rng)
    r, g, b = (np.asarray(a, np.int64) for a in (r, g, b))
    return _clamp8(_fits(yr * r, yg * g, yb * b, yo << SHIFT, 1 << (SHIFT - 1)) >> SHIFT)


def encode_chroma(rs, gs, bs, matrix=BT601, rng=LIMITED):
    """rs, gs, bs: the sums over a 2x2 block (0..1020) -> (u, v) uint8."""
    _, (_, _, _, ur, ug, ub, vr, vg, vb), _ = coeffs(matrix, rng)
    rs, gs, bs = (np.asarray(a, np.int64) for a in (rs, gs, bs))
    bias, half = 128 << (SHIFT + 2), 1 << (SHIFT + 1)
    u = _fits(ur * rs, ug * gs, ub * bs, bias, half) >> (SHIFT + 2)
    v = _fits(vr * rs, vg * gs, vb * bs, bias, half) >> (SHIFT + 2)
    return _clamp8(u), _clamp8(v)


def check_layout(fmt, h, w, pitch=0, frame_stride=0):
    """-> (pitch, frame_stride) with the zeros resolved; ValueError on what aic_frames_to_bgr rejects."""
    if fmt not in (NV12, I420):
        raise ValueError("format must be NV12 or I420")
    if not (2 <= h <= MAX_SIDE and 2 <= w <= MAX_SIDE and h % 2 == 0 and w % 2 == 0):
        raise ValueError("h and w must be even and in 2..16384")
    pitch = pitch or w
    if pitch < w or (fmt == I420 and pitch % 2):
        raise ValueError("pitch must be >= w (and even for I420)")
    fb = pitch * h * 3 // 2
    frame_stride = frame_stride or fb
    if frame_stride < fb:
        raise ValueError("frame_stride is shorter than a frame")
    return pitch, frame_stride


def frame_bytes(fmt, h, w):
    return h * w * 3 if fmt == BGR24 else h * w * 3 // 2


def buffer_bytes(fmt, n, h, w, pitch=0, frame_stride=0):
    """Bytes the calls read / write for n frames: whole strides but for the last frame."""
    pitch, frame_stride = check_layout(fmt, h, w, pitch, frame_stride)
    return 0 if n == 0 else (n - 1) * frame_stride + pitch * h * 3 // 2


def _planes(buf, fmt, n, h, w, pitch, frame_stride):
    """Views (y [n,h,w], u [n,h/2,w/2], v [n,h/2,w/2]) into the flat uint8 buffer."""
    from numpy.lib.stride_tricks import as_strided
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags["C_CONTIGUOUS"] and len(buf) >= buffer_bytes(fmt, n, h, w, pitch, frame_stride)
    y = as_strided(buf, (n, h, w), (frame_stride, pitch, 1))
    c0 = buf[pitch * h:]
    if fmt == NV12:
        u = as_strided(c0, (n, h // 2, w // 2), (frame_stride, pitch, 2))
        v = as_strided(c0[1:], (n, h // 2, w // 2), (frame_stride, pitch, 2))
    else:
        u = as_strided(c0, (n, h // 2, w // 2), (frame_stride, pitch // 2, 1))
        v = as_strided(c0[(pitch // 2) * (h // 2):], (n, h // 2, w // 2), (frame_stride, pitch // 2, 1))
    return y, u, v


def decode(yuv, fmt=NV12, hw=None, pitch=0, frame_stride=0, matrix=BT601, rng=LIMITED, n=None):
    """yuv: uint8, either [n, h*3/2, w] (tight; hw may be None) or a flat buffer with hw (and n) given -> BGR uint8 [n, h, w, 3]."""
    yuv = np.ascontiguousarray(yuv, np.uint8)
    if hw is None:
        assert yuv.ndim == 3 and not pitch and not frame_stride
        n, h, w = len(yuv), yuv.shape[1] * 2 // 3, yuv.shape[2]
    else:
        h, w = hw
    pitch, frame_stride = check_layout(fmt, h, w, pitch, frame_stride)
    buf = yuv.reshape(-1)
    if n is None:
        n = (len(buf) + frame_stride - pitch * h * 3 // 2) // frame_stride
    y, u, v = _planes(buf, fmt, n, h, w, pitch, frame_stride)
    out = np.empty((n, h, w, 3), np.uint8)
    for f in range(n):                                         # frame by frame: int64 temporaries of one frame at a time
        uu, vv = (np.repeat(np.repeat(c[f], 2, 0), 2, 1) for c in (u, v))
        r, g, b = decode_pixels(y[f], uu, vv, matrix, rng)
        out[f, :, :, 0], out[f, :, :, 1], out[f, :, :, 2] = b, g, r
    return out


def encode(bgr, fmt=NV12, pitch=0, frame_stride=0, matrix=BT601, rng=LIMITED, out=None):
    """bgr uint8 [n, h, w, 3] -> uint8: [n, h*3/2, w] when tight and out is None, else the flat buffer `out` (or a zero-filled new one)
    with only the bytes inside w written."""
    bgr = np.asarray(bgr, np.uint8)
    assert bgr.ndim == 4 and bgr.shape[3] == 3
    n, h, w = bgr.shape[:3]
    tight = not pitch and not frame_stride and out is None
    pitch, frame_stride = check_layout(fmt, h, w, pitch, frame_stride)
    if out is None:
        out = np.zeros(buffer_bytes(fmt, n, h, w, pitch, frame_stride), np.uint8)
    y, u, v = _planes(out, fmt, n, h, w, pitch, frame_stride)
    for f in range(n):
        b, g, r = (bgr[f, :, :, k].astype(np.int64) for k in range(3))
        y[f] = encode_luma(r, g, b, matrix, rng)
        rs, gs, bs = (a.reshape(h // 2, 2, w // 2, 2).sum((1, 3)) for a in (r, g, b))
        u[f], v[f] = encode_chroma(rs, gs, bs, matrix, rng)
    return out.reshape(n, h * 3 // 2, w) if tight else out
