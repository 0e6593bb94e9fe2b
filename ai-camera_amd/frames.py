"""Pixel formats at the edges of the pipeline (aic_frames_to_bgr / aic_frames_from_bgr): decoders and cameras
deliver 4:2:0 YUV (NV12, sometimes I420) on pitched surfaces and encoders want NV12 back; everything in between reads packed BGR24.
The conversion is a HIP kernel over the whole bank of frames; tests/yuv_oracle.py is its specification, bit for bit.

A tightly packed bank of n frames is uint8 [n, H*3/2, W]: H rows of luma, then H/2 rows of chroma (NV12: U,V interleaved; I420: the U
plane's H/2 rows of W/2 bytes, then the V plane's, which together fill the same H/2 rows of W bytes)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

FORMATS = {"bgr24": L.PIX_BGR24, "nv12": L.PIX_NV12, "i420": L.PIX_I420}
MATRICES = {"bt601": L.YUV_BT601, "bt709": L.YUV_BT709}
RANGES = {"limited": L.YUV_LIMITED, "full": L.YUV_FULL}


def _code(table, what, v):
    if isinstance(v, str) and v.lower() in table:
        return table[v.lower()]
    if not isinstance(v, str) and int(v) in table.values():
        return int(v)
    raise ValueError(f"{what} must be one of {sorted(table)}, not {v!r}")


def format_code(fmt):
    return _code(FORMATS, "pixel format", fmt)


def matrix_code(matrix):
    return _code(MATRICES, "yuv matrix", matrix)


def range_code(range):          # noqa: A002 -- the keyword the callers use
    return _code(RANGES, "yuv range", range)


def frame_bytes(fmt, h, w):
    """Bytes of one tightly packed h x w frame."""
    return int(h) * int(w) * 3 if format_code(fmt) == L.PIX_BGR24 else int(h) * int(w) * 3 // 2


def coeffs(matrix="bt601", range="limited"):          # noqa: A002
    """(dec int32 [5] = cy cvr cvg cug cub, enc int32 [9] = yr yg yb ur ug ub vr vg vb, y_offset): the 2^20-scaled integer coefficients."""
    dec, enc, yo = np.zeros(5, np.int32), np.zeros(9, np.int32), C.c_int32()
    L.call("aic_yuv_coeffs", matrix_code(matrix), range_code(range), L.ptr(dec), L.ptr(enc), C.byref(yo))
    return dec, enc, yo.value


def _bank_bytes(n, h, pitch, frame_stride):
    return 0 if n == 0 else (n - 1) * frame_stride + pitch * h * 3 // 2


def to_bgr(frames, fmt, hw=None, pitch=0, matrix="bt601", range="limited", frame_stride=0, device=0):          # noqa: A002
    """4:2:0 frames -> BGR uint8 [n, H, W, 3].  frames: uint8 [n, H*3/2, W] (or one frame [H*3/2, W]) when tightly packed -- hw may then be
    omitted -- or any C-contiguous uint8 buffer holding n pitched frames, with hw = (H, W), pitch and frame_stride (0 = tight) given."""
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    if hw is None:
        if f.ndim == 2:
            f = f[None]
        if f.ndim != 3 or f.shape[1] % 3 or pitch or frame_stride:
            raise ValueError("without hw the frames are uint8 [n, H*3/2, W], tightly packed")
        hw = (f.shape[1] * 2 // 3, f.shape[2])
    h, w = int(hw[0]), int(hw[1])
    if h <= 0 or w <= 0 or pitch < 0 or frame_stride < 0:
        raise ValueError("hw must be positive, pitch and frame_stride not negative")
    p = int(pitch) or w
    last = p * h * 3 // 2                                   # the last frame needs no stride tail
    fs = int(frame_stride) or last
    if f.size == 0:
        n = 0
    elif f.size >= last and (f.size - last) % fs == 0:
        n = (f.size - last) // fs + 1
    elif f.size % fs == 0:
        n = f.size // fs
    else:
        raise ValueError(f"{f.size} bytes are no whole number of {h}x{w} frames of pitch {p} and stride {fs}")
    out = np.empty((n, h, w, 3), np.uint8)
    L.call("aic_frames_to_bgr", int(device), L.ptr(f), n, h, w, format_code(fmt), int(pitch), int(frame_stride), matrix_code(matrix),
           range_code(range), L.HOST, L.ptr(out))
    return out


def from_bgr(frames_bgr, fmt, pitch=0, matrix="bt601", range="limited", frame_stride=0, out=None, device=0):          # noqa: A002
    """BGR uint8 [n, H, W, 3] (or one frame) -> 4:2:0 frames.  Tightly packed (pitch = frame_stride = 0, out None): uint8 [n, H*3/2, W].
    Otherwise a flat uint8 buffer of (n - 1) * frame_stride + pitch * H * 3 / 2 bytes -- `out` when given, whose bytes outside W (pitch
    padding, stride tails) keep their contents, else a new zero-filled one."""
    f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
    if f.ndim == 3:
        f = f[None]
    if f.ndim != 4 or f.shape[3] != 3:
        raise ValueError("frames_bgr must be uint8 [n, H, W, 3]")
    n, h, w = f.shape[:3]
    tight = not pitch and not frame_stride and out is None
    p = int(pitch) or w
    fs = int(frame_stride) or p * h * 3 // 2
    need = _bank_bytes(n, h, p, fs)
    if out is None:
        out = np.zeros(need, np.uint8)
    elif out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"] or out.size < need:
        raise ValueError(f"out must be a C-contiguous uint8 buffer of at least {need} bytes")
    L.call("aic_frames_from_bgr", int(device), L.ptr(f), n, h, w, format_code(fmt), int(pitch), int(frame_stride), matrix_code(matrix),
           range_code(range), L.HOST, L.ptr(out))
    return out.reshape(n, h * 3 // 2, w) if tight else out
