"""JPEG in: a bank of JPEG files of one picture size to [n, H, W, 3] BGR24 in one call (aic_jpegdec_*, csrc/jpegdec.hpp,
csrc/kernels_jpegdec.hip).  Baseline sequential DCT, gray or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, any tables, any restart
interval.  Integer arithmetic only; tests/jpegdec_oracle.py is the specification and the device's pixels equal it byte for byte.  A file
the decoder does not accept is refused alone: status ERR_FORMAT, a reason from REASONS, its output slot untouched."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from . import _lib as L
from . import config

REASONS = ("OK", "TRUNCATED", "NOT_JPEG", "NOT_BASELINE", "PRECISION", "COMPONENTS", "SAMPLING", "SIZE_MISMATCH", "BAD_TABLE", "MISSING_TABLE",
           "BAD_SCAN", "RESTART_SEQUENCE", "BAD_CODE", "OVERRUN")
INFO_FIELDS = ("status", "reason", "width", "height", "components", "sampling", "restart", "intervals", "entropy_offset", "entropy_bytes")


def probe(file):
    """dict(status, reason, width, height, components, sampling, restart, intervals, entropy_offset, entropy_bytes) of one file's header.
    Host only."""
    a = np.frombuffer(bytes(file), np.uint8)
    info = L.JpegdecInfo()
    L.call("aic_jpegdec_probe", L.ptr(a) if a.size else None, a.size, C.byref(info))
    return {k: int(getattr(info, k)) for k in INFO_FIELDS}


def pack(files):
    """(buffer uint8, offsets int64 [n + 1]) of a list of bytes objects, back to back."""
    offsets = np.zeros(len(files) + 1, np.int64)
    if len(files):
        np.cumsum([len(f) for f in files], out=offsets[1:])
    return np.frombuffer(b"".join(bytes(f) for f in files), np.uint8), offsets


def split_mjpeg(path):
    """(buffer uint8, offsets int64 [frames + 1]) of a Motion-JPEG file: JFIF files back to back.  The offsets come from the .json side
    file the CLI writes when it is there, else from walking SOI .. EOI on the host (marker segments are skipped by their length, entropy
    data is searched for the next marker that is neither stuffing nor RSTm)."""
    path = str(path)
    buf = np.fromfile(path, np.uint8)
    side = path + ".json"
    if os.path.exists(side):
        off = np.asarray(json.load(open(side)).get("offsets", []), np.int64)
        if off.size >= 1 and off[0] == 0 and off[-1] == buf.size and (np.diff(off) >= 0).all():
            return buf, off
    data, n, pos, offsets = buf.tobytes(), int(buf.size), 0, [0]
    while pos + 2 <= n and data[pos] == 0xFF and data[pos + 1] == 0xD8:
        p, end = pos + 2, -1
        while p + 2 <= n:                                                      # the segments up to SOS
            if data[p] != 0xFF:
                break
            m = data[p + 1]
            if m == 0xFF:
                p += 1
            elif m == 0x01 or 0xD0 <= m <= 0xD7:
                p += 2
            elif m == 0xD9:
                end = p + 2
                break
            elif m == 0xD8:                                                    # the next file starts before this one ended: a torn file of its own
                end = p
                break
            else:
                if p + 4 > n:
                    break
                p += 2 + ((data[p + 2] << 8) | data[p + 3])
                if m == 0xDA:                                                  # entropy data: on to the next real marker
                    while True:
                        p = data.find(b"\xff", p)
                        if p < 0 or p + 1 >= n:
                            p = n
                            break
                        if data[p + 1] == 0 or 0xD0 <= data[p + 1] <= 0xD7:
                            p += 2
                        elif data[p + 1] == 0xFF:
                            p += 1
                        else:
                            break
        if end < 0:
            break
        offsets.append(end)
        pos = end
    if offsets[-1] != n:                                                       # what is left is one more (truncated) file: the decoder names why
        offsets.append(n)
    return buf, np.asarray(offsets, np.int64)


class JpegDecoder:
    """JpegDecoder(height, width, max_images=16, device=0): every file of every call holds a picture of that size.  The device is first
    touched by decode."""

    def __init__(self, height, width, max_images=16, device=0):
        self.height, self.width, self.max_images = int(height), int(width), int(max_images)
        cfg = L.JpegdecConfig(self.max_images, self.height, self.width)
        self._h = C.c_void_p()
        L.call("aic_jpegdec_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_jpegdec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"launch_budget_mb": a bank is cut into launches below it (same bytes)."""
        L.call("aic_jpegdec_option", self._h, str(key).encode(), int(value))

    def counters(self):
        """dict(images, refused, bytes_in, bytes_out) since creation."""
        v = [C.c_int64() for _ in range(4)]
        L.call("aic_jpegdec_counters", self._h, *(C.byref(x) for x in v))
        return dict(images=v[0].value, refused=v[1].value, bytes_in=v[2].value, bytes_out=v[3].value)

    def _bank(self, buffer, offsets):
        """(pointer, AIC_HOST / AIC_DEVICE, offsets int64, n, keep-alive) of packed files: a uint8 NumPy array or a contiguous tensor."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("offsets must be [n + 1]")
        n = off.size - 1
        if n > self.max_images:
            raise ValueError(f"{n} images, max_images is {self.max_images}")
        if isinstance(buffer, np.ndarray):
            if buffer.dtype != np.uint8 or buffer.ndim != 1:
                raise ValueError("buffer must be a uint8 vector")
            a = np.ascontiguousarray(buffer)
            size, ptr, mem, keep = a.size, (L.ptr(a) if a.size else None), L.HOST, a
        else:
            if str(buffer.dtype) != "torch.uint8" or buffer.dim() != 1 or not buffer.is_contiguous():
                raise ValueError("buffer must be a contiguous uint8 vector")
            if buffer.is_cuda:
                import torch
                torch.cuda.current_stream(buffer.device).synchronize()        # the library reads it on its own stream
            size, ptr, mem, keep = buffer.numel(), C.c_void_p(buffer.data_ptr()), L.DEVICE if buffer.is_cuda else L.HOST, buffer
        if n and (off[0] < 0 or off[-1] > size):
            raise ValueError("offsets beyond the buffer")
        return ptr, mem, off, n, keep

    def decode_packed(self, buffer, offsets, out=None):
        """(bgr [n, H, W, 3] uint8, status [n] int32, reason [n] int32): file i is buffer[offsets[i]:offsets[i + 1]], in host memory (a
        NumPy array) or device memory (a tensor).  out: a uint8 NumPy array or device tensor of that shape to decode into (a refused
        image's slot is not written); without it a zeroed NumPy array."""
        ptr, mem, off, n, keep = self._bank(buffer, offsets)
        shape = (n, self.height, self.width, 3)
        status, reason = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if out is None:
            out = np.zeros(shape, np.uint8)
        if tuple(out.shape) != shape:
            raise ValueError(f"out of shape {tuple(out.shape)}, not {shape}")
        if isinstance(out, np.ndarray):
            if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]:
                raise ValueError("out must be a contiguous uint8 array")
            o_ptr, o_mem = L.ptr(out), L.HOST
        else:
            if str(out.dtype) != "torch.uint8" or not out.is_contiguous():
                raise ValueError("out must be a contiguous uint8 tensor")
            o_ptr, o_mem = C.c_void_p(out.data_ptr()), L.DEVICE if out.is_cuda else L.HOST
            if out.is_cuda:
                import torch
                torch.cuda.current_stream(out.device).synchronize()           # the library writes it on its own stream
        L.call("aic_jpegdec_decode", self._h, ptr, mem, L.ptr(off), n, o_ptr if n else None, o_mem, L.ptr(status), L.ptr(reason))
        return out, status, reason

    def decode(self, files):
        """(bgr [n, H, W, 3] uint8, status, reason) of a list of bytes objects; a refused image's frame is zero."""
        return self.decode_packed(*pack(files))

    def coefficients(self, buffer, offsets, image):
        """The quantised coefficients of one image of a bank, int16 [MCUs, blocks per MCU, 64] in natural order (debugging)."""
        ptr, mem, off, n, keep = self._bank(buffer, offsets)
        if not 0 <= int(image) < n:
            raise ValueError("image outside the bank")
        a = buffer[int(off[image]):int(off[image + 1])]
        info = probe(a.cpu().numpy() if not isinstance(a, np.ndarray) else a)
        if info["status"]:
            raise L.AicError(L.ERR_FORMAT, "the image is refused: " + REASONS[info["reason"]])
        hs, vs = {400: (1, 1), 444: (1, 1), 422: (2, 1), 420: (2, 2)}[info["sampling"]]
        bpm = 1 if info["components"] == 1 else hs * vs + 2
        out = np.zeros((-(-info["width"] // (8 * hs)) * -(-info["height"] // (8 * vs)), bpm, 64), np.int16)
        L.call("aic_jpegdec_coefficients", self._h, ptr, mem, L.ptr(off), n, int(image), L.ptr(out))
        return out
