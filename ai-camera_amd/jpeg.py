"""JPEG out: a bank of equally sized BGR24 images to complete JFIF files in one call (aic_jpeg_*, csrc/jpeg.hpp,
csrc/kernels_jpeg.hip).  Baseline sequential DCT, 4:2:0 or 4:4:4, the Annex K Huffman tables, restart markers
always on.  Integer arithmetic only; tests/jpeg_oracle.py is the specification and the device's bytes equal it bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config

HEADER_BYTES = 629


def tables(quality):
    """(luma [64], chroma [64]) uint8 quantisation tables of a quality (1..100), natural order.  Host only."""
    luma, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    L.call("aic_jpeg_tables", int(quality), L.ptr(luma), L.ptr(chroma))
    return luma, chroma


def header(hw, quality=85, restart=0, subsampling="420"):
    """The 629 bytes every file of this configuration starts with.  Host only."""
    out, n = np.zeros(HEADER_BYTES, np.uint8), C.c_int()
    L.call("aic_jpeg_header", int(hw[0]), int(hw[1]), int(quality), int(restart), _subsampling(subsampling), L.ptr(out), out.size, C.byref(n))
    return out[:n.value].tobytes()


def _subsampling(s):
    if str(s) not in ("420", "444"):
        raise ValueError("subsampling must be '420' or '444'")
    return int(s)


def geometry(hw, restart=0, subsampling="420"):
    """dict(mcu, bpm, n_mcu, intervals, default_max_bytes, worst_case_bytes) of a configuration, as the library computes them."""
    sub, (h, w) = _subsampling(subsampling), (int(hw[0]), int(hw[1]))
    mcu, bpm = (16, 6) if sub == 420 else (8, 3)
    mx, my = -(-w // mcu), -(-h // mcu)
    intervals = -(-(mx * my) // (int(restart) or mx))
    return dict(mcu=mcu, bpm=bpm, n_mcu=mx * my, intervals=intervals, default_max_bytes=HEADER_BYTES + 3 * mx * my * mcu * mcu + 2 * intervals + 2,
                worst_case_bytes=HEADER_BYTES + 416 * bpm * mx * my + 2 * intervals + 2)


class JpegEncoder:
    """JpegEncoder(hw, max_images=16, quality=85, restart=0, subsampling="420", max_bytes=None, device=0).  hw = (height, width) of every
    image; restart = MCUs per restart interval, 0 = one MCU row; max_bytes = the largest file an image may take (None: 629 + 3 * the
    padded pixels + 2 * intervals + 2; "worst": what no image can exceed; an image beyond it is dropped alone).  The device is first
    touched by encode."""

    def __init__(self, hw, max_images=16, quality=85, restart=0, subsampling="420", max_bytes=None, device=0):
        self.height, self.width, self.max_images = int(hw[0]), int(hw[1]), int(max_images)
        self.quality, self.restart, self.subsampling = int(quality), int(restart), _subsampling(subsampling)
        if max_bytes == "worst":
            max_bytes = geometry(hw, self.restart, subsampling)["worst_case_bytes"]
        cfg = L.JpegConfig(self.max_images, self.height, self.width, self.quality, self.restart, self.subsampling,
                           0 if max_bytes is None else int(max_bytes))
        self._h = C.c_void_p()
        self._out = None                                          # the packed buffer of the last host call, reused while it is large enough
        L.call("aic_jpeg_create", config.resolve_device(device), C.byref(cfg), C.byref(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_jpeg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"quality" 1..100, "restart" 0..65535 (both legal between calls), "launch_budget_mb" (same bytes)."""
        L.call("aic_jpeg_option", self._h, str(key).encode(), int(value))
        if key in ("quality", "restart"):
            setattr(self, key, int(value))

    def header(self):
        return header((self.height, self.width), self.quality, self.restart, self.subsampling)

    def worst_case_bytes(self):
        v = C.c_int64()
        L.call("aic_jpeg_worst_case_bytes", self._h, C.byref(v))
        return v.value

    def counters(self):
        """dict(images, bytes_in, bytes_out) since creation."""
        v = [C.c_int64() for _ in range(3)]
        L.call("aic_jpeg_counters", self._h, *(C.byref(x) for x in v))
        return dict(images=v[0].value, bytes_in=v[1].value, bytes_out=v[2].value)

    def _frames(self, frames, device_frames):
        """(pointer, AIC_HOST / AIC_DEVICE, n, keep-alive) of uint8 [n, H, W, 3]: a NumPy array or a contiguous torch tensor."""
        shape = tuple(frames.shape)
        if len(shape) != 4 or shape[1:] != (self.height, self.width, 3):
            raise ValueError(f"frames of shape {shape}, not [n, {self.height}, {self.width}, 3]")
        if shape[0] > self.max_images:
            raise ValueError(f"{shape[0]} images, max_images is {self.max_images}")
        if isinstance(frames, np.ndarray):
            if device_frames:
                raise ValueError("device_frames needs a tensor on the device")
            if frames.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            a = np.ascontiguousarray(frames)
            return L.ptr(a), L.HOST, shape[0], a
        if str(frames.dtype) != "torch.uint8" or not frames.is_contiguous():
            raise ValueError("frames must be a contiguous uint8 tensor")
        if device_frames and not frames.is_cuda:
            raise ValueError("device_frames needs a tensor on the device")
        if frames.is_cuda:
            import torch
            torch.cuda.current_stream(frames.device).synchronize()    # the library reads it on its own stream
        return C.c_void_p(frames.data_ptr()), L.DEVICE if frames.is_cuda else L.HOST, shape[0], frames

    def encode_packed(self, frames, device_frames=False, out=None, out_cap=None):
        """(buffer, offsets [n + 1] int64, status [n] int32): file i is buffer[offsets[i]:offsets[i + 1]]; status 0, or ERR_CAPACITY with
        zero length for an image larger than max_bytes.  out: a uint8 NumPy array or a device tensor to pack into (out_cap: fewer bytes
        of it); a bank that does not fit raises AicError(ERR_CAPACITY) with .offsets set, and writes nothing.  Without out the call
        sizes its own host buffer (valid until the next call)."""
        f_ptr, f_mem, n, keep = self._frames(frames, device_frames)
        offsets, status = np.zeros(n + 1, np.int64), np.zeros(n, np.int32)
        lib = L.load()

        def run(o_ptr, o_mem, cap):
            return lib.aic_jpeg_encode(self._h, f_ptr if n else None, f_mem, n, o_ptr, o_mem, cap, L.ptr(offsets), L.ptr(status))

        if out is not None:
            if isinstance(out, np.ndarray):
                if out.dtype != np.uint8 or not out.flags["C_CONTIGUOUS"]:
                    raise ValueError("out must be a contiguous uint8 array")
                o_ptr, o_mem, size = L.ptr(out), L.HOST, out.size
            else:
                if str(out.dtype) != "torch.uint8" or not out.is_contiguous():
                    raise ValueError("out must be a contiguous uint8 tensor")
                o_ptr, o_mem, size = C.c_void_p(out.data_ptr()), L.DEVICE if out.is_cuda else L.HOST, out.numel()
                if out.is_cuda:
                    import torch
                    torch.cuda.current_stream(out.device).synchronize()   # the library writes it on its own stream
            cap = size if out_cap is None else int(out_cap)
            if cap > size:
                raise ValueError("out_cap beyond out")
            rc = run(o_ptr, o_mem, cap)
            if rc == L.ERR_CAPACITY:
                e = L.AicError(rc, lib.aic_last_error().decode("utf-8", "replace"))
                e.offsets, e.status = offsets, status
                raise e
            L.check(rc)
            return out, offsets, status
        guess = n * (HEADER_BYTES + self.height * self.width * 3 // 4 + 1024)
        if self._out is None or self._out.size < guess:
            self._out = np.empty(guess, np.uint8)
        rc = run(L.ptr(self._out), L.HOST, self._out.size)
        if rc == L.ERR_CAPACITY and offsets[n] > self._out.size:              # the sizes are known now: once more, with room
            self._out = np.empty(int(offsets[n]), np.uint8)
            rc = run(L.ptr(self._out), L.HOST, self._out.size)
        L.check(rc)
        return self._out, offsets, status

    def encode(self, frames, device_frames=False):
        """One bytes object per image, None for an image larger than max_bytes."""
        buf, off, status = self.encode_packed(frames, device_frames)
        return [None if status[i] else buf[off[i]:off[i + 1]].tobytes() for i in range(len(status))]

    def coefficients(self, frames, device_frames=False):
        """The quantised coefficients int16 [n, MCUs, blocks per MCU, 64] in zigzag order, as the entropy coder reads them (debugging)."""
        f_ptr, f_mem, n, keep = self._frames(frames, device_frames)
        g = geometry((self.height, self.width), self.restart, self.subsampling)
        out = np.zeros((n, g["n_mcu"], g["bpm"], 64), np.int16)
        L.call("aic_jpeg_coefficients", self._h, f_ptr if n else None, f_mem, n, L.ptr(out))
        return out
