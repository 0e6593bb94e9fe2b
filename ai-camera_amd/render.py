"""Privacy redaction, static masks and annotation of a bank of frames in ONE launch (aic_render_*, csrc/render.hpp,
csrc/kernels_render.hip): the output stage after the path, banked like everything before it.  Tracked people
(or their heads) are pixelated or filled, fixed regions of a camera's view are blacked out, labels, the info panel, zones and lines are
drawn -- for the S frames of a tick in one call.  Tracker-agnostic: it takes the rows every tracker here delivers (x1 y1 x2 y2 id cls,
int32).  Pure integer arithmetic; tests/render_oracle.py is the specification."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from . import _lib as L
from . import config
from .zones import _int_points

MODES = {"off": 0, "box": 1, "head": 2}
STYLES = {"fill": 0, "mosaic": 1}
CELLS = (4, 8, 16, 32)
MAX_POLYS = MAX_VERTS = 32
MAX_ROWS, MAX_PRIMS = 512, 1500


def _color(c):
    b, g, r = (int(v) & 255 for v in c[:3])
    return b | g << 8 | r << 16


def check_masks(polygons, what=""):
    """Mask polygons as a list of int32 arrays [n_vert, 2], or ValueError: the limits of aic_render_set_masks."""
    if len(polygons) > MAX_POLYS:
        raise ValueError(what + "at most 32 mask polygons per camera")
    ps = [_int_points(p, what) for p in polygons]
    for p in ps:
        if not 3 <= len(p) <= MAX_VERTS:
            raise ValueError(what + "a mask polygon has 3..32 vertices")
    return ps


def load_masks_file(path_or_obj, n_cameras):
    """The CLI's --masks file: {"cameras": [{"masks": [[[x, y], ...], ...]}, ...]} -> `n_cameras` lists of integer polygons.  One entry
    serves every camera; otherwise the file names exactly n_cameras of them."""
    if isinstance(path_or_obj, (str, bytes)):
        with open(path_or_obj) as f:
            doc = json.load(f)
    else:
        doc = path_or_obj
    cams = doc.get("cameras") if isinstance(doc, dict) else None
    if not isinstance(cams, list) or not cams:
        raise ValueError('a masks file is {"cameras": [{"masks": [[[x, y], ...], ...]}, ...]} with at least one camera')
    if len(cams) == 1:
        cams = cams * int(n_cameras)
    if len(cams) != int(n_cameras):
        raise ValueError(f"the masks file names {len(cams)} cameras, the run has {n_cameras} (one entry would serve all)")
    out = []
    for i, cam in enumerate(cams):
        if not isinstance(cam, dict) or set(cam) - {"masks"}:
            raise ValueError(f"camera {i}: an object with \"masks\" only")
        out.append(check_masks(cam.get("masks", []), what=f"camera {i}: "))
    return out


def parse_style(spec):
    """"fill" or "mosaic:<cell>" (the CLI's --redact_style) -> (style, cell)."""
    if spec == "fill":
        return "fill", 16
    name, _, cell = str(spec).partition(":")
    if name != "mosaic" or (cell and not cell.isdigit()) or int(cell or 16) not in CELLS:
        raise ValueError("a redaction style is fill or mosaic:4, mosaic:8, mosaic:16 or mosaic:32")
    return "mosaic", int(cell or 16)


class Renderer:
    """Renderer(cameras=1, redact="off", style="mosaic", cell=16, fill_color=(0, 0, 0), pad=0, head_q8=64, classes=None,
    mask_color=(0, 0, 0), device=0).  redact: "off", "box" (the whole track box grown by pad) or "head" (its top head_q8 / 256);
    style: "mosaic" (cells of `cell` pixels anchored at the frame's origin) or "fill"; classes: None = every row, or the class ids (0..63)
    to redact -- a row of an unknown class is always redacted.  Colours are BGR.  The device is first touched by a render() that draws."""

    def __init__(self, cameras=1, redact="off", style="mosaic", cell=16, fill_color=(0, 0, 0), pad=0, head_q8=64, classes=None,
                 mask_color=(0, 0, 0), device=0):
        if redact not in MODES:
            raise ValueError("redact must be 'off', 'box' or 'head'")
        if style not in STYLES:
            raise ValueError("style must be 'mosaic' or 'fill'")
        self.cameras = int(cameras)
        self.n_masks = [0] * max(self.cameras, 0)
        self._h = C.c_void_p()
        L.call("aic_render_create", config.resolve_device(device), self.cameras, C.byref(self._h))
        try:
            for key, value in (("mode", MODES[redact]), ("style", STYLES[style]), ("cell", cell), ("fill_color", _color(fill_color)),
                               ("mask_color", _color(mask_color)), ("pad", pad), ("head_q8", head_q8)):
                self.option(key, value)
            self.set_classes(classes)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            L.load().aic_render_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def option(self, key, value):
        """"mode" 0 off / 1 box / 2 head (or the name), "style" 0 fill / 1 mosaic (or the name), "cell", "fill_color", "mask_color" (a BGR
        triple or B | G << 8 | R << 16), "pad", "head_q8", "class_mask", "class_all", "chunk_frames" (0 = a call's frames in one device
        buffer, k = at most k frames per upload / launch / download; same results)."""
        if key == "mode" and isinstance(value, str):
            value = MODES[value]
        if key == "style" and isinstance(value, str):
            value = STYLES[value]
        if key in ("fill_color", "mask_color") and not isinstance(value, (int, np.integer)):
            value = _color(value)
        L.call("aic_render_option", self._h, str(key).encode(), int(value))

    def set_classes(self, classes):
        if classes is None:
            return self.option("class_all", 1)
        mask = 0
        for c in classes:
            if not 0 <= int(c) <= 63:
                raise ValueError("class ids to redact are in 0..63")
            mask |= 1 << int(c)
        self.option("class_mask", mask - (1 << 64) if mask >> 63 else mask)

    def set_masks(self, camera, polygons=()):
        """The camera's static masks: polygons [[x, y], ...] of 3..32 integer-pixel vertices, painted mask_color on every frame of it."""
        ps = check_masks(list(polygons))
        nv = np.array([len(p) for p in ps], np.int32)
        xy = np.ascontiguousarray(np.concatenate(ps) if ps else np.zeros((0, 2), np.int32))
        L.call("aic_render_set_masks", self._h, int(camera), len(ps), L.ptr(nv) if ps else None, L.ptr(xy) if ps else None)
        self.n_masks[int(camera)] = len(ps)

    def rects(self, rows):
        """The redaction rectangles [m, 4] = x0 y0 x1 y1 (inclusive) a frame's rows give under the current options.  Host only."""
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 6)
        out = np.zeros((max(len(rows), 1), 4), np.int32)
        n = C.c_int(0)
        L.call("aic_render_rects", self._h, L.ptr(rows) if len(rows) else None, len(rows), L.ptr(out), C.byref(n))
        return out[:n.value]

    def render(self, frames, rows=None, counts=None, prims=None, cameras=None):
        """frames: uint8 [F, H, W, 3] BGR, a C-contiguous NumPy array (modified in place and returned) or a torch device tensor (rendered in
        place).  rows: int32 [n, 6] flat with counts [F]; prims: one visualization.PrimList (or None) per frame; cameras [F]: defaults to
        f % cameras, the tick-major order of the bank pipelines."""
        is_np = isinstance(frames, np.ndarray)
        if tuple(frames.shape[3:]) != (3,) or len(frames.shape) != 4:
            raise ValueError("frames must be [F, H, W, 3]")
        if is_np:
            if frames.dtype != np.uint8 or not frames.flags["C_CONTIGUOUS"] or not frames.flags["WRITEABLE"]:
                raise ValueError("host frames must be a writeable C-contiguous uint8 array")
            fptr, mem = L.ptr(frames), L.HOST
        else:
            if str(frames.dtype) != "torch.uint8" or not frames.is_contiguous():
                raise ValueError("device frames must be a contiguous uint8 tensor")
            if frames.is_cuda:
                import torch
                torch.cuda.current_stream(frames.device).synchronize()      # the frames are read on the library's own stream
            fptr, mem = C.c_void_p(frames.data_ptr()), L.DEVICE if frames.is_cuda else L.HOST
        F, H, W = (int(v) for v in frames.shape[:3])
        r6 = cnt = None
        if rows is not None or counts is not None:
            if rows is None or counts is None:
                raise ValueError("rows and counts come together")
            cnt = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
            r6 = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 6)
            if len(cnt) != F or int(cnt.sum()) != len(r6):
                raise ValueError("counts must name every frame and sum to len(rows)")
        pa = pc = None
        text = np.zeros(0, np.uint8)
        if prims is not None:
            if len(prims) != F:
                raise ValueError(f"{len(prims)} primitive lists for {F} frames")
            parts, texts, toff = [], [], 0
            pc = np.zeros(F, np.int32)
            for f, pl in enumerate(prims):
                if pl is None:
                    continue
                p, t = pl.arrays()
                pc[f] = len(p)
                if len(p):
                    p[p[:, 0] == 2, 6] += toff                 # text offsets index the call's one buffer
                    parts.append(p)
                texts.append(t)
                toff += len(t)
            pa = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 8), np.int32))
            text = np.ascontiguousarray(np.concatenate(texts) if texts else text)
        cam = None
        if cameras is not None:
            cam = np.ascontiguousarray(cameras, dtype=np.int32).reshape(-1)
            if len(cam) != F:
                raise ValueError("cameras must name every frame")
        L.call("aic_render_frames", self._h, fptr, F, H, W, mem, L.ptr(r6) if r6 is not None and len(r6) else None, L.ptr(cnt),
               L.ptr(pa) if pa is not None and len(pa) else None, L.ptr(pc), L.ptr(text) if len(text) else None, len(text), L.ptr(cam))
        return frames
