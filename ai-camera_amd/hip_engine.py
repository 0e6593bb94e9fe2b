"""HipEngine: the drop-in for the reference's TRTEngine (src/trt_utils/trt_engine.py:15-216).

Same surface -- ``HipEngine(engine_path, device)``, ``infer(dict[name -> torch.Tensor]) ->
dict[name -> torch.Tensor]``, ``__call__`` requiring a dict, ``get_input_details()`` /
``get_output_details()`` returning ``TensorInfo(name, dtype, shape, is_dynamic)`` -- but the engine
file is this build's graph IR + weights and the execution is the hand-written HIP graph executor
behind the C ABI (aic_model_load, aic_yolo_infer, aic_reid_infer).  torch is used only as the
caller-visible tensor container (device memory + dtype), as in the reference.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from pathlib import Path
from typing import Dict, List, NamedTuple, Tuple

import numpy as np

from . import _lib as L
from . import config

TensorInfo = NamedTuple('TensorInfo', [('name', str), ('dtype', object), ('shape', Tuple[int, ...]), ('is_dynamic', bool)])


def _torch():
    import torch
    return torch


class HipEngine:
    #: knobs the reference fixes at trtexec time (scripts/export_trt_engines.sh:37) and inside the
    #: NMS plugin (unpinned); exposed as attributes here
    default_conf, default_iou, default_max_det = config.YOLO_CONF_THRESHOLD, config.YOLO_NMS_THRESHOLD, config.YOLO_MAX_DET

    def __init__(self, engine_path, device=None, dtype="fp16", max_items=None, warm_up=True):
        self.engine_path = Path(engine_path)
        if not self.engine_path.exists():                       # trt_engine.py:46-47
            raise FileNotFoundError(f"Engine file not found: {self.engine_path}")
        self.device_index = config.resolve_device(device)
        self.device = device
        self.dtype = L.F16 if str(dtype).lower() in ("fp16", "f16", "half", "1") else L.F32
        self._h = C.c_void_p()
        kind = self._peek_kind()
        if max_items is None:
            max_items = 8 if kind == L.MODEL_YOLO else 128
        self.max_items = int(max_items)
        L.call("aic_model_load", str(self.engine_path).encode(), self.device_index, self.dtype, self.max_items, C.byref(self._h))
        k, ih, iw, od, na, fl, ncv = (C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_int())
        L.call("aic_model_info", self._h, C.byref(k), C.byref(ih), C.byref(iw), C.byref(od), C.byref(na), C.byref(fl), C.byref(ncv))
        self.kind, self.in_h, self.in_w, self.out_dim = k.value, ih.value, iw.value, od.value
        self.n_anchors, self.flops_per_item, self.n_convs = na.value, fl.value, ncv.value
        self.conf_thresh, self.iou_thresh, self.max_det = self.default_conf, self.default_iou, self.default_max_det
        if self.kind == L.MODEL_YOLO:                       # an engine imported from an ONNX file with an embedded NMS plugin carries its thresholds
            from .engine_file import engine_nms_defaults
            nms = engine_nms_defaults(str(self.engine_path))
            if nms:
                self.conf_thresh, self.iou_thresh, self.max_det = nms[0], nms[1], min(nms[2], self.default_max_det)
        t = None
        try:
            t = _torch()
        except Exception:   # torch is optional for the C-ABI paths
            pass
        f32 = t.float32 if t else np.float32
        i32 = t.int32 if t else np.int32
        if self.kind == L.MODEL_YOLO:
            self.input_info_list = [TensorInfo("images", f32, (1, 3, self.in_h, self.in_w), False)]
            self.output_info_list = [TensorInfo("num_dets", i32, (1, 1), False),
                                     TensorInfo("bboxes", f32, (1, self.max_det, 4), False),
                                     TensorInfo("scores", f32, (1, self.max_det), False),
                                     TensorInfo("labels", i32, (1, self.max_det), False)]
        else:   # dynamic batch like the reference's ReID profile (export_trt_engines.sh:32-34)
            self.input_info_list = [TensorInfo("input", f32, (-1, 3, self.in_h, self.in_w), True)]
            self.output_info_list = [TensorInfo("output", f32, (-1, self.out_dim), True)]
        if warm_up:
            self._warm_up()

    def _peek_kind(self):
        with open(self.engine_path, "rb") as f:
            head = np.frombuffer(f.read(12), "<u4")
        if len(head) < 3 or head[0] != 0x57434941:
            raise RuntimeError(f"Failed to deserialize engine from {self.engine_path}")   # trt_engine.py:55-56
        return int(head[2])

    def close(self):
        if getattr(self, "_h", None):
            L.call("aic_model_destroy", self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- raw C-ABI level (NumPy in / NumPy out) ----------------------------------------------
    def yolo_infer_np(self, images_nchw, conf=None, iou=None, max_det=None):
        x = L.as_f32(images_nchw)
        b = x.shape[0]
        md = int(max_det or self.max_det)
        nd = np.zeros(b, np.int32)
        boxes, scores, labels = np.zeros((b, md, 4), np.float32), np.zeros((b, md), np.float32), np.zeros((b, md), np.int32)
        L.call("aic_yolo_infer", self._h, L.ptr(x), b, L.HOST, float(conf if conf is not None else self.conf_thresh),
               float(iou if iou is not None else self.iou_thresh), md, L.ptr(nd), L.ptr(boxes), L.ptr(scores), L.ptr(labels))
        return nd, boxes, scores, labels

    def yolo_head_np(self, images_nchw):
        x = L.as_f32(images_nchw)
        b = x.shape[0]
        dfl = np.zeros((b, self.n_anchors, 64), np.float32)
        cls = np.zeros((b, self.n_anchors, self.out_dim), np.float32)
        L.call("aic_yolo_head", self._h, L.ptr(x), b, L.HOST, L.ptr(dfl), L.ptr(cls))
        return dfl, cls

    def yolo_decode_np(self, images_nchw):
        x = L.as_f32(images_nchw)
        b = x.shape[0]
        boxes, ml = np.zeros((b, self.n_anchors, 4), np.float32), np.zeros((b, self.n_anchors), np.float32)
        lab = np.zeros((b, self.n_anchors), np.int32)
        L.call("aic_yolo_decode", self._h, L.ptr(x), b, L.HOST, L.ptr(boxes), L.ptr(ml), L.ptr(lab))
        return boxes, ml, lab

    def yolo_postprocess_np(self, dfl_logits, cls_logits, conf=None, iou=None, max_det=None, geom=None, sentinel=None):
        """decode + select + sort + NMS (+ un-letterbox) on head logits the caller supplies (aic_yolo_postprocess, include/aicam.h):
        no conv runs.  geom: None or (pad_w, pad_h, ratio, orig_w, orig_h).  sentinel: None, or (float value, int value) every output
        array is prefilled with -- an element that still holds it was not written.  Returns a dict of the nine output arrays."""
        dfl, cls = L.as_f32(dfl_logits), L.as_f32(cls_logits)
        with open(self.engine_path, "rb") as fh:
            reg_max = int(np.frombuffer(fh.read(68), "<i4")[10])          # meta[1] of the engine file's header
        b, a = cls.shape[0], self.n_anchors
        if dfl.shape != (b, a, 4 * reg_max) or cls.shape != (b, a, self.out_dim):
            raise ValueError(f"head logits {dfl.shape} / {cls.shape} do not fit an engine of {a} anchors, reg_max {reg_max}, {self.out_dim} classes")
        md = int(max_det or self.max_det)
        fs, is_ = sentinel if sentinel is not None else (0.0, 0)
        f = lambda *s: np.full(s, fs, np.float32)            # noqa: E731
        i = lambda *s: np.full(s, is_, np.int32)             # noqa: E731
        m = max(md, 1)
        r = dict(boxes=f(b, a, 4), max_logit=f(b, a), labels=i(b, a), n_cand=i(b), num_dets=i(b), out_boxes=f(b, m, 4),
                 out_boxes_orig=f(b, m, 4), out_scores=f(b, m), out_labels=i(b, m))
        g = geom if geom is not None else (0.0, 0.0, 1.0, 0, 0)
        L.call("aic_yolo_postprocess", self._h, L.ptr(dfl), L.ptr(cls), b, float(conf if conf is not None else self.conf_thresh),
               float(iou if iou is not None else self.iou_thresh), md, int(geom is not None), float(g[0]), float(g[1]), float(g[2]),
               int(g[3]), int(g[4]), *(L.ptr(r[k]) for k in ("boxes", "max_logit", "labels", "n_cand", "num_dets", "out_boxes",
                                                              "out_boxes_orig", "out_scores", "out_labels")))
        return r

    @staticmethod
    def det_filter_np(num_dets, boxes, scores, labels, min_conf, mask, cap, device=0, sentinel=None):
        """The pipeline's on-device detection filter on host arrays (aic_det_filter, include/aicam.h).  boxes [B, max_det, 4], scores /
        labels [B, max_det], mask: two 64-bit words, bit c = class c is tracked.  sentinel as in yolo_postprocess_np.  Returns a dict
        of rank, frame_n, frame_d0, total and the compact xyxy, tlwh, conf, cls, frame_of."""
        nd = np.ascontiguousarray(num_dets, np.int32)
        bx, sc, lb = L.as_f32(boxes), L.as_f32(scores), np.ascontiguousarray(labels, np.int32)
        b, md = sc.shape
        if nd.shape != (b,) or bx.shape != (b, md, 4) or lb.shape != (b, md):
            raise ValueError(f"det_filter_np: shapes {nd.shape} {bx.shape} {sc.shape} {lb.shape} do not agree")
        cap = int(cap)
        fs, is_ = sentinel if sentinel is not None else (0.0, 0)
        c = max(cap, 1)
        r = dict(rank=np.full((b, md), is_, np.int32), frame_n=np.full(b, is_, np.int32), frame_d0=np.full(b, is_, np.int32),
                 total=np.full(2, is_, np.int32), xyxy=np.full((c, 4), fs, np.float32), tlwh=np.full((c, 4), fs, np.float32),
                 conf=np.full(c, fs, np.float32), cls=np.full(c, is_, np.int32), frame_of=np.full(c, is_, np.int32))
        mk = np.array([int(mask[0]) & (2 ** 64 - 1), int(mask[1]) & (2 ** 64 - 1)], np.uint64)
        L.call("aic_det_filter", int(device), L.ptr(nd), L.ptr(bx), L.ptr(sc), L.ptr(lb), b, md, float(min_conf), L.ptr(mk), cap,
               *(L.ptr(r[k]) for k in ("rank", "frame_n", "frame_d0", "total", "xyxy", "tlwh", "conf", "cls", "frame_of")))
        return r

    def reid_infer_np(self, crops_nchw, n_live=None):
        """n_live: run with a device-side count holding n_live in force (aic_reid_infer_live, include/aicam.h; tests): rows at and past
        it are not computed and come back as zeros."""
        x = L.as_f32(crops_nchw)
        n = x.shape[0]
        out = np.zeros((n, self.out_dim), np.float32)
        if n and n_live is None:
            L.call("aic_reid_infer", self._h, L.ptr(x), n, L.HOST, L.ptr(out), L.HOST)
        elif n:
            L.call("aic_reid_infer_live", self._h, L.ptr(x), n, int(n_live), L.HOST, L.ptr(out), L.HOST)
        return out

    def read_buffer_np(self, buf, n):
        """Activation buffer `buf` of the engine file's buffer table after the last run, items 0 .. n-1: an [n, h, w, c] NHWC array at
        the buffer's element type (float32 for an fp32 buffer or engine, else float16) and full channel width."""
        with open(self.engine_path, "rb") as f:
            head = np.frombuffer(f.read(68), "<i4")
            tab = np.frombuffer(f.read(16 * int(head[5])), "<i4").reshape(-1, 4)
        h, w, c, f32 = (int(v) for v in tab[buf])
        out = np.empty((int(n), h, w, c), np.float32 if f32 or self.dtype == L.F32 else np.float16)
        L.call("aic_model_read_buffer", self._h, int(buf), L.ptr(out), out.nbytes)
        return out

    def conv_plan(self, op, n, live=False):
        """What a launch of n items runs at op `op` of the engine file's op list (aic_model_conv_plan, include/aicam.h); live: with a
        device-side item count in force (aic_model_conv_plan_live)."""
        out = np.zeros(24, np.int32)
        L.call("aic_model_conv_plan_live" if live else "aic_model_conv_plan", self._h, int(op), int(n), L.ptr(out))
        names = ["form", "mt", "nt", "wm", "wn", "nstage", "th", "tw", "cpp", "pitch", "kord", "g", "tail", "x2", "run", "blocks"]
        forms = ["Dma", "Wide", "Pp", "PpPatch", "SpPatch", "S2Patch", "Patch", "PmPatch", "C16", "C32s2Tail", "Stream1x1", "C64Resident"]
        r = {"kind": {-2: "covered", -1: "none", 0: "conv", 1: "conv+tail", 2: "c64_block", 3: "c2f16"}[int(out[0])],
             "first_op": int(out[1]), "n_ops": int(out[2]), "ipb": int(out[3])}
        if out[0] in (0, 1):
            r.update({k: int(v) for k, v in zip(names, out[5:21])})
            r.update(form=forms[r["form"]], k_order=int(out[4]), xs=int(out[21]), y_coff=int(out[22]), x_coff=int(out[23]))
        return r

    def row_band(self, op, src_h, src_w):
        """The rows of op `op`'s output map that can depend on a src_h x src_w frame, and whether the last run on frames ran the op on a
        row window (aic_model_row_band, include/aicam.h)."""
        out = np.zeros(8, np.int32)
        L.call("aic_model_row_band", self._h, int(op), int(src_h), int(src_w), L.ptr(out))
        return {"full": bool(out[0]), "lo": int(out[1]), "hi": int(out[2]), "rows": int(out[3]), "windowed": bool(out[4]),
                "win_y0": int(out[5]), "win_rows": int(out[6]), "slots": int(out[7])}

    def sparse_box(self, force=None):
        """What the last run did with the detector's box branches (aic_model_sparse_box, include/aicam.h); force: True / False sets
        whether every eligible run takes the lists."""
        out = np.zeros(8, np.int32)
        L.call("aic_model_sparse_box", self._h, -1 if force is None else int(bool(force)), L.ptr(out))
        return {"listed": bool(out[0]), "counts": tuple(int(v) for v in out[1:5]), "counted": bool(out[5]), "shape_ok": bool(out[6]),
                "lead0": bool(out[7])}

    def read_det_np(self, n):
        """-> (boxes [n, A, 4], max logit [n, A], labels [n, A]) of the detector workspace after the last run (aic_model_read_det)."""
        b, m, l = np.zeros((n, self.n_anchors, 4), np.float32), np.zeros((n, self.n_anchors), np.float32), np.zeros((n, self.n_anchors), np.int32)
        L.call("aic_model_read_det", self._h, int(n), L.ptr(b), L.ptr(m), L.ptr(l))
        return b, m, l

    def detect_np(self, frames_bgr, conf=None, iou=None, max_det=None, n_live=None):
        """n_live: with a device-side frame count holding n_live in force (aic_detect_live; tests)."""
        f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        if f.ndim == 3:
            f = f[None]
        b, h, w, _ = f.shape
        md = int(max_det or self.max_det)
        nd = np.zeros(b, np.int32)
        boxes, scores, labels = np.zeros((b, md, 4), np.float32), np.zeros((b, md), np.float32), np.zeros((b, md), np.int32)
        tail = (float(conf if conf is not None else self.conf_thresh), float(iou if iou is not None else self.iou_thresh), md,
                L.ptr(nd), L.ptr(boxes), L.ptr(scores), L.ptr(labels))
        if n_live is None:
            L.call("aic_detect", self._h, L.ptr(f), b, h, w, L.HOST, *tail)
        else:
            L.call("aic_detect_live", self._h, L.ptr(f), b, int(n_live), h, w, L.HOST, *tail)
        return nd, boxes, scores, labels

    def detect_decode_np(self, n, hw, conf=None, iou=None, max_det=None):
        """Decode + NMS of the last detect_np run again at other thresholds, frames 0 .. n-1 of hw = (h, w) (aic_detect_decode)."""
        md = int(max_det or self.max_det)
        nd = np.zeros(n, np.int32)
        boxes, scores, labels = np.zeros((n, md, 4), np.float32), np.zeros((n, md), np.float32), np.zeros((n, md), np.int32)
        L.call("aic_detect_decode", self._h, int(n), int(hw[0]), int(hw[1]), float(conf if conf is not None else self.conf_thresh),
               float(iou if iou is not None else self.iou_thresh), md, L.ptr(nd), L.ptr(boxes), L.ptr(scores), L.ptr(labels))
        return nd, boxes, scores, labels

    def embed_boxes_np(self, frame_bgr, boxes_xyxy):
        f = np.ascontiguousarray(frame_bgr, dtype=np.uint8)
        b = L.as_f32(boxes_xyxy).reshape(-1, 4)
        n = len(b)
        emb, valid = np.zeros((n, self.out_dim), np.float32), np.zeros(n, np.int32)
        if n:
            L.call("aic_reid_embed", self._h, L.ptr(f), f.shape[0], f.shape[1], L.HOST, L.ptr(b), n, L.ptr(emb), L.ptr(valid))
        return emb, valid

    def embed_bank_np(self, frames_bgr, boxes_xyxy, frame_of=None, byte_offset=0, n_live=None):
        """One run with the crops resampled inside the fused stem from a bank of frames [F, h, w, 3], set up as the pipeline's
        device-filtered round (aic_reid_embed_bank, include/aicam.h; parity tests).  valid is prefilled with -1 and rows at and beyond
        n_live are not computed.  -> (embeddings, valid); the stem's pooled tensor is left for read_buffer_np."""
        f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        if f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("expected u8 frames [F, h, w, 3]")
        b = L.as_f32(boxes_xyxy).reshape(-1, 4)
        n = len(b)
        fo = None if frame_of is None else np.ascontiguousarray(frame_of, np.int32)
        if fo is not None and fo.shape != (n,):
            raise ValueError("frame_of must hold one index per box")
        emb, valid = np.zeros((n, self.out_dim), np.float32), np.full(n, -1, np.int32)
        L.call("aic_reid_embed_bank", self._h, L.ptr(f), f.shape[0], f.shape[1], f.shape[2], int(byte_offset), L.ptr(b), L.ptr(fo), n,
               -1 if n_live is None else int(n_live), L.ptr(emb), L.ptr(valid))
        return emb, valid

    # ---- TRTEngine surface (torch tensors) -----------------------------------------------------
    def _warm_up(self, iterations=5):   # trt_engine.py:119-149
        start = time.time()
        n = 1
        x = np.zeros((n, 3, self.in_h, self.in_w), np.float32)
        for _ in range(iterations):
            if self.kind == L.MODEL_YOLO:
                self.yolo_infer_np(x)
            else:
                self.reid_infer_np(x)
        print(f"Warm-up for '{self.engine_path.name}' finished in {time.time() - start:.3f} seconds.")

    def infer(self, inputs: Dict[str, "object"]) -> Dict[str, "object"]:
        """trt_engine.py:151-203: validate / cast / make contiguous, run, return fresh output tensors
        owned by the caller (device tensors, like the reference)."""
        torch = _torch()
        info = self.input_info_list[0]
        x = inputs.get(info.name)
        if x is None:
            raise ValueError(f"Missing input: '{info.name}'")                       # trt_engine.py:159-160
        dev = torch.device(f"cuda:{self.device_index}")
        if x.device != dev:
            x = x.to(dev)
        if x.dtype != torch.float32:
            print(f"Warning: Input tensor '{info.name}' dtype mismatch. Expected {torch.float32}, got {x.dtype}. Casting...")
            x = x.to(torch.float32)
        x = x.contiguous()
        torch.cuda.current_stream(dev).synchronize()   # the library runs on its own HIP stream
        n = int(x.shape[0])
        if n > self.max_items:
            raise RuntimeError(f"batch {n} exceeds engine capacity {self.max_items}")
        if self.kind == L.MODEL_YOLO:
            md = self.max_det
            out = {"num_dets": torch.empty((n, 1), dtype=torch.int32, device=dev),
                   "bboxes": torch.empty((n, md, 4), dtype=torch.float32, device=dev),
                   "scores": torch.empty((n, md), dtype=torch.float32, device=dev),
                   "labels": torch.empty((n, md), dtype=torch.int32, device=dev)}
            L.call("aic_yolo_infer", self._h, C.c_void_p(x.data_ptr()), n, L.DEVICE, float(self.conf_thresh),
                   float(self.iou_thresh), md, C.c_void_p(out["num_dets"].data_ptr()), C.c_void_p(out["bboxes"].data_ptr()),
                   C.c_void_p(out["scores"].data_ptr()), C.c_void_p(out["labels"].data_ptr()))
            return out
        out = {"output": torch.empty((n, self.out_dim), dtype=torch.float32, device=dev)}
        if n:
            L.call("aic_reid_infer", self._h, C.c_void_p(x.data_ptr()), n, L.DEVICE, C.c_void_p(out["output"].data_ptr()), L.DEVICE)
        return out

    def __call__(self, inputs):
        if not isinstance(inputs, dict):                                             # trt_engine.py:205-210
            raise TypeError(f"Input to {self.engine_path.name} engine must be a dictionary mapping input names to torch.Tensors.")
        return self.infer(inputs)

    def get_input_details(self) -> List[TensorInfo]:
        return self.input_info_list

    def get_output_details(self) -> List[TensorInfo]:
        return self.output_info_list


TRTEngine = HipEngine   # drop-in name
