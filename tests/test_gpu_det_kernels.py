"""decode_kernel, select_sort_nms_kernel and the det_filter kernels fed directly (aic_yolo_postprocess / aic_det_filter: the production
launchers and argument structs, no conv) on the adversarial inputs of tests/det_ref.py: more than 1024 candidates, planted ties,
thresholds hit exactly, greedy chains, max_det reached inside a tile / at a tile edge / at a chunk edge, empty images, signed zeros.
Integer outcomes are compared with the oracle (oracle/nets_oracle.py::nms on the device's own decoded boxes) with np.array_equal;
decoded boxes with the fp64 decode within the tolerance det_ref derives."""
import numpy as np
import pytest
import torch

import det_ref as R
from conftest import pkg
from oracle import nets_oracle as N

pytestmark = pytest.mark.gpu
HipEngine = pkg("hip_engine").HipEngine
ef = pkg("engine_file")
L = pkg("_lib")

FS, IS = np.float32(-12345.0), np.int32(-777)                   # sentinels: an output element that still holds one was not written
VARIANTS = {"nc80_fp16": (80, 16, "fp16"), "nc80_fp32": (80, 16, "fp32"), "nc6_fp16": (6, 16, "fp16"), "reg8_fp32": (80, 8, "fp32"),
            "reg8_fp16": (80, 8, "fp16")}
MAX_ITEMS = len(R.DISJOINT_COUNTS)


@pytest.fixture(scope="module")
def det_engines(gpu, tmp_path_factory):
    """One 320 x 320 YOLOv8n engine per variant (2100 anchors; the weights are irrelevant: nothing is convolved), built on first use."""
    d = tmp_path_factory.mktemp("det_engines")
    files, engs = {}, {}

    def get(name):
        if name not in engs:
            nc, reg_max, dtype = VARIANTS[name]
            if (nc, reg_max) not in files:
                files[nc, reg_max] = str(d / f"yolo_nc{nc}_r{reg_max}.aicw")
                ef.write_engine(files[nc, reg_max], ef.build_yolov8("n", nc=nc, in_hw=(320, 320), reg_max=reg_max, calibrate=False))
            engs[name] = HipEngine(files[nc, reg_max], dtype=dtype, max_items=MAX_ITEMS, warm_up=False)
            assert engs[name].n_anchors == 2100
        return engs[name]
    yield get
    for e in engs.values():
        e.close()


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_decode_against_fp64(det_engines, name, batch):
    """Boxes within the derived tolerance of the fp64 decode; max logit bit-equal to the fp32 maximum; label = first arg-max, planted
    exact ties included; the first and last anchor of every level on their own."""
    nc, reg_max, dtype = VARIANTS[name]
    head = R.Head(nc=nc, reg_max=reg_max)
    dfl, cls, props = R.decode_inputs(head, batch, seed=7 + batch)
    r = det_engines(name).yolo_postprocess_np(dfl, cls, conf=0.25, iou=0.5, max_det=8, sentinel=(FS, IS))
    ref, ref_ml, ref_lab = head.decode(dfl, cls, np.float64)
    tol = R.decode_tolerance(head, dfl, ref, fast_exp=dtype == "fp16")
    err = np.abs(r["boxes"].astype(np.float64) - ref)
    print(f"decode {name} batch {batch}: worst |err| {err.max():.3e} px, worst err / tol {(err / tol).max():.4f}, largest tol {tol.max():.3e} px")
    assert (err <= tol).all(), float((err / tol).max())
    assert np.array_equal(r["max_logit"], cls.max(-1))
    assert np.array_equal(r["labels"], ref_lab)
    for (b, a), j in props["ties"].items():
        assert r["labels"][b, a] == j
    e = props["edge"]
    assert (err[:, e] <= tol[:, e]).all() and np.array_equal(r["labels"][:, e], ref_lab[:, e])


def test_nc6_engine_runs_end_to_end(gpu, tmp_path):
    """A class count that is no multiple of 4 (an fp32 class tensor of 24 bytes per anchor, which the loader admits for this tensor
    alone) through the whole engine, not only the post-processing: the head logits against the oracle's evaluation of the same file
    (fp32: no further from the fp64 evaluation than torch's own fp32, the criterion of test_yolo_head_and_decode; fp16: its 0.06), the
    decode kernel bit-equal on its own head tensor, NMS identical to the oracle's on the decoded arrays."""
    path = str(tmp_path / "yolo_nc6.aicw")
    ef.write_engine(path, ef.build_yolov8("n", nc=6, in_hw=(320, 320), calibrate=False))
    x = np.random.default_rng(1).random((3, 3, 320, 320), dtype=np.float32)
    eo = N.EngineOracle(path)
    d32, c32 = (t.numpy() for t in eo.yolo_head(torch.from_numpy(x)))
    d64, c64 = (t.numpy() for t in N.EngineOracle(path, dtype=torch.float64).yolo_head(torch.from_numpy(x)))
    l_cpu = max(np.abs(d32 - d64).max(), np.abs(c32 - c64).max())
    for dtype in ("fp32", "fp16"):
        eng = HipEngine(path, dtype=dtype, max_items=3, warm_up=False)
        assert eng.out_dim == 6
        dfl, cls = eng.yolo_head_np(x)
        l_hip = max(np.abs(dfl - d64).max(), np.abs(cls - c64).max())
        print(f"nc6 [{dtype}] head logit err vs fp64: HIP {l_hip:.2e}, torch fp32 {l_cpu:.2e}")
        assert l_hip <= (max(5e-5, l_cpu) if dtype == "fp32" else 0.06)
        boxes, ml, lab = eng.yolo_decode_np(x)
        kb, kml, klab = eo.decode(dfl, cls)
        assert np.abs(boxes - kb).max() < 2e-3 and np.array_equal(ml, kml) and np.array_equal(lab, klab)
        conf = float(np.float32(1 / (1 + np.exp(-float(np.sort(ml[0])[-400])))))      # about 400 candidates in image 0
        nd, ob, osc, ol = eng.yolo_infer_np(x, conf=conf, iou=0.5, max_det=300)
        for b in range(3):
            keep = N.nms(boxes[b], ml[b], lab[b], conf, 0.5, 300)
            assert nd[b] == len(keep) and np.array_equal(ol[b, :nd[b]], lab[b][keep]) and np.array_equal(ob[b, :nd[b]], boxes[b][keep])
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ NMS
def _check_nms(eng, c, geom=None):
    dfl, cls = c.tensors()
    md = c.max_det
    r = eng.yolo_postprocess_np(dfl, cls, conf=c.conf, iou=c.iou, max_det=md, geom=geom, sentinel=(FS, IS))
    for b, s in enumerate(c.scenes):
        boxes, ml, lab = r["boxes"][b], r["max_logit"][b], r["labels"][b]
        idx = np.array(sorted(s.exact), np.int64)
        if len(idx):                                             # the planted boxes came out exactly, on either exponential
            assert np.array_equal(boxes[idx], np.array([s.exact[a] for a in idx], np.float32)), (c.id, b)
        keep = N.nms(boxes, ml, lab, c.conf, c.iou, md)
        k = len(keep)
        assert r["n_cand"][b] == c.n_cand[b] == int((ml >= N.logit_threshold(c.conf)).sum()), (c.id, b, r["n_cand"][b])
        assert r["num_dets"][b] == k, (c.id, b, r["num_dets"][b], k)
        assert np.array_equal(r["out_labels"][b, :k], lab[keep]), (c.id, b)
        assert np.array_equal(r["out_boxes"][b, :k], boxes[keep]), (c.id, b)
        assert np.allclose(r["out_scores"][b, :k], N.sigmoid32(ml[keep]), rtol=0, atol=2e-7), (c.id, b)
        assert (r["out_boxes"][b, k:] == FS).all() and (r["out_scores"][b, k:] == FS).all() and (r["out_labels"][b, k:] == IS).all(), (c.id, b)
        if geom is None:
            assert (r["out_boxes_orig"][b] == FS).all()
        else:
            assert (r["out_boxes_orig"][b, k:] == FS).all()
    return r


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("cid", [c.id for c in R.nms_cases()])
def test_nms_on_exact_boxes(det_engines, cid, dtype):
    c = [c for c in R.nms_cases() if c.id == cid][0]
    _check_nms(det_engines(f"nc80_{dtype}"), c)


def test_nms_reg_max_8_head(det_engines):
    """The exact-box scenes on the generic DFL loop (their bins stay below 8)."""
    for c in R.nms_cases(80, 8):
        if c.id in ("composite_md1024", "zeros_conf0.5", "ties_md300"):
            _check_nms(det_engines("reg8_fp16"), c)


# ------------------------------------------------------------------------------------------------------------------ un-letterbox
@pytest.mark.parametrize("frame_hw", R.UNLETTERBOX_FRAMES)
def test_unletterbox_equals_scale_bboxes(det_engines, frame_hw):
    """out_boxes_orig is bit-equal to scale_bboxes of out_boxes (same fp32 subtract, divide, clip); the stress scene's boxes reach past
    the padded area on every side, so both clips act."""
    ratio, pad = R.letterbox_geometry(*frame_hw)
    c = [c for c in R.nms_cases() if c.id == "stress_md1024_iou0.45"][0]
    r = _check_nms(det_engines("nc80_fp16"), c, geom=(pad[0], pad[1], ratio, frame_hw[1], frame_hw[0]))
    lo = hi = 0
    for b in range(len(c.scenes)):
        k = int(r["num_dets"][b])
        exp = R.unletterbox_ref(r["out_boxes"][b, :k], frame_hw, ratio, pad)
        assert np.array_equal(r["out_boxes_orig"][b, :k], exp), b
        raw = (r["out_boxes"][b, :k] - np.array([pad[0], pad[1], pad[0], pad[1]], np.float32)) / ratio
        lo += int((raw < 0).sum())
        hi += int((raw[:, [0, 2]] > frame_hw[1]).sum() + (raw[:, [1, 3]] > frame_hw[0]).sum())
    assert lo > 0 and hi > 0, (lo, hi)


# ------------------------------------------------------------------------------------------------------------------ refusals (host side)
def test_postprocess_refuses_bad_arguments(det_engines):
    eng = det_engines("nc80_fp16")
    head = R.Head()
    dfl, cls = np.zeros((1, head.A, 64), np.float32), np.zeros((1, head.A, 80), np.float32)
    for kw in (dict(max_det=1025), dict(max_det=-1), dict(conf=1.0), dict(conf=0.0), dict(iou=1.5), dict(geom=(0, 0, 0.0, 10, 10)), dict(geom=(0, 0, 1.0, 0, 10))):
        args = dict(conf=0.25, iou=0.5, max_det=10)
        args.update(kw)
        with pytest.raises(L.AicError) as e:
            eng.yolo_postprocess_np(dfl, cls, **args)
        assert e.value.code in (L.ERR_INVALID, L.ERR_CAPACITY), kw
    big = MAX_ITEMS + 1
    with pytest.raises(L.AicError):
        eng.yolo_postprocess_np(np.zeros((big, head.A, 64), np.float32), np.zeros((big, head.A, 80), np.float32), conf=0.25, iou=0.5, max_det=10)
    with pytest.raises(ValueError):
        eng.yolo_postprocess_np(dfl[:, :100], cls[:, :100])
    # a refused call leaves the engine usable, and the decode-skip state of a real run untouched
    r = eng.yolo_postprocess_np(dfl, cls, conf=0.25, iou=0.5, max_det=10)
    assert r["num_dets"][0] == 10 and r["n_cand"][0] == head.A


# ------------------------------------------------------------------------------------------------------------------ filter
@pytest.mark.parametrize("cid", [c.id for c in R.filter_cases()])
def test_det_filter_against_numpy(gpu, cid):
    c = [c for c in R.filter_cases() if c.id == cid][0]
    cap = R.filter_cap(c)
    ref = R.filter_ref(c.num_dets, c.boxes, c.scores, c.labels, c.min_conf, c.mask, cap)
    r = HipEngine.det_filter_np(c.num_dets, c.boxes, c.scores, c.labels, c.min_conf, c.mask, cap, device=gpu, sentinel=(FS, IS))
    n = int(ref["total"][0])
    assert r["total"].tolist() == ref["total"].tolist(), (r["total"], ref["total"])
    assert np.array_equal(r["frame_n"], ref["frame_n"]) and np.array_equal(r["frame_d0"], ref["frame_d0"])
    for k in ("xyxy", "tlwh", "conf", "cls", "frame_of"):
        assert np.array_equal(r[k][:n], ref[k]), k
        assert (r[k][n:] == (FS if r[k].dtype == np.float32 else IS)).all(), k
    B, md = c.scores.shape
    for f in range(B):                                           # rank: position inside the frame, -1 for a dropped detection, untouched beyond the frame
        nd = min(int(c.num_dets[f]), md)
        rk = r["rank"][f]
        assert (rk[nd:] == IS).all() and sorted(v for v in rk[:nd] if v >= 0) == list(range(int(ref["frame_n"][f])))
