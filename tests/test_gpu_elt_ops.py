"""The NHWC graph ops (max pool, SPPF pooling, upsample, average pool, L2 normalise) and the two fused stems, tensor by tensor
(tests/elt_ref.py): one small engine per case, one run, the op's input and output buffers read back (aic_model_read_buffer), the
reference computed from the input AS READ BACK, every output element compared -- bit exact where the op only selects values or the
arithmetic is fully specified, else against fp64 with a tolerance derived in elt_ref's docstring.  Cases with channel offsets also check
that the channels around the written slice still hold what was put there before the op ran.

Which kernel ran: the graph ops' launchers choose by shape; every case names its kernel and elt_ref.expected_kernel restates the rule.
What the engine fuses at load time is asked of the library (aic_model_conv_plan): the fused ReID stem's conv reports "none" (taken by
the fusion) in an fp16 engine and "conv" in an fp32 one, the upsample's reader reports no split source (the fold did not take the op).
The fused YOLO stem ran when the call left the engine's input canvas untouched.

A HIP error ends the session (_stop_on_device_error)."""
import numpy as np
import pytest

import conv_ref as R
import elt_ref as E
from conftest import pkg
from test_gpu_conv_forms import _check_plan, _stop_on_device_error

pytestmark = pytest.mark.gpu

# measured on MI355X: worst error / tolerance of the rows that have a tolerance (bit-exact rows are 0 or the case fails), recorded
# after the run; nothing is tightened from it
MEASURED = {
    "ap_4x8_c64_n37_fp16": 0.888, "ap_4x8_c64_n37_fp32": 0.118, "ap_1x1_c24_n1_fp16": 0.000, "ap_1x1_c24_n1_fp32": 0.000,
    "ap_7x3_c20_n37_fp16": 0.868, "ap_7x3_c20_n37_fp32": 0.134, "ap_13x7_c24_n1_fp16": 0.593, "ap_13x7_c24_n1_fp32": 0.038,
    "ap_13x7_c16_slice_n37_fp16": 0.913, "ap_13x7_c16_slice_n37_fp32": 0.081, "ap_7x3_c12_slice4_n37_fp16": 0.883,
    "ap_7x3_c12_slice4_n37_fp32": 0.125, "l2_c40_n5_fp16": 0.197, "l2_c40_n5_fp32": 0.116, "l2_c64_n1_fp16": 0.128,
    "l2_c64_n1_fp32": 0.123, "l2_c200_n37_fp16": 0.164, "l2_c200_n37_fp32": 0.165, "l2_c512_n5_fp16": 0.076, "l2_c512_n5_fp32": 0.105,
    "l2_c200_slice_n5_fp16": 0.136, "l2_c200_slice_n5_fp32": 0.139, "l2_c64_zero_row_n5_fp16": 0.182, "l2_c64_zero_row_n5_fp32": 0.137,
    "stem2_H16_fp16": 0.920, "stem2_H32_fp16": 0.909, "stem2_H128_fp16": 0.926, "stem1_H8_fp16": 0.915, "stem1_H24_fp16": 0.917,
    "stem1_H40_fp16": 0.926, "stem2_H32_slice_fp16": 0.920, "stem1_H24_slice_fp16": 0.914, "yolo_stem_area2_96x256": 0.908,
    "yolo_stem_down_100x300": 0.896, "yolo_stem_small_40x100": 0.931, "yolo_stem_same_64x128": 0.937,
}
MEASURED_STEM_ROWS = 0.944      # the feeding stems' channels around a written slice, against conv_ref's tolerance


def _compare(cid, rows, raw):
    for name, buf, c0, ref, tol, exact in rows:
        got = raw(buf)[..., c0:c0 + ref.shape[-1]]
        assert got.shape == ref.shape, (cid, name, got.shape, ref.shape)
        ratio, where = R.worst_ratio(got, ref, tol)
        print(f"elt op {cid} [{name}]: worst error / tolerance {ratio:.3f} at {where}" + (" (bit exact)" if exact and ratio == 0.0 else ""))
        if exact:
            assert ratio == 0.0, f"{cid} [{name}]: not bit exact, first at (image, y, x, channel) {where}: {ratio:.1f} half-ulps"
        else:
            assert ratio <= 1.0, f"{cid} [{name}]: error is {ratio:.3f} x the derived tolerance at (image, y, x, channel) {where}"


@pytest.mark.parametrize("c", E.CASES, ids=[c.id for c in E.CASES])
@_stop_on_device_error
def test_graph_op_against_reference(gpu, tmp_path, c):
    HipEngine = pkg("hip_engine").HipEngine
    B = E.build_graph(c)
    path = str(tmp_path / f"{c.id}.aicw")
    E.ef.write_engine(path, B.g)
    eng = HipEngine(path, dtype=c.dtype, max_items=c.n, warm_up=False)
    try:
        emb = eng.reid_infer_np(E.images(c))
        assert np.isfinite(emb).all()
        cache = {}

        def raw(name):
            if name not in cache:
                cache[name] = eng.read_buffer_np(B.bufs[name], c.n)
            return cache[name]
        # ---- which kernel ran
        assert E.expected_kernel(c, B) == c.kernel, f"{c.id}: expected {c.kernel}, the launcher's rule picks {E.expected_kernel(c, B)}"
        L = B.layers
        if c.op == "reid_stem":
            _check_plan(c.id, "conv0", eng.conv_plan(L["conv0"]["op"], c.n), dict(kind="none" if c.dtype == "fp16" else "conv"))
            if c.dtype == "fp16":
                assert not raw("a").any(), f"{c.id}: the fused stem wrote its conv tensor"
        assert eng.conv_plan(L["op"]["op"], c.n)["kind"] == "none"                 # (not a conv: nothing took it over either)
        if c.op == "upsample":
            _check_plan(c.id, "reader", eng.conv_plan(L["reader"]["op"], c.n), dict(kind="conv", xs=0))
        # ---- what it computed
        _compare(c.id, E.case_reference(c, B, lambda name: raw(name).astype(np.float64)), raw)
        if c.op == "l2norm":
            assert np.array_equal(emb, raw("y").reshape(emb.shape))
            if c.bias == "zero":
                y = raw("y").reshape(c.n, -1)
                assert not raw("x")[1].any() and np.array_equal(y[1], np.zeros_like(y[1])) and np.abs(y[[0, 2, 3, 4]]).max() > 0
    finally:
        eng.close()


@pytest.mark.parametrize("c", E.LIVE_CASES, ids=[c.id for c in E.LIVE_CASES])
@_stop_on_device_error
def test_graph_op_under_a_device_count(gpu, tmp_path, c):
    """maxpool3s2, avgpool, avgpool8 and l2norm with a device-side item count in force (EltArgs::n_dev, aic_reid_infer_live): the launch
    is sized for n, the kernel cuts its index range at the count.  Before every counted run the engine runs other images without a
    count; the rows below the count are compared with the same references at the same bounds as above, computed from the op's input
    as read back; the rows at and past it still hold, bit for bit, what the run before left there."""
    HipEngine = pkg("hip_engine").HipEngine
    B = E.build_graph(c)
    path = str(tmp_path / f"{c.id}.aicw")
    E.ef.write_engine(path, B.g)
    x = E.images(c)
    noise = np.ascontiguousarray(x[::-1] * np.float32(0.5) + np.float32(0.25))          # other images of the same range; a zero image is none
    eng = HipEngine(path, dtype=c.dtype, max_items=c.n, warm_up=False)
    try:
        assert E.expected_kernel(c, B) == c.kernel
        for k in E.live_counts(c):
            live = min(k, c.n)
            eng.reid_infer_np(noise)
            dirty = eng.read_buffer_np(B.bufs["y"], c.n)
            emb = eng.reid_infer_np(x, n_live=k)
            cache = {}

            def raw(name):
                if name not in cache:
                    cache[name] = eng.read_buffer_np(B.bufs[name], c.n)
                return cache[name]
            y = raw("y")
            assert np.array_equal(R.bits(y[live:]), R.bits(dirty[live:])), f"{c.id} n_live={k}: rows at and past the count were written"
            if live:
                assert not np.array_equal(R.bits(y[:live]), R.bits(dirty[:live])), f"{c.id} n_live={k}: nothing was stored below the count"
            rows = E.case_reference(c, B, lambda name: raw(name).astype(np.float64))
            _compare(f"{c.id} n_live={k}", [(nm, buf, c0, ref[:live], tol[:live], exact) for nm, buf, c0, ref, tol, exact in rows],
                     lambda name: raw(name)[:live])
            if c.op == "l2norm":
                assert np.array_equal(emb[:live], y.reshape(c.n, -1)[:live]) and not emb[live:].any()
    finally:
        eng.close()


@pytest.fixture(scope="module")
def yolo_small(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("elt") / "yolov8n_64x128.aicw")
    g = E.ef.build_yolov8("n", in_hw=E.YOLO_IN_HW, seed=5)
    E.ef.write_engine(path, g)
    return path, g


@pytest.mark.parametrize("name", list(E.YOLO_FRAMES))
@_stop_on_device_error
def test_fused_yolo_stem_against_fp64(gpu, yolo_small, name):
    """yolo_stem_fused_kernel at the smallest input it takes, two u8 frames per call: its output tensor against the integer letterbox
    + fp64 conv.  The stem's output buffer is written by op 0 alone (asserted from the graph; the load-time merge only adds buffers), so
    it still holds the stem's output when the call returns."""
    HipEngine = pkg("hip_engine").HipEngine
    path, g = yolo_small
    op0 = g.ops[0]
    b0 = op0[4]
    assert op0[0] == E.ef.OP_CONV and op0[1] == 0 and op0[6] == 16 and all(o[4] != b0 for o in g.ops[1:])
    assert g.buffers[b0][:3] == (32, 64, 16)
    w, b = g.weights[op0[15]]
    eng = HipEngine(path, dtype="fp16", max_items=2, warm_up=False)
    try:
        x0 = np.random.default_rng(3).uniform(0.0, 1.0, (2, 3) + E.YOLO_IN_HW).astype(np.float32)
        eng.yolo_infer_np(x0)                                          # the unfused path fills the input canvas
        canvas = eng.read_buffer_np(0, 2)
        assert np.array_equal(canvas[..., :3], x0.transpose(0, 2, 3, 1).astype(np.float16)) and not canvas[..., 3:].any()
        before = eng.read_buffer_np(b0, 2)
        frames = E.yolo_frames(name)
        nd = eng.detect_np(frames)[0]
        assert nd.shape == (2,) and (nd >= 0).all()
        assert np.array_equal(eng.read_buffer_np(0, 2), canvas), f"{name}: the call wrote the input canvas: the fused stem did not run"
        got = eng.read_buffer_np(b0, 2)
        assert not np.array_equal(got, before)
        ref, tol = E.yolo_stem_ref(frames, w, b)
        _compare(f"yolo_stem_{name}", [("letterbox+0.conv", None, 0, ref, tol, False)], lambda _: got)
    finally:
        eng.close()
