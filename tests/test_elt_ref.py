"""The graph-op / fused-stem harness (tests/elt_ref.py) on the CPU: for every case, honest arithmetic -- torch's own max_pool2d,
interpolate, adaptive_avg_pool2d and normalize in fp32, the stems as torch's fp32 conv followed by the pool, outputs rounded to the
engine's element type -- must pass the reference's check, and every applicable smallest bug must fail it on at least one element.
No number here comes from a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import elt_ref as E


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2)))


def _n(t):
    return t.permute(0, 2, 3, 1).numpy().astype(np.float64)


def _ratio(a, ref, tol):
    r = np.abs(a - ref) / tol
    return float("inf") if not np.isfinite(r).all() else float(r.max())


def _conv32(x, l, dtype, stride, act):
    w = torch.from_numpy(R.dev_weights(l["w"], dtype).astype(np.float32))
    y = F.conv2d(_t(x), w, torch.from_numpy(np.asarray(l["b"], np.float32)), stride, 1)
    return F.silu(y) if act == R.SILU else F.relu(y)


def _honest(c, B, vals):
    """The op under test by torch in fp32 from the same inputs, rounded to the element type -> fp64 NHWC."""
    dt = c.dtype
    if c.op == "reid_stem":
        if dt == "fp16":
            y = F.max_pool2d(_conv32(vals["inp"][..., :3], B.layers["conv0"], dt, 1, R.RELU), 3, 2, 1)
        else:
            y = F.max_pool2d(_t(vals["a"]), 3, 2, 1)
        return R.to_elem(_n(y), dt)
    x = _t(vals["x"][..., c.src_coff:c.src_coff + c.c])
    if c.op == "maxpool":
        y = F.max_pool2d(x, 3, 2, 1)
    elif c.op == "sppf":
        m5 = F.max_pool2d(x, 5, 1, 2)
        m9 = F.max_pool2d(m5, 5, 1, 2)
        y = torch.cat([m5, m9, F.max_pool2d(m9, 5, 1, 2)], 1)
    elif c.op == "upsample":
        y = F.interpolate(x, scale_factor=2, mode="nearest")
    elif c.op == "avgpool":
        y = F.adaptive_avg_pool2d(x, 1)
    elif c.op == "l2norm":
        return _n(F.normalize(x, p=2.0, dim=1, eps=1e-12))                # the op's output is fp32 in either engine
    return R.to_elem(_n(y), dt)


@pytest.mark.parametrize("c", E.CASES, ids=[c.id for c in E.CASES])
def test_reference_sits_between_honest_arithmetic_and_the_smallest_bugs(c):
    torch.set_num_threads(1)
    B = E.build_graph(c)
    assert E.expected_kernel(c, B) == c.kernel, f"{c.id}: the case table names {c.kernel}, the launcher's rule gives {E.expected_kernel(c, B)}"
    vals = E.host_inputs(c, B, E.images(c))
    read = lambda name: vals[name]                                                                             # noqa: E731
    rows = E.case_reference(c, B, read)
    k = E.rows_under_test(c)
    honest = _honest(c, B, vals)
    for name, _, _, ref, tol, exact in rows:
        assert np.isfinite(ref).all() and (tol > 0).all(), name
    for name, _, _, ref, tol, exact in rows[:k]:
        if c.op == "avgpool" and exact:                    # torch's summation order is its own: the bit-exact row is for the kernel's order,
            m, mtol = E.avgpool_ref(vals["x"][..., c.src_coff:c.src_coff + c.c], c.dtype)                      # which must itself sit inside the bound
            assert _ratio(ref, m, mtol) <= 1.0, f"{c.id}: the sequential fp32 restatement is outside the derived bound"
            continue
        r = _ratio(honest, ref, tol)
        assert (r == 0.0) if exact else (r <= 1.0), f"{c.id} {name}: honest fp32 arithmetic is {r:.3f} x the tolerance"
    # the inputs can show the bugs: a channel that is negative throughout, and (low cases) windows wholly below -65504
    src = vals["a"] if c.op == "reid_stem" else vals["x"]
    if c.bias == "mixed" and c.op != "reid_stem":
        assert (src.reshape(-1, src.shape[-1]).max(0) < 0).any(), f"{c.id}: no channel is negative throughout"
    if c.op == "reid_stem":
        assert (rows[0][3] == 0).any() and (rows[0][3] > 0).any(), f"{c.id}: no pooled value is exactly 0"
    if c.bias == "low":
        assert (rows[0][3] < -65504.0).all()
    muts = E.mutants(c)
    assert muts or (c.op == "l2norm" and c.c % 64 == 0 and c.n == 1), c.id       # (one item, whole lane passes: neither L2 mutant can show)
    for mut in muts:
        bad = E.case_reference(c, B, read, mut=mut)
        for good, b in zip(rows[:k], bad[:k]):
            r = _ratio(b[3], good[3], good[4])
            assert r > 1.0, f"{c.id} {good[0]}: the {mut} bug stays inside the check ({r:.3f} x)"


def test_every_mutant_is_applied_somewhere():
    seen = {m for c in E.CASES for m in E.mutants(c)}
    want = set(E.SLICE_MUTANTS) | {m for v in E.OP_MUTANTS.values() for m in v}
    assert seen == want, want - seen
    for op in ("maxpool", "sppf", "upsample", "avgpool", "l2norm"):
        assert any(c.op == op and c.src_coff and c.dst_coff for c in E.CASES), op
    assert {c.kernel for c in E.CASES} == {E.MP, E.UP, E.L2, E.SEP, E.DIRECT, E.AVG, E.AVG8, E.STEM1, E.STEM2}
    assert any(c.kernel == E.AVG and c.dtype == "fp16" for c in E.CASES)      # the scalar average pool in an fp16 engine


@pytest.mark.parametrize("hw", [(20, 20), (5, 3), (1, 1), (13, 13), (14, 12), (33, 32)])
def test_sppf_cascade_equals_the_5_9_13_windows(hw):
    x = np.random.default_rng(1).standard_normal((2,) + hw + (4,)) - 3.0
    assert np.array_equal(E.sppf_ref(x), E.sppf_windows(x))


@pytest.mark.parametrize("name", list(E.YOLO_FRAMES))
def test_yolo_stem_reference(name):
    """The fused YOLO stem's reference on the CPU: torch's fp32 conv of the same letterboxed pixels passes, each mutant fails."""
    torch.set_num_threads(1)
    g = E.ef.build_yolov8("n", in_hw=E.YOLO_IN_HW, seed=5)
    assert g.ops[0][0] == E.ef.OP_CONV and g.ops[0][6] == 16 and g.ops[0][9] == 2
    w, b = g.weights[g.ops[0][15]]
    frames = E.yolo_frames(name)
    ref, tol = E.yolo_stem_ref(frames, w, b)
    assert ref.shape == (2, 32, 64, 16) and np.isfinite(ref).all() and (tol > 0).all()
    honest = R.to_elem(_n(_conv32(E.yolo_stem_input(frames), dict(w=w, b=b), "fp16", 2, R.SILU)), "fp16")
    r = _ratio(honest, ref, tol)
    assert r <= 1.0, f"{name}: honest fp32 arithmetic is {r:.3f} x the tolerance"
    for mut in E.YOLO_MUTANTS:
        if not E.yolo_applicable(name, mut):
            continue
        r = _ratio(E.yolo_stem_ref(frames, w, b, mut=mut)[0], ref, tol)
        assert r > 1.0, f"{name}: the {mut} bug stays inside the tolerance ({r:.3f} x)"


def test_count_cases_cover_every_op_that_reads_a_count():
    """The cases tests/test_gpu_elt_ops.py runs under a device-side count: every kernel that cuts its range by one, in both element
    types, at 0, 1, n - 1 and n + 3; L2 normalise (four items per block) also at a count that is no multiple of four and not 1."""
    assert len(E.LIVE_CASES) == 2 * len(E.LIVE) and {c.id.rsplit("_", 1)[0] for c in E.LIVE_CASES} == set(E.LIVE)
    assert {c.kernel for c in E.LIVE_CASES} == {E.MP, E.AVG, E.AVG8, E.L2}
    for c in E.LIVE_CASES:
        assert c.kernel == E.expected_kernel(c, E.build_graph(c))
        ks = E.live_counts(c)
        assert {0, 1, c.n - 1, c.n + 3} <= set(ks) and c.n > 1
        if c.op == "l2norm":
            assert any(1 < k < c.n and k % 4 for k in ks), (c.id, ks)
