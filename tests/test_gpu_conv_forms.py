"""Every conv kernel form, per layer, against an fp64 reference (tests/conv_ref.py): one engine per case whose layer under test sees a
1x1 stem's output, one run, and the layer's OUTPUT TENSOR read back (aic_model_read_buffer) and compared pixel by pixel and channel
by channel with conv + bias (+ res) + act computed in fp64 from the layer's actual inputs, also read back.  The tolerance is derived per
element from the reference; the shapes are those where tiles hang over the map edge, M ends inside a tile or the input is odd.

Which kernel ran: every case asserts the form and tile the engine plans for its layer at its n, asked of the library itself
(aic_model_conv_plan: the launch path's own ConvArgs construction and planner call).  A moved threshold fails the case with the expected
and the planned form; it cannot pass on another kernel.

Forms that engage only at large M run P distinct images tiled to n: the input buffer is asserted exactly periodic, the reference is
computed for the P images, all n output images are compared."""
import numpy as np
import pytest

import conv_ref as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def _check_plan(cid, name, plan, expect):
    got = {k: plan.get(k) for k in expect}
    assert got == expect, f"{cid} {name}: expected {expect}, the engine plans {plan}"


def _run(c, tmp_path):
    """-> (Built, engine, read) after one run of the case's n images; read(buffer name) -> fp64 [P, h, w, c] of the P distinct images,
    after asserting that the whole buffer repeats them exactly."""
    HipEngine = pkg("hip_engine").HipEngine
    B = R.build_graph(c)
    path = str(tmp_path / f"{c.id}.aicw")
    R.ef.write_engine(path, B.g)
    base, x = R.images(c)
    P = len(base)
    eng = HipEngine(path, dtype=c.dtype, max_items=c.n, warm_up=False)
    emb = eng.reid_infer_np(x)
    assert np.isfinite(emb).all()
    raw = {}

    def read_raw(name):
        if name not in raw:
            raw[name] = eng.read_buffer_np(B.bufs[name], c.n)
        return raw[name]

    def read(name):
        a = read_raw(name)
        for j in range(P):
            assert np.array_equal(a[j::P], np.broadcast_to(a[j], a[j::P].shape)), f"{c.id}: buffer {name} is not periodic in the {P} distinct images"
        return a[:P].astype(np.float64)
    return B, eng, read, read_raw


def _stop_on_device_error(fn):
    """A HIP error ends the session: nothing more is started on a device that has just faulted."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except pkg("_lib").AicError as e:
            pytest.exit(f"{fn.__name__}: the library reported an error, stopping: {e}", returncode=1)
    return wrapped


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
@_stop_on_device_error
def test_conv_form_against_fp64(gpu, tmp_path, c):
    B, eng, read, read_raw = _run(c, tmp_path)
    try:
        L = B.layers
        # ---- which kernel ran
        if c.pattern == "block64":
            p1, p2 = eng.conv_plan(L["c1"]["op"], c.n), eng.conv_plan(L["c2"]["op"], c.n)
            if c.expect["kind"] == "c64_block":
                _check_plan(c.id, "c1", p1, dict(kind="c64_block", n_ops=2))
                _check_plan(c.id, "c2", p2, dict(kind="covered", first_op=L["c1"]["op"]))
                assert 12 <= p1["ipb"] <= 16 and c.n % p1["ipb"], (c.id, p1)             # the last block's share is partial
            else:
                _check_plan(c.id, "c1", p1, c.expect)
                _check_plan(c.id, "c2", p2, c.expect)
        elif c.pattern == "ds":
            _check_plan(c.id, "c1", eng.conv_plan(L["c1"]["op"], c.n), dict(kind="conv", k_order=3, form="Wide" if c.n == 3 else "S2Patch"))
            _check_plan(c.id, "ds", eng.conv_plan(L["ds"]["op"], c.n), dict(kind="none"))   # folded into c2 as its second source
            _check_plan(c.id, "c2", eng.conv_plan(L["c2"]["op"], c.n), dict(c.expect, kind="conv", k_order=1))
        else:
            plan = eng.conv_plan(L["layer"]["op"], c.n)
            _check_plan(c.id, "layer", plan, dict(c.expect, kind="conv+tail" if c.tail else "conv", y_coff=0 if c.tail else c.slice))
            if c.tail:
                _check_plan(c.id, "tail", eng.conv_plan(L["tail"]["op"], c.n), dict(kind="covered", first_op=L["layer"]["op"]))
        # ---- what it computed
        for name, buf, coff, ref, tol in R.case_reference(c, B, read):
            got = read_raw(buf)[..., coff:coff + ref.shape[-1]]
            ratio, where = R.worst_ratio(got, ref, tol)
            print(f"conv form {c.id} [{name}] n={c.n}: worst error / tolerance {ratio:.3f} at {where}")
            assert ratio <= 1.0, f"{c.id} [{name}]: error is {ratio:.3f} x the derived tolerance at (image, y, x, channel) {where}"
        if c.tail and "mid" in B.bufs:
            assert not read_raw("mid").any(), f"{c.id}: the fused lead wrote its intermediate"
    finally:
        eng.close()


def _c2f_reference(g, x, dt="fp16"):
    """The fused C2f of test_gpu_nets._c2f_graph from its input x [P, 24, 64, 32]: the three intermediates (cat[0:32], tmp, cat[32:48])
    live in LDS, so each is referenced rounded to fp16 and its possible disagreement with the device is propagated:
    dis = 1.1 * (accumulation bound + sum |w| * dis of what it read) + one ulp."""
    convs = [o for o in g.ops if o[0] == R.ef.OP_CONV]                        # stem, then the four convs of the block in list order
    W = {name: g.weights[convs[1 + i][15]] for i, name in enumerate(("c2f.cv1", "c2f.m0.cv1", "c2f.m0.cv2", "c2f.cv2"))}

    def level(name, xin, k, dis_in=None, res=None, last=False):
        w, b = W[name]
        extra = None if dis_in is None else R.next_slack(w, k, 1, dt, dis_in)
        ref, tol, acc = R.layer_ref(xin, w, b, k, 1, R.SILU, dt, res=res, res_mode=R.ef.RES_ACT_THEN_ADD if res is not None else 0, extra=extra)
        if last:
            return ref, tol
        v = R.to_elem(ref, dt)
        return v, 1.1 * (acc + (0.0 if extra is None else extra)) + R.ulp(v, dt)
    y1, d1 = level("c2f.cv1", x, 1)
    t, dt_ = level("c2f.m0.cv1", y1[..., 16:], 3, d1[..., 16:])
    y2, d2 = level("c2f.m0.cv2", t, 3, dt_, res=y1[..., 16:])
    d2 = d2 + d1[..., 16:]                                                    # the shortcut carries its own disagreement
    return level("c2f.cv2", np.concatenate([y1, y2], -1), 1, np.concatenate([d1, d2], -1), last=True)


@_stop_on_device_error
def test_fused_c2f_output_tensor_against_fp64(gpu, tmp_path):
    """The one-kernel C2f block: its `out` tensor (not only the embedding behind a pool) on a map where every tile touches a border."""
    from test_gpu_nets import _c2f_graph
    HipEngine = pkg("hip_engine").HipEngine
    path = str(tmp_path / "c2f.aicw")
    out, _ = _c2f_graph(path)
    g = R.ef.read_engine(path)
    n = 5
    x = np.random.default_rng(2).standard_normal((n, 3, 24, 64)).astype(np.float32)
    eng = HipEngine(path, dtype="fp16", max_items=n, warm_up=False)
    try:
        eng.reid_infer_np(x)
        op = [i for i, o in enumerate(g.ops) if o[0] == R.ef.OP_CONV][1]           # c2f.cv1: the first conv behind the stem
        _check_plan("c2f", "cv1", eng.conv_plan(op, n), dict(kind="c2f16", n_ops=4))
        b1 = g.ops[op][1]
        ref, tol = _c2f_reference(g, eng.read_buffer_np(b1, n).astype(np.float64))
        ratio, where = R.worst_ratio(eng.read_buffer_np(out, n), ref, tol)
        print(f"conv form c2f16 [out] n={n}: worst error / tolerance {ratio:.3f} at {where}")
        assert ratio <= 1.0, f"fused C2f: error is {ratio:.3f} x the derived tolerance at {where}"
    finally:
        eng.close()
