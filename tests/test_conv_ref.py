"""The per-layer conv harness (tests/conv_ref.py) on the CPU: for every case's shape at a small n, the derived tolerance must let honest
arithmetic through -- the same layer evaluated in fp32 by torch, output rounded to the engine's element type -- and must catch each of
the smallest real bugs on at least one element.  No number here comes from a kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

SMALL_N = 3


def _inputs(c):
    B = R.build_graph(c)
    base, _ = R.images(c, SMALL_N)
    vals = R.host_inputs(c, B, base)
    return B, vals


def _ratio(a, ref, tol):
    return float((np.abs(a - ref) / tol).max())


def _torch_layer(x, l, dtype, res=None, x2=None, l2=None):
    """One layer in fp32 by torch from the same inputs: conv2d, + bias, (+ res), activation, (+ res); -> fp64 NHWC."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 3, 1, 2)))      # noqa: E731
    w = torch.from_numpy(R.dev_weights(l["w"], dtype).astype(np.float32))
    y = F.conv2d(t(x), w, None, l["stride"], l["k"] // 2)
    b = torch.from_numpy(np.asarray(l["b"], np.float32))
    if x2 is not None:
        y = y + F.conv2d(t(x2), torch.from_numpy(R.dev_weights(l2["w"], dtype).astype(np.float32)), None, l2["stride"], 0)
        b = b + torch.from_numpy(np.asarray(l2["b"], np.float32))
    y = y + b.view(1, -1, 1, 1)
    if res is not None and l["res_mode"] == R.ef.RES_ADD_THEN_ACT:
        y = y + t(res)
    y = F.silu(y) if l["act"] == R.SILU else (F.relu(y) if l["act"] == R.RELU else y)
    if res is not None and l["res_mode"] == R.ef.RES_ACT_THEN_ADD:
        y = y + t(res)
    return y.permute(0, 2, 3, 1).numpy().astype(np.float64)


def _honest(c, B, vals):
    """The case's outputs by fp32 arithmetic, keyed like case_reference's rows."""
    L, dt, out = B.layers, c.dtype, {}
    rnd = lambda a: R.to_elem(a, dt)                                                                           # noqa: E731
    inp3 = vals["inp"][..., :3]
    if c.pattern == "block64":
        fused = c.expect.get("kind") == "c64_block"
        mid = rnd(_torch_layer(vals["x"], L["c1"], dt))
        if not fused:
            out["c1"] = mid
        out["c2"] = rnd(_torch_layer(mid if fused else vals["mid"], L["c2"], dt, res=vals["x"]))
    elif c.pattern == "ds":
        out["c1"] = rnd(_torch_layer(vals["x"], L["c1"], dt))
        l = dict(L["c2"], res_mode=0)
        out["c2+ds"] = rnd(_torch_layer(vals["t"], l, dt, x2=vals["x"], l2=L["ds"]))
    elif c.pattern == "xs":
        out["stem_lo"] = rnd(_torch_layer(inp3, L["stem_lo"], dt))
        xin = np.concatenate([vals["lo"].repeat(2, 1).repeat(2, 2), vals["cat"][..., 64:]], -1)
        out["layer"] = rnd(_torch_layer(xin, L["layer"], dt))
    else:
        if c.slice:
            out["stem_slice"] = rnd(_torch_layer(inp3, L["stem_slice"], dt))
        y = rnd(_torch_layer(vals["x"], L["layer"], dt, res=vals.get("r") if c.res else None))
        if c.tail:
            out["layer+tail"] = rnd(_torch_layer(y, L["tail"], dt))
        else:
            out["layer"] = y
    return out


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_tolerance_sits_between_honest_arithmetic_and_the_smallest_bugs(c):
    torch.set_num_threads(1)
    B, vals = _inputs(c)
    read = lambda name: vals[name]                                                                             # noqa: E731
    rows = R.case_reference(c, B, read)
    honest = _honest(c, B, vals)
    assert set(honest) == {r[0] for r in rows}
    for name, _, _, ref, tol in rows:
        assert np.isfinite(ref).all() and (tol > 0).all()
        assert 0.05 < np.abs(ref).mean() < 20, (name, np.abs(ref).mean())              # outputs are O(1): a dropped tap or a displaced pixel is too
        r = _ratio(honest[name], ref, tol)
        assert r <= 1.0, f"{c.id} {name}: fp32 arithmetic is {r:.2f} x the tolerance"
    under_test = rows[-1][0]
    for mut in R.MUTANTS:
        if mut == "res_order" and not (c.res or c.pattern == "block64"):
            continue
        if mut == "res_order" and c.pattern == "ds":
            continue
        bad = {r[0]: r for r in R.case_reference(c, B, read, mut=mut)}[under_test]
        good = rows[-1]
        r = _ratio(bad[3], good[3], good[4])
        assert r > 1.0, f"{c.id}: the {mut} bug stays inside the tolerance ({r:.3f} x)"


def _assert_live(res):
    """The assertions of tests/test_gpu_conv_counts.py on check_live's figures, in its order; -> the name of the first that fails."""
    if res["live"] and not res["dirty"] > 1.0:
        return "dirty"
    if not res["ratio"] <= 1.0:
        return "live rows"
    if not res["past"]:
        return "past the count"
    if res["host"] is False:
        return "same kernel, same bits"
    return None


def test_count_checks_separate_honest_results_from_the_smallest_bugs():
    """check_live on dma_2x5's shape (400 pixels per image on 128-pixel tiles), 12 images, count 9: the fp64 reference rounded to fp16 is
    the device's output below the count, another draw's reference what the run found there.  Four planted bugs, each caught by the
    assertion it belongs to; the unplanted array passes all of them."""
    c = next(c for c in R.CASES if c.id == "dma_2x5")
    n, k, B = 12, 9, R.build_graph(c)
    assert k in c.counts and k * c.Ho * c.Wo % 128 and R.live_unit(c)["bm"] == 128

    def outputs(salt):
        base, _ = R.images(c, n, salt)
        vals = R.host_inputs(c, B, base)
        name, _, _, ref, tol = R.case_reference(c, B, lambda nm: vals[nm])[-1]
        return ref, tol, ref.astype(np.float16)[np.arange(n) % len(ref)]
    ref, tol, host = outputs(0)
    _, _, dirty = outputs(1)
    honest = np.concatenate([host[:k], dirty[k:]])
    assert _assert_live(R.check_live(honest, dirty, ref, tol, k, host=host)) is None
    for count in (0, 1, n - 1, n + 3):
        good = np.concatenate([host[:count], dirty[count:]])
        assert _assert_live(R.check_live(good, dirty, ref, tol, count, host=host)) is None, count
    P, px = len(ref), c.Ho * c.Wo
    bugs = {}
    bugs["last live image left as it was"] = honest.copy()
    bugs["last live image left as it was"][k - 1] = dirty[k - 1]
    bugs["image k also written"] = honest.copy()
    bugs["image k also written"][k] = host[k]
    z = honest.copy().reshape(n * px, -1)
    z[k * px // 128 * 128:k * px] = 0                                   # the live rows of the tile that straddles the count
    bugs["straddling tile not stored"] = z.reshape(honest.shape)
    bugs["image k - 1 from image k's input"] = honest.copy()
    bugs["image k - 1 from image k's input"][k - 1] = host[k]
    want = {"last live image left as it was": "live rows", "image k also written": "past the count",
            "straddling tile not stored": "live rows", "image k - 1 from image k's input": "live rows"}
    for name, got in bugs.items():
        res = R.check_live(got, dirty, ref, tol, k, host=host)
        assert _assert_live(res) == want[name], (name, res)
    # the first bug shows only because the tensor was dirty: over a tensor that already held the right values it would pass
    clean = R.check_live(honest, honest, ref, tol, k)
    assert clean["ratio"] <= 1.0 and not clean["dirty"] > 1.0
