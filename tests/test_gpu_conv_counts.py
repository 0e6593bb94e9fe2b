"""Every conv form under a DEVICE-SIDE item count (ConvArgs::n_dev, the pipeline's default with the detection filter on the device):
the launch is sized for the bound n, the real count n_live is read by the kernel.  tests/test_gpu_conv_forms.py runs the same layers with
the count on the host; here each case of conv_ref.LIVE runs at every count of its `counts` list (conv_ref.live_counts: 0, 1, n - 1,
n + 3 and the edges of the unit the planned kernel deals its work in), through aic_reid_infer_live on one engine per case:

  plan      conv_plan(op, n, live=True) is the case's expect_live (Wide, PmPatch, Stream1x1 and C32s2Tail refuse a count, so those layers
            run the LDS-DMA implicit GEMM); the block kernel's images per block are read off the count, ceil(n_live / grid).
  dirty     before every live run the same engine runs other images of the same shape without a count; D is what that leaves in the
            layer's output buffers.
  live      rows [0, min(k, n)) of every output buffer conv_ref.case_reference names against the fp64 reference of the layer's ACTUAL
            inputs, read back for those rows after their periodicity in the P distinct images is asserted, at conv_ref's derived
            tolerance; D itself misses that reference on every live image, so an image no thread stored would show.
  past      rows [k, n) of those buffers equal D bit for bit; a fused lead's intermediate buffer stays all zero.
  same bits where the plan under the count is the plan without one, the live rows equal the rows of a run of the same images without a
            count bit for bit -- the block kernel too, whatever images per block it ran.
  output    embeddings below k are finite and of unit norm within elt_ref's l2norm bound, those at and past k are left as the call
            prefilled them.

Which forms read the count: Dma, Pp, PpPatch, SpPatch, S2Patch, Patch, C64Resident and the block kernel (conv_ref.READS_COUNT).  C16
does not (conv3x3_c16_kernel has no count; neither have Wide, PmPatch, C32s2Tail and Stream1x1, which the planner therefore refuses, nor
the fused C2f, which only YOLO graphs reach): it computes all n images and is checked on its live rows only.  In this harness the rows
it computes past the count come from inputs the count-reading stem left as the dirty run's, so they repeat D.

Counts 0 and n + 3 were read through every kernel first: each clamps with min(count, bound) (kernels_conv.hip:56, kernels_conv_pp.hip:48
and :341, kernels_conv_sp.hip:66 and :339, kernels_conv_direct.hip:366 and :637, kernels_conv_block.hip:63); at 0 the tile counts are 0
and every block leaves before its first load (the resident kernel runs zero trips and its two wave groups still meet at one barrier
each; the block kernel's n_loc == 0 prologue fetches the zero page and both groups pass five barriers).

What the rows past the count can show: the stems honour the count too, so the layer's inputs past it are still the dirty run's, and a
kernel that computed a row past the count completely and correctly would store D again -- lost time, not a wrong value, and not seen
here.  What is seen is a store of anything else: the realistic fault is a tile that straddles the count with its loads guarded and
its stores not, which writes activation(bias) there.  Run once against such a build (the LDS-DMA kernel's store guard on the bound
instead of the count; every access inside the buffers): wide_2x3, dma_2x5 and wide_2x3_slice fail "rows at and past the count were
written", the cases whose image is a whole number of tiles pass.  The same build with the block kernel's images per block rounded
down: c64_block fails its live rows at n_live = 1 with the dirty tensor's 1042 x the tolerance.

A HIP error ends the session (_stop_on_device_error).

measured on MI355X, worst error / tolerance over all counts and cases of a form (recorded after the run; nothing is tightened from it):
see MEASURED below."""
import numpy as np
import pytest

import conv_ref as R
import elt_ref as E
from conftest import pkg
from test_gpu_conv_forms import _check_plan, _stop_on_device_error

pytestmark = pytest.mark.gpu

# form under the count -> worst error / tolerance over all its cases and counts
MEASURED = {"Dma": 0.919, "Pp": 0.620, "PpPatch": 0.742, "SpPatch": 0.410, "S2Patch": 0.593, "Patch": 0.775, "C64Resident": 0.709,
            "c64_block": 0.306, "C16": 0.830}
# (Dma: wide_2x3_slice's stem channels 0.919, split_source 0.896, stream1x1_c96 0.873, the fp32 tiles 0.003; the block kernel ran 1, 2, 3
#  and 12 images per block; Patch ran 1, 2, 4, 6 and 7 live tiles, 8, and 9 / 10 / 12 as its remainder branch)

LIVE_CASES = [c for c in R.CASES if c.counts]
SAME = ("kind", "form", "mt", "nt", "wm", "wn", "th", "tw", "kord", "k_order", "tail", "x2")


def _plans(c, B, eng, live):
    """[(layer name, expected fields, plan)] of the case's layers under test."""
    L, e = B.layers, c.expect_live if live else c.expect
    plan = lambda name: eng.conv_plan(L[name]["op"], c.n, live=live)                            # noqa: E731
    if c.pattern == "block64":
        if e["kind"] == "c64_block":
            return [("c1", dict(kind="c64_block", n_ops=2), plan("c1")), ("c2", dict(kind="covered", first_op=L["c1"]["op"]), plan("c2"))]
        return [("c1", e, plan("c1")), ("c2", e, plan("c2"))]
    if c.pattern == "ds":
        small = c.n == 3
        c1 = dict(kind="conv", k_order=3, form=("Dma" if live else "Wide") if small else "S2Patch")
        return [("c1", c1, plan("c1")), ("ds", dict(kind="none"), plan("ds")), ("c2", dict(e, kind="conv", k_order=1), plan("c2"))]
    e = {k: v for k, v in e.items() if k != "blocks"}           # (the resident kernel's grid is the CU budget of the process: live_counts reads it)
    rows = [("layer", dict(e, kind="conv+tail" if c.tail else "conv", y_coff=0 if c.tail else c.slice), plan("layer"))]
    if c.tail:
        rows.append(("tail", dict(kind="covered", first_op=L["layer"]["op"]), plan("tail")))
    return rows


@pytest.mark.parametrize("c", LIVE_CASES, ids=[c.id for c in LIVE_CASES])
@_stop_on_device_error
def test_conv_form_under_a_device_count(gpu, tmp_path, c):
    HipEngine = pkg("hip_engine").HipEngine
    B = R.build_graph(c)
    path = str(tmp_path / f"{c.id}.aicw")
    R.ef.write_engine(path, B.g)
    base, x = R.images(c)
    _, noise = R.images(c, salt=1)
    P, n = len(base), c.n
    eng = HipEngine(path, dtype=c.dtype, max_items=n, warm_up=False)
    try:
        # ---- plan: what runs under the count, and whether that is the kernel that runs without one
        host_plans, live_plans = _plans(c, B, eng, False), _plans(c, B, eng, True)
        for name, expect, plan in live_plans:
            _check_plan(c.id, name + " (device count)", plan, expect)
        same = all({k: p.get(k) for k in SAME} == {k: q.get(k) for k in SAME} for (_, _, p), (_, _, q) in zip(host_plans, live_plans))
        form = c.expect_live.get("form", c.expect_live.get("kind"))
        reads_count = form in R.READS_COUNT
        head = live_plans[0][2] if c.pattern == "block64" else live_plans[-2 if c.tail else -1][2]
        counts = R.live_counts(c, head)                  # (the case's list, rebuilt from the engine's own answer: blocks and images per
        if form not in ("C64Resident", "c64_block"):     #  block follow the CU budget the process runs with)
            assert counts == c.counts, (c.id, counts, c.counts)
        grid = -(-n // head["ipb"]) if form == "c64_block" else 0
        ipb_seen = set()

        # ---- the run without a count: reference inputs, reference, the rows a same-kernel run must repeat
        eng.reid_infer_np(x)
        asked = {}

        def periodic(name, a, rows):
            for j in range(min(P, rows)):
                assert np.array_equal(R.bits(a[j:rows:P]), np.broadcast_to(R.bits(a[j]), a[j:rows:P].shape)), \
                    f"{c.id}: buffer {name} is not periodic in the {P} distinct images over its first {rows} rows"

        def read_host(name):
            if name not in asked:
                a = eng.read_buffer_np(B.bufs[name], n)
                periodic(name, a, n)
                asked[name] = a[:P].copy()
            return asked[name].astype(np.float64)
        rows0 = R.case_reference(c, B, read_host)
        out_bufs = sorted({buf for _, buf, _, _, _ in rows0})
        host = {buf: eng.read_buffer_np(B.bufs[buf], n) for buf in out_bufs}
        # ---- the dirty run
        eng.reid_infer_np(noise)
        dirty = {buf: eng.read_buffer_np(B.bufs[buf], n) for buf in out_bufs}
        if c.tail and "mid" in B.bufs:
            assert not eng.read_buffer_np(B.bufs["mid"], n).any(), f"{c.id}: the fused lead wrote its intermediate"

        T = -(-eng.out_dim // 64)
        norm_tol = (T + 10) * E.U + np.sqrt(eng.out_dim) * 2.0 ** -126         # elt_ref.l2norm_ref's bound, summed over a row
        worst = 0.0
        for k in counts:
            live = min(k, n)
            if k != counts[0]:
                eng.reid_infer_np(noise)
            emb = eng.reid_infer_np(x, n_live=k)
            if form == "c64_block" and live:
                ipb_seen.add(-(-live // grid))
            # ---- the layer's actual inputs on the live rows: periodic, and the reference they give
            m, fresh = min(live, P), {}
            for name in asked:
                a = eng.read_buffer_np(B.bufs[name], max(live, P))
                periodic(name, a, live)
                fresh[name] = a[:P]
            inputs_same = all(np.array_equal(R.bits(fresh[nm][:m]), R.bits(asked[nm][:m])) for nm in asked)
            rows = rows0 if inputs_same else R.case_reference(c, B, lambda nm: fresh[nm].astype(np.float64))
            after = {buf: eng.read_buffer_np(B.bufs[buf], n) for buf in out_bufs}
            for name, buf, coff, ref, tol in rows:
                ch = slice(coff, coff + ref.shape[-1])
                got = after[buf]
                res = R.check_live(got[..., ch], dirty[buf][..., ch], ref, tol, k, host=host[buf][..., ch] if same and inputs_same else None)
                print(f"conv count {c.id} [{name}] {form} n={n} n_live={k}: worst error / tolerance {res['ratio']:.3f} at {res['where']}, "
                      f"dirty {res['dirty']:.1f}, past {res['past']}, same bits {res['host']}")
                if live:
                    assert res["dirty"] > 1.0, f"{c.id} [{name}] n_live={k}: the dirty tensor is within the tolerance on a live image: a missing store would not show"
                assert res["ratio"] <= 1.0, f"{c.id} [{name}] n_live={k}: error is {res['ratio']:.3f} x the derived tolerance at (image, y, x, channel) {res['where']}"
                if reads_count:
                    assert np.array_equal(R.bits(got[live:]), R.bits(dirty[buf][live:])), f"{c.id} [{name}] n_live={k}: rows at and past the count were written"
                if same:
                    assert inputs_same, f"{c.id} n_live={k}: the layer's inputs differ from the run without a count"
                    assert res["host"], f"{c.id} [{name}] n_live={k}: same plan as without a count, other bits on the live rows"
                worst = max(worst, res["ratio"])
            if c.tail and "mid" in B.bufs:
                assert not eng.read_buffer_np(B.bufs["mid"], n).any(), f"{c.id} n_live={k}: the fused lead wrote its intermediate"
            # ---- the embeddings
            assert np.isfinite(emb[:live]).all() and not emb[live:].any(), (c.id, k)
            if live:
                dev = np.abs(np.sqrt((emb[:live].astype(np.float64) ** 2).sum(1)) - 1.0).max()
                assert dev <= norm_tol, f"{c.id} n_live={k}: an embedding's norm is {dev:.3e} from 1, bound {norm_tol:.3e}"
        print(f"conv count {c.id} {form}: worst error / tolerance over counts {list(counts)}: {worst:.3f}")
        if form == "c64_block":
            assert {1, 2} <= ipb_seen, f"{c.id}: the block kernel ran {sorted(ipb_seen)} images per block, 1 and 2 not both reached"
        if form == "Patch":
            tpi = R.live_unit(c, head)["tpi"]
            tiles = [k * tpi for k in counts if 0 < k < n]
            assert any(t < 8 for t in tiles) and any(t >= 8 and t % 8 for t in tiles), (c.id, tiles)
    finally:
        eng.close()
