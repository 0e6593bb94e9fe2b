"""The detect head's in-epilogue decode (tail_1x1 in csrc/conv_common.hpp), anchor by anchor: fp16 engines store the class branch's
maximum logit + first arg-max and the box branch's DFL-decoded box from inside the 1x1 tail of the detect branches, and decode_kernel
skips those levels -- what NMS, the filter and every tracker read is what that epilogue computed.

One engine per case of tests/head_ref.py (planted ties, all-negative rows under a channel mask, exact and all-equal boxes, wide spans;
non-square maps), one process, no switches.  Per case, on one handle:
  A = aic_yolo_decode            the path under test; straight after it the levels' fp32 logits buffers are read back: a branch that
                                 decoded in place has left its buffer all zeros (the logits were never written), a fallback holds its logits
  raw = aic_yolo_head            the same leads on the same plan, the plain tail storing the fp32 logits
  B = aic_yolo_postprocess(raw)  the engine's own decode_kernel on those logits
and then: A's max logit is raw's row maximum bit for bit, A's label the first arg-max (and a class); A == B in all three arrays; A's
boxes within det_ref.decode_tolerance (exp2 form) of the fp64 decode of raw's DFL logits, element by element; the exact and all-equal
plants equal their closed form at every anchor.  The builders' floors (head_ref's docstring) are asserted on raw, so a case cannot pass
by having lost its ties or its spans on the way through fp16 activations.

Which kernel ran: every lead's plan is asked of the library (aic_model_conv_plan) and compared with the case's table entry; cases that
need a large tile run at the SMALLEST n at which the planner reports it (searched with conv_plan, not copied from the planner), on P <= 5
distinct images tiled to n -- all n outputs are compared, equal images must give equal outputs.  The last test asserts that all ten
outcomes of plan_tail have carried a decoding tail."""
import functools

import numpy as np
import pytest

import head_ref as H
from conftest import pkg

pytestmark = pytest.mark.gpu

FS, IS = np.float32(-12345.0), np.int32(-777)                   # sentinels: an output element that still holds one was not written
COVERED = {k: set() for k in H.OUTCOMES}                        # outcome -> branches whose tail decoded in place on it
RAN = []


def _stop_on_device_error(fn):
    """A HIP error ends the session: nothing more is started on a device that has just faulted."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except pkg("_lib").AicError as e:
            pytest.exit(f"{fn.__name__}: the library reported an error, stopping: {e}", returncode=1)
    return wrapped


def _matches(plan, outcome):
    want = dict(H.OUTCOMES[outcome], kind="conv+tail")
    return all(plan.get(k) == v for k, v in want.items())


def _smallest_n(path, c, B):
    """The smallest n <= c.n at which the planner reports the case's wanted outcome for its lead (a handle that only answers)."""
    if not c.want:
        return c.n
    br, l, outcome = c.want
    eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=c.n, warm_up=False)
    try:
        for n in range(1, c.n + 1):
            if _matches(eng.conv_plan(B.ops[br, l][0], n), outcome):
                return n
        pytest.fail(f"{c.id}: no n <= {c.n} at which {br}{l}'s lead is planned as {outcome}: at {c.n} the engine plans {eng.conv_plan(B.ops[br, l][0], c.n)}")
    finally:
        eng.close()


def _periodic(a, P, what):
    for j in range(P):
        assert np.array_equal(a[j::P], np.broadcast_to(a[j], a[j::P].shape)), f"{what}: equal images gave different outputs (image {j} of {P})"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("c", H.CASES, ids=[c.id for c in H.CASES])
@_stop_on_device_error
def test_head_tail_decodes_anchor_by_anchor(gpu, tmp_path, c):
    B = H.build(c)
    head, P = B.head, c.P
    path = str(tmp_path / f"{c.id}.aicw")
    H.ef.write_engine(path, B.g)
    n = _smallest_n(path, c, B)
    x = H.tiled(H.base_images(c), n)
    eng = pkg("hip_engine").HipEngine(path, dtype="fp16", max_items=n, warm_up=False)
    try:
        assert eng.n_anchors == head.A and eng.out_dim == c.nc
        # ---- 1. the path under test, 2. straight after it: which branches left their logits unwritten
        Ab, Am, Al = eng.yolo_decode_np(x)
        held = {k: eng.read_buffer_np(buf, n) for k, buf in B.bufs.items()}
        # ---- 3. the raw logits of the same leads, 4. the engine's decode_kernel on them
        dfl, cls = eng.yolo_head_np(x)
        r = eng.yolo_postprocess_np(dfl, cls, sentinel=(FS, IS))
        # ---- 6. which kernel ran
        plans, partial = [], False
        for l, (_, hh, ww) in enumerate(head.levels):
            for br, outcome in zip(("box", "cls"), c.leads[l]):
                lead, one = B.ops[br, l]
                plan, p1 = eng.conv_plan(lead, n), eng.conv_plan(one, n)
                logits = held[br, l].reshape(n, hh * ww, -1)
                mine = (dfl if br == "box" else cls)[:, head.a0[l]:head.a0[l + 1]]
                if outcome is None:                                  # no tail: the 1x1 runs on its own and decode_kernel reads its logits
                    assert plan["kind"] == "conv" and p1["kind"] == "conv", (c.id, br, l, plan, p1)
                    assert logits.any() and np.array_equal(logits, mine), f"{c.id} {br}{l}: a branch without a tail did not leave its logits"
                    plans.append(f"{br}{l}: {plan['form']} + 1x1 {p1['form']}")
                    continue
                assert _matches(plan, outcome), f"{c.id} {br}{l} n={n}: expected {H.OUTCOMES[outcome]} with a tail, the engine plans {plan}"
                assert p1["kind"] == "covered" and p1["first_op"] == lead, (c.id, br, l, p1)
                assert not logits.any(), f"{c.id} {br}{l}: the tail wrote its logits: it did not decode in place"
                assert mine.any()
                COVERED[outcome].add(br)
                M = n * hh * ww
                partial |= bool(hh % plan["th"] or ww % plan["tw"]) if plan["form"] in ("Patch", "PmPatch") else bool(M % (16 * plan["mt"] * plan["wm"]))
                plans.append(f"{br}{l}: {outcome} M={M}")
        print(f"head tails {c.id} n={n}: " + ", ".join(plans))
        assert partial, f"{c.id} n={n}: no level ends inside a pixel tile"
        if c.want and n > 1:                                         # ... and n is the smallest such
            br, l, outcome = c.want
            assert not _matches(eng.conv_plan(B.ops[br, l][0], n - 1), outcome)
        # ---- 7. equal images, equal outputs; from here on the P distinct ones stand for all n
        for name, a in (("boxes", Ab), ("max logit", Am), ("labels", Al), ("raw dfl", dfl), ("raw cls", cls)):
            _periodic(a, P, f"{c.id} {name}")
        # ---- the builders' floors, on the device's own logits
        for l, (top, rest, same) in H.pair_counts(c, head, cls[:P]).items():
            print(f"head tails {c.id} level {l} pair {c.pairs[l][:2]}: strict maximum at {top} anchors, not at {rest}")
            assert same, f"{c.id} level {l}: the planted pair's logits are not equal"
            assert top >= H.PAIR_FLOOR and rest >= H.PAIR_FLOOR, (c.id, l, top, rest)
        if c.shift:
            assert cls.max() < H.NEG_BOUND, (c.id, cls.max())
        if c.box == "spans":
            sp = H.spans(head, dfl[:P])
            assert (sp >= H.SPAN_WIDE).mean() >= H.SPAN_SHARE and sp.max() <= H.SPAN_MAX, (c.id, (sp >= H.SPAN_WIDE).mean(), sp.max())
        # ---- 5. the values
        for k in ("boxes", "max_logit", "labels"):
            assert not (r[k] == (IS if k == "labels" else FS)).any(), f"{c.id}: decode_kernel left {k} unwritten"
        ml, lab = H.classify(cls, c.cls_width)
        assert np.array_equal(_bits(Am), _bits(ml)), f"{c.id}: max logit is not the row maximum of the raw logits"
        bad = np.argwhere(Al != lab)
        assert not len(bad), f"{c.id}: {len(bad)} labels are not the first arg-max, first at (image, anchor) {bad[0]}: {Al[tuple(bad[0])]} for {lab[tuple(bad[0])]}"
        assert (Al >= 0).all() and (Al < c.nc).all(), f"{c.id}: a label is no class"
        assert np.array_equal(_bits(Ab), _bits(r["boxes"])), f"{c.id}: boxes differ from decode_kernel's on the same logits"
        assert np.array_equal(_bits(Am), _bits(r["max_logit"])) and np.array_equal(Al, r["labels"]), f"{c.id}: classes differ from decode_kernel's"
        ref, tol = H.box_reference(head, dfl[:P])
        ratio = np.abs(Ab[:P].astype(np.float64) - ref) / tol
        where = np.unravel_index(int(ratio.argmax()), ratio.shape)
        print(f"head tails {c.id} n={n}: worst box error / tolerance {ratio.max():.3f} at (image, anchor, corner) {tuple(int(v) for v in where)}")
        assert ratio.max() <= 1.0, f"{c.id}: box error is {ratio.max():.3f} x the derived tolerance at (image, anchor, corner) {where}"
        if c.box != "spans":
            assert np.array_equal(Ab, np.broadcast_to(H.exact_boxes(c, head), Ab.shape)), f"{c.id}: the {c.box} plant does not decode to its closed form"
        RAN.append(c.id)
    finally:
        eng.close()


def test_every_plan_tail_outcome_carried_a_decoding_tail(gpu):
    missing = [c.id for c in H.CASES if c.id not in RAN]
    assert not missing, f"cases that did not run to their end (the coverage is over the whole table): {missing}"
    short = {k: sorted(H.NEEDS[k] - v) for k, v in COVERED.items() if H.NEEDS[k] - v}
    print("plan_tail outcomes with a decoding tail: " + ", ".join(f"{k} ({' + '.join(sorted(v))})" for k, v in COVERED.items()))
    assert not short, f"plan_tail outcomes that carried no decoding tail: {short}"
