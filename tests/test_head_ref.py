"""CPU checks of the detect-head harness (tests/head_ref.py): every case's graph, run through the fp32 oracle on the case's images,
delivers what its builder promises -- with ORACLE_MARGIN times the floors that tests/test_gpu_head_tails.py asserts again on the device's
own raw logits -- and each planted variant of the epilogue's rules changes an expected output of at least one case by more than the
GPU test tolerates: the evidence that those assertions would catch a subtly wrong tail_1x1."""
import numpy as np
import pytest

import head_ref as H

IDS = [c.id for c in H.CASES]


@pytest.fixture(scope="module")
def heads():
    """Oracle raw head (dfl, cls) of every case's distinct images, once."""
    return {c.id: H.oracle_head(c) for c in H.CASES}


def test_case_table_is_well_formed():
    assert len(set(IDS)) == len(IDS)
    for c in H.CASES:
        hh, ww = c.in_hw
        assert hh % 32 == 0 and ww % 32 == 0 and hh != ww and 1 <= c.P <= 8 and c.P <= c.n, c.id
        assert c.want or c.n == c.P, c.id                      # large n: P <= 5 distinct images tiled; small n: all distinct
        assert not c.want or c.P <= 5, c.id
        assert c.box in ("exact", "equal", "spans") and len(c.leads) == len(c.pairs) == 3, c.id
        for box, cls in c.leads:
            assert H.WIDTH_OF[box] == 64 and (cls is None) == (not c.cls_tail) and (cls is None or H.WIDTH_OF[cls] == c.cls_width), c.id
        if c.want:
            br, l, outcome = c.want
            assert c.leads[l][br == "cls"] == outcome, c.id
        assert not c.shift or c.nc in (8, 24, 40, 56), c.id
    assert {c.nc for c in H.CASES} >= {3, 8, 24, 40, 56, 64, 72, 80}
    for e in H.EXACT_BINS:
        assert len(set(e)) == 4 and {0, 15} <= set(e) and any(1 <= k <= 7 for k in e) and any(8 <= k <= 14 for k in e)
    for plant in ("exact", "equal"):                             # at one small n and at one large-tile n each
        assert {bool(c.want) for c in H.CASES if c.box == plant} == {True, False}, plant


def test_table_covers_every_plan_tail_outcome_with_a_decoding_tail():
    seen = {k: set() for k in H.OUTCOMES}
    for c in H.CASES:
        for box, cls in c.leads:
            seen[box].add("box")
            if cls:
                seen[cls].add("cls")
    short = {k: sorted(H.NEEDS[k] - v) for k, v in seen.items() if H.NEEDS[k] - v}
    assert not short, f"plan_tail outcomes without a decoding tail in the table: {short}"
    # the 64-channel outcomes reduce classes with nc <= 64 -- the only way they can -- and under a mask (nc < 64) at least once each kind of tile
    assert {c.nc for c in H.CASES if c.cls_tail and c.cls_width == 64} >= {8, 24, 40, 56, 64}


def test_pair_kinds_are_covered():
    """Same lane, across q-lanes of one 16-channel tile, across channel tiles, (nc - 2, nc - 1), (2, nc - 1); for nc = 80 a pair inside
    the odd fifth tile and one that reaches into it; every level carries a pair somewhere."""
    kinds, levels = set(), set()
    for c in H.CASES:
        for l, p in enumerate(c.pairs):
            if not p:
                continue
            j1, j2, _ = p
            levels.add(l)
            q1, q2 = int(H.lane_of(j1)), int(H.lane_of(j2))
            if j1 // 4 == j2 // 4:
                kinds.add("one_group")
            if j1 // 16 == j2 // 16 and q1 != q2:
                kinds.add("across_lanes_one_tile")
            if j1 // 16 != j2 // 16:
                kinds.add("across_tiles")
            if (j1, j2) == (c.nc - 2, c.nc - 1):
                kinds.add(f"last_two_nc{c.nc}")
            if (j1, j2) == (2, c.nc - 1):
                kinds.add("two_and_last")
            if c.nc == 80 and j1 >= 64:
                kinds.add("inside_fifth")
            if c.nc == 80 and j1 < 64 <= j2:
                kinds.add("into_fifth")
    assert kinds >= {"one_group", "across_lanes_one_tile", "across_tiles", "last_two_nc80", "last_two_nc64", "two_and_last", "inside_fifth",
                     "into_fifth"}, kinds
    assert levels == {0, 1, 2}


@pytest.mark.parametrize("c", H.CASES, ids=IDS)
def test_builder_promises_on_the_oracle(heads, c):
    B = H.build(c)
    head = B.head
    dfl, cls = heads[c.id]
    assert dfl.shape == (c.P, head.A, 64) and cls.shape == (c.P, head.A, c.nc)
    assert all(w != h for _, h, w in head.levels)
    # planted weights are fp16 numbers
    for (br, l), (_, one) in B.ops.items():
        w = B.g.weights[B.g.ops[one][15]][0]
        if br == "box" or c.pairs[l]:
            rows = slice(None) if br == "box" else list(c.pairs[l][:2])
            assert np.array_equal(w[rows], w[rows].astype(np.float16).astype(np.float32)), (c.id, br, l)
    # pairs: ORACLE_MARGIN x the floor on both sides
    floor = H.ORACLE_MARGIN * H.PAIR_FLOOR
    counts = H.pair_counts(c, head, cls)
    assert sorted(counts) == [l for l in range(3) if c.pairs[l]]
    for l, (top, rest, _) in counts.items():
        print(f"{c.id} level {l} pair {c.pairs[l][:2]}: strict maximum at {top} anchors, not at {rest}")
        assert top >= floor and rest >= floor, (c.id, l, top, rest)
    if c.shift:
        assert cls.max() < H.NEG_BOUND - 10, (c.id, cls.max())
    sp = H.spans(head, dfl)
    if c.box == "spans":
        share = float((sp >= H.SPAN_WIDE).mean())
        print(f"{c.id}: {share:.3f} of the rows span >= {H.SPAN_WIDE}, widest {sp.max():.2f}")
        assert share >= 1.5 * H.SPAN_SHARE and sp.max() <= H.SPAN_MAX_ORACLE, (c.id, share, sp.max())
        for l in range(3):                                       # ... per level too, and the weight term moves every row
            s = sp[:, head.a0[l]:head.a0[l + 1]]
            assert (s >= H.SPAN_WIDE).mean() >= H.SPAN_SHARE and s.std() > 0.05, (c.id, l)
    else:
        boxes = H.decode_boxes(head, dfl)
        assert np.array_equal(boxes, np.broadcast_to(H.exact_boxes(c, head), boxes.shape)), c.id
        assert np.array_equal(sp, np.full_like(sp, 40.0 if c.box == "exact" else 0.0))


@pytest.mark.parametrize("c", H.CASES, ids=IDS)
def test_references_agree_with_the_oracles_decode(heads, c):
    """classify / decode_boxes without a bug are the specification: nets_oracle.decode_head on the same logits."""
    head = H.head_of(c)
    dfl, cls = heads[c.id]
    ref, tol = H.box_reference(head, dfl)
    b32, ml, lab = head.decode(dfl, cls)
    gm, gl = H.classify(cls, c.cls_width)
    assert np.array_equal(gm, ml) and np.array_equal(gl, lab) and (gl < c.nc).all()
    assert (np.abs(H.decode_boxes(head, dfl).astype(np.float64) - ref) <= tol).all()
    assert (np.abs(b32.astype(np.float64) - ref) <= tol).all()


@pytest.mark.parametrize("bug", H.CLS_BUGS)
def test_class_rule_variants_change_a_label(heads, bug):
    caught = []
    for c in H.CASES:
        _, cls = heads[c.id]
        ml, lab = H.classify(cls, c.cls_width)
        bm, bl = H.classify(cls, c.cls_width, bug)
        if not (np.array_equal(bl, lab) and np.array_equal(bm, ml)):
            caught.append(c.id)
    print(f"{bug}: changes max logit or label in {caught}")
    assert caught, bug
    if bug == "mask_dropped":                                    # ... as a label that is no class, in every case with all logits negative
        assert set(caught) >= {c.id for c in H.CASES if c.shift}
    if bug == "last_max":                                        # ... exactly in the cases with a planted pair (all of them)
        assert set(caught) == {c.id for c in H.CASES if any(c.pairs)}


@pytest.mark.parametrize("bug", H.BOX_BUGS)
def test_box_rule_variants_leave_the_tolerance(heads, bug):
    caught = []
    for c in H.CASES:
        head = H.head_of(c)
        dfl, _ = heads[c.id]
        ref, tol = H.box_reference(head, dfl)
        if (np.abs(H.decode_boxes(head, dfl, bug).astype(np.float64) - ref) > tol).any():
            caught.append(c.id)
    print(f"{bug}: leaves the tolerance in {caught}")
    assert caught, bug
