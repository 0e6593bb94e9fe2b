"""CPU checks of the detection post-processing harness (tests/det_ref.py): the builders deliver what they promise, honest fp32
arithmetic stays inside the derived decode tolerance, and each planted variant of decode, NMS and filter changes an expected output of
at least one case that tests/test_gpu_det_kernels.py runs on the device -- the evidence that those assertions would catch a subtly
wrong kernel."""
import numpy as np
import pytest

import det_ref as R
from oracle import nets_oracle as N

HEADS = {"nc80": R.Head(), "nc6": R.Head(nc=6), "reg8": R.Head(reg_max=8)}


def _decode_scene(head, s):
    """fp32 NumPy decode of one scene: boxes [A,4], max logit [A], labels [A]."""
    b, ml, lab = head.decode(s.dfl[None], s.cls[None])
    return b[0], ml[0], lab[0]


@pytest.fixture(scope="module")
def decoded():
    """fp32 decode of every NMS case's scenes, once."""
    head, memo, out = HEADS["nc80"], {}, {}
    for c in R.nms_cases():
        out[c.id] = [memo.setdefault(id(s), _decode_scene(head, s)) for s in c.scenes]
    return out


# ------------------------------------------------------------------------------------------------------------------ exact boxes
@pytest.mark.parametrize("hname", ["nc80", "reg8"])
def test_exact_boxes_decode_exactly_in_fp32(hname):
    head = HEADS[hname]
    rng = np.random.default_rng(3)
    sb = R.SceneBuilder(head)
    for a in rng.permutation(head.A)[:600]:
        a = int(a)
        x, y = head.gx[a] + 0.5, head.gy[a] + 0.5
        l, t, r, b = (int(v) for v in rng.integers(0, head.reg_max, 4))
        sb.place(a, (x - l, y - t, x + r, y + b), 0, 1.0)
    s = sb.scene()
    boxes = R.decode_fp32(head, s.dfl[None])[0]
    for a, e in s.exact.items():
        assert tuple(boxes[a]) == e, (a, boxes[a], e)


def test_nms_case_boxes_are_exact(decoded):
    for c in R.nms_cases():
        for s, (b, ml, lab) in zip(c.scenes, decoded[c.id]):
            idx = np.array(sorted(s.exact), np.int64)
            if len(idx):
                assert np.array_equal(b[idx], np.array([s.exact[a] for a in idx], np.float32)), c.id


# ------------------------------------------------------------------------------------------------------------------ builders
def test_candidate_counts(decoded):
    for c in R.nms_cases():
        for n, (b, ml, lab) in zip(c.n_cand, decoded[c.id]):
            assert int((ml >= N.logit_threshold(c.conf)).sum()) == n, c.id
    assert [c.n_cand for c in R.nms_cases() if c.id == "disjoint_md7"][0] == list(R.DISJOINT_COUNTS)


def test_disjoint_scene_has_zero_iou_and_distinct_logits():
    head = HEADS["nc80"]
    s = R.disjoint_scene(head, 2100, 1)
    b, ml, lab = _decode_scene(head, s)
    assert len(np.unique(ml)) == 2100 and (lab == 0).all()
    for a in range(0, 2100, 7):
        assert not np.delete(N.box_iou_xyxy(b[a], b), a).any()
    keep = N.nms(b, ml, lab, 0.25, 0.5, 4096)
    assert keep.tolist() == s.props["order"]


def test_composite_scene_structures():
    head = HEADS["nc80"]
    s = R.composite_scene(head, 2100, 11)
    b, ml, lab = _decode_scene(head, s)
    order = N.nms(b, ml, lab, 0.25, 0.0, 1)                      # (only to make sure nms runs on it at any threshold)
    assert len(order) == 1
    thr = N.logit_threshold(0.25)
    cand = np.nonzero(ml >= thr)[0]
    ranked = cand[np.lexsort((cand, -ml[cand].astype(np.float64)))]
    rank_of = {int(a): r for r, a in enumerate(ranked)}
    keep = set(N.nms(b, ml, lab, 0.25, 0.5, 4096).tolist())
    seen = set()
    for st in s.props["structures"]:
        seen.add((st["kind"], st["placement"]))
        assert [rank_of[a] for a in st["anchors"]] == st["ranks"]
        tiles, chunks = [r // R.NMS_TILE for r in st["ranks"]], [r // R.NMS_CHUNK for r in st["ranks"]]
        if st["placement"] == "same_tile":
            assert len(set(tiles)) == 1
        elif st["placement"] == "other_tile":
            assert len(set(tiles)) == len(tiles) and len(set(chunks)) == 1
        else:
            assert len(set(chunks)) == len(chunks)
        assert [a in keep for a in st["anchors"]] == st["survive"], st
        bb = b[st["anchors"]]
        iou = [float(N.box_iou_xyxy(bb[0], bb[1:2])[0])] + ([float(N.box_iou_xyxy(bb[1], bb[2:3])[0]), float(N.box_iou_xyxy(bb[0], bb[2:3])[0])] if len(bb) > 2 else [])
        if st["kind"] == "chain":                                # A suppresses B, B overlaps C above the threshold, A does not
            assert iou[0] > 0.5 and iou[1] > 0.5 and iou[2] <= 0.5 and lab[st["anchors"]].tolist() == [lab[st["anchors"][0]]] * 3
        if st["kind"] == "iou_exact":
            assert iou[0] == 0.5
        if st["kind"] == "iou_above":
            assert iou[0] > 0.5
        if st["kind"] == "other_label":
            assert iou[0] == 1.0 and lab[st["anchors"][0]] != lab[st["anchors"][1]]
        if st["kind"] == "zero_area":
            assert np.array_equal(bb[0], bb[1]) and bb[0][0] == bb[0][2] and iou[0] == 0.0
    assert seen == {(k, p) for k in R.STRUCTURES for p in R.PLACEMENTS}
    assert [rank_of[a] for a in N.nms(b, ml, lab, 0.25, 0.5, 4096)] == s.props["kept_ranks"]
    # the max_det values the GPU cases use stop the walk in the middle of a tile, on a tile's last lane, on a chunk's last lane
    for rank, where in ((100, "mid"), (191, "tile"), (1023, "chunk")):
        md = R.max_det_at(s, rank)
        assert rank_of[int(N.nms(b, ml, lab, 0.25, 0.5, md)[-1])] == rank
        assert (rank % 64 == 63) == (where != "mid") and (rank % 1024 == 1023) == (where == "chunk")


def test_tie_threshold_and_zero_scenes():
    head = HEADS["nc80"]
    s = R.tie_scene(head, 1500, 21)
    b, ml, lab = _decode_scene(head, s)
    assert len(np.unique(ml[ml > 0])) == 3 and len(set(ml[s.props["run"]])) == 1
    assert {int(head.level[a]) for a in s.props["run"]} == {0, 1, 2}
    keep = N.nms(b, ml, lab, 0.25, 0.5, 4096).tolist()
    run_kept = [a for a in keep if a in set(s.props["run"])]
    assert run_kept == sorted(s.props["run"])                   # anchor index ascending inside the run
    for w, l in s.props["pairs"]:
        assert w < l and ml[w] == ml[l] and w in keep and l not in keep
    s = R.threshold_scene(head, 0.25, 31)
    b, ml, lab = _decode_scene(head, s)
    thr = N.logit_threshold(0.25)
    assert (ml[s.props["at"]] == thr).all() and (ml[s.props["below"]] < thr).all()
    assert (np.nextafter(ml[s.props["below"]], np.float32(np.inf)) == thr).all()
    keep = set(N.nms(b, ml, lab, 0.25, 0.5, 4096).tolist())
    assert set(s.props["at"]) <= keep and not set(s.props["below"]) & keep
    s = R.zero_scene(head, 41)
    b, ml, lab = _decode_scene(head, s)
    z = np.nonzero(ml == 0)[0]
    assert len(z) == 166 and 60 < int(np.signbit(ml[z]).sum()) < 100
    for conf in (0.5, 0.25):
        keep = N.nms(b, ml, lab, conf, 0.5, 4096).tolist()
        kz = [a for a in keep if ml[a] == 0]
        assert kz == sorted(kz)                                  # the two zeros tie: index order, whatever the sign
        signs = set()
        for w, l, sg in s.props["pairs"]:
            assert w in keep and l not in keep and bool(np.signbit(ml[w])) == (sg < 0) and np.signbit(ml[w]) != np.signbit(ml[l])
            signs.add(sg)
        assert signs == {-1, 1}                                  # both index orders of the (-0.0, +0.0) pair


# ------------------------------------------------------------------------------------------------------------------ decode tolerance
@pytest.mark.parametrize("hname", sorted(HEADS))
def test_fp32_decode_inside_tolerance_and_planted_bugs_outside(hname):
    head = HEADS[hname]
    for batch, seed in ((1, 1), (3, 2)):
        dfl, cls, props = R.decode_inputs(head, batch, seed)
        ref = head.decode(dfl, cls, np.float64)[0]
        for fast in (False, True):
            tol = R.decode_tolerance(head, dfl, ref, fast)
            err = np.abs(R.decode_fp32(head, dfl).astype(np.float64) - ref)
            assert (err <= tol).all(), float((err / tol).max())
            assert tol.max() < 0.05                              # far below the half stride the smallest decode bug moves a corner by
            for bug in R.DECODE_BUGS:
                bad = np.abs(R.decode_fp32(head, dfl, bug).astype(np.float64) - ref) > tol
                assert bad.any(), bug
                if bug == "neighbour_stride":                    # wrong only at the first anchor of levels 1 and 2: the edge anchors catch it
                    hit = np.nonzero(bad.any(-1).any(0))[0].tolist()
                    assert hit and set(hit) <= set(props["edge"]), hit
        lab = head.decode(dfl, cls)[2]
        for (b, a), j in props["ties"].items():
            assert lab[b, a] == j and (cls[b, a] == cls[b, a].max()).sum() == 2


def test_exact_scene_decode_inside_tolerance():
    head = HEADS["nc80"]
    dfl, cls = R.stack(R.nms_cases()[0].scenes)
    ref = head.decode(dfl, cls, np.float64)[0]
    for fast in (False, True):
        assert (np.abs(R.decode_fp32(head, dfl).astype(np.float64) - ref) <= R.decode_tolerance(head, dfl, ref, fast)).all()


# ------------------------------------------------------------------------------------------------------------------ planted NMS variants
def _outputs(dec, c, variant):
    return [R.nms_variant(b, ml, lab, c.conf, c.iou, c.max_det, variant).tolist() for b, ml, lab in dec]


def test_nms_restatement_is_the_oracle(decoded):
    for c in R.nms_cases():
        if c.id.startswith("disjoint") and c.max_det not in (7, 1024):
            continue
        for b, ml, lab in decoded[c.id]:
            assert R.nms_variant(b, ml, lab, c.conf, c.iou, c.max_det).tolist() == N.nms(b, ml, lab, c.conf, c.iou, c.max_det).tolist(), c.id


@pytest.mark.parametrize("variant", R.NMS_VARIANTS)
def test_planted_nms_variant_changes_a_gpu_case(decoded, variant):
    """For each deviation: at least one case of the GPU list expects something else than the deviating NMS produces."""
    flipped = [c.id for c in R.nms_cases() if not c.id.startswith("disjoint") and _outputs(decoded[c.id], c, variant) != _outputs(decoded[c.id], c, None)]
    print(variant, "changes", flipped)
    assert flipped
    expect = {"iou_ge": "composite_md1024", "thr_gt": "threshold_conf0.25", "tie_index_desc": "ties_md300", "labels_ignored": "composite_md1024",
              "suppressed_suppress": "composite_md1024", "max_det_plus_one": "composite_md300", "neg_zero_below": "zeros_conf0.5"}
    assert expect[variant] in flipped
    if variant == "neg_zero_below":                              # only the signed-zero cases tell this one
        assert all(f.startswith("zeros") for f in flipped)


def test_max_det_off_by_one_changes_the_disjoint_grid(decoded):
    c = [c for c in R.nms_cases() if c.id == "disjoint_md64"][0]
    assert _outputs(decoded[c.id], c, "max_det_plus_one") != _outputs(decoded[c.id], c, None)


# ------------------------------------------------------------------------------------------------------------------ filter
def test_filter_ref_and_planted_variants():
    seen_over, seen_cap = False, set()
    flips = {v: 0 for v in R.FILTER_VARIANTS}
    for c in R.filter_cases():
        cap = R.filter_cap(c)
        ref = R.filter_ref(c.num_dets, c.boxes, c.scores, c.labels, c.min_conf, c.mask, cap)
        B, md = c.scores.shape
        # the ten-line loop of deepsort_tracker.py:88-101, frame by frame
        rows = []
        for f in range(B):
            for i in range(min(int(c.num_dets[f]), md)):
                cid = int(c.labels[f, i])
                tracked = 0 <= cid < 128 and (c.mask[cid // 64] >> (cid % 64)) & 1
                if c.scores[f, i] >= np.float32(c.min_conf) and tracked:
                    rows.append((f, i))
        assert ref["total"].tolist() == [min(len(rows), cap), len(rows)]
        assert ref["frame_of"].tolist() == [f for f, _ in rows[:cap]]
        assert np.array_equal(ref["conf"], np.array([c.scores[f, i] for f, i in rows[:cap]], np.float32))
        assert int(ref["frame_n"].sum()) == len(rows) and ref["frame_d0"].tolist() == np.concatenate([[0], np.cumsum(ref["frame_n"])[:-1]]).tolist()
        seen_over |= bool((c.num_dets > md).any())
        seen_cap.add(np.sign(len(rows) - cap))
        kept_labels = {int(v) for v in ref["cls"]}
        assert kept_labels <= ({0, 63, 127} if c.mask == R.MASK_A else {64})
        if len(rows) > 50 and cap == len(rows):
            assert kept_labels == ({0, 63, 127} if c.mask == R.MASK_A else {64})
            assert (ref["conf"] == np.float32(c.min_conf)).any()
        for v in R.FILTER_VARIANTS:
            bad = R.filter_ref(c.num_dets, c.boxes, c.scores, c.labels, c.min_conf, c.mask, cap, v)
            flips[v] += any(not np.array_equal(bad[k], ref[k]) for k in ref)
    assert seen_over and seen_cap >= {0, 1}                  # cap equal to the total and below it (above it: a group that passes nothing)
    assert all(n > 0 for n in flips.values()), flips
    assert {c.scores.shape[0] for c in R.filter_cases()} >= {1, 64, 65, 512}


def test_det_filter_refuses_bad_arguments_on_the_host(lib):
    """aic_det_filter checks its arguments before it touches a device: the refusals are host-side and need no GPU."""
    z = np.zeros(8, np.int32)
    f = np.zeros(32, np.float32)
    m = np.zeros(2, np.uint64)
    P = lib.ptr
    good = [0, P(z), P(f), P(f), P(z), 1, 4, 0.5, P(m), 4, P(z), P(z), P(z), P(z), P(f), P(f), P(f), P(z), P(z)]
    for pos, val in ((5, 0), (6, 0), (9, 0), (5, -1), (1, None), (8, None), (13, None), (18, None)):
        args = list(good)
        args[pos] = val
        with pytest.raises(lib.AicError) as e:
            lib.call("aic_det_filter", *args)
        assert e.value.code == lib.ERR_INVALID, (pos, e.value)
