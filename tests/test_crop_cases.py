"""CPU proof that the cases of tests/crop_cases.py can fail: per output shape they reach every load alignment, the clamped right tap,
the 2x2 path, the last byte of the bank, empty boxes and every frame (asserted as conditions, from the oracle's own arithmetic), and
the expectation of each wrong kernel one can name differs from the oracle's in at least one element.  No GPU."""
import numpy as np
import pytest

import crop_cases as K

# (shape, bank) of every case the device tests run: the crop kernel's and the fused stem's
CASES = [(s, K.BANK_OF[s]) for s in K.CROP_SHAPES] + [(s, b) for s, b in K.STEM_BANK_OF.items() if K.BANK_OF[s] != b]
ids = lambda v: v if isinstance(v, str) else f"{v[0][0]}x{v[0][1]}_on_{v[1]}"      # noqa: E731


def test_banks_start_rows_and_frames_at_every_alignment():
    assert set(K.STEM_SHAPES) <= set(K.STEM_BANK_OF) and all(K.BANK_OF[s] == K.STEM_BANK_OF[s] for s in K.STEM_SHAPES)
    for name, (h, w) in K.BANKS.items():
        f = K.bank(name)
        assert f.shape == (K.N_FRAMES, h, w, 3) and f.dtype == np.uint8
        assert (w * 3) % 4 == 1, "rows must start at every byte alignment"
        assert len(np.unique(f)) == 256
    assert (45 * 139 * 3) % 4 == 1                          # ... and so must the frames of the 45-row bank
    assert not np.array_equal(K.bank("45x139")[0], K.bank("45x139")[1])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_cases_reach_every_path(case):
    shape, bank = case
    boxes, fo = K.boxes_for(shape, bank)
    assert boxes.shape == (22, 4) and boxes.dtype == np.float32 and fo.shape == (22,)
    assert set(fo.tolist()) == set(range(K.N_FRAMES)) and fo.tolist() != sorted(fo.tolist())
    r = K.stats(shape, bank)
    print(case, {k: (sorted(v) if isinstance(v, set) else v) for k, v in r.items()})
    assert r["align"] == {0, 1, 2, 3}
    assert len(r["clamped"]) >= 1
    assert len(r["interp_last"]) >= 1
    assert len(r["invalid"]) >= 3
    assert r["frames"] == set(range(K.N_FRAMES))
    assert len(r["enlarged"]) >= 1
    if K.area2_fits(shape, bank):
        assert len(r["area2"]) >= 2 and len(r["area2_last"]) >= 1
    else:                                                   # twice the crop is larger than the frame: the box was clamped, every crop interpolates
        assert not r["area2"] and len(r["interp_last"]) >= 2
    # the empty boxes sit among live ones: a dead-crop test with n_live = n - 1 cuts off a valid crop
    assert 21 not in r["invalid"] and 0 not in r["invalid"]


def test_area2_is_pinned_where_the_stem_runs():
    assert all(K.area2_fits(s, b) for s, b in K.STEM_BANK_OF.items()) and K.area2_fits((20, 24))
    assert [s for s in K.CROP_SHAPES if not K.area2_fits(s)] == [(8, 240), (128, 64)]


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_flat_restatement_equals_the_oracle(case):
    """resample_flat (which the mutants are made from) is the oracle when nothing is mutated."""
    shape, bank = case
    boxes, fo = K.boxes_for(shape, bank)
    frames = K.bank(bank)
    ref, rv = K.nchw(frames, boxes, fo, shape)
    for tag in ("trunc",) + K.EQUIVALENT:
        got, gv = K.nchw(frames, boxes, fo, shape, mut=tag)          # ("trunc" is no mutant name: the restatement as it is)
        assert np.array_equal(gv, rv) and np.array_equal(got, ref), (shape, tag)
    exp, ev = K.expected(shape, bank_name=bank)
    assert np.array_equal(exp, ref) and np.array_equal(ev, rv)
    assert exp[ev == 0].any() == False and all(exp[i].any() for i in np.flatnonzero(ev))     # noqa: E712


def test_layouts():
    shape = (16, 64)
    x, v = K.expected(shape)
    for mode, dt in K.MODES:
        t, tv = K.expected(shape, mode, dt)
        assert np.array_equal(tv, v)
        if mode == 0:
            assert t.dtype == np.float32 and t.shape == (22, 3, 16, 64)
            continue
        lanes = 8 if mode == 1 else 4
        want = np.float16 if dt == "fp16" else np.float32
        assert t.shape == (22, 16, 64, lanes) and t.dtype == want
        assert not t[..., 3:].any()
        assert np.array_equal(t[..., :3], x.transpose(0, 2, 3, 1).astype(want))
    # rounding to float16 is not the identity on these values: a kernel that stored another rounding would differ
    assert not np.array_equal(x.astype(np.float16).astype(np.float32), x)
    # no expected element looks like the 0xFF prefill of the test entry (NaN as a float of either width)
    for mode, dt in K.MODES:
        assert not np.isnan(K.expected(shape, mode, dt)[0]).any()


def test_dead_crops():
    shape = (16, 64)
    full, fv = K.expected(shape)
    for n_live in (0, 1, 21, 22, 27):
        t, v = K.expected(shape, n_live=n_live)
        k = min(n_live, 22)
        assert np.array_equal(t[:k], full[:k]) and np.array_equal(v[:k], fv[:k])
        assert not t[k:].any() and not v[k:].any()


def _applicable(case, mut):
    """From the shapes alone: a mutant that tests one dimension of the 2x2 condition needs a box twice the crop in that dimension.  No box
    of the 70 x 139 bank is 256 high (128 x 64: area2_w applies -- box 1 is clamped to 128 x 68 --, area2_h does not) and none of the
    45 x 139 bank is 480 wide (8 x 240: box 1 is clamped to 136 x 16 and 16 == 2 * 8, so area2_h applies, area2_w does not)."""
    shape, (fh, fw) = case[0], K.BANKS[case[1]]
    return {"area2_w": 2 * shape[1] <= fw, "area2_h": 2 * shape[0] <= fh}.get(mut, True)


@pytest.mark.parametrize("case,mut", [(c, m) for c in CASES for m in K.MUTANTS if _applicable(c, m)], ids=ids)
def test_every_mutant_changes_some_element(case, mut):
    shape, bank = case
    if mut == "dead":
        ref, rv = K.expected(shape, n_live=21, bank_name=bank)
        got, gv = K.expected(shape, n_live=21, mut="dead", bank_name=bank)
    else:
        ref, rv = K.expected(shape, bank_name=bank)
        got, gv = K.expected(shape, mut=mut, bank_name=bank)
    changed = [i for i in range(len(ref)) if not np.array_equal(ref[i], got[i]) or rv[i] != gv[i]]
    print(case, mut, "changes crops", changed)
    assert changed, (case, mut)
    if mut == "right_tap":                                  # ... and it is the enlarged crops that see it: the last columns' fraction is not 0
        assert set(changed) <= set(K.stats(shape, bank)["clamped"])


def test_mutants_survive_the_fp16_layouts():
    """The stem and the NHWC layouts hold float16: a mutant must still differ after that rounding (one u8 step is 1 / (255 * 0.23) = 0.017,
    float16 resolves 0.002 below 4)."""
    for shape, bank in K.STEM_BANK_OF.items():
        ref = K.expected(shape, 2, "fp16", bank_name=bank)[0]
        for mut in K.MUTANTS:
            if mut != "dead":
                assert not np.array_equal(K.expected(shape, 2, "fp16", mut=mut, bank_name=bank)[0], ref), (shape, bank, mut)
