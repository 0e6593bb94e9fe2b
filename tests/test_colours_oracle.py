"""tests/colours_oracle.py on its own (no library, no GPU): the pixel rule on the palette and at every threshold, the exactness of the
device's reciprocal division, the part geometry, the cover limit, a planted scene, the life cycle, and the saturation of the sample
counters.  It also shows that the seeded cases of tests/colours_cases.py reach every branch the GPU suite relies on."""
import numpy as np
import pytest

import colours_cases as CC
import colours_oracle as CO


def name(b, g, r):
    return CO.NAMES[CO.classify_pixel(b, g, r)]


def test_the_palette_by_name():
    for want, pixels in CC.PALETTE.items():
        for p in pixels:
            assert name(*p) == want, (want, p, name(*p))
    # the worked hue cases: pale pink is a RED hue made PINK by its low saturation; purple and magenta sit at hq = 1280 exactly
    mx, sat, hq = (int(v) for v in CO.features(np.array([203, 192, 255], np.uint8)))
    assert (mx, sat) == (255, 63) and hq == ((192 - 203) * 256 // 63) % 1536 == 1491 and name(203, 192, 255) == "pink"
    for p in ((128, 0, 128), (255, 0, 255)):
        assert int(CO.features(np.array(p, np.uint8))[2]) == 1280 and name(*p) == "purple"
    assert len(CO.NAMES) == 12 and [CO.NAMES.index(n) for n in ("black", "gray", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple",
                                                                "pink", "brown")] == list(range(12))


def test_the_reciprocal_division_is_exact_over_the_whole_domain():
    """Every (numerator, d) the hue rule can produce -- 511 differences times 256, 255 divisors -- and every saturation quotient."""
    for d in range(1, 256):
        assert CO.recip(d) < 1 << 32
        for diff in range(-255, 256):
            assert CO.floor_div_device(diff * 256, d) == (diff * 256) // d, (diff, d)
    for mx in range(1, 256):
        for d in range(mx + 1):
            assert CO.recip_div(d * 256, mx) == d * 256 // mx


def test_every_threshold_at_its_value_and_one_beside_it():
    # achromatic: mx 39 / 40, 71 / 72, 199 / 200
    assert [name(v, v, v) for v in (39, 40, 71, 72, 199, 200)] == ["black", "black", "black", "gray", "gray", "white"]
    assert name(39, 0, 0) == "black" and name(40, 0, 0) == "blue"            # below 40 the colour does not count
    # sat 39 / 40 at mx = 200: d = 31 gives 39, d = 32 gives 40
    assert 31 * 256 // 200 == 39 and 32 * 256 // 200 == 40
    assert name(169, 169, 200) == "white" and name(168, 168, 200) == "pink"
    # every hue bound, through pixels of the threshold set with exactly that hue
    ts = CC.threshold_set()
    mx, sat, hq = CO.features(ts)
    chroma = (mx >= 40) & (sat >= 40) & (mx == 255) & (sat >= 128)           # (no override reaches these)
    cls = CO.classify(ts)
    below = {64: "red", 192: "orange", 299: "yellow", 704: "green", 853: "cyan", 1109: "blue", 1300: "purple", 1472: "pink"}
    at = {64: "orange", 192: "yellow", 299: "green", 704: "cyan", 853: "blue", 1109: "purple", 1300: "pink", 1472: "red"}
    for bound in below:
        for h, want in ((bound - 1, below[bound]), (bound, at[bound])):
            hit = chroma & (hq == h)
            assert hit.any(), h
            assert {CO.NAMES[c] for c in cls[hit]} == {want}, (h, want)
    # the three overrides: orange / brown at mx 175 / 176, yellow / brown at 135 / 136, red / pink at sat 127 / 128 and mx 175 / 176
    assert name(0, 88, 176) == "orange" and name(0, 87, 175) == "brown"
    assert name(0, 136, 136) == "yellow" and name(0, 135, 135) == "brown"
    assert (176 - 88) * 256 // 176 == 128 and (176 - 89) * 256 // 176 == 126
    assert name(88, 88, 176) == "red" and name(89, 89, 176) == "pink" and name(89, 89, 175) == "red"
    # ties on the maximum go to r, then g, then b
    assert CO.hue_q(10, 200, 200) == (190 * 256 // 190) % 1536 == 256 and name(10, 200, 200) == "yellow"      # r = g: the r case
    assert CO.hue_q(200, 10, 200) == (-190 * 256 // 190) % 1536 == 1280 and name(200, 10, 200) == "purple"    # r = b: the r case
    assert CO.hue_q(200, 200, 10) == 512 + 190 * 256 // 190 == 768 and name(200, 200, 10) == "cyan"           # g = b: the g case
    # the vector form is the scalar form, on the threshold set and on noise
    px = np.concatenate([ts, np.random.default_rng(1).integers(0, 256, (4096, 3)).astype(np.uint8)])
    assert np.array_equal(CO.classify(px), np.array([CO.classify_pixel(*p) for p in px], np.uint8))
    for m in CC.MX_EDGES:
        assert (mx == m).any()
    for s in CC.SAT_EDGES:
        assert ((sat == s) & (mx >= 40)).any()
    assert set(cls.tolist()) == set(range(12))


def test_part_geometry():
    # defaults on a box of 40 x 100 at (10, 20): inset (39 * 64) >> 8 = 9; torso rows 20 + 19 .. 20 + 49, legs 20 + 54 .. 20 + 88
    r = CC.row(10, 20, 40, 100, 1)
    assert CO.part_of(r, (51, 128), 64) == (19, 39, 40, 69) and CO.part_of(r, (141, 230), 64) == (19, 74, 40, 108)
    # a box half outside the frame: the part comes from the unclipped box, then it is clipped
    o = CO.ColoursOracle((72, 101), min_w=4, min_h=4)
    half = CC.row(-20, 30, 40, 60, 1)
    assert CO.part_of(half, (51, 128), 64) == (-11, 41, 10, 59) and CO.clip(CO.part_of(half, (51, 128), 64), 72, 101) == (0, 41, 10, 59)
    assert CO.clip(CO.part_of(half, (141, 230), 64), 72, 101) == (0, 62, 10, 71)
    frame = CC.texture(np.random.default_rng(2), 72, 101)
    got = o.measure(frame, CC.rows_of(half))
    assert len(got) == 1 and got[0][3] is not None and sum(got[0][3]) <= 256 and got[0][4] is not None
    # 1 x 1: both parts are the pixel itself
    one = CC.row(50, 50, 1, 1, 2)
    assert CO.part_of(one, (51, 128), 64) == CO.part_of(one, (141, 230), 64) == (50, 50, 50, 50)
    o1 = CO.ColoursOracle((72, 101), min_w=1, min_h=1)
    m = o1.measure(frame, CC.rows_of(one))[0]
    assert m[3] == m[4] and sum(m[3]) == 256 and m[3][CO.classify_pixel(*frame[50, 50])] == 256
    assert o.measure(frame, CC.rows_of(one))[0][3:] == (None, None)          # counted all the same
    # min_w / min_h at and one below: a part of 4 x 4 is sampled at (4, 4), not at (5, 4) or (4, 5)
    box = [10, 10, 13, 13, 3, 0]
    for kw, sampled in ((dict(min_w=4, min_h=4), True), (dict(min_w=5, min_h=4), False), (dict(min_w=4, min_h=5), False)):
        oo = CO.ColoursOracle((72, 101), torso_q8=(0, 256), legs_q8=(0, 256), inset_q8=0, **kw)
        assert (oo.measure(frame, CC.rows_of(box))[0][3] is not None) == sampled, kw


def test_max_cover_at_and_one_above():
    frame = CC.texture(np.random.default_rng(3), 72, 101)
    me = [10, 10, 25, 25, 1, 0]                                              # the whole box as the torso: 16 x 16 = 256 pixels
    kw = dict(torso_q8=(0, 256), legs_q8=(0, 256), inset_q8=0)
    for cols, cover in ((4, 64), (5, 80)):
        front = [10, 0, 10 + cols - 1, 40, 2, 0]                             # its feet lower: an occluder over `cols` columns
        rows = CC.rows_of(me, front)
        assert CO.cover_q8(rows, 0, (10, 10, 25, 25), 72, 101) == cover
        assert (CO.ColoursOracle((72, 101), max_cover_q8=64, **kw).measure(frame, rows)[0][3] is not None) == (cover <= 64)
        assert CO.ColoursOracle((72, 101), max_cover_q8=80, **kw).measure(frame, rows)[0][3] is not None
    # equal feet: the earlier row stands in front; the same id and an invalid row never cover
    a, b = [10, 10, 25, 25, 1, 0], [10, 10, 25, 25, 2, 0]
    assert CO.cover_q8(CC.rows_of(a, b), 0, (10, 10, 25, 25), 72, 101) == 0 and CO.cover_q8(CC.rows_of(a, b), 1, (10, 10, 25, 25), 72, 101) == 256
    assert CO.cover_q8(CC.rows_of(a, [0, 0, 100, 70, 1, 0], [0, 70, 100, 0, 5, 0]), 0, (10, 10, 25, 25), 72, 101) == 0


def test_the_planted_scene_reads_red_over_blue():
    frames, rows = CC.planted_scene()
    o = CO.ColoursOracle(frames.shape[2:4])
    out, pend, status, tags = o.update(frames[:, 0], [r[0] for r in rows], 16)
    assert (out, pend, status) == ([], 0, 0) and o.log["covered"] == 12 and o.log["sampled"] == 24
    assert tags[0][0].tolist()[:2] == [CO.RED, CO.BLUE] and tags[1][0].tolist()[:2] == [CO.RED, CO.BLUE]      # the covered tick keeps the tag
    ev = {int(e[2]): e for e in o.flush(16)[0]}
    e = ev[7]
    assert (e[0], e[6], e[7], e[8]) == (CO.FLUSHED, 12, 6, 6)
    assert e[9] == CO.RED and e[11] == CO.BLUE and e[16 + CO.RED] >= 200 and e[28 + CO.BLUE] >= 200 and not e[40:].any() and not e[14:16].any()


def test_seeded_cases_reach_every_branch():
    logs, finals, stopped, pend = {}, 0, 0, 0
    for case in CC.CASES:
        res, oracles = CC.run_oracle(case)
        for o in oracles:
            for k, v in o.log.items():
                logs[k] = logs.get(k, 0) + v
        finals += sum(int(r[0].sum()) for r in res)
        stopped += sum(int((r[4] != 0).sum()) for r in res)
        pend += sum(int(r[3].sum()) for r in res)
        for r, (frames, rows) in zip(res, case["calls"]):
            assert len(r[2]) == sum(len(x) for tick in rows for x in tick)
    assert logs["sampled"] > 50 and logs["covered"] > 10 and logs["small"] > 10 and logs["reused_in_call"] >= 2
    assert finals >= 6 and stopped == 1 and pend >= 3


def test_life_cycle():
    a, b, c = CC.row(2, 4, 20, 40, 1), CC.row(30, 4, 20, 40, 2), CC.row(60, 4, 20, 40, 3)
    rng = np.random.default_rng(4)
    fr = lambda n: [CC.texture(rng, 72, 101) for _ in range(n)]             # noqa: E731
    # expiry: unseen for more than forget_after ticks
    o = CO.ColoursOracle((72, 101), forget_after=1, max_tracks=4)
    out, pend, st, _ = o.update(fr(4), [CC.rows_of(a, b), CC.rows_of(a), CC.rows_of(a), CC.rows_of(a)], 16)
    assert [(int(e[0]), int(e[2]), int(e[5]), int(e[13])) for e in out] == [(CO.EXPIRED, 2, 0, 1)] and pend == 0
    # cap 1 with pending, then drains
    o = CO.ColoursOracle((72, 101), forget_after=0, max_tracks=4)
    out, pend, st, _ = o.update(fr(2), [CC.rows_of(a, b, c), CC.EMPTY], 1)
    assert [int(e[2]) for e in out] == [1] and pend == 2
    before = [e.tolist() for e in o.export()]
    assert [e.tolist() for e in o.export()] == before and [e[0] for e in before] == [CO.EXPIRED, CO.EXPIRED]      # export changes nothing
    out, pend, _, _ = o.update([], [], 1)
    assert [int(e[2]) for e in out] == [2] and pend == 1
    out, pend, _, _ = o.update([], [], 1)
    assert [int(e[2]) for e in out] == [3] and pend == 0
    # flush: the live ones end FLUSHED
    o = CO.ColoursOracle((72, 101), max_tracks=4)
    o.update(fr(1), [CC.rows_of(a, b)], 16)
    assert [e[0] for e in o.export()] == [CO.LIVE, CO.LIVE]
    out, pend, _, _ = o.flush(16)
    assert [(int(e[0]), int(e[2])) for e in out] == [(CO.FLUSHED, 1), (CO.FLUSHED, 2)] and o.export() == []
    # reset of one stream of three
    bank = [CO.ColoursOracle((72, 101), stream=s) for s in range(3)]
    frames = np.stack([np.stack(fr(3)) for _ in range(2)])
    rows = [[CC.rows_of(a), CC.rows_of(b), CC.rows_of(c)]] * 2
    CO.run_bank(bank, frames, rows, 4)
    bank[1].reset()
    assert bank[1].export() == [] and bank[1].frame == 0 and [len(o.export()) for o in bank] == [1, 0, 1] and bank[0].frame == 2
    # capacity stop and rescue
    o = CO.ColoursOracle((72, 101), max_tracks=2)
    out, pend, st, tags = o.update(fr(3), [CC.rows_of(a, b), CC.rows_of(a, b, c), CC.rows_of(a)], 4)
    assert st == CO.ERR_CAPACITY and o.frame == 1 and tags[1].tolist() == [[-1] * 4] * 3 and tags[2].tolist() == [[-1] * 4] and tags[0][0, 0] >= 0
    assert len(o.export()) == 2                                              # what it had can be rescued: export, flush
    out, pend, st, _ = o.flush(4)
    assert len(out) == 2 and st == CO.ERR_CAPACITY
    o.reset()
    assert o.update(fr(1), [CC.rows_of(c)], 4)[2] == 0


def test_samples_saturate_at_2_pow_20():
    frame = CC.texture(np.random.default_rng(5), 72, 101)
    a = CC.row(2, 4, 20, 40, 1)
    o = CO.ColoursOracle((72, 101))
    o.update([frame], [CC.rows_of(a)], 4)
    t = o.slots[0]
    s = list(t["acc"][0])
    assert t["samples"] == [1, 1] and sum(s) <= 256
    t["samples"][0], t["acc"][0] = CO.SAMPLES_MAX - 1, [v * (CO.SAMPLES_MAX - 1) for v in s]      # a state planted one below the limit
    o.update([frame], [CC.rows_of(a)], 4)
    assert t["samples"][0] == CO.SAMPLES_MAX and t["acc"][0] == [v * CO.SAMPLES_MAX for v in s] and o.log["saturated"] == 0
    assert max(t["acc"][0]) <= 256 * CO.SAMPLES_MAX < 1 << 31                # inside int32
    o.update([frame], [CC.rows_of(a)], 4)
    assert t["samples"] == [CO.SAMPLES_MAX, 3] and t["acc"][0] == [v * CO.SAMPLES_MAX for v in s] and o.log["saturated"] == 1
    assert o.export()[0][16:28].tolist() == s                                # the histogram is the one sample's, still
