"""The comparer and the registry of tests/poison_scenarios.py on the CPU: what tests/test_gpu_poison.py relies on
when it says that two children's recordings are the same bytes."""
import os
import re

import numpy as np

import poison_scenarios as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rec():
    r = np.random.default_rng(3)
    return {"a_boxes": r.random((4, 7, 4)).astype(np.float32), "a_nd": np.arange(4, dtype=np.int32), "a_u8": r.integers(0, 256, (3, 5), dtype=np.uint8),
            "scalar": np.array(5, np.int64), "empty": np.zeros((0, 6), np.float64)}


def test_equal_recordings_give_no_finding():
    assert P.compare(rec(), rec()) == []


def test_one_byte_is_flagged_with_key_and_index():
    a, b = rec(), rec()
    b["a_boxes"].view(np.uint8).reshape(4, 7, 4, 4)[2, 5, 1, 0] ^= 1            # the lowest mantissa bit of one float
    b["a_u8"][2, 4] += 1
    assert P.compare(a, b) == [("a_boxes", "bytes", (2, 5, 1)), ("a_u8", "bytes", (2, 4))]
    b = rec()
    b["scalar"] = np.array(6, np.int64)
    assert P.compare(a, b) == [("scalar", "bytes", ())]


def test_first_differing_index_is_reported():
    a, b = rec(), rec()
    b["a_nd"][1:] += 1
    assert P.compare(a, b) == [("a_nd", "bytes", (1,))]


def test_dtype_shape_and_keys():
    a = rec()
    b = rec()
    b["a_nd"] = b["a_nd"].astype(np.int64)                                     # equal values, another type
    assert P.compare(a, b) == [("a_nd", "dtype", None)]
    b = rec()
    b["a_boxes"] = b["a_boxes"].reshape(4, 4, 7)                               # equal bytes, another shape
    assert P.compare(a, b) == [("a_boxes", "shape", None)]
    b = rec()
    del b["a_u8"]
    b["extra"] = np.zeros(1)
    assert P.compare(a, b) == [("a_u8", "missing", None), ("extra", "unexpected", None)]
    b = rec()
    b["empty"] = np.zeros((0, 5), np.float64)
    assert P.compare(a, b) == [("empty", "shape", None)]


def test_nans_of_equal_bits_are_equal_and_of_other_bits_are_not():
    a = {"x": np.array([1.0, np.nan, -0.0], np.float32)}
    b = {"x": a["x"].copy()}
    assert not np.array_equal(a["x"], b["x"]) and P.compare(a, b) == []
    b["x"].view(np.uint32)[1] ^= 1                                             # still a NaN, another payload
    assert np.isnan(b["x"][1]) and P.compare(a, b) == [("x", "bytes", (1,))]
    b = {"x": np.array([1.0, np.nan, 0.0], np.float32)}                        # +0.0 for -0.0: equal as numbers, not as bytes
    assert P.compare(a, b) == [("x", "bytes", (2,))]


def test_exceptions_mask_exactly_their_entries():
    cand = np.zeros((2, 6), bool)
    cand[0, 1] = cand[1, 4] = True
    a = {"edges_wsbox": np.ones((2, 6, 4), np.float32), "edges_wscand": cand, "edges_boxes": np.ones((2, 3, 4), np.float32), "edges_allbox": np.ones((2, 6, 4), np.float32)}
    b = {k: v.copy() for k, v in a.items()}
    b["edges_wsbox"][0, 0] = 7                                                 # no candidate there: workspace the header calls stale
    assert P.compare(a, b, "detector") == []
    assert P.compare(a, b) == [("edges_wsbox", "bytes", (0, 0, 0))]            # without a group nothing is masked
    assert P.compare(a, b, "reid") == [("edges_wsbox", "bytes", (0, 0, 0))]    # ... nor in a group the table does not name
    b["edges_wsbox"][1, 4, 2] = 7                                              # at a candidate: compared
    assert [f[:2] for f in P.compare(a, b, "detector")] == [("edges_wsbox", "bytes")]
    for k in ("edges_boxes", "edges_allbox", "edges_wscand"):                  # nothing else of the group is masked
        c = {kk: v.copy() for kk, v in a.items()}
        c[k].reshape(-1)[-1] = 0 if k != "edges_wscand" else True
        assert [f[0] for f in P.compare(a, c, "detector")] == [k]
    assert P.excepted("detector", "live_wsbox") and not P.excepted("detector", "live_boxes") and not P.excepted("pipeline", "live_wsbox")


def test_probe_shows_tells_the_modes_apart():
    fills = {"zero": (0, 0, 0), "big": (0x7B7B7B7B, 31611, 123), "nan": (0xFFFFFFFF, -1, 255)}
    recs = {m: {"probe_f32": np.full(4, f, np.uint32).view(np.float32), "probe_i32": np.full(4, i, np.int32), "probe_u8": np.full(4, u, np.uint8),
                "probe_pinned_u8": np.full(4, u, np.uint8)} for m, (f, i, u) in fills.items()}
    for m in P.MODES:
        for other in P.MODES:
            assert P.probe_shows(m, recs[other]) == (m == other), (m, other)
    r = {k: v.copy() for k, v in recs["big"].items()}
    r["probe_i32"][3] = 0x7B7B7B7B                                             # bytes where the typed value belongs
    assert not P.probe_shows("big", r)
    f = P.compare(recs["zero"], recs["nan"])
    assert f == [(k, "bytes", (0,)) for k in sorted(P.PROBE_KEYS)]


def test_every_group_of_the_gpu_test_exists():
    src = open(os.path.join(ROOT, "tests", "test_gpu_poison.py")).read()       # (importing it would need nothing more, but it is a GPU module)
    names = re.search(r"^GROUP_NAMES = \(([^)]*)\)", src, re.M).group(1)
    names = [n.strip().strip('"') for n in names.split(",") if n.strip()]
    assert names and sorted(names) == sorted(P.GROUPS), (names, sorted(P.GROUPS))
    limits = re.search(r"^TIMEOUT_S = \{([^}]*)\}", src, re.M).group(1)
    assert sorted(re.findall(r'"(\w+)":', limits)) == sorted(names)
    assert set(P.DIRTY) <= set(P.GROUPS) and all(callable(f) for f in P.GROUPS.values())


def test_every_exception_cites_a_line_of_the_public_header():
    lines = open(os.path.join(ROOT, "include", "aicam.h")).read().splitlines()
    assert P.EXCEPTIONS
    for group, pattern, line in P.EXCEPTIONS:
        assert group in P.GROUPS and line.strip() and line in lines, (group, pattern, line)
        assert "stale" in line or "only candidate anchors hold" in line, line   # the line has to be the one that ALLOWS the stale read
