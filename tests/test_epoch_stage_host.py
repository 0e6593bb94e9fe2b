"""The one staging layout of the tracker calls (ai-camera_amd/csrc/epoch_stage.hpp) on the CPU.

tests/epoch_stage_check.cpp is built with the system g++ under the address and undefined-behaviour sanitizers and run as a child
process: a stand-alone program, no hipcc, no GPU.  It builds the layout of every call site with the structs the call sites use and
prints every field's offset and size; here those are compared with the formulas the call sites carried before they shared the
header, restated below one function per call site (from Tracker::update_device / update_batch, EpochBank::update,
DeepSortBank::update and the pipeline's stage_b_device as they were), and checked for alignment and overlap.  The fill and delivery
routines run in the same program on exact-size host buffers.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_BYTES, HDR_BYTES = 32, 32                 # sizeof(EpochStreamPlan), sizeof(DevTrkHdr): 8 int32 each (trk_dev.hpp)
ALIGNED = ("frame_n", "tlwh", "n_tracks", "warps", "feat", "feat_n", "hdr", "dbg")
OUTPUT_HALF = ("n_tracks", "rows", "oconf", "hdr", "dbg", "feat_n")


def up(x):
    return (x + 15) // 16 * 16


# ---- the call sites' layouts as they were written out by hand -----------------------------------------------------------------
def tracker_was(F, n, cap, dbg):
    """Tracker::update_batch (dbg = its stride 2 * 512 + 8) and, with F = 1, cap = 512, dbg = 0, Tracker::update_device."""
    o = {"frame_n": 0, "frame_d0": F * 4, "tlwh": (F * 8 + 15) // 16 * 16}
    o["conf"] = o["tlwh"] + n * 16
    o["cls"] = o["conf"] + n * 4
    o["valid"] = o["cls"] + n * 4
    o["n_tracks"] = (o["valid"] + n * 4 + 15) // 16 * 16
    o["rows"] = o["n_tracks"] + (F * 4 + 15) // 16 * 16
    o["oconf"] = o["rows"] + F * cap * 24
    if dbg:
        o["dbg"] = (o["oconf"] + F * cap * 4 + 15) // 16 * 16
        return o, o["dbg"] + F * dbg * 4
    return o, o["oconf"] + F * cap * 4


def update_device_was(n):
    o = {"frame_n": 0, "frame_d0": 4, "tlwh": 16, "conf": 16 + n * 16}
    o["cls"] = o["conf"] + n * 4
    o["valid"] = o["cls"] + n * 4
    o["n_tracks"] = (o["valid"] + n * 4 + 15) // 16 * 16
    o["rows"] = o["n_tracks"] + 16
    o["oconf"] = o["rows"] + 512 * 24
    return o, o["oconf"] + 512 * 4


def bank_was(S, F, n, cap, dim, valid, warps, feat):
    o = {"plan": 0, "frame_n": up(S * 8)}
    o["frame_d0"] = o["frame_n"] + F * 4
    o["tlwh"] = up(o["frame_d0"] + F * 4)
    o["conf"] = o["tlwh"] + n * 16
    o["cls"] = o["conf"] + n * 4
    in_end, feat_bytes = o["cls"] + n * 4, 0
    if valid:
        o["valid"], in_end = in_end, in_end + n * 4
    if warps:
        o["warps"] = up(in_end)
        in_end = o["warps"] + F * 24
    if feat and n:
        o["feat"], feat_bytes = up(in_end), n * dim * 4
        in_end = o["feat"] + feat_bytes
    o["n_tracks"] = up(in_end)
    o["rows"] = o["n_tracks"] + up(F * 4)
    o["oconf"] = o["rows"] + F * cap * 24
    size = o["oconf"] + F * cap * 4
    o["feat_n"] = up(size)
    return o, size


def deepsort_was(S, F, n, cap, dim, E, feats):
    o = {"plans": 0, "row_map": E * S * PLAN_BYTES}
    o["frame_e0"] = o["row_map"] + n * 4
    o["stream_f0"] = up(o["frame_e0"] + F * 4)
    o["stream_k"] = o["stream_f0"] + S * 4
    o["frame_n"] = up(o["stream_k"] + S * 4)
    o["frame_d0"] = o["frame_n"] + F * 4
    o["tlwh"] = up(o["frame_d0"] + F * 4)
    o["conf"] = o["tlwh"] + n * 16
    o["cls"] = o["conf"] + n * 4
    o["valid"] = o["cls"] + n * 4
    o["feat"] = up(o["valid"] + n * 4)
    feat_bytes = n * dim * 4 if feats else 0
    o["n_tracks"] = up(o["feat"] + feat_bytes)
    o["rows"] = o["n_tracks"] + up(F * 4)
    o["oconf"] = o["rows"] + F * cap * 24
    o["hdr"] = up(o["oconf"] + F * cap * 4)
    size = o["hdr"] + S * HDR_BYTES
    o["feat_n"] = up(size)
    return o, size


def pipeline_was(F, cap):
    o = {"n_tracks": 0, "rows": (F * 4 + 15) // 16 * 16}
    o["oconf"] = o["rows"] + F * cap * 24
    return o, o["oconf"] + F * cap * 4


WAS = {"tracker": tracker_was, "update_device": update_device_was, "bank": bank_was, "deepsort": deepsort_was, "pipeline": pipeline_was}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the staging test builds tests/epoch_stage_check.cpp with the system compiler")
    exe = str(tmp_path_factory.mktemp("epoch_stage") / "epoch_stage_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "epoch_stage_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def layout_lines(printed):
    for line in printed:
        site = line.split(" ", 1)[0]
        if site not in WAS:
            continue
        head, tail = line.split(" | ")
        params = {k: int(v) for k, v in (t.split("=") for t in head.split()[1:])}
        fields, size = {}, None
        for t in tail.split():
            k, v = t.split("=")
            if k == "bytes":
                size = int(v)
            else:
                fields[k] = tuple(int(x) for x in v.split(":"))
        yield site, params, fields, size, line


def test_every_offset_is_where_the_call_sites_had_it(printed):
    seen = {s: 0 for s in WAS}
    for site, params, fields, size, line in layout_lines(printed):
        was, was_size = WAS[site](**params)
        assert {k: v[0] for k, v in fields.items()} == was, line
        assert size == was_size, line
        seen[site] += 1
    # the whole cross product: F x n x cap (x dbg | x S x dim x extras | x S x dim x E x feats)
    assert seen == {"tracker": 5 * 6 * 3 * 2, "pipeline": 5 * 6 * 3, "bank": 5 * 6 * 3 * 4 * 3 * 8, "deepsort": 5 * 6 * 3 * 4 * 3 * 3 * 2,
                    "update_device": 6}


def test_cases_cover_the_values_and_every_optional_field(printed):
    vals = {}
    for site, params, _, _, _ in layout_lines(printed):
        for k, v in params.items():
            vals.setdefault(k, set()).add(v)
    assert vals["S"] == {1, 2, 3, 256} and vals["F"] == {0, 1, 3, 5, 17} and vals["n"] == {0, 1, 3, 4, 5, 513}
    assert vals["cap"] == {0, 1, 7} and vals["dim"] == {0, 4, 512}
    assert vals["valid"] == vals["warps"] == vals["feat"] == vals["feats"] == {0, 1}


def test_alignment_overlap_and_the_input_half(printed):
    for site, params, fields, size, line in layout_lines(printed):
        for name in ALIGNED:
            if name in fields:
                assert fields[name][0] % 16 == 0, (name, line)
        spans = sorted((off, off + n, name) for name, (off, n) in fields.items() if n)
        for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
            assert a1 <= b0, (an, bn, line)
        o_out = fields["n_tracks"][0]
        for name, (off, n) in fields.items():
            if name in OUTPUT_HALF:
                assert off >= o_out, (name, line)
            else:
                assert off + n <= o_out, (name, line)       # the upload [0, o_out) carries every input
            if name != "feat_n":
                assert off + n <= size, (name, line)        # (feat_n is device only, behind the mirrored bytes)


def rows_of(printed, prefix):
    hit = [ln for ln in printed if ln.startswith(prefix + " ") or ln == prefix]
    assert len(hit) >= 1, prefix
    return [ln[len(prefix):].split() for ln in hit]


def bits(tokens):
    return np.array([int(t, 16) for t in tokens], np.uint32).view(np.float32)


def test_fill(printed):
    boxes = bits(rows_of(printed, "fill boxes")[0]).reshape(5, 4)
    for form in ("tlwh", "xyxy"):
        assert rows_of(printed, f"fill {form} frame_n") == [["2", "0", "3"]]
        assert rows_of(printed, f"fill {form} frame_d0") == [["0", "2", "2"]]
        got = bits(rows_of(printed, f"fill {form} tlwh")[0]).reshape(5, 4)
        if form == "tlwh":
            exp = boxes
        else:                                              # EpochBank::update's fp32 expression: b[0], b[1], b[2] - b[0], b[3] - b[1]
            exp = np.stack([boxes[:, 0], boxes[:, 1], boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]], 1)
            assert exp.dtype == np.float32
        assert got.tobytes() == exp.tobytes(), form
        assert bits(rows_of(printed, f"fill {form} conf")[0]).tobytes() == np.array([0.9, 0.8, 0.7, 0.6, 0.5], np.float32).tobytes()
        assert rows_of(printed, f"fill {form} cls") == [["0", "1", "2", "3", "4"]]
    # (any_feat && (!has || has[j])) ? 1 : 0
    assert rows_of(printed, "valid has=NULL") == [["1"] * 5] * 2
    assert rows_of(printed, "valid has=mixed") == [["1", "0", "1", "1", "0"]] * 2
    assert rows_of(printed, "valid no_features") == [["0"] * 5] * 2


def test_delivery(printed):
    cap, F, sentinel = 2, 5, -77
    n_out = np.array(rows_of(printed, "deliver n_out")[0], np.int64)
    out6 = np.array(rows_of(printed, "deliver out6")[0], np.int64).reshape(F, cap, 6)
    conf = np.array(rows_of(printed, "deliver out_conf")[0], np.float64).reshape(F, cap)
    # streams of 2 and 3 frames, counts 1 3 | 0 2 5, good = 2 and 1 frames: stream 1 delivers its first frame only
    assert n_out.tolist() == [1, 3, 0, 0, 0]
    exp6, expc = np.full((F, cap, 6), sentinel, np.int64), np.full((F, cap), float(sentinel))
    for f, kept in ((0, 1), (1, 2)):
        exp6[f, :kept] = 1000 * (f + 1) + np.arange(kept * 6).reshape(kept, 6)
        expc[f, :kept] = 10.0 * (f + 1) + np.arange(kept) + 0.5
    assert np.array_equal(out6, exp6)
    assert np.array_equal(conf, expc)


def test_shared_validation(printed):
    got = {ln.split(" | ")[0][len("check "):]: ln.split(" | ")[1] for ln in printed if ln.startswith("check ")}
    assert got["ok"] == "F=5 kmax_s=3 total=518 nmax=512 capacity=0 err="
    assert got["negative_frames"].endswith("capacity=0 err=negative frame count / row capacity")
    assert got["negative_count"].endswith("capacity=0 err=negative detection count")
    assert got["too_many"].endswith("capacity=1 err=X: more than 512 detections in one frame")
    assert got["no_arrays"].endswith("capacity=0 err=NULL detection arrays")
    assert got["max_total"].endswith("capacity=0 err=too many detections in one call")
