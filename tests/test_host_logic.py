"""Host-side product code that runs without a GPU: the C-ABI surface, the C++ LSAP / thresholded
matching (pinned against SciPy and the reference fixtures), engine files, synthetic scenes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment as scipy_lsa

from conftest import ROOT, pkg
from oracle import deepsort_oracle as O


def test_abi_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "aicam.h")).read()
    declared = set(re.findall(r"\b(aic_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 40
    handle = C.CDLL(lib.LIB_PATH)
    missing = [n for n in sorted(declared) if not hasattr(handle, n)]
    assert not missing, missing
    assert declared == set(lib.EXPORTS), declared ^ set(lib.EXPORTS)
    assert handle.aic_abi_version() == 2


def test_no_cpu_fallback(lib):
    """Without a GPU every compute entry point fails loudly; host logic still works."""
    if lib.device_count() > 0:
        pytest.skip("GPU present")
    z = np.zeros((1, 4), np.float32)
    with pytest.raises(lib.NoDeviceError):
        lib.call("aic_kf_initiate", 0, lib.ptr(z), 1, lib.ptr(np.zeros((1, 8), np.float32)), lib.ptr(np.zeros((1, 64), np.float32)))
    with pytest.raises(lib.NoDeviceError):
        pkg("core.tracker_core").TrackerCore()
    with pytest.raises(RuntimeError):
        pkg("config").resolve_device("cpu")


def test_missing_engine_file_raises(lib):
    he = pkg("hip_engine")
    with pytest.raises(FileNotFoundError):      # trt_engine.py:46-47
        he.HipEngine("/nonexistent/engine.aicw")
    with pytest.raises(FileNotFoundError):      # reid_model.py:57-58
        pkg("reid_model").ReIDModel("/nonexistent/reid.aicw")


def _lsap(lib, m):
    m = np.ascontiguousarray(m, np.float64)
    k = min(m.shape)
    r, c = np.zeros(k, np.int64), np.zeros(k, np.int64)
    lib.call("aic_lsap", lib.ptr(m), m.shape[0], m.shape[1], lib.ptr(r), lib.ptr(c))
    return r, c


def test_lsap_matches_scipy(lib):
    rng = np.random.default_rng(7)
    for it in range(4000):
        r, c = rng.integers(1, 48, 2)
        kind = it % 6
        if kind == 0:
            m = rng.uniform(0, 1, (r, c))
        elif kind == 1:
            m = rng.integers(0, 3, (r, c)).astype(float)
        elif kind == 2:
            m = np.round(rng.uniform(0, 0.5, (r, c)), 1)
        elif kind == 3:
            m = np.full((r, c), 0.25)
        elif kind == 4:
            m = rng.uniform(0, 0.3, (r, c)).astype(np.float32).astype(float)
            m[m > 0.2] = np.float32(0.20001)
        else:
            m = rng.uniform(-5, 5, (r, c))
            m[rng.uniform(size=(r, c)) < 0.3] = 1e5
        ri, ci = _lsap(lib, m)
        sr, sc = scipy_lsa(m)
        assert np.array_equal(ri, sr) and np.array_equal(ci, sc), (it, m.shape)
    assert _lsap(lib, np.zeros((0, 5)))[0].size == 0
    with pytest.raises(lib.AicError):
        _lsap(lib, np.array([[np.nan, 1.0]]))
    with pytest.raises(lib.AicError):
        _lsap(lib, np.array([[np.inf, np.inf]]))       # infeasible, as SciPy raises


def test_min_cost_matching_matches_reference_fixtures(lib, golden):
    g = golden("assign")
    la = pkg("core.linear_assignment")
    for k in range(int(g["n_cases"])):
        m = g[f"c{k}_cost"]
        rows, cols = list(range(0, 2 * m.shape[0], 2)), list(range(100, 100 + m.shape[1]))
        for name, thr in (("cos", 0.2), ("iou", 0.7)):
            mt, ut, ud = la.min_cost_matching(lambda *a, m=m: m.copy(), thr, None, None, list(rows), list(cols))
            assert np.array_equal(np.array(mt, np.int32).reshape(-1, 2), g[f"c{k}_{name}_m"]), (k, name)
            assert ut == g[f"c{k}_{name}_ut"].tolist() and ud == g[f"c{k}_{name}_ud"].tolist()
    # reference self-test scenario (linear_assignment.py:267-276): (0,0),(1,1) matched, track 2 / det 2 left
    cost = np.array([[0.1, 0.9, 0.9], [0.9, 0.15, 0.9], [0.9, 0.9, 0.9]], np.float32)
    mt, ut, ud = la.min_cost_matching(lambda *a: cost.copy(), 0.2, None, None, [0, 1, 2], [0, 1, 2])
    assert mt == [(0, 0), (1, 1)] and ut == [2] and ud == [2]
    assert la.min_cost_matching(lambda *a: cost, 0.2, None, None, [], [0, 1]) == ([], [], [0, 1])


def test_min_cost_matching_shortcuts_vs_scipy(lib):
    """min_cost_matching (csrc/lsap.cpp) answers without the solver when every entry is above the threshold (empty matching) and when
    the optimum can be read off the rows (strict row minima in pairwise different columns).  Both must give what SciPy's assignment
    followed by linear_assignment.py:70-88 gives -- on matrices built to sit on both sides of each shortcut: unique minima, tied
    minima, two rows wanting one column, rows without an admissible entry, wide / square / tall shapes, quantised costs."""
    rng = np.random.default_rng(23)
    hits = {"empty": 0, "some": 0}
    for it in range(6000):
        nr, nc = (int(v) for v in rng.integers(1, 28, 2))
        kind = it % 6
        thr = 0.2 if it % 2 else 0.7
        if kind == 0:                                    # mostly above the threshold, a few admissible entries
            m = rng.uniform(thr + 0.01, 1.0, (nr, nc))
            for _ in range(int(rng.integers(0, min(nr, nc) + 1))):
                m[rng.integers(nr), rng.integers(nc)] = rng.uniform(0, thr)
        elif kind == 1:                                  # a planted permutation of clear minima (the crowded cascade's usual case)
            m = rng.uniform(thr + 0.05, 1.0, (nr, nc))
            k = min(nr, nc)
            for r, c in zip(rng.permutation(nr)[:k], rng.permutation(nc)[:k]):
                if rng.uniform() < 0.8: m[r, c] = rng.uniform(0, thr)
        elif kind == 2:                                  # quantised: ties everywhere
            m = np.round(rng.uniform(0, 2 * thr, (nr, nc)), 1)
        elif kind == 3:                                  # two rows compete for one column
            m = rng.uniform(thr + 0.05, 1.0, (nr, nc))
            c = int(rng.integers(nc))
            m[rng.integers(nr), c] = 0.05
            m[rng.integers(nr), c] = 0.06
            if nc > 1: m[rng.integers(nr), (c + 1) % nc] = 0.07
        elif kind == 4:                                  # nothing admissible at all
            m = rng.uniform(thr + 1e-3, 5.0, (nr, nc))
        else:
            m = rng.uniform(0, 1, (nr, nc))
        m = m.astype(np.float32)
        mr, mc, nm = np.zeros(32, np.int32), np.zeros(32, np.int32), np.zeros(1, np.int32)
        lib.call("aic_min_cost_matching", lib.ptr(m), nr, nc, float(thr), lib.ptr(mr), lib.ptr(mc), lib.ptr(nm))
        c = m.copy()
        c[c > thr] = thr + 1e-5                          # linear_assignment.py:59 (float32 array, Python-float threshold)
        ri, ci = scipy_lsa(c)
        keep = c[ri, ci] <= thr                          # :76
        assert mr[:nm[0]].tolist() == ri[keep].tolist() and mc[:nm[0]].tolist() == ci[keep].tolist(), (it, kind, m.shape)
        hits["some" if nm[0] else "empty"] += 1
    assert hits["empty"] > 500 and hits["some"] > 2000


def test_match_cascade_matches_oracle(lib):
    """aic_match_cascade (csrc/assoc_host.cpp) vs the oracle cascade on random frames with ties, gated entries, tentative /
    confirmed / stale tracks and empty sides (linear_assignment.py:91-157, tracker_core.py:83-177)."""
    from asan_driver import random_frame
    rng = np.random.default_rng(3)
    for it in range(300):
        app, maha, iou, state, tsu = random_frame(rng, it)
        t, n = app.shape
        max_age = int(rng.integers(1, 7))
        mt, md = np.zeros(max(min(t, n), 1), np.int32), np.zeros(max(min(t, n), 1), np.int32)
        ut, ud = np.zeros(max(t, 1), np.int32), np.zeros(max(n, 1), np.int32)
        nm, nut, nud = (np.zeros(1, np.int32) for _ in range(3))
        lib.call("aic_match_cascade", lib.ptr(app), lib.ptr(maha), lib.ptr(iou), t, n, lib.ptr(state), lib.ptr(tsu), 0.2, 0.7, max_age,
                 lib.ptr(mt), lib.ptr(md), lib.ptr(nm), lib.ptr(ut), lib.ptr(nut), lib.ptr(ud), lib.ptr(nud))
        em, eut, eud = O.cascade_on_matrices(app, maha, iou, state.tolist(), tsu.tolist(), 0.2, 0.7, max_age)
        assert list(zip(mt[:nm[0]].tolist(), md[:nm[0]].tolist())) == [(int(a), int(b)) for a, b in em], it
        assert ut[:nut[0]].tolist() == [int(v) for v in eut] and ud[:nud[0]].tolist() == [int(v) for v in eud], it


def test_engine_file_graphs():
    ef = pkg("engine_file")
    g = ef.build_yolov8("n", calibrate=False)
    assert len(g.weights) == 63 and g.conv_macs() == 4_371_456_000 and g.meta[2] == 8400
    assert abs(g.n_params() - 3_151_888) < 10
    gm = ef.build_yolov8("m", calibrate=False)
    assert len(gm.weights) == 83 and abs(gm.conv_macs() / 1e9 - 39.468) < 1e-3
    gr = ef.build_reid(calibrate=False)
    assert len(gr.weights) == 21 and abs(gr.conv_macs() / 1e9 - 1.1217) < 1e-3           # 20 convs + embed FC
    blob = ef.serialize(gr)
    back = ef.parse(blob)
    assert back.ops == gr.ops and back.buffers == gr.buffers and back.outputs == gr.outputs
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(back.weights, gr.weights))
    from oracle.nets_oracle import EngineOracle
    eo = EngineOracle(blob)
    assert eo.ops == gr.ops and [tuple(b) for b in eo.buffers] == gr.buffers
    # every channel slice is 16-byte aligned in fp16 (what the conv kernel's vector loads need)
    for o in g.ops + gm.ops + gr.ops:
        assert o[2] % 8 == 0 and o[5] % 4 == 0


def test_synthetic_scene_is_deterministic():
    syn = pkg("synthetic")
    a, b = syn.Scene(seed=3, n_targets=5, width=320, height=240), syn.Scene(seed=3, n_targets=5, width=320, height=240)
    assert np.array_equal(a.render(17), b.render(17))
    ba, ca, _, ia = a.detections(17)
    bb, cb, _, ib = b.detections(17)
    assert np.array_equal(ba, bb) and np.array_equal(ca, cb) and np.array_equal(ia, ib)
    assert ba.dtype == np.float32 and (ba[:, 2] > ba[:, 0]).all() and ba[:, [0, 2]].max() <= 320
    f = syn.identity_features([0, 1, 0], 3, dim=64)
    d = O.cosine_distance(f, f)
    assert d[0, 2] < 1e-5 and d[0, 1] > 0.5
    sc = syn.Scene(seed=1, n_targets=4, gaps=[(2, 5, 9)], births={3: 7})
    assert sc.visible(6).tolist() == [True, True, False, False] and sc.visible(10).all()


def test_no_conv_kernel_spills():
    """Every matrix-core kernel of the built library keeps its tile in registers: no scratch, no spilled VGPRs.

    Read from the code-object metadata inside libaicam.so (tools/kernel_resources.py), so it needs no GPU.  The fp32 patch kernels
    once spilled 11 KB per lane (8x slower) while every parity test stayed green: DESIGN.md §12.
    """
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so")
    assert len(tab) > 100, len(tab)                      # every .hip source contributed its bundle
    hot = {k: r for k, r in tab.items() if re.search(r"conv|c2f|stem", k)}
    assert len(hot) > 60, len(hot)
    # fp32 and fp16 instantiations (fp32 engines run the LDS-DMA implicit GEMM only since round 5; the patch kernels are fp16)
    assert any("conv_igemm_dma_kernelIf" in k for k in hot) and any("patch_kernelIDF16_" in k for k in hot) and any("sp_patch_kernel" in k for k in hot)
    assert sum("conv_wide_kernel" in k for k in hot) >= 12           # the few-tiles kernel: plain, second-source and tail forms (kernels_conv_wide.hip)
    # (up to four dwords parked ONCE per block across the K loop -- an address pair that is written before the loop and read by the
    # epilogue -- are tolerated: the 512 x 128 ping-pong patch kernel sits exactly at its 256-register cap; anything inside a loop shows up as far more)
    bad = {k: r for k, r in hot.items() if r["scratch"] > 16 or r["vgpr_spills"] > 4}
    assert not bad, bad
    # the rest of the library: no spilled registers anywhere.  Scratch: the single-block association kernels call the LSAP variants out of
    # line (kernels_trk_dev.hip: inlined twice each they pushed the kernel past its 256 registers and every phase ran 2x slower on spills) --
    # their 400 bytes are the callees' frames and the table handle passed by reference on the rare path, not spills
    spilled = {k: r["vgpr_spills"] for k, r in tab.items() if k not in hot and r["vgpr_spills"]}
    assert not spilled, spilled
    others = {k: r["scratch"] for k, r in tab.items() if k not in hot and r["scratch"] > (512 if re.search(r"trk_epoch_kernel|trk_cascade_test", k) else 64)}
    assert not others, others


def test_switches_match_design_table():
    """The environment switches the library reads are exactly the ones DESIGN.md §11 lists, and every switch a test or tool names is one
    the library reads: a reference-path test whose switch no longer exists would compare a path with itself and still pass.  The one
    exception is written into the table: a row of class "retired" (a switch whose effect is now unconditional) is read nowhere."""
    name = re.compile(r"\bAICAM_[A-Z0-9][A-Z0-9_]*")
    src = os.path.join(ROOT, "ai-camera_amd")
    read = set()
    for f in sorted(os.listdir(os.path.join(src, "csrc"))):
        if f.endswith((".hip", ".cpp", ".hpp")):
            text = open(os.path.join(src, "csrc", f)).read()
            read |= set(re.findall(r'getenv\("(' + name.pattern[2:] + r')"\)', text))
            read |= set(re.findall(r"#\s*ifn?def\s+(" + name.pattern[2:] + ")", text))
            read |= set(re.findall(r"defined\s*\(\s*(" + name.pattern[2:] + ")", text))
    for dirpath, _, files in os.walk(src):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                read |= set(re.findall(r"""os\.(?:environ\.get\(|environ\[|getenv\()\s*["'](""" + name.pattern[2:] + ")", text))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("\n## 11."):design.index("\n## 12.")]
    rows = [l for l in table.splitlines() if l.startswith("|")]
    # a row of class "retired": a variable that had an effect once and has none now -- the library must not read it any more
    retired = set(name.findall("\n".join(l for l in rows if l.split("|")[2].strip() == "retired")))
    listed = set(name.findall("\n".join(rows))) - retired
    assert not (retired & read), sorted(retired & read)
    assert read == listed, (sorted(read - listed), sorted(listed - read))
    named = {}
    for d in ("tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith((".py", ".sh")):
                    for n in name.findall(open(os.path.join(dirpath, f)).read()):
                        named.setdefault(n, os.path.relpath(os.path.join(dirpath, f), ROOT))
    stale = {n: f for n, f in named.items() if n not in read and n not in retired}
    assert not stale, stale
