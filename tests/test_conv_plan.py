"""The conv planner (ai-camera_amd/csrc/conv_plan.cpp) on the CPU: built with the system g++ beside a test-only probe
(tests/conv_plan_probe.cpp), no hipcc, no GPU.

The table below holds the project's conv layers -- YOLOv8n at 640 x 640, ReID at 128 x 64 (names as profiles/r05_conv_layers.txt), the
YOLOv8m layers tests/test_gpu_configs.py runs -- at 1 / 16 / 512 frames (28 / 480 / 15 360 crops), fp16 and fp32, with the plan each gets.
The plans are the parent commit's launches (kernel, grid, workgroup and LDS per queue matched on an MI355X); a change to the tree shows
up here as a changed row."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai-camera_amd", "csrc")
F32, F16 = 0, 1
FORMS = ["Dma", "Wide", "Pp", "PpPatch", "SpPatch", "S2Patch", "Patch", "PmPatch", "C16", "C32s2Tail", "Stream1x1", "C64Resident"]
FIELDS = ["form", "mt", "nt", "wm", "wn", "nstage", "th", "tw", "cpp", "pitch", "kord", "g", "tail", "x2", "run", "blocks"]

# name: (H, W, Cin, Ho, Wo, Cout, K, stride, act, res_mode, tail Cout, Cin2, Cs); act 1 = SiLU, 2 = ReLU; res_mode 1 = add then act, 2 = act then add
YOLO_N = {
    "yolo 1.conv": (320, 320, 16, 160, 160, 32, 3, 2, 1, 0, 0, 0, 0),
    "yolo 3.conv+4.c2f.cv1": (160, 160, 32, 80, 80, 64, 3, 2, 1, 0, 64, 0, 0),
    "yolo 4.c2f.m0.cv1": (80, 80, 32, 80, 80, 32, 3, 1, 1, 0, 0, 0, 0),
    "yolo 4.c2f.m0.cv2": (80, 80, 32, 80, 80, 32, 3, 1, 1, 2, 0, 0, 0),
    "yolo 4.c2f.cv2": (80, 80, 128, 80, 80, 64, 1, 1, 1, 0, 0, 0, 0),
    "yolo 5.conv": (80, 80, 64, 40, 40, 128, 3, 2, 1, 0, 0, 0, 0),
    "yolo 6.c2f.cv1": (40, 40, 128, 40, 40, 128, 1, 1, 1, 0, 0, 0, 0),
    "yolo 6.c2f.m0.cv1": (40, 40, 64, 40, 40, 64, 3, 1, 1, 0, 0, 0, 0),
    "yolo 6.c2f.m0.cv2": (40, 40, 64, 40, 40, 64, 3, 1, 1, 2, 0, 0, 0),
    "yolo 6.c2f.cv2": (40, 40, 256, 40, 40, 128, 1, 1, 1, 0, 0, 0, 0),
    "yolo 7.conv": (40, 40, 128, 20, 20, 256, 3, 2, 1, 0, 0, 0, 0),
    "yolo 8.c2f.cv1": (20, 20, 256, 20, 20, 256, 1, 1, 1, 0, 0, 0, 0),
    "yolo 8.c2f.m0.cv1": (20, 20, 128, 20, 20, 128, 3, 1, 1, 0, 0, 0, 0),
    "yolo 8.c2f.cv2": (20, 20, 384, 20, 20, 256, 1, 1, 1, 0, 0, 0, 0),
    "yolo 9.sppf.cv1": (20, 20, 256, 20, 20, 128, 1, 1, 1, 0, 0, 0, 0),
    "yolo 9.sppf.cv2": (20, 20, 512, 20, 20, 256, 1, 1, 1, 0, 0, 0, 0),
    "yolo 12.c2f.cv1": (40, 40, 384, 40, 40, 128, 1, 1, 1, 0, 0, 0, 256),
    "yolo 12.c2f.cv2": (40, 40, 192, 40, 40, 128, 1, 1, 1, 0, 0, 0, 0),
    "yolo 15.c2f.cv1": (80, 80, 192, 80, 80, 64, 1, 1, 1, 0, 0, 0, 128),
    "yolo 15.c2f.cv2": (80, 80, 96, 80, 80, 64, 1, 1, 1, 0, 0, 0, 0),
    "yolo 16.conv": (80, 80, 64, 40, 40, 64, 3, 2, 1, 0, 0, 0, 0),
    "yolo 19.conv": (40, 40, 128, 20, 20, 128, 3, 2, 1, 0, 0, 0, 0),
    "yolo 22.box0.0": (80, 80, 64, 80, 80, 64, 3, 1, 1, 0, 0, 0, 0),
    "yolo 22.cls0.0": (80, 80, 64, 80, 80, 80, 3, 1, 1, 0, 0, 0, 0),
    "yolo 22.box0.1+.2": (80, 80, 64, 80, 80, 64, 3, 1, 1, 0, 64, 0, 0),
    "yolo 22.cls0.1+.2": (80, 80, 80, 80, 80, 80, 3, 1, 1, 0, 80, 0, 0),
    "yolo 22.box1.0+cls.0": (40, 40, 128, 40, 40, 144, 3, 1, 1, 0, 0, 0, 0),
    "yolo 22.box1.1+.2": (40, 40, 64, 40, 40, 64, 3, 1, 1, 0, 64, 0, 0),
    "yolo 22.cls1.1+.2": (40, 40, 80, 40, 40, 80, 3, 1, 1, 0, 80, 0, 0),
    "yolo 22.box2.0+cls.0": (20, 20, 256, 20, 20, 144, 3, 1, 1, 0, 0, 0, 0),
    "yolo 22.box2.1+.2": (20, 20, 64, 20, 20, 64, 3, 1, 1, 0, 64, 0, 0),
}
YOLO_M = {                                         # the YOLOv8m layers whose shapes YOLOv8n does not have
    "yolo-m 1.conv": (320, 320, 48, 160, 160, 96, 3, 2, 1, 0, 0, 0, 0),
    "yolo-m 2.c2f.m0.cv1": (160, 160, 48, 160, 160, 48, 3, 1, 1, 0, 0, 0, 0),
    "yolo-m 4.c2f.m0.cv1": (80, 80, 96, 80, 80, 96, 3, 1, 1, 0, 0, 0, 0),
    "yolo-m 6.c2f.m0.cv1": (40, 40, 192, 40, 40, 192, 3, 1, 1, 0, 0, 0, 0),
    "yolo-m 8.c2f.m0.cv1": (20, 20, 288, 20, 20, 288, 3, 1, 1, 0, 0, 0, 0),
    "yolo-m 22.box0.0": (80, 80, 192, 80, 80, 64, 3, 1, 1, 0, 0, 0, 0),
    "yolo-m 22.cls0.0": (80, 80, 192, 80, 80, 80, 3, 1, 1, 0, 0, 0, 0),
}
REID = {
    "reid layer1.0.conv1": (64, 32, 64, 64, 32, 64, 3, 1, 2, 0, 0, 0, 0),
    "reid layer1.0.conv2": (64, 32, 64, 64, 32, 64, 3, 1, 2, 1, 0, 0, 0),
    "reid layer2.0.conv1": (64, 32, 64, 32, 16, 128, 3, 2, 2, 0, 0, 0, 0),
    "reid layer2.0.conv2+ds": (32, 16, 128, 32, 16, 128, 3, 1, 2, 0, 0, 64, 0),
    "reid layer2.1.conv1": (32, 16, 128, 32, 16, 128, 3, 1, 2, 0, 0, 0, 0),
    "reid layer2.1.conv2": (32, 16, 128, 32, 16, 128, 3, 1, 2, 1, 0, 0, 0),
    "reid layer3.0.conv1": (32, 16, 128, 16, 8, 256, 3, 2, 2, 0, 0, 0, 0),
    "reid layer3.0.conv2+ds": (16, 8, 256, 16, 8, 256, 3, 1, 2, 0, 0, 128, 0),
    "reid layer3.1.conv1": (16, 8, 256, 16, 8, 256, 3, 1, 2, 0, 0, 0, 0),
    "reid layer4.0.conv1": (16, 8, 256, 8, 4, 512, 3, 2, 2, 0, 0, 0, 0),
    "reid layer4.0.conv2+ds": (8, 4, 512, 8, 4, 512, 3, 1, 2, 0, 0, 256, 0),
    "reid layer4.1.conv1": (8, 4, 512, 8, 4, 512, 3, 1, 2, 0, 0, 0, 0),
    "reid embed_fc": (1, 1, 512, 1, 1, 512, 1, 1, 0, 0, 0, 0, 0),
}
BATCHES = {"yolo": (1, 16, 512), "reid": (28, 480, 15360)}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the planner test builds conv_plan.cpp with the system compiler")
    so = str(tmp_path_factory.mktemp("conv_plan") / "libconvplan.so")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", os.path.join(CSRC, "conv_plan.cpp"),
                    os.path.join(ROOT, "tests", "conv_plan_probe.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.probe_plan.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_long)]
    lib.probe_plan.restype = ctypes.c_int
    lib.probe_c64_block.argtypes = [ctypes.c_int] * 3
    lib.probe_c64_block.restype = ctypes.c_int

    def plan(dtype, layer, n, cu_budget=256, n_dev=False):
        H, W, Cin, Ho, Wo, Cout, K, stride, act, res, tail, cin2, cs = layer
        L = (ctypes.c_int * 16)(H, W, Cin, Ho, Wo, Cout, K, stride, act, res, n, tail, cin2, cs, 0, int(n_dev))
        out = (ctypes.c_long * 20)()
        rc = lib.probe_plan(dtype, L, cu_budget, out)
        r = {"k_order": out[0], "tail_ok": out[17], "x2_ok": out[18], "xs_ok": out[19]}
        if rc == 0:
            r.update({f: out[1 + i] for i, f in enumerate(FIELDS)})
            r["form"] = FORMS[r["form"]]
        return r
    plan.c64_block = lambda H, n, cu_budget=256: lib.probe_c64_block(H, n, cu_budget)
    return plan


def summary(p):
    """One line per plan: the form and the fields its launcher reads."""
    if "form" not in p:
        return "refused"
    s = f"{p['form']} {p['mt']}x{p['nt']}/{p['wm']}x{p['wn']}"
    if p["nstage"]: s += f" s{p['nstage']}"
    if p["th"]: s += f" t{p['th']}x{p['tw']}"
    if p["cpp"]: s += f" c{p['cpp']}"
    if p["pitch"]: s += f" p{p['pitch']}"
    if p["kord"]: s += f" k{p['kord']}"
    if p["g"]: s += f" g{p['g']}"
    if p["tail"]: s += " tail"
    if p["x2"]: s += " x2"
    if p["run"] != 1: s += f" run{p['run']}"
    if p["blocks"]: s += f" b{p['blocks']}"
    return s


def rows(plan):
    out = {}
    for nets, batches in ((YOLO_N, BATCHES["yolo"]), (YOLO_M, BATCHES["yolo"]), (REID, BATCHES["reid"])):
        for name, layer in nets.items():
            for dt, dname in ((F16, "fp16"), (F32, "fp32")):
                # a tail / second / split source only where the engine would attach one (its predicate accepts the layer)
                probe = plan(dt, layer, batches[0])
                lay = layer[:10] + (layer[10] if probe["tail_ok"] or not layer[10] else 0,
                                    layer[11] if probe["x2_ok"] or not layer[11] else 0,
                                    layer[12] if probe["xs_ok"] or not layer[12] else 0)
                for n in batches:
                    out[f"{name} {dname} n={n}"] = summary(plan(dt, lay, n))
    return out


GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plans.json")


def test_plans_match_the_table(planner):
    got = rows(planner)
    want = json.load(open(GOLDEN))
    assert got == want, {k: (want.get(k), got.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


def all_layers():
    for nets, batches in ((YOLO_N, BATCHES["yolo"]), (YOLO_M, BATCHES["yolo"]), (REID, BATCHES["reid"])):
        for name, layer in nets.items():
            yield name, layer, batches[-1]


def sweep(nmax):
    n = 1
    while n <= nmax:
        yield n
        n = n * 2 if n < 64 else n + max(1, n // 3)
    yield nmax


@pytest.mark.parametrize("dtype", [F16, F32])
def test_k_order_does_not_depend_on_the_batch(planner, dtype):
    """The K order is a property of the layer shape: every batch size plans a kernel that walks K in that order."""
    walks = {"Dma": {0, 1, 2, 3}, "Wide": {0, 1, 2, 3}, "Pp": {0, 1, 3}, "PpPatch": {1}, "SpPatch": {1}, "S2Patch": {3},
             "Patch": {0, 2}, "PmPatch": {0}, "C16": {0}, "C32s2Tail": {0}, "Stream1x1": {0}, "C64Resident": {2}}
    for name, layer, nmax in all_layers():
        bare = layer[:10] + (0, 0, 0)
        orders = set()
        for n in sweep(nmax):
            p = planner(dtype, bare, n)
            orders.add(p["k_order"])
            assert p["form"] in FORMS, (name, n)
            assert p["k_order"] in walks[p["form"]], (name, n, summary(p), p["k_order"])
            if p["form"] == "Patch":
                assert p["kord"] == p["k_order"], (name, n)
        assert len(orders) == 1, (name, orders)


def test_predicates_agree_with_the_planner(planner):
    """A layer that conv_tail_supported / conv_x2_supported / conv_xs_supported accepts plans with its tail / second / split source
    at every batch size; fp32 has none of them."""
    for name, layer, nmax in all_layers():
        for dt in (F16, F32):
            probe = planner(dt, layer, 1)
            for i, key in ((10, "tail_ok"), (11, "x2_ok"), (12, "xs_ok")):
                if not layer[i] or not probe[key]:
                    continue
                assert dt == F16 or key != "tail_ok", name
                lay = layer[:10] + tuple(layer[j] if j == i else 0 for j in (10, 11, 12))
                for n in sweep(nmax):
                    p = planner(dt, lay, n)
                    assert "form" in p, (name, dt, key, n)
                    assert p["tail"] == (key == "tail_ok"), (name, n, summary(p))
                    if key == "x2_ok":
                        assert p["x2"] or p["form"] in ("Dma", "Pp"), (name, n, summary(p))


def test_fp32_stays_on_the_implicit_gemm(planner):
    """fp32 engines (the parity mode) run the LDS-DMA implicit GEMM family only."""
    for name, layer, nmax in all_layers():
        for n in sweep(nmax):
            p = planner(F32, layer[:10] + (0, 0, 0), n)
            assert p["form"] in ("Dma", "Wide"), (name, n, summary(p))
            assert p["nstage"] == 4 and p["wm"] * p["wn"] == 4, (name, n, summary(p))


# ------------------------------------------------------------------------------------------------ the cases of tests/conv_ref.py
import conv_ref as R  # noqa: E402


def case_layers(c):
    """The layers of a conv_ref case that its `expect` / `expect_live` describe, as probe tuples: [(name, layer)]."""
    if c.pattern == "ds":
        return [("c2", (c.Ho, c.Wo, 128, c.Ho, c.Wo, 128, 3, 1, R.RELU, 0, 0, 64, 0))]
    if c.pattern == "xs":
        return [("layer", (c.H, c.W, 96, c.H, c.W, 64, 1, 1, c.act, 0, 0, 0, 64))]
    if c.pattern == "block64":
        return [(nm, (c.H, c.W, 64, c.H, c.W, 64, 3, 1, R.RELU, rm, 0, 0, 0)) for nm, rm in (("c1", 0), ("c2", 1))]
    return [("layer", (c.H, c.W, c.cin, c.Ho, c.Wo, c.cout, c.k, c.stride, c.act, c.res, c.tail, 0, 0))]


def case_plans(planner, c, n_dev):
    dt = F16 if c.dtype == "fp16" else F32
    out = []
    for name, layer in case_layers(c):
        p = planner(dt, layer, c.n, n_dev=n_dev)
        assert "form" in p, (c.id, name)
        if layer[10]:
            assert p["tail_ok"], (c.id, "the engine would not attach this tail")
        if layer[11]:
            assert p["x2_ok"], (c.id, "the engine would not fold this second source")
        if layer[12]:
            assert p["xs_ok"], (c.id, "the engine would not fold this split source")
        out.append((name, p))
    return out


@pytest.mark.parametrize("n_dev", [False, True], ids=["host_count", "device_count"])
def test_conv_ref_cases_plan_as_they_expect(planner, n_dev):
    """Every case's hand-written plan -- `expect`, and `expect_live` under a device-side item count -- is what plan_conv_launch answers."""
    for c in R.CASES:
        want = c.expect_live if n_dev else c.expect
        if want.get("kind") == "c64_block":
            ipb = planner.c64_block(c.H, c.n)
            assert 12 <= ipb <= 16 and (not n_dev or ipb == want["ipb"]), (c.id, ipb)
            continue
        for name, p in case_plans(planner, c, n_dev):
            w = {k: v for k, v in want.items() if k in p}
            assert {k: p[k] for k in w} == w, (c.id, name, want, summary(p), p["k_order"])


def _live_fields(planner, c):
    """expect_live's fields as the planner gives them now (the block kernel: its images per block)."""
    if c.expect_live.get("kind") == "c64_block":
        return dict(kind="c64_block", ipb=planner.c64_block(c.H, c.n))
    return case_plans(planner, c, True)[-1][1]


def test_counts_follow_the_construction_rules(planner):
    """Every case's `counts` is what live_counts builds from the planner's CURRENT answer, and satisfies the rules it was built by, with the
    unit (BM, NI, run, tiles per image, blocks, grid) recomputed here from that answer."""
    cdiv = lambda a, b: -(-a // b)                                                      # noqa: E731
    forms = set()
    for c in R.CASES:
        if not c.counts:
            assert c.id not in R.LIVE
            continue
        p, n, ks = _live_fields(planner, c), c.n, set(c.counts)
        form = p.get("form", p.get("kind"))
        forms.add(form)
        assert c.counts == R.live_counts(c, p), (c.id, c.counts, R.live_counts(c, p))
        assert {0, 1, n - 1, n + 3} <= ks and all(0 <= k < n or k == n + 3 for k in ks), (c.id, c.counts)
        px = c.Ho * c.Wo
        if form in ("Dma", "Pp"):
            bm = p["wm"] * p["mt"] * 16
            edges = [k for k in range(1, n - 1) if k * px % bm == 0]
            if edges:
                assert any(k in ks and k - 1 in ks and k + 1 in ks for k in edges), (c.id, bm, px, c.counts)
            assert any(k * px % bm for k in ks if 0 < k < n) or px % bm == 0, (c.id, "no count ends inside a tile")
        elif form in ("PpPatch", "SpPatch", "S2Patch"):
            ni = p["wm"] * (p["mt"] or 8) * 16 // (p["th"] * p["tw"])
            cout = 128 if c.pattern == "ds" else c.cout
            tpg = cdiv(cout, p["wn"] * 64) * ((c.Ho // p["th"]) * (c.Wo // p["tw"]) if form == "PpPatch" else 1)
            assert p["blocks"] == cdiv(cdiv(n, ni) * tpg, p["run"]), (c.id, summary(p))          # the grid is the bound's
            if ni > 1:
                assert {ni - 1, ni, ni + 1} <= ks, (c.id, ni, c.counts)
            if p["run"] > 1:
                live = [cdiv(k, ni) * tpg for k in ks if 0 < k < n]
                assert any(t % p["run"] for t in live) and any(t % p["run"] == 0 for t in live), (c.id, p["run"], c.counts)
        elif form == "Patch":
            tpi = cdiv(c.Wo, p["tw"]) * cdiv(c.Ho, p["th"])
            live = [k * tpi for k in ks if 0 < k < n]
            assert any(t < 8 for t in live) and any(t >= 8 and t % 8 == 0 for t in live), (c.id, tpi, c.counts)
            want = {1, 7} if tpi % 2 else ({2, 6} if tpi % 4 else {4})          # an even tile count per image never leaves 1 or 7
            assert any(t >= 8 and t % 8 in want for t in live), (c.id, tpi, c.counts)
        elif form == "C64Resident":
            tpi = (c.W // 32) * (c.H // 8)
            assert any(0 < k * tpi < p["blocks"] for k in ks) and any(k * tpi > p["blocks"] for k in ks if k < n), (c.id, c.counts)
        elif form == "c64_block":
            g = cdiv(n, p["ipb"])
            assert {1, g - 1, g, g + 1, 2 * g + 1} <= ks, (c.id, g, c.counts)
            assert [cdiv(k, g) for k in (1, g, g + 1, 2 * g + 1)] == [1, 1, 2, 3]             # images per block the kernel works out
        else:
            assert form == "C16", (c.id, form)                                               # reads no count: live rows only
    assert forms >= set(R.READS_COUNT), set(R.READS_COUNT) - forms
    patch = [(cdiv(c.Wo, c.expect_live["tw"]) * cdiv(c.Ho, c.expect_live["th"]), c) for c in R.CASES if c.counts and c.expect_live.get("form") == "Patch"]
    assert any(t % 2 and any(k * t >= 8 and (k * t) % 8 in (1, 7) for k in c.counts) for t, c in patch)
