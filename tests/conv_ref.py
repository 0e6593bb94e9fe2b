"""Per-layer conv harness: one conv layer (or fused pattern) per engine, an fp64 reference of it computed from the layer's ACTUAL inputs
as read back from the device, and a per-element tolerance derived from that reference -- never from a run.  Plain NumPy, no GPU here:
tests/test_gpu_conv_forms.py runs the cases on the device, tests/test_conv_ref.py checks on the CPU that the tolerance separates
honest fp32 arithmetic from the smallest real bugs.  Every case also says what the planner answers under a device-side item count
(expect_live) and, for the cases of LIVE, at which counts tests/test_gpu_conv_counts.py runs it (live_counts, check_live below).

Tolerance per output element (u = 2^-24, K products, S = sum |x * w| + |b| + |res| in fp64):
  accumulation     2 * (K + 2) * u * S      any-order fp32 summation bound, doubled: MFMA's internal rounding is not documented as IEEE
  activation       x 1.1 for SiLU           its Lipschitz constant; ReLU / none <= 1
  output rounding  fp16: 2^-11 * |ref| + 2^-14 (the floor covers a flush of fp16 subnormals); fp32: 4 * 2^-24 * |ref|
A fused pattern whose intermediate never exists on the device (lead + 1x1 tail, the 64-channel BasicBlock pair) is referenced with the
intermediate rounded to the engine's element type; the pre-activation bound of the conv that reads it gains sum |w_next| * ulp(intermediate)
for a one-ulp disagreement there.  The fused C2f has three such levels: there the bound is propagated, each intermediate's disagreement
being 1.1 * (its own accumulation bound + sum |w| * the disagreement of what it read) + one ulp."""
import importlib
from dataclasses import dataclass, field

import numpy as np

ef = importlib.import_module("ai-camera_amd.engine_file")

U = 2.0 ** -24
NONE, SILU, RELU = ef.ACT_NONE, ef.ACT_SILU, ef.ACT_RELU


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    id: str
    H: int
    W: int
    cin: int
    cout: int
    n: int
    expect: dict                     # plan fields the engine must report for the layer under test at this n
    k: int = 3
    stride: int = 1
    act: int = SILU
    res: int = 0                     # ef.RES_*: the residual comes from a buffer a second stem wrote
    tail: int = 0                    # Cout of a 1x1 conv behind the layer (fused into its epilogue at load time)
    tail_act: int = NONE
    dtype: str = "fp16"
    pattern: str = "conv"            # conv | block64 | ds | xs
    slice: int = 0                   # > 0: the layer (its tail, if any) writes channels [slice, slice + Cout) of a buffer whose first channels a stem wrote
    P: int = 7                       # distinct images, tiled to n
    seed: int = 0
    expect_live: dict = None         # the same under a device-side item count (ConvArgs::n_dev): the planner refuses some forms then
    counts: tuple = ()               # the n_live values tests/test_gpu_conv_counts.py runs the case at (live_counts below); (): none

    @property
    def Ho(self):
        return (self.H + 2 * (self.k // 2) - self.k) // self.stride + 1

    @property
    def Wo(self):
        return (self.W + 2 * (self.k // 2) - self.k) // self.stride + 1


def _cases():
    C = []

    def add(id, H, W, cin, cout, n, expect, live=None, **kw):
        # live: the plan under a device-side count where it differs, written from conv_plan.cpp's tree (Wide, PmPatch, Stream1x1 and
        # C32s2Tail refuse a count); tests/test_conv_plan.py asks the planner itself
        C.append(Case(id, H, W, cin, cout, n, expect, seed=len(C) + 1, expect_live=dict(expect) if live is None else live, **kw))
    W_, D = "Wide", "Dma"
    t4 = lambda f, mt, nt, wm=4, wn=1: dict(form=f, mt=mt, nt=nt, wm=wm, wn=wn)          # noqa: E731
    # ---- Wide / Dma, 4-wave tiles: odd maps, M ends inside a tile, Cout not filling the channel tile
    add("wide_2x3", 13, 7, 32, 48, 5, t4(W_, 2, 3), live=t4(D, 2, 3))
    add("wide_4x2", 13, 7, 32, 24, 5, t4(W_, 4, 2), live=t4(D, 4, 2))
    add("dma_4x1_1x1", 13, 7, 64, 16, 5, t4(D, 4, 1), k=1)
    add("wide_2x2_2x2", 13, 7, 64, 200, 5, t4(W_, 2, 2, 2, 2), live=t4(D, 2, 2, 2, 2), act=RELU)
    add("wide_2x5", 20, 20, 64, 80, 70, t4(W_, 2, 5), live=t4(D, 2, 5))
    add("dma_2x5", 20, 20, 64, 80, 101, t4(D, 2, 5))
    add("wide_2x9", 10, 6, 128, 144, 7, t4(W_, 2, 9), live=t4(D, 2, 9))
    add("wide_2x3_slice", 13, 7, 32, 48, 5, t4(W_, 2, 3), live=t4(D, 2, 3), slice=16)
    # ---- Dma, 8-wave tiles: large tiles, ragged last tile
    add("dma_512x80", 20, 20, 64, 80, 331, t4(D, 4, 5, 8, 1))
    add("dma_256x256", 10, 6, 32, 256, 855, t4(D, 8, 4, 2, 4), act=RELU)
    add("dma_256x128", 10, 6, 32, 128, 1707, t4(D, 4, 4, 4, 2), act=RELU)
    add("dma_256x144", 10, 6, 128, 144, 2201, t4(D, 4, 9, 4, 1))
    add("dma_512x80_slice", 20, 20, 64, 80, 331, t4(D, 4, 5, 8, 1), slice=16)
    # ---- Pp: im2col ping-pong on a map that tiles nothing
    add("pp_256", 10, 6, 64, 256, 855, dict(form="Pp", wm=2, wn=4), act=RELU)
    add("pp_128", 10, 6, 64, 128, 1707, dict(form="Pp", wm=4, wn=2), act=RELU)
    add("pp_128_slice", 10, 6, 64, 128, 1707, dict(form="Pp", wm=4, wn=2), act=RELU, slice=16)
    # ---- PpPatch: all three tile shapes, several tiles per image, odd image count
    pp = lambda th, tw: dict(form="PpPatch", th=th, tw=tw, x2=0, run=1)                          # noqa: E731
    add("pppatch_32x16", 32, 16, 64, 128, 201, pp(32, 16), act=RELU)
    add("pppatch_32x16_res", 32, 16, 64, 128, 201, pp(32, 16), act=RELU, res=ef.RES_ADD_THEN_ACT)
    add("pppatch_64x32", 64, 32, 64, 128, 51, pp(32, 16), act=RELU)
    add("pppatch_16x8", 16, 8, 64, 256, 401, pp(16, 8), act=RELU)
    add("pppatch_8x4", 8, 4, 64, 256, 1601, pp(8, 4), act=RELU)
    add("pppatch_32x16_slice", 32, 16, 64, 128, 201, pp(32, 16), act=RELU, slice=16)
    # ---- PpPatch / Wide with a second source: a ReID-style downsample block (3x3/2 + 3x3 + 1x1/2 downsample as the residual)
    add("ds_block_wide", 64, 32, 64, 128, 3, dict(form=W_, x2=1), live=dict(t4(D, 2, 2, 2, 2), x2=0), pattern="ds", stride=2, act=RELU, P=3)
    add("ds_block_pppatch", 64, 32, 64, 128, 201, dict(form="PpPatch", x2=1, th=32, tw=16, run=1), pattern="ds", stride=2, act=RELU)
    # ---- SpPatch: whole-image tiles
    sp = lambda th, tw: dict(form="SpPatch", th=th, tw=tw, run=1)                                # noqa: E731
    add("sppatch_32x16", 32, 16, 128, 128, 201, sp(32, 16), act=RELU)
    add("sppatch_16x8", 16, 8, 128, 256, 401, sp(16, 8), act=RELU)
    add("sppatch_8x4", 8, 4, 256, 512, 801, sp(8, 4), act=RELU)
    add("sppatch_16x8_slice", 16, 8, 128, 256, 401, sp(16, 8), act=RELU, slice=16)
    # ---- S2Patch: the space-to-depth walk at its borders
    add("s2patch_32x16", 64, 32, 64, 128, 201, dict(form="S2Patch", th=32, tw=16, k_order=3, run=1), stride=2, act=RELU)
    add("s2patch_16x8", 32, 16, 128, 256, 401, dict(form="S2Patch", th=16, tw=8, k_order=3, run=1), stride=2, act=RELU)
    add("s2_wide_k3", 64, 32, 64, 128, 3, dict(form=W_, k_order=3), live=dict(t4(D, 2, 2, 2, 2), k_order=3), stride=2, act=RELU, P=3)
    add("s2patch_32x16_slice", 64, 32, 64, 128, 201, dict(form="S2Patch", th=32, tw=16, k_order=3, run=1), stride=2, act=RELU, slice=16)
    # ---- Patch: overhanging tiles
    pt = lambda th, tw, kord=0, tail=0: dict(form="Patch", th=th, tw=tw, kord=kord, tail=tail)      # noqa: E731
    add("patch_16x16_exact", 16, 16, 64, 64, 783, pt(16, 16))
    add("patch_16x16_overhang", 12, 24, 64, 64, 695, pt(16, 16))
    add("patch_8x32_overhang", 12, 40, 64, 64, 417, pt(8, 32))
    add("patch_c80", 12, 24, 64, 80, 695, pt(16, 16))
    add("patch_c32_res", 12, 24, 32, 32, 695, pt(16, 16), res=ef.RES_ACT_THEN_ADD)
    add("patch_relu_k2", 8, 32, 64, 64, 783, pt(8, 32, kord=2), act=RELU)
    add("patch_tail24", 8, 32, 64, 64, 783, pt(8, 32, tail=1), tail=24)
    add("patch_16x16_overhang_slice", 12, 24, 64, 64, 695, pt(16, 16), slice=16)
    # ---- PmPatch: strips, overhang with a tail
    pm = lambda th, tw, tail=0: dict(form="PmPatch", th=th, tw=tw, tail=tail)            # noqa: E731
    add("pmpatch_strip_c64", 40, 8, 64, 64, 157, pm(40, 8), live=t4(D, 2, 4))
    add("pmpatch_strip_c64_res", 40, 8, 64, 64, 157, pm(40, 8), live=t4(D, 2, 4), res=ef.RES_ACT_THEN_ADD)
    add("pmpatch_strip_c144", 40, 8, 128, 144, 157, pm(40, 8), live=t4(D, 2, 9))
    add("pmpatch_c80_tail80", 16, 16, 80, 80, 196, pm(16, 16, 1), live=dict(t4(D, 2, 5), tail=1), tail=80)
    add("pmpatch_c80_tail48_overhang", 14, 28, 80, 80, 128, pm(16, 16, 1), live=dict(t4(D, 2, 5), tail=1), tail=48)
    add("pmpatch_c64_tail64_overhang", 14, 28, 64, 64, 128, pm(16, 16, 1), live=dict(t4(D, 2, 4), tail=1), tail=64)
    add("pmpatch_strip_c64_slice", 40, 8, 64, 64, 157, pm(40, 8), live=t4(D, 2, 4), slice=16)
    # ---- C16: odd input size under stride 2
    add("c16_s1", 8, 32, 16, 16, 3, dict(form="C16"), P=3)
    add("c16_s1_res", 8, 32, 16, 16, 3, dict(form="C16"), res=ef.RES_ACT_THEN_ADD, P=3)
    add("c16_s2_odd", 15, 63, 16, 32, 3, dict(form="C16"), stride=2, P=3)
    add("c16_s2_odd_slice", 15, 63, 16, 32, 3, dict(form="C16"), stride=2, P=3, slice=16)
    # ---- C32s2Tail: odd input, narrow tail
    add("c32s2_tail64", 32, 32, 32, 64, 512, dict(form="C32s2Tail", tail=1), live=dict(t4(D, 4, 4), tail=1), stride=2, tail=64)
    add("c32s2_tail40_odd", 31, 31, 32, 64, 512, dict(form="C32s2Tail", tail=1), live=dict(t4(D, 4, 4), tail=1), stride=2, tail=40)
    add("c32s2_tail64_wide", 32, 32, 32, 64, 3, dict(form=W_, tail=1), live=dict(t4(D, 2, 4), tail=1), stride=2, tail=64, P=3)
    add("c32s2_tail40_odd_wide", 31, 31, 32, 64, 3, dict(form=W_, tail=1), live=dict(t4(D, 2, 4), tail=1), stride=2, tail=40, P=3)
    add("c32s2_tail40_odd_slice", 31, 31, 32, 64, 512, dict(form="C32s2Tail", tail=1), live=dict(t4(D, 4, 4), tail=1), stride=2, tail=40, slice=16)
    # ---- Stream1x1: M not a multiple of its step
    for cin in (96, 64, 128):
        add(f"stream1x1_c{cin}", 10, 6, cin, 64, 2501, dict(form="Stream1x1"), live=t4(D, 4, 4), k=1)
    add("stream1x1_c96_slice", 10, 6, 96, 64, 2501, dict(form="Stream1x1"), live=t4(D, 4, 4), k=1, slice=16)
    # ---- C64Resident: persistent blocks, last partial share
    add("c64_resident", 8, 64, 64, 64, 2930, dict(form="C64Resident"), live=dict(form="C64Resident", blocks=256), act=RELU)
    add("c64_resident_res", 8, 64, 64, 64, 2930, dict(form="C64Resident"), live=dict(form="C64Resident", blocks=256), act=RELU, res=ef.RES_ADD_THEN_ACT)
    add("c64_resident_slice", 8, 64, 64, 64, 2930, dict(form="C64Resident"), live=dict(form="C64Resident", blocks=256), act=RELU, slice=16)
    # ---- the 64-channel BasicBlock kernel on the smallest map it takes (intermediate in LDS), and the same pair as two launches
    add("c64_block", 4, 32, 64, 64, 11720, dict(kind="c64_block"), live=dict(kind="c64_block", ipb=12), pattern="block64", act=RELU)
    add("c64_block_two_launches", 4, 32, 64, 64, 3, dict(kind="conv", k_order=2), live=dict(t4(D, 2, 4), kind="conv", k_order=2), pattern="block64", act=RELU, P=3)
    # ---- split source: the first 64 of 96 input channels come from a 6 x 4 tensor through the upsample fold
    add("split_source", 12, 8, 96, 64, 3, dict(form=D, xs=1), live=dict(t4(D, 2, 4), xs=1), k=1, pattern="xs", P=3)
    # ---- fp32 engine: the six plan_f32 tiles, stride 1 on an odd map and stride 2 on an odd input
    for cout, (mt, nt, wm, wn) in ((16, (4, 1, 4, 1)), (32, (4, 2, 4, 1)), (48, (2, 3, 4, 1)), (64, (2, 4, 4, 1)), (80, (1, 5, 4, 1)), (128, (2, 4, 2, 2))):
        add(f"f32_c{cout}", 13, 7, 32, cout, 5, t4(D, mt, nt, wm, wn), dtype="fp32", P=5)
        add(f"f32_c{cout}_s2", 15, 9, 32, cout, 5, t4(D, mt, nt, wm, wn), dtype="fp32", stride=2, P=5)
    for c in C:
        if c.id in LIVE:
            c.counts = live_counts(c)
    return C


# ------------------------------------------------------------------------------------------------------------------ counts
# The cases tests/test_gpu_conv_counts.py runs under a device-side count: one or two per form the planner hands out then, the residual
# variants, the second-source block, the fused tail, the split source, the direct C16 kernel and two fp32 tiles.
LIVE = ("wide_2x3", "dma_2x5", "dma_512x80", "wide_2x3_slice", "c32s2_tail64", "ds_block_wide", "pmpatch_strip_c64_res",
        "pmpatch_c80_tail80", "stream1x1_c96", "split_source", "f32_c48", "f32_c128_s2", "pp_256", "pp_128", "pppatch_32x16_res",
        "pppatch_64x32", "pppatch_16x8", "pppatch_8x4", "ds_block_pppatch", "sppatch_16x8", "sppatch_8x4", "s2patch_32x16",
        "s2patch_16x8", "patch_16x16_exact", "patch_c32_res", "patch_tail24", "patch_8x32_overhang", "c64_resident",
        "c64_resident_res", "c64_block", "c16_s1", "c16_s1_res")
READS_COUNT = ("Dma", "Pp", "PpPatch", "SpPatch", "S2Patch", "Patch", "C64Resident", "c64_block")     # rows past the count stay as they were


def live_unit(c: Case, e=None):
    """What the kernel planned under a count deals its work in, from the plan fields e (default: the case's expect_live):
    dict(form, and per form bm | ni, tpg, run | tpi | tpi, blocks | grid).  The map is the output map of the layer the fields describe."""
    e = c.expect_live if e is None else e
    form = e.get("form", e.get("kind"))
    px = c.Ho * c.Wo
    if form in ("Dma", "Pp"):
        return dict(form=form, bm=e["wm"] * e.get("mt", 8) * 16, px=px)
    if form in ("PpPatch", "SpPatch", "S2Patch"):
        wm, wn = (4, 2) if e["th"] == 32 else (2, 4)                   # 512 x 128 tile on 32 x 16 patches, 256 x 256 on 16 x 8 and 8 x 4
        cout = 128 if c.pattern == "ds" else c.cout
        ny = -(-cout // (wn * 64))
        tpg = ny * ((c.Ho // e["th"]) * (c.Wo // e["tw"]) if form == "PpPatch" else 1)
        return dict(form=form, ni=wm * 128 // (e["th"] * e["tw"]), tpg=tpg, run=e["run"])
    if form == "Patch":
        return dict(form=form, tpi=-(-c.Wo // e["tw"]) * -(-c.Ho // e["th"]))
    if form == "C64Resident":
        return dict(form=form, tpi=(c.W // 32) * (c.H // 8), blocks=e["blocks"])
    if form == "c64_block":
        return dict(form=form, grid=-(-c.n // e["ipb"]))
    return dict(form=form)


def live_counts(c: Case, e=None):
    """The n_live values of a case, built from live_unit: 0, 1, n - 1 and n + 3 (the count may exceed the bound), and the edges of the
    unit the kernel deals work in.  Values outside [0, n) other than n + 3 are dropped (the unit does not fit this n)."""
    from math import gcd
    u, n = live_unit(c, e), c.n
    ks = {0, 1, n - 1, n + 3}
    first = lambda ok, lo=1: next((k for k in range(lo, n) if ok(k)), None)                      # noqa: E731
    if "bm" in u:                                                      # the first count that ends on a tile edge, and its neighbours
        k0 = u["bm"] // gcd(u["bm"], u["px"])
        if k0 + 1 < n:
            ks |= {k0 - 1, k0, k0 + 1}
    elif "ni" in u:
        ni, tpg, run = u["ni"], u["tpg"], u["run"]
        if ni > 1:
            ks |= {ni - 1, ni, ni + 1}
        tiles = lambda k: -(-k // ni) * tpg                                                     # noqa: E731
        if run > 1:                                                    # the last live tile inside a block's run / at its end
            ks |= {first(lambda k: tiles(k) % run, ni + 2), first(lambda k: tiles(k) % run == 0, ni + 2)}
    elif u["form"] == "Patch":                                         # live tiles: below 8, a multiple of 8, the nearest remainders to one
        t = u["tpi"]
        near = min(min(r, 8 - r) for r in {(j * t) % 8 for j in range(8)} - {0})
        ks |= {max(k for k in range(1, 8) if k * t < 8), first(lambda k: k * t >= 8 and (k * t) % 8 == 0),
               first(lambda k: k * t >= 8 and min((k * t) % 8, 8 - (k * t) % 8) == near and (k * t) % 8)}
    elif u["form"] == "C64Resident":                                   # fewer live tiles than blocks, exactly as many, one image more
        kb = u["blocks"] // u["tpi"]
        ks |= {kb - 1, kb, kb + 1}
    elif u["form"] == "c64_block":                                     # images per block 1 | 1, last block idle | 1 | 2, half the grid idle | 3
        g = u["grid"]
        ks |= {g - 1, g, g + 1, 2 * g + 1}
    return tuple(sorted(k for k in ks if k is not None and (0 <= k < n or k == n + 3)))


CASES = _cases()


# ------------------------------------------------------------------------------------------------------------------ graphs
@dataclass
class Built:
    g: object
    layers: dict = field(default_factory=dict)       # name -> dict(op, w, b, k, stride, act, res_mode, src=(buf, coff, c), dst=(buf, coff, c), res=(buf, coff))
    bufs: dict = field(default_factory=dict)         # name -> buffer index


def build_graph(c: Case) -> Built:
    """KIND_REID engine: 1x1 stems 3 -> C with no activation (both signs reach the layer), the layer or pattern under test, then
    AVGPOOL -> L2NORM for the loader."""
    g = ef.Graph(ef.KIND_REID, c.H, c.W)
    wg = ef._WeightGen(1000 + c.seed)
    B = Built(g)
    inp = g.buf(c.H, c.W, ef.IN_C)
    B.bufs["inp"] = inp

    def conv(name, src, dst, cin, cout, k, s, act, gain=1.0, **kw):
        w, b = wg(cout, cin, k, act, gain)
        g.conv(name, src, dst, cin, cout, k, s, act, wb=(w, b), **kw)
        res = kw.get("res")
        B.layers[name] = dict(op=len(g.ops) - 1, w=w, b=b, k=k, stride=s, act=act, res_mode=kw.get("res_mode", 0),
                              src=(src, kw.get("src_coff", 0), cin), dst=(dst, kw.get("dst_coff", 0), cout), res=res)

    def stem(name, dst, cout, coff=0, k=1, s=1):
        conv(name, inp, dst, 3, cout, k, s, NONE, dst_coff=coff)

    def finish(last, ch):
        p = g.buf(1, 1, ch)
        g.simple(ef.OP_AVGPOOL, last, p, ch)
        e = g.buf(1, 1, ch, ef.DT_F32)
        g.simple(ef.OP_L2NORM, p, e, ch)
        g.outputs.append([e, ch, 0, 0, 0, 0, 0, 0])
        g.meta = [ch, 0, 0, 0, 0, 0, 0, 0]
        return B

    H, W, Ho, Wo = c.H, c.W, c.Ho, c.Wo
    if c.pattern == "block64":
        x, mid, out = g.buf(H, W, 64), g.buf(H, W, 64), g.buf(H, W, 64)
        B.bufs.update(x=x, mid=mid, out=out)
        stem("stem", x, 64)
        conv("c1", x, mid, 64, 64, 3, 1, RELU)
        conv("c2", mid, out, 64, 64, 3, 1, RELU, gain=0.5, res=(x, 0), res_mode=ef.RES_ADD_THEN_ACT)
        return finish(out, 64)
    if c.pattern == "ds":
        x, t, d, out = g.buf(H, W, 64), g.buf(Ho, Wo, 128), g.buf(Ho, Wo, 128), g.buf(Ho, Wo, 128)
        B.bufs.update(x=x, t=t, d=d, out=out)
        stem("stem", x, 64)
        conv("c1", x, t, 64, 128, 3, 2, RELU)
        conv("ds", x, d, 64, 128, 1, 2, NONE, gain=0.5)
        conv("c2", t, out, 128, 128, 3, 1, RELU, gain=0.5, res=(d, 0), res_mode=ef.RES_ADD_THEN_ACT)
        return finish(out, 128)
    if c.pattern == "xs":
        lo, cat, out = g.buf(H // 2, W // 2, 64), g.buf(H, W, 96), g.buf(H, W, 64)
        B.bufs.update(lo=lo, cat=cat, out=out)
        stem("stem_lo", lo, 64, k=3, s=2)
        g.simple(ef.OP_UPSAMPLE2X, lo, cat, 64)
        stem("stem_hi", cat, 32, coff=64)
        conv("layer", cat, out, 96, 64, 1, 1, c.act)
        return finish(out, 64)
    x = g.buf(H, W, c.cin)
    B.bufs["x"] = x
    stem("stem", x, c.cin)
    last_c = c.tail or c.cout
    out = g.buf(Ho, Wo, c.slice + last_c)
    B.bufs["out"] = out
    if c.slice:
        stem("stem_slice", out, c.slice, k=c.k if c.stride > 1 else 1, s=c.stride)
    kw = {}
    if c.res:
        r = g.buf(Ho, Wo, c.cout)
        B.bufs["r"] = r
        stem("stem_res", r, c.cout, k=c.k if c.stride > 1 else 1, s=c.stride)
        kw = dict(res=(r, 0), res_mode=c.res)
    if c.tail:
        mid = g.buf(Ho, Wo, c.cout)
        B.bufs["mid"] = mid
        conv("layer", x, mid, c.cin, c.cout, c.k, c.stride, c.act, **kw)
        conv("tail", mid, out, c.cout, c.tail, 1, 1, c.tail_act, dst_coff=c.slice)
    else:
        conv("layer", x, out, c.cin, c.cout, c.k, c.stride, c.act, gain=0.5 if c.res else 1.0, dst_coff=c.slice, **kw)
    return finish(out, c.slice + last_c)


def images(c: Case, n=None, salt=0):
    """-> ([P, 3, H, W] distinct images, [n, 3, H, W] = those tiled: image i is base[i % P]).  salt: another draw of the same shape."""
    n = c.n if n is None else n
    P = min(c.P, n)
    base = np.random.default_rng(77 + c.seed + 1000 * salt).standard_normal((P, 3, c.H, c.W)).astype(np.float32)
    return base, base[np.arange(n) % P]


# ------------------------------------------------------------------------------------------------------------------ reference
def act_fn(y, act):
    if act == SILU:
        return y / (1.0 + np.exp(-y))
    return np.maximum(y, 0.0) if act == RELU else y


def to_elem(y, dtype):
    """fp64 -> the engine's element type (round to nearest even) -> fp64."""
    return np.asarray(y, np.float64).astype(np.float16 if dtype == "fp16" else np.float32).astype(np.float64)


def ulp(v, dtype):
    t = np.float16 if dtype == "fp16" else np.float32
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(t)).astype(np.float64)


def dev_weights(w, dtype):
    """The loader packs OIHW fp32 weights to the engine's element type (engine.cpp pack_weights: f32_to_f16_bits, round to nearest
    even); the bias stays fp32."""
    return to_elem(w, dtype)


def im2col(x, k, s):
    """[P, H, W, C] -> [P, Ho, Wo, k * k * C], K ordered (kh, kw, c); zero padding k // 2."""
    p = k // 2
    P, H, W, C = x.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = np.zeros((P, H + 2 * p, W + 2 * p, C), np.float64)
    xp[:, p:p + H, p:p + W] = x
    return np.concatenate([xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s] for kh in range(k) for kw in range(k)], -1)


def wmat(w):
    """[O, I, k, k] -> [k * k * I, O], rows ordered (kh, kw, ci)."""
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0]))


def out_rounding(ref, f16_out):
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -14 if f16_out else 4.0 * U * np.abs(ref)


def layer_ref(x, w, b, k, stride, act, dtype, res=None, res_mode=0, x2=None, w2=None, b2=None, s2=1, extra=None, mut=None):
    """conv + bias (+ res) + act in fp64 of the device's own inputs.  x [P, H, W, Cin], res [P, Ho, Wo, Cout]: fp64 copies of what the
    device holds; w / b: the engine file's fp32 weights.  x2 / w2 / b2 / s2: a 1x1 / stride s2 second source folded into the same
    GEMM.  extra: per-element pre-activation slack for a disagreement in a fused intermediate.
    mut: None, or one of the bugs of tests/test_conv_ref.py.  -> (ref, tol, acc) with acc = the pre-activation accumulation bound."""
    wq = dev_weights(w, dtype)
    bq = np.asarray(b, np.float32)
    if mut == "tap":
        wq = wq.copy()
        wq[:, :, k // 2, k - 1] = 0.0
    cols, wm = im2col(x, k, stride), wmat(wq)
    K = wm.shape[0]
    if x2 is not None:
        bq = bq + np.asarray(b2, np.float32)                       # summed in fp32 at load time
        c2, wm2 = im2col(x2, 1, s2), wmat(dev_weights(w2, dtype))
        cols, wm = np.concatenate([cols, c2], -1), np.concatenate([wm, wm2], 0)
        K = wm.shape[0]
    bq = bq.astype(np.float64)
    pre = cols @ wm + (2.0 * bq if mut == "bias" else bq)
    S = np.abs(cols) @ np.abs(wm) + np.abs(bq)
    if mut == "res_order" and res is not None:
        res_mode = 3 - res_mode
    if res is not None and res_mode == ef.RES_ADD_THEN_ACT:
        pre = pre + res
    ref = act_fn(pre, act)
    if res is not None and res_mode == ef.RES_ACT_THEN_ADD:
        ref = ref + res
    if res is not None:
        S = S + np.abs(res)
    acc = 2.0 * (K + 2) * U * S
    tol = (1.1 if act == SILU else 1.0) * (acc + (0.0 if extra is None else extra)) + out_rounding(ref, dtype == "fp16")
    if mut == "column":
        ref = ref.copy()
        if ref.shape[2] > 1:
            ref[:, :, -1] = ref[:, :, -2]
        else:
            ref[:, -1] = ref[:, -2]
    elif mut == "row":
        ref = ref.copy()
        ref[:, -1] = ref[:, -2]
    elif mut == "image":
        ref = ref.copy()
        ref[[-1, -2]] = ref[[-2, -1]]
    return ref, tol, acc


def next_slack(w_next, k, stride, dtype, dis):
    """Pre-activation slack of the conv (weights w_next) that reads an intermediate which may disagree by `dis` per element."""
    return im2col(dis, k, stride) @ np.abs(wmat(dev_weights(w_next, dtype)))


MUTANTS = ("tap", "column", "row", "image", "bias", "res_order")


def case_reference(c: Case, B: Built, read, mut=None):
    """The outputs to compare for one case: a list of (name, buffer name, channel offset, ref, tol).  read(buffer name) -> fp64
    [P, h, w, c] array of what that buffer holds for the P distinct images."""
    L, dt = B.layers, c.dtype

    def lay(name, x, **kw):
        l = L[name]
        return layer_ref(x, l["w"], l["b"], l["k"], l["stride"], l["act"], dt, res_mode=l["res_mode"], **kw)
    outs = []
    if c.pattern == "block64":
        x = read("x")
        fused = c.expect.get("kind") == "c64_block"
        if fused:                       # the intermediate lives in LDS: reference it rounded, allow a one-ulp disagreement
            m_ref, _, _ = lay("c1", x)
            mid = to_elem(m_ref, dt)
            slack = next_slack(L["c2"]["w"], 3, 1, dt, ulp(mid, dt))
        else:
            mid, slack = read("mid"), None
            outs.append(("c1", "mid", 0) + lay("c1", x, mut=mut)[:2])
        outs.append(("c2", "out", 0) + lay("c2", mid, res=x, extra=slack, mut=mut)[:2])
        return outs
    if c.pattern == "ds":
        x, t = read("x"), read("t")
        outs.append(("c1", "t", 0) + lay("c1", x, mut=mut)[:2])
        d = L["ds"]
        outs.append(("c2+ds", "out", 0) + layer_ref(t, L["c2"]["w"], L["c2"]["b"], 3, 1, RELU, dt, x2=x, w2=d["w"], b2=d["b"], s2=2, mut=mut)[:2])
        return outs
    if c.pattern == "xs":
        lo, cat = read("lo"), read("cat")
        outs.append(("stem_lo", "lo", 0) + lay("stem_lo", read("inp")[..., :3])[:2])
        xin = np.concatenate([lo.repeat(2, 1).repeat(2, 2), cat[..., 64:]], -1)
        outs.append(("layer", "out", 0) + lay("layer", xin, mut=mut)[:2])
        return outs
    x = read("x")
    res = read("r") if c.res else None
    if c.slice:
        outs.append(("stem_slice", "out", 0) + lay("stem_slice", read("inp")[..., :3])[:2])
    if c.tail:
        m_ref, _, _ = lay("layer", x, res=res, mut=mut if mut in ("tap", "bias", "res_order") else None)
        mid = to_elem(m_ref, dt)
        slack = next_slack(L["tail"]["w"], 1, 1, dt, ulp(mid, dt))
        outs.append(("layer+tail", "out", c.slice) + lay("tail", mid, extra=slack, mut=mut if mut in ("column", "row", "image") else None)[:2])
    else:
        outs.append(("layer", "out", c.slice) + lay("layer", x, res=res, mut=mut)[:2])
    return outs


def host_inputs(c: Case, B: Built, base):
    """CPU stand-in for the device read-back (tests/test_conv_ref.py): every buffer the reference reads, computed by this module's
    own reference of the stems from the P distinct images."""
    P = len(base)
    vals = {"inp": np.zeros((P, c.H, c.W, ef.IN_C))}
    vals["inp"][..., :3] = to_elem(base.transpose(0, 2, 3, 1), c.dtype)
    for name, l in B.layers.items():
        if l["src"][0] != B.bufs["inp"]:
            continue
        bname = next(k for k, v in B.bufs.items() if v == l["dst"][0])
        ref = to_elem(layer_ref(vals["inp"][..., :3], l["w"], l["b"], l["k"], l["stride"], l["act"], c.dtype)[0], c.dtype)
        if bname not in vals:
            hw = B.g.buffers[l["dst"][0]]
            vals[bname] = np.zeros((P, hw[0], hw[1], hw[2]))
        vals[bname][..., l["dst"][1]:l["dst"][1] + l["dst"][2]] = ref
    if c.pattern == "ds":
        l = B.layers["c1"]
        vals["t"] = to_elem(layer_ref(vals["x"], l["w"], l["b"], 3, 2, RELU, c.dtype)[0], c.dtype)
    if c.pattern == "block64":
        l = B.layers["c1"]
        vals["mid"] = to_elem(layer_ref(vals["x"], l["w"], l["b"], 3, 1, RELU, c.dtype)[0], c.dtype)
    return vals


def worst_ratio(got, ref, tol):
    """got [n, h, w, c] (device element type) against ref / tol [P, h, w, c]: image i is compared with ref[i % P].
    -> (max error / tolerance, index of that element)."""
    P, worst, where = len(ref), 0.0, None
    for j in range(P):
        r = np.abs(got[j::P].astype(np.float64) - ref[j]) / tol[j]
        if not np.isfinite(r).all():
            return float("inf"), (j,) + tuple(int(v) for v in np.argwhere(~np.isfinite(r))[0])
        m = float(r.max()) if r.size else 0.0
        if m > worst:
            i = np.unravel_index(int(r.argmax()), r.shape)
            worst, where = m, (j + P * int(i[0]),) + tuple(int(v) for v in i[1:])
    return worst, where


# ------------------------------------------------------------------------------------------------------------------ under a count
def bits(a):
    """The array's bit patterns (a NaN equals itself, -0 differs from 0)."""
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def image_ratios(a, ref, tol, live):
    """max |a[i] - ref[i % P]| / tol[i % P] per image i < live -> [live] (inf for a non-finite element).  An image that repeats image
    i % P of `a` bit for bit takes that image's figure instead of being computed again."""
    P, out = len(ref), np.zeros(live)

    def one(img, j):
        r = np.abs(img.astype(np.float64) - ref[j]) / tol[j]
        return float(r.max()) if np.isfinite(r).all() else float("inf")
    for j in range(min(P, live)):
        rows = a[j:live:P]
        out[j:live:P] = one(a[j], j)
        same = (bits(rows) == bits(a[j])).reshape(len(rows), -1).all(1)
        for t in np.nonzero(~same)[0]:
            out[j + P * int(t)] = one(rows[t], j)
    return out


def check_live(got, dirty, ref, tol, k, host=None):
    """One output tensor after a run under the device-side count k, in figures (tests/test_gpu_conv_counts.py asserts them; tests/
    test_conv_ref.py plants bugs).  got / dirty [n, h, w, c]: the tensor after the run and before it (what a run of other images of
    the same shape left there); ref / tol [P, h, w, c]: fp64 reference and tolerance of the P distinct images (rows at and past the
    count are not looked at); host: the same tensor after a run of the same images without a count, or None.
    -> dict(live = min(k, n), ratio / where: the worst error / tolerance over the live images (worst_ratio's), dirty: the SMALLEST
    per-image worst ratio of `dirty` against the reference over the live images (> 1: a kernel that stored nothing for an image would
    show), past: rows at and past the count equal `dirty` bit for bit, host: the live rows equal `host` bit for bit, or None)."""
    n = len(got)
    live = max(0, min(k, n))
    r = image_ratios(got, ref, tol, live)
    res = dict(live=live, ratio=0.0, where=None, dirty=float("inf"), host=None)
    if live:
        i = int(r.argmax())
        res["ratio"] = float(r[i])
        e = np.nan_to_num(np.abs(got[i].astype(np.float64) - ref[i % len(ref)]) / tol[i % len(ref)], nan=np.inf)
        res["where"] = (i,) + tuple(int(v) for v in np.unravel_index(int(e.argmax()), e.shape))
        res["dirty"] = float(image_ratios(dirty, ref, tol, live).min())
    res["past"] = bool(np.array_equal(bits(got[live:]), bits(dirty[live:])))
    if host is not None:
        res["host"] = bool(np.array_equal(bits(got[:live]), bits(host[:live])))
    return res
