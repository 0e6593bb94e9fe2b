"""Tensor-level harness for the NHWC graph ops of csrc/kernels_elt.hip (max pool 3x3/2, SPPF pooling, 2x upsample, global average pool,
L2 normalise) and the two fused stems (ReID conv 3x3 + ReLU + max pool, YOLO letterbox + conv 3x3/2 + SiLU): one small engine per case
in which a 1x1 stem conv with NO activation feeds the op under test, references computed from the op's ACTUAL input as read back
from the device, every output element compared.  Plain NumPy, no GPU here: tests/test_gpu_elt_ops.py runs the cases on the device,
tests/test_elt_ref.py proves on the CPU that references and tolerances let honest fp32 arithmetic through and catch the smallest bugs.

Inputs.  Images are uniform in [-1, 1] and every third channel of a feeding conv has the bias -(sum |w| + 0.5): that channel is negative
at every pixel of every image, so a maximum that starts at 0, or a border tap read as 0 instead of ignored, shows in it.  The "low" cases
put the bias -1e5 on every channel (fp32 engines): whole windows lie below -65504, the lowest finite fp16 value.

No tolerance here comes from a run (u = 2^-24):

  max pool, SPPF pooling, upsample   bit exact.  They only select among values the device already holds.  (Reported through
                     worst_ratio with tol = ulp / 2: an element that differs at all differs by >= one ulp and gives a ratio >= 2.)
  average pool, 1    bit exact against avgpool_f32: sum = 0; for p = 0 .. hw-1: sum = fl32(sum + x[p]); out = elem(fl32(sum / fl32(hw))).
                     The kernels do exactly that per channel (both of them: avgpool8_kernel only loads eight channels at a time) and the
                     build has -ffp-contract=off and no fast math, so IEEE fp32 addition and division give these bits.
  average pool, 2    against the fp64 mean m:  |out - m| <= (hw - 1) * u * sum |x| / hw        sequential fp32 summation, first order
                                                           + u * |m|                             the division's rounding
                                                           + out_rounding(m)                     as in conv_ref: fp16 2^-11 |m| + 2^-14,
                                                                                                 fp32 4 u |m|
                     (fp32's 4 u |m| also holds the second-order terms the first line drops: hw <= 91 here, (hw u)^2 << u.)
  L2 normalise       out[c] = x[c] / max(sqrt(ss), 1e-12), fp32 out.  ss is summed per lane over T = ceil(c / 64) squares (one rounding
                     for the square, T - 1 for the lane's additions: the first adds to 0 exactly) and then through a six-step butterfly
                     (6 more): every square carries at most T + 6 roundings and all terms are >= 0, so ss is within (T + 6) u of exact,
                     relatively; the square root halves that and adds its own rounding u, the division adds u:
                     ((T + 6) / 2 + 2) u.  Doubled, as conv_ref doubles its accumulation bound (it then also holds a square root or a
                     division that is within one ulp rather than correctly rounded):
                         |out - ref| <= (T + 10) * u * |ref| + 2^-126                          (the floor: fp32's smallest normal)
                     An all-zero row gives ss = 0, x / 1e-12 = 0: exactly zero.
  fused ReID stem    conv 3x3/1 + bias + ReLU by conv_ref.layer_ref at fp16 (K = 27: accumulation 2 (K + 2) u S, output rounding
                     2^-11 |ref| + 2^-14), then the 3x3/2 maximum in fp64.  Rounding to fp16 is monotone, so it commutes with the
                     maximum: the kernel's pool-then-round equals round-then-pool.  |max a_i - max b_i| <= max |a_i - b_i|, so a pooled
                     element's tolerance is the largest tolerance in its window.
  fused YOLO stem    the integer letterbox of oracle/image_oracle.py (bit exact against the letterbox kernel, tests/test_gpu_pre_tracker.py),
                     / 255 in fp32, rounded to fp16, BGR -> RGB; then conv 3x3/2 + SiLU by layer_ref at fp16 with its tolerance.

Which kernel ran.  The launchers of the graph ops choose by shape alone; expected_kernel() restates their rules and every case names the
kernel it is there for -- a case whose shape no longer reaches its kernel fails on the CPU (tests/test_elt_ref.py) and on the device.
What the engine fuses or folds at load time is asked of the library itself (HipEngine.conv_plan) in tests/test_gpu_elt_ops.py.

measured on MI355X: see the table in tests/test_gpu_elt_ops.py."""
from dataclasses import dataclass

import numpy as np

import conv_ref as R
from oracle import image_oracle as I

ef = R.ef
U = R.U
NONE, SILU, RELU = R.NONE, R.SILU, R.RELU
NEG_INF = -np.inf


# ------------------------------------------------------------------------------------------------------------------ cases
@dataclass
class Case:
    id: str
    op: str                          # maxpool | sppf | upsample | avgpool | l2norm | reid_stem
    H: int                           # the op's SOURCE map (reid_stem: the engine input, W = 64)
    W: int
    c: int                           # channels the op reads
    n: int                           # items; every image is distinct
    dtype: str
    kernel: str                      # the kernel this case is there for: expected_kernel() must agree
    src_coff: int = 0
    dst_coff: int = 0                # > 0: the destination buffer is wider than the written slice and a stem (or a first op) filled all of it
    inplace: bool = False            # sppf: src == dst, dst_coff == c, as the YOLO graph does it
    bias: str = "mixed"              # mixed | low (every channel -1e5) | zero (every bias 0 and image 1 all zero)
    seed: int = 0


MP, UP, L2 = "maxpool3s2_kernel", "upsample2x_kernel", "l2norm_kernel"
SEP, DIRECT = "sppf_pool_sep_kernel", "sppf_pool_kernel"
AVG, AVG8 = "avgpool_kernel", "avgpool8_kernel"
STEM1, STEM2 = "reid_stem_pool_kernel", "reid_stem_pool2_kernel"


def _cases():
    C = []

    def add(id, op, H, W, c, n, kernel, dtypes=("fp16", "fp32"), **kw):
        for dt in dtypes:
            C.append(Case(f"{id}_{dt}", op, H, W, c, n, dt, kernel[dt] if isinstance(kernel, dict) else kernel, seed=len(C) + 1, **kw))
    # ---- max pool 3x3/2: odd both ways, even, one row, one column, smaller than the window; 13x7 c24 n5 is more than one block
    add("mp_13x7_c24", "maxpool", 13, 7, 24, 5, MP)
    add("mp_12x8_c8", "maxpool", 12, 8, 8, 1, MP)
    add("mp_1x9_c8", "maxpool", 1, 9, 8, 5, MP)
    add("mp_9x1_c24", "maxpool", 9, 1, 24, 1, MP)
    add("mp_2x2_c8", "maxpool", 2, 2, 8, 5, MP)
    add("mp_13x7_c24_slice", "maxpool", 13, 7, 24, 5, MP, src_coff=8, dst_coff=16)
    add("mp_13x7_c8_low", "maxpool", 13, 7, 8, 5, MP, dtypes=("fp32",), bias="low")        # whole windows below -65504
    # (the 64-channel max pool is the unfused fp32 run of the ReID stem graph, below)
    # ---- SPPF pooling.  launch_sppf_pool: the separable LDS kernel when 4 * h * w * 16 bytes <= 64 KB, i.e. h * w <= 1024, for both
    # element types; else the direct kernel.  20x20: the real map; 5x3, 1x1: every far tap clipped; 13x13, 14x12: the 6-tap reach ends
    # exactly at / one past the edge; 32x32: h * w == 1024, the last map the LDS form takes, four pixels per thread
    add("sppf_20x20_inplace", "sppf", 20, 20, 8, 2, SEP, inplace=True)
    add("sppf_5x3", "sppf", 5, 3, 8, 2, SEP)
    add("sppf_1x1", "sppf", 1, 1, 8, 2, SEP)
    add("sppf_13x13", "sppf", 13, 13, 8, 2, SEP)
    add("sppf_14x12_slice", "sppf", 14, 12, 8, 2, SEP, src_coff=8, dst_coff=8)
    add("sppf_32x32", "sppf", 32, 32, 8, 2, SEP)
    add("sppf_33x32_direct_slice", "sppf", 33, 32, 8, 2, DIRECT, src_coff=8, dst_coff=8)
    add("sppf_26x40_direct_inplace", "sppf", 26, 40, 8, 2, DIRECT, inplace=True)
    add("sppf_33x32_direct_low", "sppf", 33, 32, 8, 1, DIRECT, dtypes=("fp32",), bias="low")
    # ---- upsample 2x (H, W: the source)
    add("up_6x4_c16", "upsample", 6, 4, 16, 2, UP)
    add("up_1x1_c8", "upsample", 1, 1, 8, 2, UP)
    add("up_7x5_c24_slice", "upsample", 7, 5, 24, 2, UP, src_coff=8, dst_coff=8)
    # ---- global average pool.  launch_avgpool: avgpool8_kernel in an fp16 engine when c, both channel strides and both offsets are
    # multiples of 8; the scalar kernel otherwise (an fp16 graph reaches it with c = 20 or a destination offset of 4: buffers are whole
    # 16-byte vectors wide and source offsets whole vectors, channel counts and destination offsets of a non-conv op are free)
    add("ap_4x8_c64_n37", "avgpool", 4, 8, 64, 37, dict(fp16=AVG8, fp32=AVG))
    add("ap_1x1_c24_n1", "avgpool", 1, 1, 24, 1, dict(fp16=AVG8, fp32=AVG))
    add("ap_7x3_c20_n37", "avgpool", 7, 3, 20, 37, AVG)
    add("ap_13x7_c24_n1", "avgpool", 13, 7, 24, 1, dict(fp16=AVG8, fp32=AVG))
    add("ap_13x7_c16_slice_n37", "avgpool", 13, 7, 16, 37, dict(fp16=AVG8, fp32=AVG), src_coff=8, dst_coff=8)
    add("ap_7x3_c12_slice4_n37", "avgpool", 7, 3, 12, 37, AVG, src_coff=8, dst_coff=4)
    # ---- L2 normalise: c below, at and above one lane pass, four items per block
    add("l2_c40_n5", "l2norm", 1, 1, 40, 5, L2)
    add("l2_c64_n1", "l2norm", 1, 1, 64, 1, L2)
    add("l2_c200_n37", "l2norm", 1, 1, 200, 37, L2)
    add("l2_c512_n5", "l2norm", 1, 1, 512, 5, L2)
    add("l2_c200_slice_n5", "l2norm", 1, 1, 200, 5, L2, src_coff=8, dst_coff=8)
    add("l2_c64_zero_row_n5", "l2norm", 1, 1, 64, 5, L2, bias="zero")
    # ---- fused ReID stem (fp16): conv 3x3/1 3 -> 64 ReLU + max pool 3x3/2 at W = 64.  launch_reid_stem_pool: the second form when
    # reid_stem2_usable(H, W) = W == 64 and H % 16 == 0 and (H + 2) * 66 * 8 <= 150 KB; the load-time fusion also takes H % 8 == 0,
    # which then runs the first form.  H = 16: one pooled row per wave; H = 8: one row group
    for H in (16, 32, 128):
        add(f"stem2_H{H}", "reid_stem", H, 64, 64, 3, STEM2, dtypes=("fp16",))
    for H in (8, 24, 40):
        add(f"stem1_H{H}", "reid_stem", H, 64, 64, 3, STEM1, dtypes=("fp16",))
    add("stem2_H32_slice", "reid_stem", 32, 64, 64, 3, STEM2, dtypes=("fp16",), dst_coff=8)
    add("stem1_H24_slice", "reid_stem", 24, 64, 64, 3, STEM1, dtypes=("fp16",), dst_coff=8)
    # the same graph in an fp32 engine runs unfused: the max pool's 64-channel case
    add("stem_unfused_H16", "reid_stem", 16, 64, 64, 3, MP, dtypes=("fp32",))
    return C


CASES = _cases()

# ---- under a device-side item count (EltArgs::n_dev): the ops that cut their index range by it (kernels_elt.hip: maxpool3s2, avgpool,
# avgpool8, l2norm; the SPPF pool and the upsample belong to YOLO graphs and have none), the smallest cases of each in both element types
LIVE = ("mp_13x7_c24", "mp_13x7_c24_slice", "ap_4x8_c64_n37", "ap_7x3_c20_n37", "ap_13x7_c16_slice_n37", "l2_c40_n5", "l2_c200_n37",
        "l2_c200_slice_n5")
LIVE_CASES = [c for c in CASES if c.id.rsplit("_", 1)[0] in LIVE]


def live_counts(c: Case):
    """0, 1, n - 1 and n + 3 (a count may exceed the bound); L2 normalise, four items per block: also a count that is no multiple of
    four and not 1, so that a block's last wavefronts leave while its first ones work."""
    ks = {0, 1, c.n - 1, c.n + 3}
    if c.op == "l2norm":
        ks.add(next(k for k in (6, 3) if k < c.n))
    return tuple(sorted(ks))


def expected_kernel(c: Case, B) -> str:
    """The launchers' own rules (csrc/kernels_elt.hip, csrc/kernels_conv_direct.hip), restated from the case's graph."""
    if c.op == "sppf":
        return SEP if 4 * c.H * c.W * 16 <= 64 * 1024 else DIRECT
    if c.op == "avgpool":
        o = B.g.ops[B.layers["op"]["op"]]
        s_cs, d_cs = B.g.buffers[o[1]][2], B.g.buffers[o[4]][2]
        return AVG8 if c.dtype == "fp16" and o[3] % 8 == 0 and (s_cs | o[2] | d_cs | o[5]) % 8 == 0 else AVG
    if c.op == "reid_stem":
        if c.dtype != "fp16":
            return MP
        assert c.W == 64 and c.H % 8 == 0, "the load-time fusion does not take this map"
        return STEM2 if c.H % 16 == 0 and (c.H + 2) * 66 * 8 <= 150 * 1024 else STEM1
    return {"maxpool": MP, "upsample": UP, "l2norm": L2}[c.op]


# ------------------------------------------------------------------------------------------------------------------ graphs
def input_hw(c: Case):
    if c.op == "upsample":
        return 2 * c.H, 2 * c.W
    return c.H, c.W


def _up8(v):
    return (v + 7) // 8 * 8


def _bias(w, b, mode):
    b = b.copy()
    if mode == "mixed":                  # inputs lie in [-1, 1]: |w . x| <= sum |w|, so these channels are negative throughout
        neg = np.arange(len(b)) % 3 == 1
        b[neg] = -(np.abs(w).sum((1, 2, 3))[neg] + 0.5)
    elif mode == "low":
        b[:] = -1.0e5
    elif mode == "zero":
        b[:] = 0.0
    return b.astype(np.float32)


def build_graph(c: Case) -> R.Built:
    """KIND_REID engine: 1x1 stems 3 -> C with no activation, the op under test (layers["op"]), AVGPOOL -> L2NORM for the loader."""
    Hin, Win = input_hw(c)
    g = ef.Graph(ef.KIND_REID, Hin, Win)
    wg = ef._WeightGen(2000 + c.seed)
    B = R.Built(g)
    inp = g.buf(Hin, Win, ef.IN_C)
    B.bufs["inp"] = inp

    def conv(name, src, dst, cin, cout, k, s, act, bias=None, **kw):
        w, b = wg(cout, cin, k, act)
        b = _bias(w, b, c.bias if bias is None else bias)
        g.conv(name, src, dst, cin, cout, k, s, act, wb=(w, b), **kw)
        B.layers[name] = dict(op=len(g.ops) - 1, w=w, b=b, k=k, stride=s, act=act, res_mode=0, src=(src, kw.get("src_coff", 0), cin),
                              dst=(dst, kw.get("dst_coff", 0), cout), res=None)

    def elt(name, op, src, dst, ch, sc=0, dc=0):
        g.simple(op, src, dst, ch, src_coff=sc, dst_coff=dc)
        B.layers[name] = dict(op=len(g.ops) - 1)

    def out(e, ch):
        g.outputs.append([e, ch, 0, 0, 0, 0, 0, 0])
        g.meta = [ch, 0, 0, 0, 0, 0, 0, 0]
        return B

    def finish(last, ch):
        p = g.buf(1, 1, ch)
        g.simple(ef.OP_AVGPOOL, last, p, ch)
        e = g.buf(1, 1, ch, ef.DT_F32)
        g.simple(ef.OP_L2NORM, p, e, ch)
        return out(e, ch)

    H, W, ch, sc, dc = c.H, c.W, c.c, c.src_coff, c.dst_coff
    pad = 8 if dc else 0                                   # channels behind the written slice
    if c.op == "maxpool":
        oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x, y = g.buf(H, W, sc + ch), g.buf(oh, ow, dc + ch + pad)
        B.bufs.update(x=x, y=y)
        conv("stem", inp, x, 3, sc + ch, 1, 1, NONE)
        if dc:
            conv("stem_dst", inp, y, 3, dc + ch + pad, 1, 2, NONE)
        elt("op", ef.OP_MAXPOOL3S2, x, y, ch, sc, dc)
        return finish(y, dc + ch + pad)
    if c.op == "sppf":
        if c.inplace:
            x = y = g.buf(H, W, 4 * ch)
            conv("stem", inp, x, 3, 4 * ch, 1, 1, NONE)    # all four slices: the pool overwrites three of them
            sc, dc = 0, ch
        else:
            x, y = g.buf(H, W, sc + ch), g.buf(H, W, dc + 3 * ch + pad)
            conv("stem", inp, x, 3, sc + ch, 1, 1, NONE)
            if dc:
                conv("stem_dst", inp, y, 3, dc + 3 * ch + pad, 1, 1, NONE)
        B.bufs.update(x=x, y=y)
        elt("op", ef.OP_SPPF_POOL, x, y, ch, sc, dc)
        return finish(y, g.buffers[y][2])
    if c.op == "upsample":
        cd = dc + ch + 8
        x, y, r = g.buf(H, W, sc + ch), g.buf(2 * H, 2 * W, cd), g.buf(2 * H, 2 * W, 16)
        B.bufs.update(x=x, y=y, r=r)
        conv("stem", inp, x, 3, sc + ch, 1, 2, NONE)
        conv("stem_dst", inp, y, 3, cd, 1, 1, NONE)        # a second writer of the slice and ...
        elt("op", ef.OP_UPSAMPLE2X, x, y, ch, sc, dc)
        conv("reader", y, r, cd, 16, 3, 1, SILU, bias="plain")     # ... a 3x3 reader: the load-time fold into a 1x1 reader cannot take the op
        return finish(r, 16)
    if c.op == "avgpool":
        cd = _up8(dc + ch) + pad
        x, y = g.buf(H, W, _up8(sc + ch)), g.buf(1, 1, cd)
        B.bufs.update(x=x, y=y)
        conv("stem", inp, x, 3, _up8(sc + ch), 1, 1, NONE)
        if dc:                                             # a 1x1 map has no stem: a first average pool fills the whole destination
            pre = g.buf(H, W, cd)
            B.bufs["pre"] = pre
            conv("stem_pre", inp, pre, 3, cd, 1, 1, NONE)
            elt("prefill", ef.OP_AVGPOOL, pre, y, cd)
        elt("op", ef.OP_AVGPOOL, x, y, ch, sc, dc)
        e = g.buf(1, 1, cd, ef.DT_F32)
        g.simple(ef.OP_L2NORM, y, e, cd)
        return out(e, cd)
    if c.op == "l2norm":
        cd = dc + ch + pad
        x, y = g.buf(1, 1, sc + ch), g.buf(1, 1, cd, ef.DT_F32)
        B.bufs.update(x=x, y=y)
        conv("stem", inp, x, 3, sc + ch, 1, 1, NONE)
        if dc:
            pre = g.buf(1, 1, cd)
            B.bufs["pre"] = pre
            conv("stem_pre", inp, pre, 3, cd, 1, 1, NONE)
            elt("prefill", ef.OP_L2NORM, pre, y, cd)
        elt("op", ef.OP_L2NORM, x, y, ch, sc, dc)
        return out(y, cd)
    if c.op == "reid_stem":
        assert W == 64 and ch == 64 and H % 2 == 0
        cd = dc + 64 + pad
        a, y = g.buf(H, W, 64), g.buf(H // 2, W // 2, cd)
        B.bufs.update(a=a, y=y)
        if dc:
            conv("stem_dst", inp, y, 3, cd, 1, 2, NONE)
        conv("conv0", inp, a, 3, 64, 3, 1, RELU)           # every third channel negative over every neighbourhood: pooled values exactly 0
        elt("op", ef.OP_MAXPOOL3S2, a, y, 64, 0, dc)
        return finish(y, cd)
    raise ValueError(c.op)


def images(c: Case):
    """[n, 3, Hin, Win] fp32, uniform in [-1, 1], every image distinct; bias == "zero": image 1 is all zero."""
    Hin, Win = input_hw(c)
    x = np.random.default_rng(99 + c.seed).uniform(-1.0, 1.0, (c.n, 3, Hin, Win)).astype(np.float32)
    if c.bias == "zero":
        x[1] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------------ references
def _window_max(x, ry, rx, sy=1, sx=1, oy=0, ox=0, fill=NEG_INF, oh=None, ow=None):
    """out[y, x] = max over |dy| <= ry, |dx| <= rx of x[sy * y + oy + dy, sx * x + ox + dx]; taps outside the map count as `fill`
    (-inf: ignored).  x [n, H, W, C] fp64."""
    n, H, W, C = x.shape
    oh = (H - 1) // sy + 1 if oh is None else oh
    ow = (W - 1) // sx + 1 if ow is None else ow
    py, px = ry + abs(oy) + sy, rx + abs(ox) + sx
    xp = np.full((n, H + 2 * py, W + 2 * px, C), fill, np.float64)
    xp[:, py:py + H, px:px + W] = x
    out = np.full((n, oh, ow, C), NEG_INF)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            y0, x0 = py + oy + dy, px + ox + dx
            out = np.maximum(out, xp[:, y0:y0 + sy * (oh - 1) + 1:sy, x0:x0 + sx * (ow - 1) + 1:sx])
    return out


def maxpool3s2_ref(x, mut=None):
    """PyTorch max_pool2d(3, 2, 1): out-of-image taps ignored."""
    kw = {"border0": dict(fill=0.0), "row": dict(oy=1), "col": dict(ox=1), "centre": dict(oy=1, ox=1)}.get(mut, {})
    return _window_max(x, 1, 1, 2, 2, **kw)


def sppf_ref(x, mut=None):
    """Three cascaded 5x5/1 max pools with -inf padding -> (m5, m9, m13) side by side in the channels."""
    kw = {"border0": dict(fill=0.0), "row": dict(oy=1), "col": dict(ox=1)}.get(mut, {})
    m5 = _window_max(x, 2, 2, **kw)
    m9 = _window_max(m5, 2, 2, **kw)
    m13 = _window_max(m9, 2, 2, **kw)
    if mut == "m9_reach":
        m9 = m13
    return np.concatenate([m5, m9, m13], -1)


def sppf_windows(x):
    """The same three tensors as the 5, 9 and 13 windows of the input."""
    return np.concatenate([_window_max(x, r, r) for r in (2, 4, 6)], -1)


def upsample2x_ref(x, mut=None):
    if mut == "round":                                   # source index rounded instead of floored
        iy = np.minimum((np.arange(2 * x.shape[1]) + 1) >> 1, x.shape[1] - 1)
        ix = np.minimum((np.arange(2 * x.shape[2]) + 1) >> 1, x.shape[2] - 1)
        return x[:, iy][:, :, ix]
    return x.repeat(2, 1).repeat(2, 2)


def avgpool_f32(x, dtype, mut=None):
    """The kernels' arithmetic restated: sequential fp32 sum over p = 0 .. hw-1, / fp32 hw, rounded to the element type.
    x [n, H, W, C] (values of the element type) -> fp64 [n, 1, 1, C]."""
    n, H, W, C = x.shape
    v = np.asarray(x, np.float32).reshape(n, H * W, C)
    s = np.zeros((n, C), np.float32)
    for p in range(H * W):
        s = (s + v[:, p]).astype(np.float32)
    hw = np.float32(H * W + (1 if mut == "divisor" else 0))
    return R.to_elem((s / hw).astype(np.float32), dtype).reshape(n, 1, 1, C)


def avgpool_ref(x, dtype):
    """-> (fp64 mean, tolerance): see the module docstring."""
    n, H, W, C = x.shape
    hw = H * W
    m = x.reshape(n, hw, C).mean(1)
    tol = (hw - 1) * U * np.abs(x).reshape(n, hw, C).sum(1) / hw + U * np.abs(m) + R.out_rounding(m, dtype == "fp16")
    return m.reshape(n, 1, 1, C), tol.reshape(n, 1, 1, C)


def l2norm_ref(x, mut=None):
    """x [n, 1, 1, C] -> (fp64 x / max(|x|, 1e-12), tolerance)."""
    C = x.shape[-1]
    xs = x[..., :C // 64 * 64] if mut == "tail_dropped" else x          # the channels past a multiple of 64 left out of the sum
    nrm = np.maximum(np.sqrt((xs * xs).sum(-1, keepdims=True)), 1e-12)
    ref = x / nrm
    T = -(-C // 64)
    return ref, (T + 10) * U * np.abs(ref) + 2.0 ** -126


def exact_tol(ref, dtype):
    """Bit exactness through worst_ratio: any element that differs is at least one ulp away, i.e. a ratio >= 2."""
    return R.ulp(ref, dtype) / 2


def _edge_conv(x, l, dtype):
    """conv0 with its zero padding replaced by edge replication (a stem mutant): the "same" conv of the edge-padded input, whose inner
    outputs never touch layer_ref's own zero padding."""
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    return R.layer_ref(xp, l["w"], l["b"], 3, 1, RELU, dtype)[0][:, 1:-1, 1:-1]


def reid_stem_ref(x, l, mut=None):
    """x [n, H, 64, 3] (the input buffer as read back) -> (pooled reference, pooled tolerance) of conv0 + ReLU + max pool at fp16."""
    act = NONE if mut == "no_relu" else RELU
    ref, tol, _ = R.layer_ref(x, l["w"], l["b"], 3, 1, act, "fp16")
    if mut == "edge_pad":
        ref = _edge_conv(x, l, "fp16")
    pooled, ptol = maxpool3s2_ref(ref), maxpool3s2_ref(tol)
    if mut == "tile":                                    # pooled column 8, 16, 24 takes its left neighbour from pixel 15 of its OWN 16-pixel tile
        pooled = pooled.copy()
        for px in (8, 16, 24):
            col = np.stack([ref[:, :, 2 * px + 15], ref[:, :, 2 * px], ref[:, :, 2 * px + 1]], 2)        # [n, H, 3, C]
            pooled[:, :, px] = _window_max(col, 1, 1, 2, 1)[:, :, 1]
    elif mut == "groups":                                # two 8-channel groups swapped
        pooled = np.concatenate([pooled[..., 8:16], pooled[..., 0:8], pooled[..., 16:]], -1)
    return pooled, ptol


STEM_MUTANTS = ("tile", "groups", "no_relu", "edge_pad")
OP_MUTANTS = {"maxpool": ("border0", "row", "col", "centre", "init65504"), "sppf": ("border0", "row", "col", "m9_reach", "init65504"),
              "upsample": ("round",), "avgpool": ("divisor",), "l2norm": ("tail_dropped",), "reid_stem": STEM_MUTANTS}
SLICE_MUTANTS = ("coff", "image")


def applicable(c: Case, mut):
    """Whether a mutant CAN change the case's output, from the shape alone (written down, not found by trying):
    border0: some window hangs over the border -- every map here for the pools (2x2 and 1x9 included); row / col shift of a 3- or
    5-window: the last output row loses input row H - 3 (3x3/2: row 2 enters window 0), so H >= 3 / W >= 3; m9_reach: some 13-window
    sees more than the 9-window, max(H, W) > 5; round: a source larger than one pixel; tail_dropped: c % 64 != 0; init65504: the low
    cases; coff: a source offset; image: more than one item."""
    fused = c.op == "reid_stem" and c.dtype == "fp16"
    if c.op == "reid_stem" and not fused:
        return mut in ("row", "col", "centre", "image")          # (its pool sees ReLU outputs: a border tap read as 0 changes nothing)
    if mut in STEM_MUTANTS:
        return fused
    return {"border0": c.bias != "zero", "row": c.H >= 3, "col": c.W >= 3, "centre": c.H >= 3 or c.W >= 3, "m9_reach": max(c.H, c.W) > 5,
            "round": c.H > 1 or c.W > 1, "divisor": True, "tail_dropped": c.c % 64 != 0, "init65504": c.bias == "low",
            "coff": c.src_coff > 0, "image": c.n > 1}[mut]


def mutants(c: Case):
    ops = OP_MUTANTS["maxpool"] if c.op == "reid_stem" and c.dtype != "fp16" else OP_MUTANTS[c.op]
    return tuple(m for m in ops + SLICE_MUTANTS if applicable(c, m))


def case_reference(c: Case, B, read, mut=None):
    """-> rows (name, buffer name, first channel, ref, tol, exact) to compare; read(buffer name) -> fp64 [n, h, w, C] of what the device
    holds.  The first row is the op under test; the others are the channels around the written slice (and, in place, the source slice),
    which must still hold what the stem put there.  mut: None or one of mutants(c), applied to the first row's reference."""
    L, dt = B.layers, c.dtype
    sc, dc, ch = c.src_coff, c.dst_coff, c.c
    if c.op == "sppf" and c.inplace:
        sc, dc = 0, ch
    rows = []

    def stem_rows(name, buf, skip0, skip1):
        """The stem's own reference for the channels of `buf` outside [skip0, skip1)."""
        l = L[name]
        ref, tol, _ = R.layer_ref(read("inp")[..., :3], l["w"], l["b"], l["k"], l["stride"], l["act"], dt)
        for c0, c1 in ((0, skip0), (skip1, ref.shape[-1])):
            if c1 > c0:
                rows.append((f"{name}[{c0}:{c1}]", buf, c0, ref[..., c0:c1], tol[..., c0:c1], False))

    if c.op == "reid_stem":
        if dt == "fp16":
            ref, tol = reid_stem_ref(read("inp")[..., :3], L["conv0"], mut=mut if mut in STEM_MUTANTS else None)
            if mut == "image":
                ref = np.roll(ref, -1, 0)
            rows.append(("conv0+pool", "y", dc, ref, tol, False))
        else:
            a = read("a")
            a = np.roll(a, -1, 0) if mut == "image" else a
            ref = maxpool3s2_ref(a, mut)
            rows.append(("pool", "y", dc, ref, exact_tol(ref, dt), True))
        if dc:
            stem_rows("stem_dst", "y", dc, dc + 64)
        return rows

    xfull = read("x")
    x = xfull[..., 0:ch] if mut == "coff" else xfull[..., sc:sc + ch]
    if mut == "image":
        x = np.roll(x, -1, 0)
    opmut = mut if mut in OP_MUTANTS[c.op] else None
    if c.op in ("maxpool", "sppf", "upsample"):
        ref = {"maxpool": maxpool3s2_ref, "sppf": sppf_ref, "upsample": upsample2x_ref}[c.op](x, None if opmut == "init65504" else opmut)
        if opmut == "init65504":                         # the maximum started at the lowest finite fp16 value in an fp32 engine
            ref = np.maximum(ref, -65504.0)
        rows.append((c.op, "y", dc, ref, exact_tol(ref, dt), True))
        if c.op == "sppf" and c.inplace:
            stem_rows("stem", "y", ch, 4 * ch)           # the source slice is unchanged
        elif "stem_dst" in L:
            stem_rows("stem_dst", "y", dc, dc + ref.shape[-1])
        return rows
    if c.op == "avgpool":
        bits = avgpool_f32(x, dt, opmut)
        m, tol = avgpool_ref(x, dt)
        rows.append(("avgpool bits", "y", dc, bits, exact_tol(bits, dt), True))
        rows.append(("avgpool fp64", "y", dc, m if mut is None else bits, tol, False))      # a mutant: what the wrong kernel would store
        cd = B.g.buffers[B.bufs["y"]][2]
        outside = avgpool_f32(read("pre"), dt) if dc else np.zeros((c.n, 1, 1, cd))      # no first pool: the loader's zeros
        for c0, c1 in ((0, dc), (dc + ch, cd)):
            if c1 > c0:
                rows.append((f"outside[{c0}:{c1}]", "y", c0, outside[..., c0:c1], exact_tol(outside[..., c0:c1], dt), True))
        return rows
    if c.op == "l2norm":
        ref, tol = l2norm_ref(x, opmut)
        rows.append(("l2norm", "y", dc, ref, tol, False))
        if dc:
            o, otol = l2norm_ref(read("pre"))
            for c0, c1 in ((0, dc), (dc + ch, o.shape[-1])):
                rows.append((f"outside[{c0}:{c1}]", "y", c0, o[..., c0:c1], otol[..., c0:c1], False))
        return rows
    raise ValueError(c.op)


def rows_under_test(c: Case):
    """How many of case_reference's first rows belong to the op under test."""
    return 2 if c.op == "avgpool" else 1


def host_inputs(c: Case, B, x):
    """CPU stand-in for the device read-back (tests/test_elt_ref.py): every buffer a conv writes straight from the input, computed by
    conv_ref's reference from the images x [n, 3, Hin, Win] and rounded to the element type."""
    Hin, Win = input_hw(c)
    vals = {"inp": np.zeros((c.n, Hin, Win, ef.IN_C))}
    vals["inp"][..., :3] = R.to_elem(x.transpose(0, 2, 3, 1), c.dtype)
    for l in B.layers.values():
        if "src" not in l or l["src"][0] != B.bufs["inp"]:
            continue
        bname = next(k for k, v in B.bufs.items() if v == l["dst"][0])
        ref = R.to_elem(R.layer_ref(vals["inp"][..., :3], l["w"], l["b"], l["k"], l["stride"], l["act"], c.dtype)[0], c.dtype)
        if bname not in vals:
            hw = B.g.buffers[l["dst"][0]]
            vals[bname] = np.zeros((c.n, hw[0], hw[1], hw[2]))
        vals[bname][..., l["dst"][1]:l["dst"][1] + l["dst"][2]] = ref
    return vals


# ------------------------------------------------------------------------------------------------------------------ fused YOLO stem
YOLO_IN_HW = (64, 128)                   # the smallest input the fused stem takes: 32 x 64 stem outputs = rows % 8 == 0, columns % 32 == 0
# frame (h, w) -> what the letterbox does with it at 64 x 128.  Two frames per call: the last pixels of the second one reach the byte
# loads behind `frames_limit` where the 2 x 2 area path would read 12 bytes past the frames handed in.
YOLO_FRAMES = {
    "area2_96x256": (96, 256),           # exactly 2:1 -> 48 x 128, 8 padding rows above and below: the aligned 12-byte loads and their byte fallback
    "down_100x300": (100, 300),          # ratio 0.4267 -> 43 x 128: the generic resampler, 10 / 11 padding rows
    "small_40x100": (40, 100),           # smaller than the canvas: the letterbox never enlarges (scaleup=False), so the generic resampler
                                         # runs at scale 1 and the frame is padded on all four sides
    "same_64x128": (64, 128),            # already at the target size: no padding at all
}
YOLO_MUTANTS = ("pad0", "bgr", "parity")


def yolo_frames(name):
    h, w = YOLO_FRAMES[name]
    rng = np.random.default_rng(500 + sorted(YOLO_FRAMES).index(name))
    return rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)


def yolo_applicable(name, mut):
    return name != "same_64x128" if mut == "pad0" else True                  # pad colour: only where there is padding


def yolo_stem_input(frames, mut=None):
    """u8 BGR frames -> what the stem convolves: the integer letterbox, / 255 in fp32, rounded to fp16, RGB; fp64 [n, 64, 128, 3]."""
    lb = np.stack([I.letterbox_u8(f, YOLO_IN_HW, color=0 if mut == "pad0" else 114)[0] for f in frames])
    assert lb.shape[1:] == YOLO_IN_HW + (3,)
    x = (lb.astype(np.float32) / np.float32(255.0)).astype(np.float16).astype(np.float64)
    if mut != "bgr":
        x = x[..., ::-1]
    if mut == "parity":                                  # even and odd input columns taken for each other
        x = x.reshape(x.shape[0], x.shape[1], -1, 2, 3)[:, :, :, ::-1].reshape(x.shape)
    return np.ascontiguousarray(x)


def yolo_stem_ref(frames, w, b, mut=None):
    """-> (ref, tol) [n, 32, 64, 16] of 0.conv (3x3/2, SiLU) on the letterboxed frames at fp16."""
    return R.layer_ref(yolo_stem_input(frames, mut), w, b, 3, 2, SILU, "fp16")[:2]
