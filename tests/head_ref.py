"""Detect-head harness: small YOLOv8n engines with planted detect-branch 1x1s, the references for what the conv epilogue decodes in
place (tail_1x1 in csrc/conv_common.hpp: max logit + first arg-max per anchor, the DFL-decoded box), and the case table.  Plain NumPy /
torch on the CPU: tests/test_gpu_head_tails.py runs the cases on the device, tests/test_head_ref.py checks on the CPU -- through
oracle.nets_oracle.EngineOracle on the case's images -- that every builder delivers what it promises and that each planted variant of
the epilogue's rules changes an expected output of at least one case.

Engines: engine_file.build_yolov8("n", nc, in_hw, seed) on NON-SQUARE inputs (w != h on every level), so that cell / width and
cell / height, and one level's first anchor and the next one's, give different answers.  With scale "n" the box branch leads with 64
channels and the class branch with max(64, nc): nc = 80 is the five-tile (NT = 5) epilogue without padding, nc <= 64 the four-tile one
whose channels nc .. 63 are padding (zero weight rows, zero bias: they hold 0 + 0), nc = 72 a lead no tail takes, nc = 3 a tail the
planner refuses (its fp32 output's channel stride is no multiple of 8).

Plants, into the weights (w, b) of `22.box{l}.2` / `22.cls{l}.2`.  Every planted WEIGHT is exactly representable in fp16, so the
engine's rounding of weights changes nothing in what was planted (biases stay fp32 on the device):
  pairs    class ties at the maximum: row j2 := row j1, the pair's weights times a gain (rounded to fp16), the bias copied as it is
           (the seeded class bias sits near -4 for every row: a gain on it would sink or lift the pair as a whole, on the weights it
           widens the pair's spread around the other rows' level, which is what makes it the maximum at a share of the anchors; where
           the row's products lean negative on the case's images the gain is negative).  Both
           rows are the same numbers through the same K-steps: equal fp32 logits at every anchor.  Expected label: the lower channel.
  shift    all real logits negative: every class bias minus 120 (the planted pairs reach up to 80 above the rest).  The padded channels of the 64-wide tile hold 0 and would win.
  exact    box weights zero, bias +40 at one bin per side (EXACT_BINS: four different bins per level, with 0, 15, one of 1 .. 7 and one
           of 8 .. 14): every anchor decodes to ((gx + .5 - k_l) s, (gy + .5 - k_t) s, (gx + .5 + k_r) s, (gy + .5 + k_b) s), exact in
           fp32 (det_ref's docstring), a function of level, column and row.
  equal    box weights zero, a constant bias per level: sum = 16, expectation = 120, dist = 7.5 exactly.
  spans    the seeded box weights times a small per-level gain (rounded to fp16) on top of a bias row per side whose span is 24, 10, 22
           or 4 (values on a grid of 1/8).  A row's span lies within the bias span -/+ the range of the weight term; the gains keep
           that range below 4 on the oracle, so the sides of span 24 (a quarter of the rows) stay in 20 .. 28: wide, dependent on the
           anchor, and inside the range det_ref.decode_tolerance is argued for (<= 30).  (The seeded weights alone, whatever the gain:
           where a tenth of the rows reaches 20 the widest passes 30 -- the spread of a range of 16 values over thousands of rows.)

Floors, asserted on the device's own raw logits by the GPU test: per planted pair PAIR_FLOOR anchors (of the DISTINCT images) where
the pair is the strict row maximum and as many where it is not; SPAN_SHARE of the rows with a span >= 20, none above SPAN_MAX; every
real logit below NEG_BOUND under a shift.  The device's fp16 activations differ a little from the fp32 oracle's, so gains and seeds are
chosen for ORACLE_MARGIN times the anchor floors on the oracle (test_head_ref; the oracle's figures stand next to each case)."""
import functools
from dataclasses import dataclass

import numpy as np

import det_ref as R
from conftest import pkg
from oracle import nets_oracle as N

ef = pkg("engine_file")

PAIR_FLOOR, ORACLE_MARGIN = 32, 4
SPAN_WIDE, SPAN_SHARE, SPAN_MAX = 20.0, 0.10, 30.0
SPAN_MAX_ORACLE, WEIGHT_RANGE_ORACLE = 28.5, 4.0               # what the oracle must show: 5 % of room for the fp16 activations
NEG_SHIFT, NEG_BOUND = np.float32(-120.0), -20.0
HOT = np.float32(40.0)
EXACT_BINS = ((0, 15, 3, 12), (15, 0, 9, 6), (5, 10, 0, 15))    # per level: (left, top, right, bottom)
EQUAL_BIAS = (0.5, 1.5, -2.25)                                 # (not 0: a buffer of zeros is what "never written" looks like)
SPAN_SIDES = (24.0, 10.0, 22.0, 4.0)                            # bias spans of the four sides, rotated by the level

# plan_tail's ten outcomes (csrc/conv_plan.cpp), as aic_model_conv_plan reports them
OUTCOMES = {
    "pm16x80": dict(form="PmPatch", mt=4, nt=5, th=16, tw=16),
    "pm40x64": dict(form="PmPatch", mt=5, nt=4, th=40, tw=8),
    "pm16x64": dict(form="PmPatch", mt=4, nt=4, th=16, tw=16),
    "patch": dict(form="Patch", mt=4, nt=4, wm=4, wn=1),
    "dma4x4": dict(form="Dma", mt=4, nt=4, wm=4, wn=1),
    "dma2x4": dict(form="Dma", mt=2, nt=4, wm=4, wn=1),
    "wide2x4": dict(form="Wide", mt=2, nt=4, wm=4, wn=1),
    "dma4x5": dict(form="Dma", mt=4, nt=5, wm=8, wn=1),
    "dma2x5": dict(form="Dma", mt=2, nt=5, wm=4, wn=1),
    "wide2x5": dict(form="Wide", mt=2, nt=5, wm=4, wn=1),
}
WIDTH_OF = {k: 16 * v["nt"] for k, v in OUTCOMES.items()}        # channels of the lead
NEEDS = {k: ({"box", "cls"} if WIDTH_OF[k] == 64 else {"cls"}) for k in OUTCOMES}   # the 80-channel leads only carry class tails


@dataclass(frozen=True)
class Case:
    id: str
    in_hw: tuple                # (H, W), multiples of 32, H != W
    nc: int
    seed: int
    P: int                      # distinct images; n images = these tiled
    n: int                      # images per run -- or, with `want`, the cap below which the smallest n is searched
    want: tuple                 # () or (branch, level, outcome): run at the smallest n at which that lead is planned as `outcome`
    leads: tuple                # per level (box outcome, class outcome); class outcome None: no tail, decode_kernel classifies
    pairs: tuple                # per level None or (j1, j2, gain)
    shift: bool                 # every class bias + NEG_SHIFT
    box: str                    # "exact" / "equal" / "spans"
    box_gain: tuple = (0, 0, 0)  # spans: per-level gain of the seeded weights
    cls_cin64: bool = False     # `22.cls{l}.1` of levels 1, 2 reads channels 64 .. 127 of the level's feature map instead, with seeded weights [nc, 64, 3, 3]

    @property
    def cls_width(self):
        return max(64, min(self.nc, 100))

    @property
    def cls_tail(self):
        """Whether the class 1x1 rides in its lead's epilogue at all (conv_tail_supported)."""
        return self.cls_width in (64, 80) and self.nc % 8 == 0


W24, W25, D25 = ("wide2x4", "wide2x4"), ("wide2x4", "wide2x5"), ("wide2x4", "dma2x5")
# Shapes: A = 64 x 128 (levels 8x16, 4x8, 2x4: neither strips nor 16 x 16 cover), B = 320 x 64 (40x8: strips), C = 96 x 128 (12x16: 16 x 16
# tiles cover it within + 50 %, a quarter of each tile hangs over the edge), D = 160 x 96 (20x12: too narrow for Patch), F = 192 x 320
# (24x40, 12x20, 6x10: the small-n cases, with enough anchors on every level for a pair).
# Oracle figures per planted pair: (anchors where the pair is the strict maximum / where it is not) of the P distinct images.
CASES = (
    # nc = 80: the odd fifth tile.  (66, 77): inside it, across its lanes; (2, 79): reaches into it; (78, 79): one lane of it
    Case("pm16_nc80", (96, 128), 80, 11, 5, 320, ("cls", 0, "pm16x80"), (("pm16x64", "pm16x80"), D25, D25),
         ((66, 77, 3.0), None, None), False, "spans", (0.059, 0.076, 0.069)),       # pair 488 / 472
    Case("patch_nc80", (64, 128), 80, 12, 5, 1700, ("box", 0, "patch"), (("patch", "dma4x5"), ("dma2x4", "dma2x5"), D25),
         ((2, 79, 6.0), None, None), False, "exact"),                                    # 301 / 339
    Case("small_nc80", (192, 320), 80, 13, 8, 8, (), (D25, D25, D25),
         ((78, 79, 4.0), (5, 50, -2.0), (3, 12, -8.0)), False, "equal"),                   # 3165 / 4515, 1482 / 438, 247 / 233
    # (the wide-step kernel wants Cin % 32 == 0, and every 80-channel lead build_yolov8 makes reads 80 channels: the one way to its 2 x 5
    #  tail is a class lead re-pointed at 64 channels of the level's feature map -- cls_cin64, on the levels whose map is wider than that)
    Case("cin64_nc80", (192, 320), 80, 14, 8, 8, (), (D25, W25, W25),
         ((1, 2, 16.0), (66, 77, -2.0), (2, 79, -3.0)), False, "spans", (0.13, 0.14, 0.125), True),   # 3636 / 4044, 917 / 1003, 278 / 202
    # nc <= 64: the four-tile reduction, channels nc .. 63 padding
    Case("strips_nc56", (320, 64), 56, 15, 5, 200, ("box", 0, "pm40x64"), (("pm40x64", "pm40x64"), W24, W24),
         ((2, 55, -8.0), (54, 55, 3.0), None), True, "equal"),                             # 659 / 941, 217 / 183
    Case("dma4_nc40", (160, 96), 40, 16, 5, 320, ("box", 0, "dma4x4"), (("dma4x4", "dma4x4"), W24, W24),
         ((3, 12, 8.0), None, None), True, "spans", (0.094, 0.064, 0.077)),                # 524 / 676
    Case("patch_nc24", (64, 128), 24, 17, 5, 1700, ("box", 0, "patch"), (("patch", "patch"), ("dma2x4", "dma2x4"), W24),
         ((1, 2, -4.0), None, None), True, "spans", (0.165, 0.195, 0.19)),                 # 299 / 341
    Case("pm16_nc8", (96, 128), 8, 18, 5, 320, ("box", 0, "pm16x64"), (("pm16x64", "pm16x64"), W24, W24),
         ((6, 7, 6.0), None, None), True, "exact"),                                       # 462 / 498
    Case("dma2_nc64", (64, 128), 64, 19, 5, 320, ("box", 0, "dma2x4"), (("dma2x4", "dma2x4"), W24, W24),
         ((5, 50, -16.0), None, None), False, "spans", (0.1, 0.092, 0.105)),               # 332 / 308
    Case("small_nc64", (192, 320), 64, 20, 8, 8, (), (W24, W24, W24),
         ((62, 63, -8.0), (2, 63, 4.0), (1, 2, -6.0)), False, "exact"),                    # 3479 / 4201, 886 / 1034, 212 / 268
    # fallbacks: the class half is decode_kernel's, the box half still the tail's
    Case("fallback_nc3", (160, 96), 3, 21, 3, 3, (), (("wide2x4", None), ("wide2x4", None), ("wide2x4", None)),
         ((1, 2, 0.5), None, None), False, "spans", (0.125, 0.12, 0.11)),                  # 222 / 498
    Case("fallback_nc72", (160, 96), 72, 22, 3, 3, (), (("wide2x4", None), ("wide2x4", None), ("wide2x4", None)),
         ((2, 71, -3.0), None, None), False, "exact"),                                    # 376 / 344
)


def levels_of(in_hw):
    return tuple((s, in_hw[0] // s, in_hw[1] // s) for s in (8, 16, 32))


def head_of(c):
    return R.Head(levels=levels_of(c.in_hw), nc=c.nc)


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def _conv(g, name):
    """-> (op index, weight index) of conv `name`, through the op list."""
    wi = g.names.index(name)
    return next(i for i, o in enumerate(g.ops) if o[0] == ef.OP_CONV and o[15] == wi), wi


def _span_bias(rng, span):
    v = rng.integers(0, int(span * 8) + 1, 16).astype(np.float32) / np.float32(8)
    v[0], v[1] = 0.0, span
    return rng.permutation(v)


@dataclass
class Built:
    g: object
    head: object
    ops: dict                   # (branch, level) -> (lead op, 1x1 op)
    bufs: dict                  # (branch, level) -> the level's fp32 logits buffer


@functools.lru_cache(maxsize=None)
def build(c):
    """The case's graph with its plants."""
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                     # (the calibration's convs are tiny: a thread pool only gets in their way)
    try:
        g = ef.build_yolov8("n", nc=c.nc, in_hw=c.in_hw, seed=c.seed)
    finally:
        torch.set_num_threads(threads)
    rng = np.random.default_rng(1000 + c.seed)
    ops, bufs = {}, {}
    for l in (1, 2) if c.cls_cin64 else ():
        lead, wi = _conv(g, f"22.cls{l}.1")
        stem = g.ops[_conv(g, f"22.box{l}.0")[0]]                # reads the level's feature map, 128 / 256 channels wide
        assert stem[3] >= 128 and g.ops[lead][6] == c.cls_width
        g.ops[lead][1:4] = [stem[1], stem[2] + 64, 64]           # (a slice no other conv reads: the engine merges convs that read the same one)
        w = rng.standard_normal((c.cls_width, 64, 3, 3)) / np.sqrt(0.356 * 576)       # (engine_file._WeightGen's scale for a SiLU conv)
        g.weights[wi] = (w.astype(np.float32), np.array(g.weights[wi][1], np.float32))
    for l in range(3):
        for br in ("box", "cls"):
            lead, _ = _conv(g, f"22.{br}{l}.1")
            one, wi = _conv(g, f"22.{br}{l}.2")
            assert g.ops[one][1] == g.ops[lead][4] and g.ops[one][4] == g.outputs[l][br == "cls"]
            ops[br, l], bufs[br, l] = (lead, one), g.ops[one][4]
            w, b = (np.array(v, np.float32) for v in g.weights[wi])
            if br == "cls":
                if c.pairs[l]:
                    j1, j2, gain = c.pairs[l]
                    assert 0 <= j1 < j2 < c.nc
                    w[j1] = w[j2] = _f16(w[j1] * np.float32(gain))
                    b[j2] = b[j1]
                if c.shift:
                    b += NEG_SHIFT
            elif c.box == "exact":
                w[:], b[:] = 0.0, 0.0
                for sd, k in enumerate(EXACT_BINS[l]):
                    b[16 * sd + k] = HOT
            elif c.box == "equal":
                w[:], b[:] = 0.0, EQUAL_BIAS[l]
            else:
                w = _f16(w * np.float32(c.box_gain[l]))
                for sd in range(4):
                    b[16 * sd:16 * sd + 16] = _span_bias(rng, SPAN_SIDES[(sd + l) % 4])
            g.weights[wi] = (w, b)
    return Built(g, head_of(c), ops, bufs)


def base_images(c):
    return np.random.default_rng(c.seed).random((c.P, 3) + tuple(c.in_hw), dtype=np.float32)


def tiled(base, n):
    return np.ascontiguousarray(base[np.arange(n) % len(base)])


def oracle_head(c):
    """The fp32 oracle's raw head of the case's distinct images: dfl [P, A, 64], cls [P, A, nc]."""
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        dfl, cls = N.EngineOracle(ef.serialize(build(c).g)).yolo_head(torch.from_numpy(base_images(c)))
    finally:
        torch.set_num_threads(threads)
    return dfl.numpy(), cls.numpy()


# ---------------------------------------------------------------------------------------------------------------- what a builder promises
def exact_boxes(c, head):
    """[A, 4] closed form of the exact / equal plants."""
    f = np.float32
    k = np.array([EXACT_BINS[l] if c.box == "exact" else (7.5,) * 4 for l in head.level], f)
    cx, cy, st = head.gx.astype(f) + f(0.5), head.gy.astype(f) + f(0.5), head.stride.astype(f)
    return np.stack([(cx - k[:, 0]) * st, (cy - k[:, 1]) * st, (cx + k[:, 2]) * st, (cy + k[:, 3]) * st], -1).astype(f)


def pair_counts(c, head, cls):
    """Per level with a planted pair: (anchors where the pair is the strict row maximum, where it is not, whether the two rows are equal
    everywhere) over cls [P, A, nc]."""
    out = {}
    for l, p in enumerate(c.pairs):
        if p:
            v = cls[:, head.a0[l]:head.a0[l + 1]]
            rest = np.delete(v, [p[0], p[1]], -1).max(-1)
            top = np.minimum(v[..., p[0]], v[..., p[1]]) > rest
            out[l] = (int(top.sum()), int((~top).sum()), bool(np.array_equal(v[..., p[0]], v[..., p[1]])))
    return out


def spans(head, dfl):
    d = np.asarray(dfl, np.float64).reshape(dfl.shape[0], head.A, 4, head.reg_max)
    return d.max(-1) - d.min(-1)


# ---------------------------------------------------------------------------------------------------------------- the epilogue's rules
CLS_BUGS = ("last_max", "lowest_lane", "mask_dropped")
BOX_BUGS = ("gy_by_height", "a0_previous", "upper_bins_restart", "sides_permuted", "neighbour_stride")


def lane_of(ch):
    """The q-lane that holds channel ch in tail_1x1: eight channels per lane and tile pair, four in the odd fifth tile."""
    ch = np.asarray(ch)
    return np.where(ch < 64, (ch % 32) // 8, (ch - 64) // 4)


def classify(cls, width, bug=None):
    """(max logit, label) per anchor of raw class logits [B, A, nc] as the `width`-channel epilogue must reduce them: the maximum, the
    first channel that holds it -- or with one rule broken."""
    v = np.asarray(cls, np.float32)
    nc = v.shape[-1]
    if bug == "mask_dropped" and width > nc:                     # the padded channels (0 + 0) take part
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (width - nc,), np.float32)], -1)
    if bug == "last_max":
        return v.max(-1), (v.shape[-1] - 1 - v[..., ::-1].argmax(-1)).astype(np.int32)
    if bug == "lowest_lane":                                     # the lane merge lets the lower channel index win whatever the value
        ch = np.nonzero(lane_of(np.arange(nc)) == 0)[0]
        return v[..., ch].max(-1), ch[v[..., ch].argmax(-1)].astype(np.int32)
    return v.max(-1), v.argmax(-1).astype(np.int32)


def decode_boxes(head, dfl, bug=None):
    """fp32 NumPy decode of raw DFL logits [B, A, 64] with the head's geometry -- or with one rule broken."""
    if bug in (None, "sides_permuted", "neighbour_stride"):
        return R.decode_fp32(head, dfl, bug)
    f = np.float32
    d = np.asarray(dfl, f).reshape(dfl.shape[0], head.A, 4, head.reg_max)
    e = np.exp(d - d.max(-1, keepdims=True)).astype(f)
    bins = np.arange(head.reg_max, dtype=f)
    lo = 8 if bug == "upper_bins_restart" else 0                 # the odd lane starts its two sums from zero
    dist = ((e * bins)[..., lo:].sum(-1, dtype=f) / e[..., lo:].sum(-1, dtype=f)).astype(f)
    gx, gy = head.gx, head.gy
    if bug == "gy_by_height":
        cell = np.arange(head.A) - head.a0[head.level]
        hh = np.array([h for _, h, _ in head.levels])[head.level]
        gy = cell // hh
        gx = cell - gy * hh
    cx, cy, st = gx.astype(f) + f(0.5), gy.astype(f) + f(0.5), head.stride.astype(f)
    out = np.stack([(cx - dist[..., 0]) * st, (cy - dist[..., 1]) * st, (cx + dist[..., 2]) * st, (cy + dist[..., 3]) * st], -1).astype(f)
    if bug == "a0_previous":                                     # level l stored from level l - 1's first anchor
        moved = np.zeros_like(out)
        for l in range(len(head.levels)):
            a0 = int(head.a0[max(l - 1, 0)])
            moved[:, a0:a0 + head.a0[l + 1] - head.a0[l]] = out[:, head.a0[l]:head.a0[l + 1]]
        out = moved
    return out


def box_reference(head, dfl):
    """-> (fp64 boxes, per-element bound for the device's exp2 form) of raw DFL logits."""
    ref = head.decode(dfl, np.zeros(dfl.shape[:2] + (1,), np.float32), np.float64)[0]
    return ref, R.decode_tolerance(head, dfl, ref, fast_exp=True)
