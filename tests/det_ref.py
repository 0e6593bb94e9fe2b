"""Detection post-processing harness: references, exact-box scene builders and the case lists for decode_kernel, select_sort_nms_kernel
and the two det_filter kernels.  Plain NumPy, no GPU here: tests/test_gpu_det_kernels.py runs the cases on the device through
aic_yolo_postprocess / aic_det_filter, tests/test_det_ref.py checks on the CPU that every builder delivers what it promises and that
each planted variant of decode, NMS and filter changes an expected output of at least one of those cases.

References: decode = oracle.nets_oracle.decode_head in fp64, NMS = oracle.nets_oracle.nms, un-letterbox = oracle.image_oracle.scale_bboxes,
filter = filter_ref below (deepsort_tracker.py:88-101).

Exact boxes.  A DFL side whose logits are 0 except +40 at bin k decodes to exactly k in fp32 on both exponential forms: the other bins
contribute exp(-40) = 4.2e-18 each, so the running sum rounds to 1 and the running expectation to k (for k = 0 the expectation is
~5e-16, which vanishes when it is subtracted from a cell centre >= 0.5).  Every corner is then (cell + 0.5 -/+ k) * stride, an exact
small integer, and areas, intersections and IoUs such as 2/4 are exact in fp32.

Decode tolerance, per box element, from the fp64 reference (u = 2^-24, R = reg_max, S = max - min of the side's R logits):
  e_k = exp(v_k - max)   expf form:  the subtraction rounds (relative error of e: u * S), expf within 4 ulp (8u)       -> d = (S + 8) u
                         exp2 form:  exp2((v_k - max) * log2 e): subtraction, the rounded constant and the product put
                                     3u * |t| on the argument t, |t| <= S log2 e, i.e. 3u * S relative on e (the input-rounding
                                     term that grows with the span); v_exp_f32 within 4 ulp (8u)                       -> d = (4 S + 8) u
  dist = sum(e_k k) / sum(e_k): a mean of k in [0, R-1] whose weights are off by d each moves by at most 2 d (R - 1); the two
                         R-term fp32 sums of positive terms add (R - 1) u each, the product e_k * k and the division u each, all
                         relative to dist <= R - 1                                  -> |dist - dist64| <= (R - 1) (2 d + (2 R + 2) u)
  corner = (c -/+ dist) * stride: c is exact, the add rounds once (u * |corner| / stride), the stride is a power of two
                                                                                    -> tol = stride * |dist - dist64|_max + 2 u |corner64|
For R = 16, S = 30, stride 32 this is 8.3e-3 px on the exp2 form and 3.2e-3 px on the expf form; a decode bug (a bin shifted, sides
swapped, the half-cell offset dropped, a neighbouring level's stride) moves a corner by at least half a stride."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import image_oracle as I
from oracle import nets_oracle as N

U = 2.0 ** -24
LEVELS_320 = ((8, 40, 40), (16, 20, 20), (32, 10, 10))          # (stride, h, w) of a 320 x 320 YOLOv8 head: 2100 anchors, three 1024-chunks
HOT = np.float32(40.0)
BACKGROUND = np.float32(-30.0)                                   # class logit of an anchor that is no candidate at any conf used here
NMS_TILE, NMS_CHUNK = 64, 1024                                   # wave tile / chunk of select_sort_nms_kernel's greedy walk


class Head:
    """Anchor geometry of a detect head: level-major, row-major."""

    def __init__(self, levels=LEVELS_320, nc=80, reg_max=16):
        self.levels, self.nc, self.reg_max = tuple(levels), nc, reg_max
        self.a0 = np.cumsum([0] + [h * w for _, h, w in levels])
        self.A = int(self.a0[-1])
        self.level = np.concatenate([np.full(h * w, l, np.int32) for l, (_, h, w) in enumerate(levels)])
        self.stride = np.concatenate([np.full(h * w, s, np.int32) for s, h, w in levels])
        self.gx = np.concatenate([np.tile(np.arange(w), h) for _, h, w in levels]).astype(np.int32)
        self.gy = np.concatenate([np.repeat(np.arange(h), w) for _, h, w in levels]).astype(np.int32)

    def anchor(self, level, gx, gy):
        return int(self.a0[level] + gy * self.levels[level][2] + gx)

    def edge_anchors(self):
        """First and last anchor of every level."""
        return sorted({int(self.a0[l]) for l in range(len(self.levels))} | {int(self.a0[l + 1] - 1) for l in range(len(self.levels))})

    def decode(self, dfl, cls, ft=np.float32):
        return N.decode_head([(s, h, w) for s, h, w in self.levels], self.reg_max, dfl, cls, ft)


# ---------------------------------------------------------------------------------------------------------------- decode
def decode_tolerance(head, dfl, ref_boxes, fast_exp):
    """[B,A,4] bound on |fp32 box - fp64 box| (module docstring).  ref_boxes: the fp64 decode of dfl."""
    R = head.reg_max
    d = np.asarray(dfl, np.float64).reshape(dfl.shape[0], head.A, 4, R)
    span = d.max(-1) - d.min(-1)
    delta = ((4.0 * span if fast_exp else span) + 8.0) * U
    dist_err = (R - 1) * (2.0 * delta + (2 * R + 2) * U)
    return head.stride[None, :, None] * dist_err + 2.0 * U * np.abs(ref_boxes)


def decode_inputs(head, batch, seed):
    """Head logits for the decode checks: per side, random rows of span 1 .. 30, one-hot rows of several heights, all-equal rows; class
    rows with planted exact ties of the maximum (inside a group of four, across groups, in the last classes).  -> dfl, cls, props."""
    rng = np.random.default_rng(seed)
    A, R, nc = head.A, head.reg_max, head.nc
    dfl = np.zeros((batch, A, 4, R), np.float32)
    kind = rng.integers(0, 8, (batch, A, 4))
    spans = np.array([1, 2, 5, 10, 20, 30], np.float32)
    u = rng.random((batch, A, 4, R), dtype=np.float32)
    u[..., 0], u[..., 1] = 0.0, 1.0                            # the row's span is exactly the chosen one
    u = rng.permuted(u, axis=-1)
    for k, s in enumerate(spans):
        m = kind == k
        dfl[m] = (u[m] - np.float32(0.5)) * s + rng.uniform(-3, 3, (int(m.sum()), 1)).astype(np.float32)
    m = kind == 6                                                # one-hot rows: +1, +8 or +40 at one bin
    hot = np.zeros((int(m.sum()), R), np.float32)
    hot[np.arange(len(hot)), rng.integers(0, R, len(hot))] = rng.choice(np.array([1, 8, 40], np.float32), len(hot))
    dfl[m] = hot
    m = kind == 7                                                # all-equal rows
    dfl[m] = rng.uniform(-5, 5, (int(m.sum()), 1)).astype(np.float32) * np.ones(R, np.float32)
    cls = (rng.standard_normal((batch, A, nc)) * 3).astype(np.float32)
    ties = {}
    pairs = [(0, 1), (3, 4), (2, nc - 1), (nc - 2, nc - 1), (1, 2), (nc - 3, nc - 1)]
    edge = head.edge_anchors()
    planted = edge + [int(a) for a in rng.choice(A, 64, replace=False) if int(a) not in edge]
    for b in range(batch):
        for i, a in enumerate(planted):
            j1, j2 = pairs[(i + b) % len(pairs)]
            top = cls[b, a].max() + np.float32(1.0)
            cls[b, a, j1] = cls[b, a, j2] = top
            ties[(b, a)] = j1
    return dfl.reshape(batch, A, 4 * R), cls, dict(ties=ties, edge=edge)


DECODE_BUGS = ("bin_shift", "sides_permuted", "no_half_cell", "neighbour_stride")


def decode_fp32(head, dfl, bug=None):
    """fp32 NumPy decode of the boxes, optionally with one planted bug."""
    f = np.float32
    R = head.reg_max
    d = np.asarray(dfl, f).reshape(dfl.shape[0], head.A, 4, R)
    e = np.exp(d - d.max(-1, keepdims=True)).astype(f)
    bins = np.arange(R, dtype=f) + (f(1) if bug == "bin_shift" else f(0))
    dist = ((e * bins).sum(-1, dtype=f) / e.sum(-1, dtype=f)).astype(f)
    if bug == "sides_permuted":
        dist = dist[..., [1, 0, 3, 2]]
    half = f(0) if bug == "no_half_cell" else f(0.5)
    cx, cy, st = head.gx.astype(f) + half, head.gy.astype(f) + half, head.stride.astype(f).copy()
    if bug == "neighbour_stride":
        for l in range(1, len(head.levels)):
            st[head.a0[l]] = head.levels[l - 1][0]
    return np.stack([(cx - dist[..., 0]) * st, (cy - dist[..., 1]) * st, (cx + dist[..., 2]) * st, (cy + dist[..., 3]) * st], -1).astype(f)


# ---------------------------------------------------------------------------------------------------------------- exact scenes
@dataclass
class Scene:
    """One image's head tensors and what its builder promises about them."""
    dfl: np.ndarray                      # [A, 4 * reg_max]
    cls: np.ndarray                      # [A, nc]
    exact: dict                          # anchor -> exact box (x1, y1, x2, y2) in pixels, for every anchor a builder placed
    props: dict = field(default_factory=dict)


class SceneBuilder:
    def __init__(self, head):
        self.h = head
        self.dfl = np.zeros((head.A, 4, head.reg_max), np.float32)
        self.cls = np.full((head.A, head.nc), BACKGROUND, np.float32)
        self.exact = {}

    def free(self, a):
        return a not in self.exact

    def place(self, a, box_cells, label, logit):
        """Anchor a gets the box (x1, y1, x2, y2), given in units of its level's cells, exactly: every corner must lie an integer number
        of cells (0 .. reg_max - 1) from the anchor's centre."""
        assert self.free(a), a
        c = (self.h.gx[a] + 0.5, self.h.gy[a] + 0.5)
        bins = (c[0] - box_cells[0], c[1] - box_cells[1], box_cells[2] - c[0], box_cells[3] - c[1])
        for sd, k in enumerate(bins):
            assert k == int(k) and 0 <= k < self.h.reg_max, (a, box_cells, bins)
            self.dfl[a, sd, int(k)] = HOT
        self.cls[a, label] = np.float32(logit)
        self.exact[a] = tuple(float(v) * int(self.h.stride[a]) for v in box_cells)

    def place_near(self, level, box_cells, label, logit):
        """The same, from the first free anchor of `level` whose centre lies inside the box (identical or overlapping boxes need
        several anchors)."""
        _, hh, ww = self.h.levels[level]
        for gy in range(max(0, math.ceil(box_cells[1] - 0.5)), min(hh - 1, math.floor(box_cells[3] - 0.5)) + 1):
            for gx in range(max(0, math.ceil(box_cells[0] - 0.5)), min(ww - 1, math.floor(box_cells[2] - 0.5)) + 1):
                a = self.h.anchor(level, gx, gy)
                if self.free(a):
                    self.place(a, box_cells, label, logit)
                    return a
        raise AssertionError(("no free anchor inside", box_cells))

    def filler(self, a, logit, label=0):
        """A box that overlaps no other filler: the anchor's own cell on level 0 (shifted half a cell so the corners stay exact; cells
        tile without overlap), a zero-area point on the coarser levels."""
        x, y = self.h.gx[a] + 0.5, self.h.gy[a] + 0.5
        self.place(a, (x - 1, y - 1, x, y) if self.h.level[a] == 0 else (x, y, x, y), label, logit)

    def scene(self, **props):
        return Scene(self.dfl.reshape(self.h.A, -1).copy(), self.cls.copy(), dict(self.exact), props)


def empty_scene(head):
    return SceneBuilder(head).scene(n_cand=0)


def rank_logit(r):
    """Distinct, exactly representable, descending in the rank: 8 - r / 512 (> 3.8 for r < 2100)."""
    return np.float32(8.0 - r / 512.0)


def disjoint_scene(head, n, seed):
    """n candidates of one label whose pairwise IoU is 0, distinct logits, sorted order unrelated to the anchor order."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    anchors = rng.permutation(head.A)[:n]
    for r, a in enumerate(anchors):
        sb.filler(int(a), rank_logit(r))
    return sb.scene(n_cand=n, order=[int(a) for a in anchors])


# structures, in level-0 cells relative to a slot origin: (name, [(box, label offset)] in the order keeper / A first, survivors expected)
STRUCTURES = {
    "cluster": ([((0, 0, 4, 2), 0), ((1, 0, 5, 2), 0), ((0, 0, 4, 2), 0)], [True, False, False]),         # IoU 0.6 and 1 with the keeper
    "chain": ([((0, 0, 4, 1), 0), ((1, 0, 5, 1), 0), ((2, 0, 6, 1), 0)], [True, False, True]),            # AB = BC = 0.6, AC = 1/3
    "iou_exact": ([((0, 0, 3, 1), 0), ((1, 0, 4, 1), 0)], [True, True]),                                  # 2 / 4 == iou_thr: strict >
    "iou_above": ([((0, 0, 5, 1), 0), ((1, 0, 6, 1), 0)], [True, False]),                                 # 4 / 6
    "other_label": ([((0, 0, 4, 2), 0), ((0, 0, 4, 2), 1)], [True, True]),                                # identical boxes, labels differ
    "zero_area": ([((2, 0, 2, 2), 0), ((2, 0, 2, 2), 0)], [True, True]),                                  # identical zero-width boxes: IoU 0
}
PLACEMENTS = {"same_tile": (1, 2), "other_tile": (NMS_TILE, 2 * NMS_TILE + 5), "other_chunk": (NMS_CHUNK, 2 * NMS_CHUNK - 30)}


def _slot(i):
    """Origin (level-0 cells, box coordinates) of structure slot i: 8 x 2 cells, a free row and column between slots."""
    return 1.5 + 9 * (i % 4), 1.5 + 3 * (i // 4)


def composite_scene(head, n, seed):
    """n candidates with distinct logits: every structure of STRUCTURES placed three ways (its members in one wave tile, in different
    tiles, in different 1024-chunks of the sorted candidates; what fits below n), the remaining ranks filled with label-0 boxes that
    suppress nothing.  Structure s uses labels 1 + 2 s and 2 + 2 s; its boxes overlap no other structure's.
    props: n_cand, structures [{kind, placement, ranks, anchors, survive}], kept_ranks (sorted ranks the NMS keeps at iou 0.5)."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    taken, structs = {}, []
    q = 0
    for pname, offs in PLACEMENTS.items():
        for kind, (members, survive) in STRUCTURES.items():
            base = 2 + 5 * q
            ranks = [base] + [base + o for o in offs[:len(members) - 1]]
            for i in range(len(ranks)):                          # no two members on one rank; ranks 63 mod 64 stay with the fillers
                while ranks[i] in taken or ranks[i] % NMS_TILE == NMS_TILE - 1 or ranks[i] in ranks[:i]:
                    ranks[i] += 1
            if ranks[-1] >= n:
                q += 1
                continue
            x0, y0 = _slot(q)
            lab0 = 1 + 2 * q
            anchors = []
            for (bx, dl), r in zip(members, ranks):
                a = sb.place_near(0, (x0 + bx[0], y0 + bx[1], x0 + bx[2], y0 + bx[3]), lab0 + dl, rank_logit(r))
                anchors.append(a)
                taken[r] = a
            structs.append(dict(kind=kind, placement=pname, ranks=ranks, anchors=anchors, survive=list(survive)))
            q += 1
    free = [int(a) for a in rng.permutation(head.A) if sb.free(int(a))]
    for r in range(n):
        if r not in taken:
            sb.filler(free.pop(), rank_logit(r))
    dead = {s["ranks"][i] for s in structs for i in range(len(s["ranks"])) if not s["survive"][i]}
    return sb.scene(n_cand=n, structures=structs, kept_ranks=[r for r in range(n) if r not in dead])


def max_det_at(scene, rank):
    """The max_det with which the greedy walk of `scene` stops exactly at sorted candidate `rank` (which the scene keeps)."""
    kept = scene.props["kept_ranks"]
    assert rank in kept, rank
    return kept.index(rank) + 1


def tie_scene(head, n, seed):
    """n candidates whose logits take three values only: long runs of equal logits, one of them across both level boundaries (the
    anchors around 1600 and 2000 all tie), so the order is decided by the anchor index.  Overlapping equal-logit pairs (label 1, IoU
    0.6): the lower anchor index must win.  props: n_cand, run (anchors of the planted run), pairs [(winner, loser)]."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    vals = np.array([1.0, 2.0, 3.0], np.float32)
    pairs = []
    for i in range(6):
        x0, y0 = _slot(i)
        a = sb.place_near(0, (x0, y0, x0 + 4, y0 + 1), 1, vals[i % 3])
        b = sb.place_near(0, (x0 + 1, y0, x0 + 5, y0 + 1), 1, vals[i % 3])
        pairs.append((min(a, b), max(a, b)))
    run = [a for a in list(range(1590, 1611)) + list(range(1995, 2006)) if sb.free(a)]
    for a in run:
        sb.filler(a, vals[1])
    rest = [int(a) for a in rng.permutation(head.A) if sb.free(int(a))][:n - len(run) - 12]
    for a in rest:
        sb.filler(a, vals[rng.integers(0, 3)])
    return sb.scene(n_cand=n, run=run, pairs=pairs)


def threshold_scene(head, conf, seed, n_at=70, n_below=70, n_above=90):
    """Candidates exactly on logit_threshold(conf) (they pass: >=), anchors one ulp below it (they do not), and some well above."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    thr = N.logit_threshold(conf)
    below = np.nextafter(thr, np.float32(-np.inf))
    perm = [int(a) for a in rng.permutation(head.A)]
    at, bl, ab = perm[:n_at], perm[n_at:n_at + n_below], perm[n_at + n_below:n_at + n_below + n_above]
    for a in at:
        sb.filler(a, thr)
    for a in bl:
        sb.filler(a, below)
    for i, a in enumerate(ab):
        sb.filler(a, thr + np.float32(1 + i / 64.0))
    return sb.scene(n_cand=n_at + n_above, at=at, below=bl)


def zero_scene(head, seed, extra=200):
    """+0.0 / -0.0 logits (both are candidates at conf <= 0.5, and they tie: the anchor index decides).  Isolated zeros of both signs
    in random anchor order, and overlapping pairs (label 1, IoU 0.6, different boxes) with the -0.0 on the lower index and on the higher
    one: the lower index must survive.  Plus `extra` candidates at 1 + i/64 and, for conf = 0.25, at -0.5 - i/512.
    props: n_cand_05 / n_cand_025, pairs [(winner, loser, sign of the winner's zero)]."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    pz, nz = np.float32(0.0), np.float32(-0.0)
    pairs = []
    for i in range(8):
        x0, y0 = _slot(i)
        a = sb.place_near(0, (x0, y0, x0 + 4, y0 + 1), 1, 0.0)
        b = sb.place_near(0, (x0 + 1, y0, x0 + 5, y0 + 1), 1, 0.0)
        lo, hi = min(a, b), max(a, b)
        sb.cls[lo, 1], sb.cls[hi, 1] = (nz, pz) if i % 2 == 0 else (pz, nz)
        pairs.append((lo, hi, -1 if i % 2 == 0 else 1))
    free = [int(a) for a in rng.permutation(head.A) if sb.free(int(a))]
    zeros = free[:150]
    for i, a in enumerate(zeros):
        sb.filler(a, nz if i % 2 else pz)
    for i, a in enumerate(free[150:150 + extra]):
        sb.filler(a, np.float32(1 + i / 64.0))
    for i, a in enumerate(free[150 + extra:150 + 2 * extra]):
        sb.filler(a, np.float32(-0.5 - i / 512.0))
    return sb.scene(n_cand_05=16 + 150 + extra, n_cand_025=16 + 150 + 2 * extra, pairs=pairs, zeros=zeros)


def stress_scene(head, seed, n=1500, labels=20):
    """~n candidates with random exact boxes (0 .. 6 cells to each side) on all levels: overlapping clusters over `labels` labels, logits
    on a grid of 1/8 so that ties occur."""
    rng = np.random.default_rng(seed)
    sb = SceneBuilder(head)
    for a in rng.permutation(head.A)[:n]:
        a = int(a)
        x, y = head.gx[a] + 0.5, head.gy[a] + 0.5
        l, t, r, b = (int(v) for v in rng.integers(0, 7, 4))
        sb.place(a, (x - l, y - t, x + r, y + b), int(rng.integers(0, labels)), np.float32(rng.integers(-4, 64) / 8.0))
    return sb.scene(n_cand=int((sb.cls.max(-1) >= N.logit_threshold(0.25)).sum()))


def stack(scenes):
    return np.stack([s.dfl for s in scenes]), np.stack([s.cls for s in scenes])


# ---------------------------------------------------------------------------------------------------------------- NMS cases
DISJOINT_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 2100)
DISJOINT_MAX_DET = (1, 7, 64, 65, 300, 1024)
STRESS_SEEDS = (101, 102, 103, 104, 105, 106)
IOU_BELOW_HALF = float(np.nextafter(np.float32(0.5), np.float32(0)))     # with this threshold an IoU of exactly 0.5 suppresses


@dataclass
class NmsCase:
    id: str
    scenes: list
    conf: float
    iou: float
    max_det: int
    n_cand: list                         # promised candidates per image

    def tensors(self):
        return stack(self.scenes)


@functools.lru_cache(maxsize=None)
def nms_cases(nc=80, reg_max=16):
    """Every NMS case of the GPU test (the CPU test runs the planted variants over the same list)."""
    head = Head(nc=nc, reg_max=reg_max)
    C = []
    empty = empty_scene(head)
    comp = [composite_scene(head, 2100, 11), empty, composite_scene(head, 1500, 12)]
    nc_comp = [2100, 0, 1500]
    # max_det reached in the middle of a wave tile, on the last candidate of a tile, on the last candidate of a chunk (image 0)
    for name, rank in (("mid_tile", 100), ("tile_edge", 191), ("chunk_edge", 1023)):
        C.append(NmsCase(f"composite_{name}", comp, 0.25, 0.5, max_det_at(comp[0], rank), nc_comp))
    C.append(NmsCase("composite_md300", comp, 0.25, 0.5, 300, nc_comp))
    C.append(NmsCase("composite_md1024", comp, 0.25, 0.5, 1024, nc_comp))
    C.append(NmsCase("composite_iou_just_below_half", comp, 0.25, IOU_BELOW_HALF, 1024, nc_comp))
    ties = [tie_scene(head, 1500, 21), empty, tie_scene(head, 700, 22)]
    for md in (64, 300, 1024):
        C.append(NmsCase(f"ties_md{md}", ties, 0.25, 0.5, md, [1500, 0, 700]))
    # (the C ABI takes conf as a float: 0.6 is given as the fp32 number nearest to it, so that both sides take the logit of the same value)
    for name, conf in (("0.25", 0.25), ("0.6", float(np.float32(0.6)))):
        th = [threshold_scene(head, conf, 31), empty, threshold_scene(head, conf, 32, n_at=3, n_below=200, n_above=1)]
        C.append(NmsCase(f"threshold_conf{name}", th, conf, 0.5, 300, [160, 0, 4]))
    zs = [zero_scene(head, 41), empty, zero_scene(head, 42, extra=30)]
    C.append(NmsCase("zeros_conf0.5", zs, 0.5, 0.5, 300, [s.props.get("n_cand_05", 0) for s in zs]))
    C.append(NmsCase("zeros_conf0.25", zs, 0.25, 0.5, 1024, [s.props.get("n_cand_025", 0) for s in zs]))
    dis = [disjoint_scene(head, n, 50 + i) for i, n in enumerate(DISJOINT_COUNTS)]
    for md in DISJOINT_MAX_DET:
        C.append(NmsCase(f"disjoint_md{md}", dis, 0.25, 0.5, md, list(DISJOINT_COUNTS)))
    st = [stress_scene(head, s) for s in STRESS_SEEDS]
    C.append(NmsCase("stress_md300", st[:3], 0.25, 0.5, 300, [s.props["n_cand"] for s in st[:3]]))
    C.append(NmsCase("stress_md1024_iou0.45", st[3:], 0.25, 0.45, 1024, [s.props["n_cand"] for s in st[3:]]))
    return C


NMS_VARIANTS = ("iou_ge", "thr_gt", "tie_index_desc", "labels_ignored", "suppressed_suppress", "max_det_plus_one", "neg_zero_below")


def nms_variant(boxes, max_logit, labels, conf, iou_thresh, max_det, variant=None):
    """nets_oracle.nms restated with one switchable deviation (variant None: the specification itself; asserted equal on the CPU)."""
    thr = N.logit_threshold(conf)
    cand = np.nonzero(max_logit > thr if variant == "thr_gt" else max_logit >= thr)[0]
    v = max_logit[cand]
    keys = [cand if variant != "tie_index_desc" else -cand]
    if variant == "neg_zero_below":
        keys.append((np.signbit(v) & (v == 0)).astype(np.int64))
    keys.append(-v.astype(np.float64))
    order = cand[np.lexsort(keys)]
    limit = max_det + 1 if variant == "max_det_plus_one" else max_det
    b, lab = boxes[order], labels[order]
    alive = np.ones(len(order), bool)
    keep = []
    it = np.float32(iou_thresh)
    for i in range(len(order)):
        if alive[i]:
            keep.append(int(order[i]))
            if len(keep) >= limit:
                break
        elif variant != "suppressed_suppress":
            continue
        rest = np.nonzero(alive[i + 1:] & ((lab[i + 1:] == lab[i]) | (variant == "labels_ignored")))[0] + i + 1
        if len(rest):
            iou = N.box_iou_xyxy(b[i], b[rest])
            alive[rest[iou >= it if variant == "iou_ge" else iou > it]] = False
    return np.asarray(keep, np.int64)


# ---------------------------------------------------------------------------------------------------------------- un-letterbox
def letterbox_geometry(h, w, out_hw=(320, 320)):
    """image_processing.py:7-70 (auto = False, scaleup = True): ratio, (pad_w, pad_h) of an h x w frame letterboxed to out_hw."""
    r = min(out_hw[0] / h, out_hw[1] / w)
    unpad_w, unpad_h = int(round(w * r)), int(round(h * r))
    return np.float32(r), (np.float32((out_hw[1] - unpad_w) / 2), np.float32((out_hw[0] - unpad_h) / 2))


UNLETTERBOX_FRAMES = ((720, 1280), (100, 37), (333, 2000))        # (h, w): 1280 x 720, 37 x 100 and 2000 x 333 frames


def unletterbox_ref(boxes, frame_hw, ratio, pad):
    return I.scale_bboxes(boxes, frame_hw, (ratio, ratio), pad)


# ---------------------------------------------------------------------------------------------------------------- filter
FILTER_VARIANTS = ("conf_gt", "mask_wrong_word", "order_reversed")


def filter_ref(num_dets, boxes, scores, labels, min_conf, mask, cap, variant=None):
    """deepsort_tracker.py:88-101 over a launch group: per frame, in order, the detections with score >= min_conf whose class bit is set
    in mask (two 64-bit words, classes 0 .. 127); rows beyond cap are dropped but counted.  -> dict like HipEngine.det_filter_np's."""
    B, md = scores.shape
    rows, frame_n, frame_d0 = [], [], []
    for f in range(B):
        frame_d0.append(len(rows))
        idx = range(min(max(int(num_dets[f]), 0), md))
        idx = reversed(idx) if variant == "order_reversed" else idx
        for i in idx:
            c = int(labels[f, i])
            word = (c >> 6) ^ (variant == "mask_wrong_word")
            ok_cls = 0 <= c < 128 and (int(mask[word]) >> (c & 63)) & 1
            ok_conf = scores[f, i] > np.float32(min_conf) if variant == "conf_gt" else scores[f, i] >= np.float32(min_conf)
            if ok_cls and ok_conf:
                rows.append((f, i))
        frame_n.append(len(rows) - frame_d0[-1])
    n = min(len(rows), cap)
    fi = np.array(rows[:n], np.int64).reshape(-1, 2)
    xyxy = boxes[fi[:, 0], fi[:, 1]].reshape(-1, 4)
    tlwh = np.stack([xyxy[:, 0], xyxy[:, 1], xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1]], 1).astype(np.float32)
    return dict(frame_n=np.array(frame_n, np.int32), frame_d0=np.array(frame_d0, np.int32), total=np.array([n, len(rows)], np.int32),
                xyxy=xyxy, tlwh=tlwh, conf=scores[fi[:, 0], fi[:, 1]], cls=labels[fi[:, 0], fi[:, 1]], frame_of=fi[:, 0].astype(np.int32))


FILTER_LABELS = (-1, 0, 63, 64, 127, 128)
FILTER_FRAME_COUNTS = (0, 1, 63, 64, 65, 300)
MASK_A = ((1 << 0) | (1 << 63), (1 << 63))                       # tracks 0, 63, 127: excludes 64
MASK_B = (0, (1 << 0))                                            # tracks 64 only: excludes 0, 63, 127


@dataclass
class FilterCase:
    id: str
    num_dets: np.ndarray
    boxes: np.ndarray
    scores: np.ndarray
    labels: np.ndarray
    min_conf: float
    mask: tuple
    cap: int                             # > 0, or 0 / -1 / -k: the total the filter passes, one below it, a k-th of it


def _filter_inputs(batch, max_det, seed, min_conf):
    """Frames whose detection counts cycle through FILTER_FRAME_COUNTS, max_det and max_det + 7 (clamped by the kernel); labels from
    FILTER_LABELS; a quarter of the scores exactly min_conf, the rest on either side of it."""
    rng = np.random.default_rng(seed)
    counts = [c for c in FILTER_FRAME_COUNTS if c <= max_det] + [max_det, max_det + 7]
    nd = np.array([counts[(f + seed) % len(counts)] for f in range(batch)], np.int32)
    boxes = rng.uniform(0, 1000, (batch, max_det, 4)).astype(np.float32)
    boxes[..., 2:] += boxes[..., :2]
    scores = rng.uniform(0.05, 0.99, (batch, max_det)).astype(np.float32)
    scores[rng.random((batch, max_det)) < 0.25] = np.float32(min_conf)
    labels = rng.choice(np.array(FILTER_LABELS, np.int32), (batch, max_det))
    return nd, boxes, scores, labels


@functools.lru_cache(maxsize=None)
def filter_cases():
    C = []
    for batch, md in ((1, 300), (64, 300), (65, 300), (512, 70), (3, 1024)):
        for mi, mask in enumerate((MASK_A, MASK_B)):
            nd, bx, sc, lb = _filter_inputs(batch, md, 7 * batch + mi, 0.4)
            for cap in ((0, -1, -5) if mi == 0 else (0,)):
                C.append(FilterCase(f"b{batch}_md{md}_mask{'AB'[mi]}_cap{cap}", nd, bx, sc, lb, 0.4, mask, cap))
    return C


def filter_cap(case):
    """The case's cap in rows: the count the filter passes, one below it, or a fraction of it (at least 1)."""
    if case.cap > 0:
        return case.cap
    total = int(filter_ref(case.num_dets, case.boxes, case.scores, case.labels, case.min_conf, case.mask, 1 << 30)["total"][1])
    return max(1, total if case.cap == 0 else total - 1 if case.cap == -1 else total // -case.cap)
