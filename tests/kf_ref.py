"""The xyah Kalman filter of DeepSORT / ByteTrack in float64, the fixed list of cases the device copies of it are checked on, and the
metrics of those checks.  Plain NumPy written from the textbook formulas, nothing from the package under test and nothing from
oracle/deepsort_oracle.py.  tests/test_kf_ref.py checks on the CPU that this reference reproduces the states the real reference wrote
(tests/golden/kf.npz, kf_dt.npz) and that the cases deliver the conditions the device tests (tests/test_gpu_kf_paths.py) lean on.

Reference (float64 on the fp32 inputs as given; x = (cx, cy, a, h, vx, vy, va, vh)):
  initiate   x = (z, 0), P = diag((2 wp h)^2, (2 wp h)^2, 1e-4, (2 wp h)^2, (10 wv h)^2, (10 wv h)^2, 1e-10, (10 wv h)^2)
  predict    x <- F x, P <- F P F^T + Q(h), F = I + fp32(dt) [position <- velocity], Q = diag((wp h)^2 x2, 1e-4, (wp h)^2, (wv h)^2 x2, 1e-10, (wv h)^2)
  project    H x, S = H P H^T + R(h), R = diag((wp h)^2, (wp h)^2, 1e-2, (wp h)^2)
  update     K = P H^T S^-1, x + K (z - H x), P - K S K^T
  gating     (z - H x)^T S^-1 (z - H x) on the first 2 or all 4 components; +inf for every z when that block of S is not positive definite
wp = fp32(1/20), wv = fp32(1/160): the weights the device holds; h is the fp32 input state's (or measurement's) height.

Metrics (the covariance of these filters spans 1e-10 (P[6][6]) to 1e8, so neither a relative nor a max(1, .) metric says anything):
  covariance element (i, j)   |got - ref| / sqrt(Pm[i][i] Pm[j][j]), Pm the float64 covariance the step STARTED from (for predict: ref)
  mean element i              |got - ref| / (|xm[i]| + sum_a |K[i][a]| |z[a] - xm[a]|), the magnitudes the result was summed from
  gating                      |d2 - ref| / max(1, ref), and the "sure" rule around CHI2_4 of tests/test_gpu_trk_costs.py::check_costs
An allowance is max(4 x the fp32 NumPy restatement's own figure on the same inputs, FLOOR), never a figure of the device's.

Cases: CASES, a fixed seeded list of (state, measurement); the grid of heights x centres x preparation, then one case each with large
velocities, a predicted h <= 0, h < 0 on entry, a = 0.05, a = 8, a dense covariance and a dense NON-symmetric one.  Real states of this
filter only couple a coordinate with its own velocity (P[i][j] = 0 unless i = j mod 4), so an index slip between coordinates multiplies
zeros there; the two dense cases are what such a slip moves."""
from dataclasses import dataclass

import numpy as np

CHI2_4 = 9.487729036781154
W_POS, W_VEL = float(np.float32(1.0 / 20)), float(np.float32(1.0 / 160))
U = 2.0 ** -24
FLOOR = 8 * U                                   # two operands of the size of the scale, each rounded once, should the restatement land exactly
_H = np.eye(4, 8)
MAX_AGE = 70


# ------------------------------------------------------------------------------------------------------------------ the filter, float64
def motion(dt=1.0):
    f = np.eye(8)
    for i in range(4):
        f[i, 4 + i] = float(np.float32(dt))
    return f


def initiate(z):
    z = np.asarray(z, np.float64)
    h = z[3]
    std = np.array([2 * W_POS * h, 2 * W_POS * h, 1e-2, 2 * W_POS * h, 10 * W_VEL * h, 10 * W_VEL * h, 1e-5, 10 * W_VEL * h])
    return np.concatenate([z, np.zeros(4)]), np.diag(std * std)


def predict(mean, cov, dt=1.0):
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    h = m[3]
    std = np.array([W_POS * h, W_POS * h, 1e-2, W_POS * h, W_VEL * h, W_VEL * h, 1e-5, W_VEL * h])
    f = motion(dt)
    return f @ m, f @ p @ f.T + np.diag(std * std)


def project(mean, cov):
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    h = m[3]
    std = np.array([W_POS * h, W_POS * h, 1e-1, W_POS * h])
    return _H @ m, _H @ p @ _H.T + np.diag(std * std)


def gain(mean, cov):
    """(H x, S, K).  K S = P H^T solved as S^T K^T = (P H^T)^T: nothing here assumes that P is symmetric outside its measured block."""
    p = np.asarray(cov, np.float64)
    pm, s = project(mean, cov)
    return pm, s, np.linalg.solve(s.T, (p @ _H.T).T).T


def update(mean, cov, z):
    m, p = np.asarray(mean, np.float64), np.asarray(cov, np.float64)
    pm, s, k = gain(m, p)
    return m + k @ (np.asarray(z, np.float64) - pm), p - k @ s @ k.T


def is_pd(s):
    try:
        np.linalg.cholesky(s)
        return True
    except np.linalg.LinAlgError:
        return False


def gating(mean, cov, zs, only_position=False):
    pm, s = project(mean, cov)
    n = 2 if only_position else 4
    zs = np.asarray(zs, np.float64).reshape(-1, 4)
    if not is_pd(s[:n, :n]):
        return np.full(len(zs), np.inf)
    d = (zs[:, :n] - pm[:n]).T
    return np.sum(d * np.linalg.solve(s[:n, :n], d), axis=0)


def mean_to_tlwh(mean):
    """w = a h while h > 0, else 0 with h clamped at 0; top-left corner from the centre."""
    m = np.asarray(mean, np.float64)
    h = max(m[3], 0.0)
    w = m[2] * m[3] if m[3] > 0 else 0.0
    return np.array([m[0] - w / 2, m[1] - h / 2, w, h])


def xyah32(tlwh):
    """What the device makes of a detection box before the filter sees it (fp32: x + w / 2, y + h / 2, w / h or 0, h): the measurement
    every copy of the filter gets, so the INPUT of the reference, not part of it."""
    b = np.asarray(tlwh, np.float32).reshape(-1, 4)
    two = np.float32(2)
    a = np.divide(b[:, 2], b[:, 3], out=np.zeros(len(b), np.float32), where=b[:, 3] > 0)
    return np.stack([b[:, 0] + b[:, 2] / two, b[:, 1] + b[:, 3] / two, a, b[:, 3]], 1).astype(np.float32)


def iou(a, b):
    """IoU of two tlwh boxes, float64."""
    iw = max(0.0, min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]))
    ih = max(0.0, min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]))
    return iw * ih / max(a[2] * a[3] + b[2] * b[3] - iw * ih, 1e-300)


# ------------------------------------------------------------------------------------------------------------------ metrics
def cov_err(got, ref, p_start):
    """[8, 8] (or [4, 4]) of |got - ref| / sqrt(Pm_ii Pm_jj)."""
    d = np.sqrt(np.abs(np.diag(p_start)))
    return np.abs(np.asarray(got, np.float64) - ref) / np.outer(d, d)


def scaled_err(got, ref, scale):
    """|got - ref| / scale; where the scale is 0 every summand was 0 and only the exact value passes."""
    e = np.abs(np.asarray(got, np.float64) - ref)
    return np.where(scale > 0, e / np.where(scale > 0, scale, 1.0), np.where(e == 0, 0.0, np.inf))


def predict_errs(got_mean, got_cov, mean32, cov32, dt=1.0):
    """(covariance figure, mean figure) of one predict from the fp32 state."""
    m, p = predict(mean32, cov32, dt)
    x = np.asarray(mean32, np.float64)
    scale = np.abs(x) + np.concatenate([np.abs(float(np.float32(dt)) * x[4:]), np.zeros(4)])
    return float(cov_err(got_cov, p, p).max()), float(scaled_err(got_mean, m, scale).max())


def update_errs(got_mean, got_cov, mean32, cov32, z32):
    """(covariance figure, mean figure) of one update of the fp32 state (mean32, cov32) with the fp32 measurement z32."""
    x, p, z = np.asarray(mean32, np.float64), np.asarray(cov32, np.float64), np.asarray(z32, np.float64)
    pm, s, k = gain(x, p)
    m2, p2 = update(x, p, z)
    scale = np.abs(x) + np.abs(k) @ np.abs(z - pm)
    return float(cov_err(got_cov, p2, p).max()), float(scaled_err(got_mean, m2, scale).max())


def gating_err(got, ref):
    """|x - ref| / max(1, ref) over the finite cells; the cells where ref is +inf must be +inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    inf = np.isinf(ref)
    assert np.array_equal(np.isposinf(got), inf), "the +inf cells differ"
    return float((np.abs(got[~inf] - ref[~inf]) / np.maximum(1.0, ref[~inf])).max()) if (~inf).any() else 0.0


def allow(oracle_figure):
    return max(4 * oracle_figure, FLOOR)


# ------------------------------------------------------------------------------------------------------------------ cases
HEIGHTS = (0.5, 2.0, 20.0, 179.3, 2000.0)
CENTRES = (10.0, 4000.0, 30000.0)
ROUNDS = (0, 30)
PREDICTS = (0, 1, MAX_AGE)
DTS = (0.5, 2.0, 1.0 / 30)


@dataclass
class Case:
    name: str
    mean: np.ndarray          # [8] fp32
    cov: np.ndarray           # [8, 8] fp32
    z: np.ndarray             # [4] fp32 xyah: the measurement of form 1's update, applied to (mean, cov) as they are
    trackable: bool = True    # the predicted box is a box (h > 0): the state can be planted in a tracker and matched to a detection


def _prepared(rng, cx, cy, a, h, rounds, predicts, vel=(0.01, -0.015, 0.0, 0.002)):
    """initiate at (cx, cy, a, h), `rounds` x (predict, update with the object's noisy position), `predicts` x predict; float64, then
    rounded to fp32 once (the covariance symmetrised first: a real state is symmetric to the last bit only by luck, a case is by design)."""
    m, p = initiate(np.array([cx, cy, a, h]))
    v = np.array([vel[0] * h, vel[1] * h, vel[2], vel[3] * h])
    pos = np.array([cx, cy, a, h])
    for _ in range(rounds):
        m, p = predict(m, p)
        pos = pos + v
        z = pos + rng.standard_normal(4) * np.array([0.01 * h, 0.01 * h, 0.002 * a, 0.01 * h])
        m, p = update(m, p, z)
    for _ in range(predicts):
        m, p = predict(m, p)
    return m.astype(np.float32), ((p + p.T) / 2).astype(np.float32)


def _measurement(rng, mean32, cov32):
    """A measurement about one sigma of S from the state's projection, fp32."""
    pm, s = project(mean32, cov32)
    return (pm + rng.uniform(-1, 1, 4) * np.sqrt(np.abs(np.diag(s)))).astype(np.float32)


def _dense(rng, cov32):
    """The covariance with every coordinate coupled to every other: D (I + 0.2 N) C (I + 0.2 N)^T D, C the correlation matrix."""
    p = np.asarray(cov32, np.float64)
    d = np.sqrt(np.diag(p))
    g = np.eye(8) + 0.2 * rng.uniform(-1, 1, (8, 8))
    q = (g @ (p / np.outer(d, d)) @ g.T) * np.outer(d, d)
    return (q + q.T) / 2


def _cases():
    rng = np.random.default_rng(20240607)
    out = []

    def add(name, mean, cov, trackable=True):
        out.append(Case(name, mean, cov, _measurement(rng, mean, cov), trackable))
    for h in HEIGHTS:
        for c in CENTRES:
            for r in ROUNDS:
                for k in PREDICTS:
                    add(f"h{h:g} c{c:g} r{r} p{k}", *_prepared(rng, c, 0.75 * c + 5, 0.5, h, r, k))
    m, p = _prepared(rng, 700.0, 300.0, 0.4, 90.0, 30, 0, vel=(0.9, -0.6, 0.004, 0.05))            # 81 px and -54 px a frame
    add("large velocities", m, p)
    m, p = _prepared(rng, 900.0, 500.0, 0.5, 2.0, 5, 0)
    m[7] = np.float32(-5.0)                                                                        # predicted h = -3
    add("predicted h <= 0", m, p, trackable=False)
    m, p = (a.astype(np.float32) for a in predict(m, p))
    add("h < 0 on entry", m, (p + p.T) / 2, trackable=False)                                        # std = w h < 0 must square to the same noise
    add("a 0.05", *_prepared(rng, 1200.0, 640.0, 0.05, 400.0, 30, 1))
    add("a 8", *_prepared(rng, 2500.0, 200.0, 8.0, 40.0, 30, 1))
    m, p = _prepared(rng, 1800.0, 900.0, 0.45, 150.0, 30, 1)
    dense = _dense(rng, p)
    add("dense P", m, dense.astype(np.float32))
    # not symmetric, and still not after a predict, although S is before and after: position-velocity blocks X + A above and X^T - A
    # below with A diagonal, so their sum (what a predict adds to the measured block) stays symmetric and they are no transposes
    q = _dense(rng, p)
    a = 0.05 * np.diag(np.sqrt(np.diag(q)[:4] * np.diag(q)[4:]))
    q[:4, 4:] += a
    q[4:, :4] -= a
    add("dense P, not symmetric", m, q.astype(np.float32))
    return out


CASES = _cases()
GRID = len(HEIGHTS) * len(CENTRES) * len(ROUNDS) * len(PREDICTS)


def batch(idx):
    """(mean [n, 8], cov [n, 8, 8], z [n, 4]) fp32 of the cases idx."""
    return (np.stack([CASES[i].mean for i in idx]), np.stack([CASES[i].cov for i in idx]), np.stack([CASES[i].z for i in idx]))


def cyclic(n, start=0):
    return [(start + i) % len(CASES) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ form 1, measured
def measure(kf, n_list=(len(CASES),), project_n=(len(CASES),)):
    """The figures of an implementation `kf` (initiate / predict(dt) / project / update on fp32 BATCHES) on every case, in batches of
    the sizes given (the cases taken cyclically).  Returns {operation: (covariance figure, mean figure)} -- the maxima."""
    out = {}

    def worst(key, c, m):
        a = out.get(key, (0.0, 0.0))
        out[key] = (max(a[0], c), max(a[1], m))
    for bi, n in enumerate(n_list):
        idx = cyclic(n, 7 * bi)
        mean, cov, z = batch(idx)
        for dt in (1.0,) + DTS:
            gm, gc = kf.predict(mean, cov, dt)
            for k in range(n):
                worst(f"predict dt {dt:.4g}", *predict_errs(gm[k], gc[k], mean[k], cov[k], dt))
        gm, gc = kf.update(mean, cov, z)
        for k in range(n):
            worst("update", *update_errs(gm[k], gc[k], mean[k], cov[k], z[k]))
        gm, gc = kf.initiate(z)
        for k in range(n):
            m64, p64 = initiate(z[k])
            worst("initiate", float(cov_err(gc[k], p64, p64).max()), float(np.abs(gm[k] - m64).max()))
    for bi, n in enumerate(project_n):
        idx = cyclic(n, 11 * bi)
        mean, cov, _ = batch(idx)
        gm, gs = kf.project(mean, cov)
        for k in range(n):
            pm, s = project(mean[k], cov[k])
            worst("project", float(cov_err(gs[k], s, s).max()), float(np.abs(gm[k] - pm).max()))
    return out


# ------------------------------------------------------------------------------------------------------------------ gating cases
GATE_TARGETS = (0.0, 0.5, 3.0, CHI2_4 * (1 - 1e-2), CHI2_4 * (1 + 1e-2), 9.0, CHI2_4 * (1 - 1e-3), 12.0, CHI2_4 * (1 + 1e-3), 30.0, 200.0)
GATE_M = (1, 63, 64, 65, 200)


def _not_pd_states():
    """(a) S not positive definite in the first pivot, (b) h = 0 with P = 0: the pivot is exactly 0, (c) P[3][3] so negative that the
    4 x 4 factorisation fails and the 2 x 2 does not."""
    base = CASES[3 * 6 + 3]                                       # h 2, centre 10, thirty rounds
    m, p = base.mean.copy(), base.cov.copy()
    _, s = project(m, p)
    pa = p.copy()
    pa[0, 0] = np.float32(-((s[0, 0] - float(p[0, 0])) + 1.0))    # -(R00 + 1)
    mb = m.copy()
    mb[3] = 0
    pc = p.copy()
    pc[3, 3] = np.float32(-4.0 * s[3, 3])
    return [("a", m, pa), ("b", mb, np.zeros((8, 8), np.float32)), ("c", m, pc)]


def gate_groups():
    """Groups of five tracks for aic_kf_gating (n = 5; n = 1 takes the first track of a group): the predicted state of every
    trackable case, and the three states that are not positive definite at rows 1, 3 and 4 of three different groups."""
    tracks = []
    for c in CASES:
        if c.trackable:
            m, p = predict(c.mean, c.cov)
            tracks.append((c.name, m.astype(np.float32), p.astype(np.float32)))
    npd = _not_pd_states()
    groups = [tracks[i:i + 5] for i in range(0, len(tracks) - 4, 5)]
    groups[0] = [groups[0][0], npd[0]] + groups[0][1:4]
    groups[1] = groups[1][:3] + [npd[1]] + groups[1][3:4]
    groups[2] = groups[2][:4] + [npd[2]]
    groups.append([npd[2], npd[0], npd[1], tracks[0], tracks[1]])   # n = 1 reaches a state that is not positive definite too
    return groups


def gate_measurements(group, gi, m, shared_z):
    """zs fp32: [m, 4] around track 0 of the group (shared_z) or [n, m, 4], every track its own.  Measurement j sits at squared distance
    GATE_TARGETS[j mod 11] from the track in the metric of S (of |S| where S is not positive definite), in a seeded direction, so the cells
    straddle CHI2_4 at a relative 1e-2 and 1e-3 (case d) and run out to 200."""
    rng = np.random.default_rng(1000 * gi + 10 * m + shared_z)
    per = []
    for _, mean, cov in (group[:1] if shared_z else group):
        pm, s = project(mean, cov)
        lo = np.linalg.cholesky(s) if is_pd(s) else np.diag(np.sqrt(np.abs(np.diag(s)) + 1e-4))
        u = rng.standard_normal((m, 4))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        r = np.sqrt(np.array([GATE_TARGETS[(j + gi) % len(GATE_TARGETS)] for j in range(m)]))
        per.append((pm + (u * r[:, None]) @ lo.T).astype(np.float32))
    return per[0] if shared_z else np.stack(per)


def gate_ref(group, zs, shared_z, only_position):
    return np.stack([gating(mean, cov, zs if shared_z else zs[t], only_position) for t, (_, mean, cov) in enumerate(group)])


# ------------------------------------------------------------------------------------------------------------------ tracker-path cases
DIM = 16
NEW_H = (1.0 / 3, 179.3, 1e-3)
NEW_AT = ((-540.0, -3.0), (-700.0, -100.0), (-520.0, 8.0))       # left of every track's box, at coordinates whose fp32 spacing (6e-5) is below the smallest box


def feature(k):
    """+e_k for k < 16, -e_(k - 16) above: 32 unit vectors of dim 16 at cosine distance 1 or 2 from each other."""
    f = np.zeros(DIM, np.float32)
    f[k % DIM] = 1.0 if (k // DIM) % 2 == 0 else -1.0
    return f


def track_case_ids():
    """Every fourth case of the grid (all heights, centres and preparations occur) and the trackable extra cases: 28 states."""
    return list(range(0, GRID, 4)) + [i for i in range(GRID, len(CASES)) if CASES[i].trackable]


@dataclass
class Plan:
    mean: np.ndarray          # [T, 8] fp32 planted states, list order (decoys included)
    cov: np.ndarray           # [T, 8, 8]
    state: np.ndarray         # [T] 2 = confirmed, 1 = tentative (a decoy: far from every detection, deleted by the frame)
    feat: np.ndarray          # [T, DIM] the one gallery row of a confirmed track (decoys have no gallery)
    det: np.ndarray           # [n, 4] fp32 tlwh, shuffled
    det_feat: np.ndarray      # [n, DIM]
    pair: dict                # list position of a confirmed track -> detection row
    new: list                 # detection rows that match nothing (new tracks), ascending


def plan(ids, offsets=None, decoy_every=3, seed=0, new=True):
    """plan_states of the states of the cases `ids`, translated by offsets[k] when given."""
    mean = [CASES[ci].mean.copy() for ci in ids]
    if offsets is not None:
        for k, m in enumerate(mean):
            m[:2] += np.asarray(offsets[k], np.float32)
    return plan_states(mean, [CASES[ci].cov for ci in ids], decoy_every, seed, new)


def plan_states(means, covs, decoy_every=3, seed=0, new=True):
    """The planted frame: the given states as confirmed tracks, a tentative decoy after every `decoy_every` of them (so that a track's
    position among the matched differs from its list position and Kalman slot; the frame prunes the decoys, and from the next frame
    on list position and slot differ too), one detection per confirmed track -- its PREDICTED box moved by 2 % of its width and
    -3 % of its height and grown by 2 % -- with the track's own feature, three detections that belong to nobody, all rows shuffled."""
    rng = np.random.default_rng(4242 + seed)
    mean, cov, state, feat, boxes, dfeat, owner = [], [], [], [], [], [], []
    for k, (m, c) in enumerate(zip(means, covs)):
        mean.append(np.asarray(m, np.float32)), cov.append(np.asarray(c, np.float32)), state.append(2), feat.append(feature(k))
        owner.append(len(mean) - 1)
        pm, _ = predict(m, c)
        x, y, w, h = mean_to_tlwh(pm)
        boxes.append((x + 0.01 * w, y - 0.04 * h, 1.02 * w, 1.02 * h))      # centre + (0.02 w, -0.03 h), sides x 1.02
        dfeat.append(feature(k))
        if decoy_every and k % decoy_every == decoy_every - 1:
            d = CASES[(5 * k + 1) % GRID]
            dm = d.mean.copy()
            dm[:2] = (-9000.0 - 300.0 * k, -9000.0)
            mean.append(dm), cov.append(d.cov), state.append(1), feat.append(np.zeros(DIM, np.float32))
    n_own = len(boxes)
    if new:
        for q, h in enumerate(NEW_H):
            boxes.append((NEW_AT[q][0], NEW_AT[q][1], 0.4 * h, h))
            dfeat.append(feature(n_own + q))
    perm = rng.permutation(len(boxes))
    det = np.asarray(boxes, np.float64)[perm].astype(np.float32)
    row_of = {int(src): r for r, src in enumerate(perm)}
    return Plan(np.stack(mean), np.stack(cov), np.asarray(state, np.int32), np.stack(feat), det, np.stack(dfeat)[perm],
                {owner[k]: row_of[k] for k in range(n_own)}, sorted(row_of[k] for k in range(n_own, len(boxes))))


def drift_frames(p, k):
    """k frames of detection boxes [n, 4] fp32, the first the plan's own: every planned detection goes on along its track's predicted
    velocity (all four components) and drifts by a further 0.3 % of its size a frame; the detections of nobody stand still."""
    z0 = xyah32(p.det).astype(np.float64)
    vel = np.zeros((len(p.det), 4))
    for t, j in p.pair.items():
        vel[j] = predict(p.mean[t], p.cov[t])[0][4:]
    out = [p.det]
    for f in range(1, k):
        z = z0 + f * vel
        h = z[:, 3]
        w = z[:, 2] * h
        out.append(np.stack([z[:, 0] - w / 2 + 0.003 * f * w, z[:, 1] - h / 2 + 0.003 * f * h, w, h], 1).astype(np.float32))
    return out


def expected_step(p):
    """Float64 update(predict(state), z) of every matched track of the plan: {list position: (mean, cov, predicted mean, predicted cov)}."""
    z = xyah32(p.det)
    out = {}
    for t, j in p.pair.items():
        pm, pp = predict(p.mean[t], p.cov[t])
        m2, p2 = update(pm, pp, z[j])
        out[t] = (m2, p2, pm, pp)
    return out


def step_errs(got_mean, got_cov, mean32, cov32, z32):
    """(covariance figure, mean figure) of update(predict(state), z): the update's metrics, from the float64 predicted state."""
    pm, pp = predict(mean32, cov32)
    _, s, k = gain(pm, pp)
    m2, p2 = update(pm, pp, z32)
    scale = np.abs(pm) + np.abs(k) @ np.abs(np.asarray(z32, np.float64) - pm[:4])
    return float(cov_err(got_cov, p2, pp).max()), float(scaled_err(got_mean, m2, scale).max())


# ---- ByteTrack: no import, so the states are raised by frames
BT_OBJECTS = ((0.5, 30000.0), (2.0, 10.0), (20.0, 4000.0), (179.3, 30000.0), (2000.0, 4000.0), (20.0, 10.0))     # (h, centre), far apart
BT_ABSENT, BT_GONE = 2, range(5, 9)                                # object 2 is not detected in frames 5 .. 8 (1-based) and returns in 9


def bt_boxes(f):
    """xyxy fp32 of frame f (1-based) and which object each row is.  An object drifts by h / 64 a frame, grows by 1 % of its first
    height a frame and its aspect by 0.002 from 0.5: every component of every update has an innovation, and a track that is lost has
    a height velocity to lose."""
    rows, who = [], []
    for k, (h0, c) in enumerate(BT_OBJECTS):
        if k == BT_ABSENT and f in BT_GONE:
            continue
        h, a = h0 * (1 + 0.01 * (f - 1)), 0.5 + 0.002 * (f - 1)
        cx, cy = c + (f - 1) * h0 / 64, 0.75 * c + 5 - (f - 1) * h0 / 128
        rows.append((cx - 0.5 * a * h, cy - 0.5 * h, cx + 0.5 * a * h, cy + 0.5 * h))
        who.append(k)
    order = np.random.default_rng(f).permutation(len(rows))
    return np.asarray(rows, np.float32)[order], [who[i] for i in order]


# ---- the epoch kernel's choice between its two update forms (kernels_trk_dev.hip: `72 * T <= L.arena_floats`)
def epoch_arena_floats(cap, nmax, k, lds_bytes=159 * 1024, n_waves=8, kf_slots=96):
    """lds_carve() of kernels_trk_dev.hip restated: what is left of the launch's dynamic LDS (epoch_lds_bytes() = 159 KiB) after the
    tables of a tracker of `cap` slots, an epoch of k frames and at most nmax detections a frame; every array rounded up to 16 bytes."""
    r16 = lambda b: (b + 15) // 16 * 16
    mx = max(cap, nmax)
    used = 3 * r16(8 * mx)                        # u, v, dist (double)
    used += 15 * r16(4 * cap)                     # id state hits age tsu cls slot glen ghead sm napp glen0 mdet rows feas
    used += 6 * r16(4 * mx)                       # pred rowof colof todo pos asg
    used += r16(4 * cap) + r16(16 * cap)          # conf, tbox
    used += r16(2 * cap * k)                      # newrow
    used += r16(4 * cap)                          # free_slots
    used += r16(4 * 72 * kf_slots)                # kf
    used += 2 * r16(16 * nmax) + r16(4 * nmax)    # tlwh, xyah, dconf
    used += 5 * r16(4 * nmax)                     # dcls dhas mtrk und cols
    used += r16(4 * (n_waves + 8))                # wcnt
    return (lds_bytes - used) // 4


def first_fallback_tracks(extra_dets=len(NEW_H), cap=512, k=1):
    """The smallest number of tracks T (one detection each, plus extra_dets) for which 72 * T > arena_floats: the epoch kernel then
    gives every matched track a wave (kf_update_wave) instead of a thread per (track, row)."""
    for t in range(1, cap + 1):
        if 72 * t > epoch_arena_floats(cap, t + extra_dets, k):
            return t
    return None


# ------------------------------------------------------------------------------------------------------------------ gating, measured
def gate_runs(fn, n_one=(0, 1, 2, -1)):
    """fn(mean [n, 8], cov [n, 8, 8], zs, shared_z, only_position) -> d2 [n, m] on every group at n = 5, and at n = 1 on the groups n_one;
    every m of GATE_M, shared and own measurements, all four components and position only.  Returns the records
    (group, n, m, shared_z, only_position, ref [n, m] float64, got [n, m])."""
    recs = []
    groups = gate_groups()
    one = {i % len(groups) for i in n_one}
    for gi, group in enumerate(groups):
        for n in (5, 1) if gi in one else (5,):
            g = group[:n]
            mean, cov = np.stack([t[1] for t in g]), np.stack([t[2] for t in g])
            for m in GATE_M:
                for shared in (0, 1):
                    zs = gate_measurements(g, gi, m, shared)
                    for op in (0, 1):
                        got = np.asarray(fn(mean, cov, zs, shared, op), np.float64).reshape(n, m)
                        recs.append((gi, n, m, shared, op, gate_ref(g, zs, shared, op), got))
    return recs


def gate_figure(recs):
    return max(gating_err(r[6], r[5]) for r in recs)


def gate_sure(recs, oracle_figure):
    """Per record the cells whose side of CHI2_4 is beyond 4 x the restatement's deviation (check_costs' rule)."""
    return [np.abs(r[5] - CHI2_4) > 4 * oracle_figure * np.maximum(1.0, np.where(np.isinf(r[5]), 1.0, r[5])) for r in recs]
