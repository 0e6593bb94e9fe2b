"""The executable specification of the heat-map stage (aic_heat_*): Python ints and NumPy integer arrays only, one
stream per HeatOracle.  The device is held to it with np.array_equal (tests/test_gpu_heat.py).

A tick of a stream is rows [n, 6] int32 = x1 y1 x2 y2 id cls, what every tracker here delivers; only render() sees frames.

Grid.  Frame H x W, cells of `cell` x `cell` pixels (4, 8, 16, 32): GW = ceil(W / cell), GH = ceil(H / cell), at most 32768 cells.  Twelve
int32 layers [GH, GW]: VISITS, DWELL, STARTS, ENDS, DIR0..DIR7.

A row is VALID if its four coordinates are within +-2^20 and x2 >= x1, y2 >= y1; FIRST if no earlier valid row of the frame has its id;
NONEMPTY if x1 < W, x2 >= 0, y1 < H, y2 >= 0.  A row with all three is COUNTED.  Its anchor, in doubled pixels: fx = clamp(x1 + x2, 0,
2 W - 1); fy = clamp(2 y2, 0, 2 H - 1) (foot) or clamp(y1 + y2, 0, 2 H - 1) (centre); its cell is ((fx >> 1) // cell, (fy >> 1) // cell).

The life cycle of the slot table -- expiry by forget_after, the capacity rule (a tick that would exceed max_tracks commits nothing, the
layers included, and the stream stops with ERR_CAPACITY), emission in slot order while the call's list has room, the lowest free slot
for a new id -- is the colour stage's (tests/colours_oracle.py, DESIGN.md sections 38 and 48) to the letter.

A new slot: STARTS, VISITS, DWELL of the row's cell += 1; the slot keeps cell, fx, fy, start fx fy, path 0, in_cell 1, max_step 0,
cells 1, moving 0.  A slot seen again: dx, dy from the slot's fx, fy; step = max(|dx|, |dy|); DWELL[cell] += 1; a cell other than the
slot's: VISITS[cell] += 1, cells += 1, in_cell = 1, else in_cell += 1; step >= min_move: DIR[octant(dx, dy)][cell] += 1, moving += 1;
path = min(path + step, 2^30), max_step = max(max_step, step).  Every slot counter and every layer cell stops at 2^30.

ENDS[the slot's cell] += 1 when the track's event LEAVES THE TABLE (is emitted), not when the slot expires: a track waiting in pending
is not yet in ENDS.

An event is 16 ints: reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, cells, start_fx, start_fy,
end_fx, end_fy, path, max_step, moving, last cell index (cy * GW + cx).  Row tags [rows, 4]: cell index, in_cell, step (0 for a new
slot), octant or -1 (no step of min_move) for a counted row; -1, 0, 0, -1 for every other row and for a stopped stream."""
import numpy as np

LIVE, EXPIRED, FLUSHED = 0, 1, 2
COORD_MAX = 1 << 20
MAX_ROWS = MAX_TRACKS = 512
CELLS_MAX = 32768
ERR_CAPACITY = -5
SAT = 1 << 30
Q_MAX = 65280
LAYERS = ("visits", "dwell", "starts", "ends", "dir0", "dir1", "dir2", "dir3", "dir4", "dir5", "dir6", "dir7")
VISITS, DWELL, STARTS, ENDS, DIR0 = 0, 1, 2, 3, 4
FOOT, CENTRE = 0, 1
LINEAR, LOG = 0, 1
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "cells", "start_fx", "start_fy", "end_fx", "end_fy",
                "path", "max_step", "moving", "last_cell")
LUT_ANCHORS = ((0, (0, 0, 160)), (64, (0, 160, 255)), (128, (0, 255, 0)), (192, (255, 255, 0)), (255, (255, 0, 0)))      # L, RGB


# ---------------------------------------------------------------------------------------------------- arithmetic
def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def valid_row(row):
    return all(abs(int(v)) <= COORD_MAX for v in row[:4]) and int(row[2]) >= int(row[0]) and int(row[3]) >= int(row[1])


def octant(dx, dy):
    """Image coordinates, y down, clockwise from east; (dx, dy) != (0, 0).  5 / 12 stands for tan 22.5 degrees."""
    ax, ay = abs(dx), abs(dy)
    if 12 * ay < 5 * ax:
        return 0 if dx > 0 else 4
    if 12 * ax < 5 * ay:
        return 2 if dy > 0 else 6
    return (1 if dx > 0 else 3) if dy > 0 else (7 if dx > 0 else 5)


def log_q8(v):
    """u(v): the Q8 base-2 logarithm of v + 1: floor(log2) << 8 | the next 8 bits below the leading one (zero-filled)."""
    n = int(v) + 1
    b = n.bit_length() - 1
    m = n >> (b - 8) if b >= 8 else n << (8 - b)
    return (b << 8) | (m & 255)


def level(v, M, scale):
    v, M = int(v), int(M)
    return v * Q_MAX // M if scale == LINEAR else log_q8(v) * Q_MAX // log_q8(M)


def levels(layer, scale):
    """(M, uint16 levels) of one layer; M = 0: no levels."""
    M = int(layer.max())
    if M == 0:
        return 0, None
    return M, np.array([level(v, M, scale) for v in layer.reshape(-1)], np.int64).reshape(layer.shape)


def axis(n_px, cell, n_cells):
    """(i0, i1, w) per pixel along one axis, int64 arrays: neighbours clamped, w in 0 .. 2 cell - 1 the weight of i1."""
    d = 2 * np.arange(n_px, dtype=np.int64) + 1 - cell
    i = d // (2 * cell)                                                      # floor: -1 in the first half cell
    return np.clip(i, 0, n_cells - 1), np.clip(i + 1, 0, n_cells - 1), d - 2 * cell * i


def bilinear(q, H, W, cell):
    """L [H, W] in 0..255 from the levels q [GH, GW]."""
    GH, GW = q.shape
    y0, y1, wy = axis(H, cell, GH)
    x0, x1, wx = axis(W, cell, GW)
    c2 = 2 * cell
    q = q.astype(np.int64)
    top = q[y0][:, x0] * (c2 - wx) + q[y0][:, x1] * wx
    bot = q[y1][:, x0] * (c2 - wx) + q[y1][:, x1] * wx
    total = top * (c2 - wy)[:, None] + bot * wy[:, None] + 4 * cell * cell * 128
    assert total.max() < 1 << 28                                             # 65280 * 4096 + 128 * 4096 at the most
    return total >> ((4 * cell * cell).bit_length() - 1 + 8)


def default_lut():
    """uint8 [256, 3] BGR: the integer piecewise-linear ramp through LUT_ANCHORS."""
    lut = np.zeros((256, 3), np.uint8)
    for (a, p), (b, q) in zip(LUT_ANCHORS, LUT_ANCHORS[1:]):
        n = b - a
        for k in range(n + 1):
            lut[a + k] = [(p[c] * (n - k) + q[c] * k + n // 2) // n for c in (2, 1, 0)]
    return lut


def render(frames, cameras, layers_of, layer, H, W, cell, scale=LOG, alpha_q8=160, floor=8, lut=None):
    """frames uint8 [n, H, W, 3] -> a rendered copy.  cameras[f] = the camera of frame f; layers_of(camera) -> its [12, GH, GW] layers."""
    lut = default_lut() if lut is None else np.asarray(lut, np.uint8).reshape(256, 3)
    out = np.array(frames, np.uint8, copy=True)
    cache = {}
    for f, cam in enumerate(cameras):
        if cam not in cache:
            M, q = levels(layers_of(cam)[layer], scale)
            cache[cam] = None if M == 0 else bilinear(q, H, W, cell)
        L = cache[cam]
        if L is None:
            continue
        px = out[f].astype(np.int64)
        new = (px * (256 - alpha_q8) + lut[L].astype(np.int64) * alpha_q8 + 128) >> 8
        out[f] = np.where((L >= floor)[..., None], new, px).astype(np.uint8)
    return out


class HeatOracle:
    def __init__(self, frame_hw, cell=16, max_tracks=128, forget_after=70, anchor=FOOT, min_move=4, stream=0):
        self.H, self.W, self.cell = int(frame_hw[0]), int(frame_hw[1]), int(cell)
        assert 1 <= self.H <= 16384 and 1 <= self.W <= 16384 and cell in (4, 8, 16, 32) and 1 <= max_tracks <= MAX_TRACKS and forget_after >= 0
        assert anchor in (FOOT, CENTRE) and 1 <= min_move <= 1 << 20
        self.GW, self.GH = -(-self.W // cell), -(-self.H // cell)
        assert self.GW * self.GH <= CELLS_MAX
        self.max_tracks, self.forget_after, self.anchor, self.min_move, self.stream = max_tracks, forget_after, anchor, min_move, stream
        # what tests/test_heat_oracle.py counts
        self.log = dict(new=0, same_cell=0, new_cell=0, moved=0, still=0, octants=[0] * 8, clamp_left=0, clamp_right=0, clamp_top=0, clamp_bottom=0,
                        duplicate=0, expired=0, flushed=0, capacity_stop=0, pending_over_cap=0, saturated=0)
        self.reset()

    def reset(self):
        self.frame, self.status = 0, 0
        self.slots = [None] * self.max_tracks
        self.layers = np.zeros((12, self.GH, self.GW), np.int32)

    # ------------------------------------------------------------------------------------------------ rows of one frame
    def anchor_of(self, row):
        x1, y1, x2, y2 = (int(v) for v in row[:4])
        fx, fy = x1 + x2, (2 * y2 if self.anchor == FOOT else y1 + y2)
        self.log["clamp_left"] += fx < 0
        self.log["clamp_right"] += fx > 2 * self.W - 1
        self.log["clamp_top"] += fy < 0
        self.log["clamp_bottom"] += fy > 2 * self.H - 1
        return clamp(fx, 0, 2 * self.W - 1), clamp(fy, 0, 2 * self.H - 1)

    def measure(self, rows):
        """[(row index, id, cls, fx, fy, cy, cx)] of the counted rows, in row order."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        assert len(rows) <= MAX_ROWS
        out, seen = [], set()
        for i, r in enumerate(rows):
            if not valid_row(r):
                continue
            if int(r[4]) in seen:
                self.log["duplicate"] += 1
                continue
            seen.add(int(r[4]))
            if not (r[0] < self.W and r[2] >= 0 and r[1] < self.H and r[3] >= 0):
                continue
            fx, fy = self.anchor_of(r)
            out.append((i, int(r[4]), int(r[5]), fx, fy, (fy >> 1) // self.cell, (fx >> 1) // self.cell))
        return out

    def _add(self, adds, layer, cy, cx):
        adds[(layer, cy, cx)] = adds.get((layer, cy, cx), 0) + 1

    def _apply(self, adds):
        """min(old + n, 2^30) per cell, n = the adds of one tick (or of one emission)."""
        for (layer, cy, cx), n in adds.items():
            v = int(self.layers[layer, cy, cx]) + n
            self.log["saturated"] += v > SAT
            self.layers[layer, cy, cx] = min(v, SAT)

    # ------------------------------------------------------------------------------------------------ events
    def _event(self, s, reason):
        t = self.slots[s]
        return np.array([reason, self.stream, t["id"], t["cls"], t["first"], t["last"], t["sightings"], t["cells"], t["sfx"], t["sfy"], t["fx"], t["fy"],
                         t["path"], t["max_step"], t["moving"], t["cy"] * self.GW + t["cx"]], np.int32)

    def _emit(self, out, cap):
        adds = {}
        for s, t in enumerate(self.slots):
            if t is not None and t["ended"] and len(out) < cap:
                out.append(self._event(s, t["ended"]))
                self._add(adds, ENDS, t["cy"], t["cx"])
                self.slots[s] = None
        self._apply(adds)
        self.log["pending_over_cap"] += self.pending() > 0

    def pending(self):
        return sum(t is not None and t["ended"] != 0 for t in self.slots)

    # ------------------------------------------------------------------------------------------------ one tick
    def step(self, rows, out, cap):
        """One tick; returns its row tags [n, 4]."""
        tags = np.tile(np.array([-1, 0, 0, -1], np.int32), (len(rows), 1))
        if self.status:
            return tags
        f = self.frame
        counted = self.measure(rows)
        live = {t["id"]: s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] <= self.forget_after}
        expiring = [s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] > self.forget_after]
        ended = [s for s, t in enumerate(self.slots) if t is not None and (t["ended"] or s in expiring)]          # slot order
        kept = ended[max(0, cap - len(out)):]                                # no room in the output list: they keep their slots
        occupied = len(live) + sum(self.slots[s]["ended"] != 0 for s in ended) + sum(s in expiring for s in kept)
        if occupied + sum(c[1] not in live for c in counted) > self.max_tracks:
            self.status = ERR_CAPACITY
            self.log["capacity_stop"] += 1
            return tags
        for s in expiring:
            self.slots[s]["ended"] = EXPIRED
            self.log["expired"] += 1
        self._emit(out, cap)
        adds = {}
        for i, tid, cls, fx, fy, cy, cx in counted:
            step, oc = 0, -1
            if tid in live:
                s = live[tid]
                t = self.slots[s]
                dx, dy = fx - t["fx"], fy - t["fy"]
                step = max(abs(dx), abs(dy))
                if (cy, cx) != (t["cy"], t["cx"]):
                    self._add(adds, VISITS, cy, cx)
                    t["cells"], t["in_cell"] = min(t["cells"] + 1, SAT), 1
                    self.log["new_cell"] += 1
                else:
                    t["in_cell"] = min(t["in_cell"] + 1, SAT)
                    self.log["same_cell"] += 1
                if step >= self.min_move:
                    oc = octant(dx, dy)
                    self._add(adds, DIR0 + oc, cy, cx)
                    t["moving"] = min(t["moving"] + 1, SAT)
                    self.log["moved"] += 1
                    self.log["octants"][oc] += 1
                else:
                    self.log["still"] += 1
                t["path"], t["max_step"] = min(t["path"] + step, SAT), max(t["max_step"], step)
            else:
                s = self.slots.index(None)
                t = self.slots[s] = dict(id=tid, first=f, sightings=0, ended=0, sfx=fx, sfy=fy, path=0, in_cell=1, max_step=0, cells=1, moving=0)
                self._add(adds, STARTS, cy, cx)
                self._add(adds, VISITS, cy, cx)
                self.log["new"] += 1
            self._add(adds, DWELL, cy, cx)
            t.update(last=f, cls=cls, sightings=t["sightings"] + 1, fx=fx, fy=fy, cy=cy, cx=cx)
            tags[i] = [cy * self.GW + cx, t["in_cell"], step, oc]
        self._apply(adds)
        self.frame += 1
        return tags

    # ------------------------------------------------------------------------------------------------ calls
    def update(self, rows, cap):
        """rows[t] for the ticks of one call -> ([event], pending, status, [row tags per tick]); no ticks: a drain."""
        out = []
        if len(rows) == 0:
            self._emit(out, cap)
        tags = [self.step(r, out, cap) for r in rows]
        return out, self.pending(), self.status, tags

    def flush(self, cap):
        out = []
        for t in self.slots:
            if t is not None and not t["ended"]:
                t["ended"] = FLUSHED
                self.log["flushed"] += 1
        self._emit(out, cap)
        return out, self.pending(), self.status, []

    def export(self):
        return [self._event(s, t["ended"]) for s, t in enumerate(self.slots) if t is not None]

    # ------------------------------------------------------------------------------------------------ ageing and persistence
    def decay(self, layer_mask, shift):
        assert 0 < layer_mask < 1 << 12 and 1 <= shift <= 31
        for l in range(12):
            if layer_mask >> l & 1:
                self.layers[l] >>= shift

    def export_layers(self, layer_mask=0xFFF):
        return np.stack([self.layers[l] for l in range(12) if layer_mask >> l & 1]).copy()

    def import_layers(self, layer_mask, values):
        values = np.asarray(values)
        ls = [l for l in range(12) if layer_mask >> l & 1]
        assert values.shape == (len(ls), self.GH, self.GW)
        if values.min() < 0 or values.max() > SAT:
            raise ValueError("a layer value outside 0..2^30")
        for k, l in enumerate(ls):
            self.layers[l] = values[k]


def pack(results, cap, ticks=0):
    """[(finals, pending, status, tags per tick)] per stream -> the flat outputs of aic_heat_update / _flush: n_final [S], events
    [S, cap, 16], row_tags [rows, 4] (tick-major), pending [S], status [S]."""
    S = len(results)
    n_final, pending, status = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    events = np.zeros((S, cap, 16), np.int32)
    for s, (out, pend, st, _) in enumerate(results):
        n_final[s], pending[s], status[s] = len(out), pend, st
        for k, ev in enumerate(out):
            events[s, k] = ev
    tags = [results[s][3][t] for t in range(ticks) for s in range(S)]
    row_tags = np.concatenate(tags).reshape(-1, 4).astype(np.int32) if tags else np.zeros((0, 4), np.int32)
    return n_final, events, row_tags, pending, status


def run_bank(oracles, rows, cap):
    """rows[t][s] = rows array.  One call of a bank, packed."""
    T = len(rows)
    res = [o.update([rows[t][s] for t in range(T)], cap) for s, o in enumerate(oracles)]
    return pack(res, cap, T)


def flush_bank(oracles, cap, stream=None):
    res = [o.flush(cap) if stream is None or stream == s else ([], o.pending(), o.status, []) for s, o in enumerate(oracles)]
    return pack(res, cap)


def layers_bank(oracles):
    return np.stack([o.layers for o in oracles])
