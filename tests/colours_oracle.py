"""The executable specification of the clothing-colour stage (aic_colours_*): Python ints and NumPy integer
arrays only, one stream per ColoursOracle.  The device is held to it with np.array_equal (tests/test_gpu_colours.py).

A tick of a stream is one BGR frame [H, W, 3] uint8 and rows [n, 6] int32 = x1 y1 x2 y2 id cls, what every tracker here delivers.

VALID, COUNTED and OCCLUDER are section 38's: a row is VALID if its four coordinates are within +-COORD_MAX and x2 >= x1, y2 >= y1;
rows that are not are ignored altogether.  A row is COUNTED if it is the first valid row of its id in row order and its box clipped to
the frame is not empty (a later row of the same id is never counted, whatever became of the first).  An occluder of row i is a valid row
j of another id with y2_j > y2_i, or y2_j == y2_i and j < i; Bj is its box clipped to the frame.

Parts.  With bw = x2 - x1, bh = y2 - y1 on the unclipped box and inset = (bw * inset_q8) >> 8, the part with fractions (a, b) is the
inclusive rectangle x1 + inset .. x2 - inset, y1 + ((bh * a) >> 8) .. y1 + ((bh * b) >> 8); P is the part clipped to the frame, pw x ph
(an empty P has pw = ph = 0 and is never sampled: min_w, min_h >= 1).  A part is SAMPLED if pw >= min_w, ph >= min_h and the largest
area(P & Bj) * 256 // (pw * ph) over the occluders is <= max_cover_q8.  An unsampled part adds nothing; the row still claims its slot.

Pixel class: classify() below.  Sample of a sampled part: counts c[12] over its n = pw * ph pixels, shares s[k] = c[k] * 256 // n; the
slot accumulates acc[part][k] += s[k], samples[part] += 1 -- every sighting weighs the same.  samples[part] stops at SAMPLES_MAX = 2^20
and later samples of that part are ignored, so acc <= 256 * 2^20 = 2^28 stays inside int32.

Tick f of a stream (f counts every committed tick): section 38's steps with "the shot" replaced by "the accumulators":
  1. the counted rows.
  2. capacity: the live slots that do not expire now, the ENDED slots not yet emitted, the slots that expire now but for which this
     call's output list has no room left (they stay ENDED and keep their slot), plus the counted rows of unknown ids, may not exceed
     max_tracks.  Otherwise the stream STOPS with ERR_CAPACITY: this tick is not committed, later ticks deliver nothing until reset();
     export, flush and a ticks = 0 drain still work.
  3. every live slot with f - last_seen > forget_after becomes ENDED (reason EXPIRED): frozen, never matched by an id again.
  4. ENDED slots are emitted in slot order while the call's output list has room (cap per stream per call) and become free.
  5. the counted rows in row order: an unknown id takes the lowest free slot; last_seen, cls and the sighting count are updated; every
     sampled part is accumulated.
An event is 48 ints: reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, samples_upper,
samples_lower, top_upper, second_upper, top_lower, second_lower, slot, 0, 0, hist_upper[12], hist_lower[12], 8 zeros.  hist[k] =
acc[k] // samples (0 without samples); top = the bin of the largest acc, lowest index on ties (-1 without samples); second = the
largest of the other bins, lowest index on ties, if its acc > 0 and acc * 4 >= acc[top], else -1.
Row tags [rows, 4] = top_upper, top_lower, hist_upper[top_upper], hist_lower[top_lower] from the row's slot AFTER its tick; -1 (share 0)
where the part has no sample yet; four times -1 for a row that is not counted or that belongs to a stopped stream (the rows of the tick
a stream stops at included: that tick is not committed).

Readings this file decides.  (a) The counted test is on the BOX clipped to the frame, not on a part: a row whose parts are both empty or
too small still claims its slot.  (b) min_w / min_h and the cover are measured on the clipped part P.  (c) An occluder covers with its
whole clipped box.  (d) The capacity rule is section 38's to the letter, the output-list term included."""
import numpy as np

LIVE, EXPIRED, FLUSHED = 0, 1, 2
COORD_MAX = 1 << 20
MAX_ROWS = MAX_TRACKS = 512
ERR_CAPACITY = -5
SAMPLES_MAX = 1 << 20
NAMES = ("black", "gray", "white", "red", "orange", "yellow", "green", "cyan", "blue", "purple", "pink", "brown")
BLACK, GRAY, WHITE, RED, ORANGE, YELLOW, GREEN, CYAN, BLUE, PURPLE, PINK, BROWN = range(12)
EVENT_FIELDS = ("reason", "stream", "id", "cls", "first_frame", "last_seen", "sightings", "samples_upper", "samples_lower", "top_upper",
                "second_upper", "top_lower", "second_lower", "slot")
HUE_BOUNDS = ((64, RED), (192, ORANGE), (299, YELLOW), (704, GREEN), (853, CYAN), (1109, BLUE), (1300, PURPLE), (1472, PINK), (1536, RED))


# ---------------------------------------------------------------------------------------------------- the pixel rule
def hue_q(b, g, r):
    """hq in 0..1535 (256 = 60 degrees) of a chromatic pixel; Python's // is floor division."""
    mx, d = max(b, g, r), max(b, g, r) - min(b, g, r)
    if mx == r:
        return ((g - b) * 256 // d) % 1536
    if mx == g:
        return 512 + (b - r) * 256 // d
    return 1024 + (r - g) * 256 // d


def classify_pixel(b, g, r):
    b, g, r = int(b), int(g), int(r)
    mx, mn = max(b, g, r), min(b, g, r)
    d = mx - mn
    if mx < 40:
        return BLACK
    sat = d * 256 // mx
    if sat < 40:
        return BLACK if mx < 72 else GRAY if mx < 200 else WHITE
    hq = hue_q(b, g, r)
    c = next(name for bound, name in HUE_BOUNDS if hq < bound) if hq >= 64 else RED
    if c == ORANGE and mx < 176:
        c = BROWN
    if c == YELLOW and mx < 136:
        c = BROWN
    if c == RED and sat < 128 and mx >= 176:
        c = PINK
    return c


def features(px):
    """uint8 [..., 3] BGR -> int64 (mx, sat, hq) arrays; sat and hq are 0 where the rule does not reach them (mx = 0, d = 0)."""
    p = np.asarray(px).astype(np.int64)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    mx, mn = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    d = mx - mn
    sat = d * 256 // np.maximum(mx, 1)
    dd = np.maximum(d, 1)
    hq = np.where(mx == r, ((g - b) * 256 // dd) % 1536, np.where(mx == g, 512 + (b - r) * 256 // dd, 1024 + (r - g) * 256 // dd))
    return mx, sat, hq


def classify(px):
    """uint8 [..., 3] BGR -> uint8 [...] bins: classify_pixel over an array."""
    mx, sat, hq = features(px)
    c = np.full(hq.shape, RED, np.int64)
    for bound, name in reversed(HUE_BOUNDS[:-1]):
        c = np.where(hq < bound, name, c)
    c = np.where((c == ORANGE) & (mx < 176), BROWN, c)
    c = np.where((c == YELLOW) & (mx < 136), BROWN, c)
    c = np.where((c == RED) & (sat < 128) & (mx >= 176), PINK, c)
    c = np.where(sat < 40, np.where(mx < 72, BLACK, np.where(mx < 200, GRAY, WHITE)), c)
    return np.where(mx < 40, BLACK, c).astype(np.uint8)


def recip(d):
    """The device's reciprocal of d in 1..255: ceil(2^31 / d)."""
    return ((1 << 31) + d - 1) // d


def recip_div(n, d):
    """n // d as the device computes it for 0 <= n < 2^17: the high 32 bits of (2 n) * recip(d)."""
    return (2 * n * recip(d)) >> 32


def floor_div_device(num, d):
    """num // d for any sign as the device computes it: a negative numerator goes through -((-num + d - 1) // d)."""
    return recip_div(num, d) if num >= 0 else -recip_div(-num + d - 1, d)


# ---------------------------------------------------------------------------------------------------- geometry
def clip(rect, H, W):
    """The inclusive rectangle clipped to the frame, or None if nothing is left."""
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], W - 1), min(rect[3], H - 1)
    return (x0, y0, x1, y1) if x1 >= x0 and y1 >= y0 else None


def valid_row(row):
    return all(abs(int(v)) <= COORD_MAX for v in row[:4]) and int(row[2]) >= int(row[0]) and int(row[3]) >= int(row[1])


def part_of(row, frac, inset_q8):
    x1, y1, x2, y2 = (int(v) for v in row[:4])
    bw, bh = x2 - x1, y2 - y1
    inset = (bw * inset_q8) >> 8
    return (x1 + inset, y1 + ((bh * frac[0]) >> 8), x2 - inset, y1 + ((bh * frac[1]) >> 8))


def cover_q8(rows, i, P, H, W):
    """The largest share (q8) of P that one occluder of row i covers."""
    x0, y0, x1, y1 = P
    area = (x1 - x0 + 1) * (y1 - y0 + 1)
    rid, y2i, best = int(rows[i][4]), int(rows[i][3]), 0
    for j, r in enumerate(rows):
        if int(r[4]) == rid or not valid_row(r):
            continue
        if not (int(r[3]) > y2i or (int(r[3]) == y2i and j < i)):
            continue
        B = clip(tuple(int(v) for v in r[:4]), H, W)
        if B is None:
            continue
        iw, ih = min(x1, B[2]) - max(x0, B[0]) + 1, min(y1, B[3]) - max(y0, B[1]) + 1
        if iw > 0 and ih > 0:
            best = max(best, (iw * ih * 256) // area)
    return best


def describe(acc, samples):
    """(top, second, hist[12]) of one part."""
    if samples <= 0:
        return -1, -1, [0] * 12
    top = max(range(12), key=lambda k: (acc[k], -k))
    others = [k for k in range(12) if k != top]
    sec = max(others, key=lambda k: (acc[k], -k))
    if not (acc[sec] > 0 and acc[sec] * 4 >= acc[top]):
        sec = -1
    return top, sec, [int(a) // samples for a in acc]


class ColoursOracle:
    def __init__(self, frame_hw, max_tracks=128, forget_after=70, torso_q8=(51, 128), legs_q8=(141, 230), inset_q8=64, min_w=4, min_h=4,
                 max_cover_q8=64, stream=0):
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        assert 1 <= self.H <= 16384 and 1 <= self.W <= 16384 and 1 <= max_tracks <= MAX_TRACKS and forget_after >= 0
        assert all(0 <= a < b <= 256 for a, b in (torso_q8, legs_q8)) and 0 <= inset_q8 < 128 and min_w >= 1 and min_h >= 1
        self.max_tracks, self.forget_after, self.fracs, self.inset_q8 = max_tracks, forget_after, (tuple(torso_q8), tuple(legs_q8)), inset_q8
        self.min_w, self.min_h, self.max_cover_q8, self.stream = min_w, min_h, max_cover_q8, stream
        self.log = dict(sampled=0, covered=0, small=0, reused_in_call=0, saturated=0)    # what tests/test_colours_oracle.py counts
        self.reset()

    def reset(self):
        self.frame, self.status, self._freed = 0, 0, set()
        self.slots = [None] * self.max_tracks   # dict(id, cls, first, last, sightings, ended (0 or reason), samples [2], acc [2][12])

    # ------------------------------------------------------------------------------------------------ rows of one frame
    def sample_part(self, frame, rows, i, part):
        """s[12] of part 0 / 1 of row i, or None if it is not sampled."""
        P = clip(part_of(rows[i], self.fracs[part], self.inset_q8), self.H, self.W)
        if P is None or P[2] - P[0] + 1 < self.min_w or P[3] - P[1] + 1 < self.min_h:
            self.log["small"] += 1
            return None
        if cover_q8(rows, i, P, self.H, self.W) > self.max_cover_q8:
            self.log["covered"] += 1
            return None
        px = frame[P[1]:P[3] + 1, P[0]:P[2] + 1]
        n = px.shape[0] * px.shape[1]
        c = np.bincount(classify(px).reshape(-1), minlength=12)
        self.log["sampled"] += 1
        return [int(v) * 256 // n for v in c]

    def measure(self, frame, rows):
        """[(row index, id, cls, s_upper | None, s_lower | None)] of the counted rows, in row order."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        assert len(rows) <= MAX_ROWS
        out, seen = [], set()
        for i, r in enumerate(rows):
            if not valid_row(r) or int(r[4]) in seen:
                continue
            seen.add(int(r[4]))
            if clip(tuple(int(v) for v in r[:4]), self.H, self.W) is None:
                continue
            out.append((i, int(r[4]), int(r[5]), self.sample_part(frame, rows, i, 0), self.sample_part(frame, rows, i, 1)))
        return out

    # ------------------------------------------------------------------------------------------------ events
    def _event(self, s, reason):
        t = self.slots[s]
        (tu, su, hu), (tl, sl, hl) = describe(t["acc"][0], t["samples"][0]), describe(t["acc"][1], t["samples"][1])
        ev = [reason, self.stream, t["id"], t["cls"], t["first"], t["last"], t["sightings"], t["samples"][0], t["samples"][1], tu, su, tl, sl, s, 0, 0]
        return np.array(ev + hu + hl + [0] * 8, np.int32)

    def _tag(self, s):
        t = self.slots[s]
        (tu, _, hu), (tl, _, hl) = describe(t["acc"][0], t["samples"][0]), describe(t["acc"][1], t["samples"][1])
        return [tu, tl, hu[tu] if tu >= 0 else 0, hl[tl] if tl >= 0 else 0]

    def _emit(self, out, cap):
        for s, t in enumerate(self.slots):
            if t is not None and t["ended"] and len(out) < cap:
                out.append(self._event(s, t["ended"]))
                self.slots[s] = None
                self._freed.add(s)

    def pending(self):
        return sum(t is not None and t["ended"] != 0 for t in self.slots)

    # ------------------------------------------------------------------------------------------------ one tick
    def step(self, frame, rows, out, cap):
        """One tick; returns its row tags [n, 4]."""
        tags = np.full((len(rows), 4), -1, np.int32)
        if self.status:
            return tags
        f = self.frame
        counted = self.measure(frame, rows)
        live = {t["id"]: s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] <= self.forget_after}
        expiring = [s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] > self.forget_after]
        ended = [s for s, t in enumerate(self.slots) if t is not None and (t["ended"] or s in expiring)]          # slot order
        kept = ended[max(0, cap - len(out)):]                                # no room in the output list: they keep their slots
        occupied = len(live) + sum(self.slots[s]["ended"] != 0 for s in ended) + sum(s in expiring for s in kept)
        if occupied + sum(c[1] not in live for c in counted) > self.max_tracks:
            self.status = ERR_CAPACITY
            return tags
        for s in expiring:
            self.slots[s]["ended"] = EXPIRED
        self._emit(out, cap)
        for i, tid, cls, su, sl in counted:
            if tid in live:
                s = live[tid]
                t = self.slots[s]
            else:
                s = self.slots.index(None)
                self.log["reused_in_call"] += s in self._freed
                t = self.slots[s] = dict(id=tid, cls=cls, first=f, last=f, sightings=0, ended=0, samples=[0, 0], acc=[[0] * 12, [0] * 12])
            t["last"], t["cls"], t["sightings"] = f, cls, t["sightings"] + 1
            for part, sh in enumerate((su, sl)):
                if sh is None:
                    continue
                if t["samples"][part] >= SAMPLES_MAX:
                    self.log["saturated"] += 1
                    continue
                t["acc"][part] = [a + v for a, v in zip(t["acc"][part], sh)]
                t["samples"][part] += 1
            tags[i] = self._tag(s)
        self.frame += 1
        return tags

    # ------------------------------------------------------------------------------------------------ calls
    def update(self, frames, rows, cap):
        """frames[t], rows[t] for the ticks of one call -> ([event], pending, status, [row tags per tick]); ticks = 0 drains."""
        out, self._freed = [], set()
        if len(frames) == 0:
            self._emit(out, cap)
        tags = [self.step(fr, r, out, cap) for fr, r in zip(frames, rows)]
        return out, self.pending(), self.status, tags

    def flush(self, cap):
        out, self._freed = [], set()
        for t in self.slots:
            if t is not None and not t["ended"]:
                t["ended"] = FLUSHED
        self._emit(out, cap)
        return out, self.pending(), self.status, []

    def export(self):
        return [self._event(s, t["ended"]) for s, t in enumerate(self.slots) if t is not None]


def pack(results, cap, ticks=0):
    """[(finals, pending, status, tags per tick)] per stream -> the flat outputs of aic_colours_update / _flush: n_final [S], events
    [S, cap, 48], row_tags [rows, 4] (tick-major), pending [S], status [S]."""
    S = len(results)
    n_final, pending, status = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    events = np.zeros((S, cap, 48), np.int32)
    for s, (out, pend, st, _) in enumerate(results):
        n_final[s], pending[s], status[s] = len(out), pend, st
        for k, ev in enumerate(out):
            events[s, k] = ev
    tags = [results[s][3][t] for t in range(ticks) for s in range(S)]
    row_tags = np.concatenate(tags).reshape(-1, 4).astype(np.int32) if tags else np.zeros((0, 4), np.int32)
    return n_final, events, row_tags, pending, status


def run_bank(oracles, frames, rows, cap):
    """frames [ticks, S, H, W, 3]; rows[t][s] = rows array.  One call of a bank, packed."""
    T = len(frames)
    res = [o.update([frames[t][s] for t in range(T)], [rows[t][s] for t in range(T)], cap) for s, o in enumerate(oracles)]
    return pack(res, cap, T)


def flush_bank(oracles, cap, stream=None):
    res = [o.flush(cap) if stream is None or stream == s else ([], o.pending(), o.status, []) for s, o in enumerate(oracles)]
    return pack(res, cap)
