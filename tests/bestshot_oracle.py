"""The executable specification of the best-shot stage (aic_bestshot_*): Python ints and NumPy integer arrays
only, one stream per BestShotOracle.  The device is held to it with np.array_equal (tests/test_gpu_bestshot.py).

A tick of a stream is one BGR frame [H, W, 3] uint8 and rows [n, 6] int32 = x1 y1 x2 y2 id cls, what every tracker here delivers.

Region of a row (the arithmetic of aic_render_rects): box = (x1 - pad, y1 - pad, x2 + pad, y2 + pad) inclusive; head = the same x
range, y from y1 - pad to y1 + (((y2 - y1) * head_q8) >> 8).  C = the region clipped to the frame, cw x ch pixels.
A row is VALID if its four coordinates are within +-COORD_MAX and x2 >= x1, y2 >= y1; rows that are not are ignored altogether (they
do not claim their id, they occlude nothing).  A row is COUNTED if it is the first valid row of its id in row order and C is not
empty; a counted row is a CANDIDATE if cw >= min_w and ch >= min_h.

Thumbnail of a candidate, TH x TW x 3: column u covers source columns [xa, xb), xa = C.x0 + (u * cw) // TW, xb = C.x0 + ((u + 1) * cw)
// TW, xb = xa + 1 where that is empty; rows alike with ch and TH; a channel is (sum + n // 2) // n over the n pixels of the window.
Score: g = (29 B + 150 G + 77 R + 128) >> 8 on the thumbnail; sharp = sum |4 g(u, v) - g(u-1, v) - g(u+1, v) - g(u, v-1) - g(u, v+1)|
over the interior; fill_q8 = min(256, cw * ch * 256 // (TW * TH)); cover_q8 = max over the occluders j of area(C & Bj) * 256 // (cw *
ch), an occluder being a valid row of another id with y2_j > y2_i, or y2_j == y2_i and j < i, Bj its unpadded box clipped to the frame;
trunc = 1 if the frame clipped the region; score = (sharp * fill_q8 * (256 - cover_q8)) >> (16 + trunc).

Tick f of a stream (f counts every committed tick):
  1. the counted rows.
  2. capacity: the live slots that do not expire now, the ENDED slots not yet emitted, the slots that expire now but for which this
     call's output list has no room left (they stay ENDED and keep their slot), plus the counted rows of unknown ids, may not exceed
     max_tracks.  Otherwise the stream STOPS with ERR_CAPACITY: this tick is not committed, later ticks deliver nothing until reset();
     export, flush and a ticks = 0 drain still work.
  3. every live slot with f - last_seen > forget_after becomes ENDED (reason EXPIRED): frozen, never matched by an id again.
  4. ENDED slots are emitted in slot order while the call's output list has room (cap per stream per call) and become free.
  5. the counted rows in row order: an unknown id takes the lowest free slot; last_seen, cls and the sighting count are updated; a
     candidate replaces the slot's shot if there is none or score > best_score (strictly: the earlier of two equal shots stays).
An event is 16 ints: reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, has_shot, best_frame,
score, C.x0, C.y0, C.x1, C.y1, slot, 0 -- with its thumbnail, all zero when has_shot == 0 (best_frame, score and C are zero then)."""
import numpy as np

LIVE, EXPIRED, FLUSHED = 0, 1, 2
COORD_MAX = 1 << 20
MAX_ROWS = MAX_TRACKS = 512
ERR_CAPACITY = -5


def region_of(row, region="box", head_q8=64, pad=0):
    x1, y1, x2, y2 = (int(v) for v in row[:4])
    if region == "box":
        return (x1 - pad, y1 - pad, x2 + pad, y2 + pad)
    return (x1 - pad, y1 - pad, x2 + pad, y1 + (((y2 - y1) * head_q8) >> 8))


def clip(rect, H, W):
    """The inclusive rectangle clipped to the frame, or None if nothing is left."""
    x0, y0, x1, y1 = max(rect[0], 0), max(rect[1], 0), min(rect[2], W - 1), min(rect[3], H - 1)
    return (x0, y0, x1, y1) if x1 >= x0 and y1 >= y0 else None


def valid_row(row):
    return all(abs(int(v)) <= COORD_MAX for v in row[:4]) and int(row[2]) >= int(row[0]) and int(row[3]) >= int(row[1])


def windows(c0, cn, tn):
    """[(a, b)] for the tn thumbnail columns (rows) over cn source columns (rows) from c0: half-open, never empty."""
    out = []
    for u in range(tn):
        a, b = c0 + (u * cn) // tn, c0 + ((u + 1) * cn) // tn
        out.append((a, b if b > a else a + 1))
    return out


def thumbnail(frame, C, TW, TH):
    """uint8 [TH, TW, 3]: the integer area average of frame over C."""
    x0, y0, x1, y1 = C
    cw, ch = x1 - x0 + 1, y1 - y0 + 1
    crop = frame[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    integral = np.zeros((ch + 1, cw + 1, 3), np.int64)
    integral[1:, 1:] = crop.cumsum(0).cumsum(1)
    xs, ys = windows(0, cw, TW), windows(0, ch, TH)
    xa, xb = np.array([a for a, _ in xs]), np.array([b for _, b in xs])
    ya, yb = np.array([a for a, _ in ys]), np.array([b for _, b in ys])
    total = integral[yb][:, xb] - integral[ya][:, xb] - integral[yb][:, xa] + integral[ya][:, xa]
    n = ((yb - ya)[:, None] * (xb - xa)[None, :])[:, :, None]
    return ((total + n // 2) // n).astype(np.uint8)


def sharpness(thumb):
    t = thumb.astype(np.int64)
    g = (29 * t[:, :, 0] + 150 * t[:, :, 1] + 77 * t[:, :, 2] + 128) >> 8
    lap = 4 * g[1:-1, 1:-1] - g[1:-1, :-2] - g[1:-1, 2:] - g[:-2, 1:-1] - g[2:, 1:-1]
    return int(np.abs(lap).sum())


def cover_q8(rows, i, C, H, W):
    """The largest share (q8) of C that one occluder of row i covers."""
    x0, y0, x1, y1 = C
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


def score_of(thumb, C, trunc, cover, TW, TH):
    cw, ch = C[2] - C[0] + 1, C[3] - C[1] + 1
    fill = min(256, (cw * ch * 256) // (TW * TH))
    return (sharpness(thumb) * fill * (256 - cover)) >> (16 + trunc)


class BestShotOracle:
    def __init__(self, frame_hw, thumb=(64, 128), max_tracks=128, forget_after=70, region="box", head_q8=64, pad=0, min_w=8, min_h=16,
                 stream=0):
        self.H, self.W = int(frame_hw[0]), int(frame_hw[1])
        self.TW, self.TH = int(thumb[0]), int(thumb[1])
        assert 1 <= self.H <= 16384 and 1 <= self.W <= 16384
        assert 16 <= self.TW <= 128 and 16 <= self.TH <= 256 and self.TW % 8 == 0 and self.TH % 8 == 0
        assert 1 <= max_tracks <= MAX_TRACKS and forget_after >= 0 and region in ("box", "head") and 0 <= pad <= 64
        self.max_tracks, self.forget_after, self.region, self.head_q8, self.pad = max_tracks, forget_after, region, head_q8, pad
        self.min_w, self.min_h, self.stream = min_w, min_h, stream
        self.log = dict(replaced=0, tie_kept=0, reused_in_call=0)          # what tests/test_bestshot_oracle.py counts
        self.reset()

    def reset(self):
        self.frame, self.status, self._freed = 0, 0, set()
        self.slots = [None] * self.max_tracks   # dict(id, cls, first, last, sightings, ended (0 or reason), shot = None | (frame, score, C, thumb))

    # ------------------------------------------------------------------------------------------------ rows of one frame
    def measure(self, frame, rows):
        """[(row index, id, cls, C, candidate, trunc, score, thumb)] of the counted rows, in row order."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, 6)
        assert len(rows) <= MAX_ROWS
        out, seen = [], set()
        for i, r in enumerate(rows):
            if not valid_row(r) or int(r[4]) in seen:
                continue
            seen.add(int(r[4]))
            reg = region_of(r, self.region, self.head_q8, self.pad)
            C = clip(reg, self.H, self.W)
            if C is None:
                continue
            cw, ch = C[2] - C[0] + 1, C[3] - C[1] + 1
            cand = cw >= self.min_w and ch >= self.min_h
            trunc, score, thumb = int(C != reg), 0, None
            if cand:
                thumb = thumbnail(frame, C, self.TW, self.TH)
                score = score_of(thumb, C, trunc, cover_q8(rows, i, C, self.H, self.W), self.TW, self.TH)
            out.append((i, int(r[4]), int(r[5]), C, cand, trunc, score, thumb))
        return out

    # ------------------------------------------------------------------------------------------------ events
    def _event(self, s, reason):
        t = self.slots[s]
        shot = t["shot"]
        ev = [reason, self.stream, t["id"], t["cls"], t["first"], t["last"], t["sightings"], int(shot is not None)]
        ev += [shot[0], shot[1], *shot[2]] if shot else [0] * 6
        thumb = shot[3] if shot else np.zeros((self.TH, self.TW, 3), np.uint8)
        return np.array(ev + [s, 0], np.int32), thumb

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
        if self.status:
            return
        f = self.frame
        counted = self.measure(frame, rows)
        live = {t["id"]: s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] <= self.forget_after}
        expiring = [s for s, t in enumerate(self.slots) if t is not None and not t["ended"] and f - t["last"] > self.forget_after]
        ended = [s for s, t in enumerate(self.slots) if t is not None and (t["ended"] or s in expiring)]          # slot order
        kept = ended[max(0, cap - len(out)):]                                # no room in the output list: they keep their slots
        occupied = len(live) + sum(self.slots[s]["ended"] != 0 for s in ended) + sum(s in expiring for s in kept)
        if occupied + sum(c[1] not in live for c in counted) > self.max_tracks:
            self.status = ERR_CAPACITY
            return
        for s in expiring:
            self.slots[s]["ended"] = EXPIRED
        self._emit(out, cap)
        for _, tid, cls, C, cand, trunc, score, thumb in counted:
            if tid in live:
                t = self.slots[live[tid]]
            else:
                s = self.slots.index(None)
                self.log["reused_in_call"] += s in self._freed
                t = self.slots[s] = dict(id=tid, cls=cls, first=f, last=f, sightings=0, ended=0, shot=None)
            t["last"], t["cls"], t["sightings"] = f, cls, t["sightings"] + 1
            if cand:
                if t["shot"] is None or score > t["shot"][1]:
                    self.log["replaced"] += t["shot"] is not None
                    t["shot"] = (f, score, C, thumb)
                else:
                    self.log["tie_kept"] += score == t["shot"][1]
        self.frame += 1

    # ------------------------------------------------------------------------------------------------ calls
    def update(self, frames, rows, cap):
        """frames[t], rows[t] for the ticks of one call -> ([(event, thumb)], pending, status); ticks = 0 drains."""
        out, self._freed = [], set()
        if len(frames) == 0:
            self._emit(out, cap)
        for fr, r in zip(frames, rows):
            self.step(fr, r, out, cap)
        return out, self.pending(), self.status

    def flush(self, cap):
        out, self._freed = [], set()
        for t in self.slots:
            if t is not None and not t["ended"]:
                t["ended"] = FLUSHED
        self._emit(out, cap)
        return out, self.pending(), self.status

    def export(self):
        return [self._event(s, t["ended"]) for s, t in enumerate(self.slots) if t is not None]


def pack(results, cap, TW, TH):
    """[(finals, pending, status)] per stream -> the flat outputs of aic_bestshot_update / _flush: n_final [S], events [S, cap, 16],
    thumbs [S, cap, TH, TW, 3], pending [S], status [S]."""
    S = len(results)
    n_final, pending, status = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    events, thumbs = np.zeros((S, cap, 16), np.int32), np.zeros((S, cap, TH, TW, 3), np.uint8)
    for s, (out, pend, st) in enumerate(results):
        n_final[s], pending[s], status[s] = len(out), pend, st
        for k, (ev, th) in enumerate(out):
            events[s, k], thumbs[s, k] = ev, th
    return n_final, events, thumbs, pending, status


def run_bank(oracles, frames, rows, cap):
    """frames [ticks, S, H, W, 3]; rows[t][s] = rows array.  One call of a bank, packed."""
    res = [o.update([frames[t][s] for t in range(len(frames))], [rows[t][s] for t in range(len(frames))], cap) for s, o in enumerate(oracles)]
    return pack(res, cap, oracles[0].TW, oracles[0].TH)


def flush_bank(oracles, cap, stream=None):
    res = [o.flush(cap) if stream is None or stream == s else ([], o.pending(), o.status) for s, o in enumerate(oracles)]
    return pack(res, cap, oracles[0].TW, oracles[0].TH)
